// One `spzk` request: the subcommands of the command line as a re-entrant function (spzk_run.cpp).  The one-shot binary runs it once
// on the process's own argv, stdout and stderr (spzk_main.cpp); `spzk serve` runs it once per request on a worker thread, with the
// request's sinks, the client's working directory and generators from its cache (spzk_serve.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <functional>
#include <vector>
#include "../../include/otti_spartan.h"

// Where a request's generators come from.  The one-shot's provider makes them (the caller owns what it gets); the server's lends cached
// handles, valid until the provider object — one per request — is destroyed, and never freed by the borrower.
struct GensProvider {
    virtual ~GensProvider() {}
    virtual int nizk_gens(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, otti_gens **out) = 0;       // NIZKGens::new, or the cache's
    virtual int prepare(otti_instance *inst, otti_gens *gens) = 0;   // instance and window table on the device ahead of a proof (otti_prepare_device, or the shared table)
    virtual int snark_gens(uint64_t num_cons, uint64_t num_vars, uint64_t num_inputs, uint64_t num_ops, otti_snark_gens **out) = 0;
    virtual const char *gens_word() const { return "built"; }        // the served line's words: generators cached | built,
    virtual const char *table_word() const { return "own"; }         // table adopted | built | own (none: the request needed no table)
};

struct RunEnv {
    FILE *out, *err;              // the request's stdout and stderr
    const char *cwd;              // relative paths resolve against it; nullptr: the process's own
    GensProvider *gens;
    // served: a request among many in a process that lives on — nothing is set in the environment, nothing ends the process, everything made
    // is freed.  Not served (the one-shot): OTTI_MSM_WINDOW=10 unless set, the HIP runtime warmed on a thread beside the parsing, no frees, and
    // _exit behind the last line (the runtime's teardown is skipped).
    bool served;
    double queue_ms;              // served: accepted connection to worker; reported in the `* served:` line
    // served: the frees of what the request made (zkif arrays, instance, witness, proof: tens of ms at 2^20) are handed over here instead of being
    // run before spzk_run returns, so that the server can answer first; it runs them in order.  nullptr: freed before the return.
    std::vector<std::function<void()>> *after_answer;
    double t_before_main;         // one-shot: process creation to main(), for the `* process start to main()` line
};
// argv as main() gets it (argv[0] is not looked at).  Returns the exit status.
int spzk_run(int argc, char **argv, const RunEnv &E);
