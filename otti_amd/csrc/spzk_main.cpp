// spzk — the process around one request (spzk_run.cpp has the subcommands), or, as `spzk serve`, around many (spzk_serve.cpp).
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "spzk_run.h"
#include "spzk_serve.h"

// milliseconds from the creation of this process (execve) to now: /proc/self/stat's start time (clock ticks since boot) against
// CLOCK_BOOTTIME — what the dynamic loader spent mapping libamdhip64 and its dependencies before main() ran (10 ms resolution)
static double ms_since_process_start() {
    FILE *f = fopen("/proc/self/stat", "r"); if (!f) return -1;
    char buf[1024]; size_t n = fread(buf, 1, sizeof buf - 1, f); fclose(f); buf[n] = 0;
    const char *p = strrchr(buf, ')'); if (!p) return -1;
    unsigned long long start = 0; int field = 2;                  // p points at the end of field 2 (comm)
    for (p++; *p && field < 22; p++) if (*p == ' ') { field++; if (field == 22) { start = strtoull(p + 1, nullptr, 10); break; } }
    if (!start) return -1;
    struct timespec ts; if (clock_gettime(CLOCK_BOOTTIME, &ts) != 0) return -1;
    return (ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6) - 1e3 * (double)start / (double)sysconf(_SC_CLK_TCK);
}

// one proof per process: generators are made for it and belong to it
struct OneShotGens : GensProvider {
    int nizk_gens(uint64_t nc, uint64_t nv, uint64_t ni, otti_gens **out) override { return otti_gens_new(nc, nv, ni, out); }
    int prepare(otti_instance *inst, otti_gens *gens) override { return otti_prepare_device(inst, gens); }
    int snark_gens(uint64_t nc, uint64_t nv, uint64_t ni, uint64_t nops, otti_snark_gens **out) override { return otti_snark_gens_new(nc, nv, ni, nops, out); }
};

int main(int argc, char **argv) {
    const double t_before_main = ms_since_process_start();
    if (argc >= 2 && !strcmp(argv[1], "serve")) return spzk_serve_main(argc, argv);
    OneShotGens gens;
    const RunEnv E{stdout, stderr, nullptr, &gens, false, 0.0, nullptr, t_before_main};
    return spzk_run(argc, argv, E);
}
