// spzk — drop-in for the reference's spartan-zkinterface binary.
//   spzk verify --nizk <X.zkif> <X.inp.zkif> <X.wit.zkif>      [REF /root/reference/run.py:58 (via cargo run), run.py:100 (binary)]
// Reads the three zkInterface files, builds the R1CS instance, proves it on the MI355X, verifies the proof, prints
// "Verification successful" plus stage runtimes [REF /root/reference/README.md:46-48], exit status 0 on success.
// Without --nizk the same files go through SNARK mode (upstream spartan-zkinterface's default [RECALL]): SNARK::encode commits to the
// circuit, SNARK::prove adds the R1CSEvalProof, SNARK::verify checks it against the commitment alone.
// Additive options: --seed <hex32>, --proof-out <file>, --label <transcript label>, `spzk synth <n> <prefix>` to emit a
// synthetic zkif triple; `spzk check` and --check: does the assignment satisfy the circuit, and if not, which constraints fail
// (otti_witness_check_sat: on the device, on the uploaded assignment; no generators are made for `check`).
// SNARK mode across processes: `spzk encode` writes the computation commitment, `spzk prove --comm-in` completes its copy of it
// (otti_comp_comm_attach) and proves, `spzk verify <inputs> --comm-in --proof-in` checks the proof holding nothing but the commitment
// and the public inputs — no circuit, no witness, no GPU.
// This file is ONE request as a re-entrant function (spzk_run.h): the one-shot process runs it once (spzk_main.cpp), `spzk serve` once per request
// on a worker thread (spzk_serve.cpp).  What differs between the two is behind RunEnv::served, and nowhere else.
#include <stdio.h>
#include <thread>
#include <time.h>
#include <unistd.h>
#include <sys/stat.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <chrono>
#include <algorithm>
#include <unistd.h>
#include <functional>
#include "spzk_run.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int fail(const RunEnv &E, const char *what, int rc) {
    char msg[512]; otti_last_error(msg, sizeof msg);
    std::string m = msg;
    if (E.cwd) {                                                // the library names files as it was given them: say them as the client did
        const std::string prefix = std::string(E.cwd) + "/";
        for (size_t at = m.find(prefix); at != std::string::npos; at = m.find(prefix, at)) m.erase(at, prefix.size());
    }
    fprintf(E.err, "spzk: %s failed (%d): %s\n", what, rc, m.c_str());
    return 1;
}
static int usage(const RunEnv &E) {
    fprintf(E.err, "usage: spzk verify [--nizk] <circuit.zkif> <inputs.inp.zkif> <witness.wit.zkif> [--seed HEX64] [--proof-out FILE] [--label STR] [--check]\n"
                    "            (the reference's invocation: prove, then verify, in one process; without --nizk: SNARK mode)\n"
                    "       spzk prove  --nizk <circuit.zkif> <inputs.inp.zkif> <witness.wit.zkif> --proof-out FILE [--seed HEX64] [--label STR] [--check]\n"
                    "       spzk verify --nizk <circuit.zkif> <inputs.inp.zkif> --proof-in FILE [--label STR]\n"
                    "       spzk encode <circuit.zkif> [<inputs.inp.zkif>] --comm-out FILE\n"
                    "            (SNARK::encode: writes the computation commitment)\n"
                    "       spzk prove  <circuit.zkif> <inputs.inp.zkif> <witness.wit.zkif> [--comm-in FILE] --proof-out FILE [--seed HEX64] [--label STR] [--check] [--verify-comm]\n"
                    "            (SNARK::prove from a stored commitment; --verify-comm: recompute it and compare first; without --comm-in: encodes itself)\n"
                    "       spzk verify <inputs.inp.zkif> --comm-in FILE --proof-in FILE [--label STR]\n"
                    "            (SNARK::verify from the commitment and the public inputs alone: no circuit, no witness, no GPU)\n"
                    "       spzk check [--nizk] <circuit.zkif> <inputs.inp.zkif> <witness.wit.zkif>\n"
                    "            (does the assignment satisfy the circuit? exit 0: yes; 1: no, with the failing constraints; no proof is made)\n"
                    "            --check: the same test after the upload, before proving; an unsatisfied assignment is reported and not proved\n"
                    "       spzk synth <num_constraints> <out_prefix> [num_inputs] [seed]\n");
    return 2;
}

// The end of a request whose lines are all printed and whose files are written.  The one-shot leaves at once, skipping the HIP runtime's
// teardown; a served request returns to its worker.
static int done(const RunEnv &E, int status) {
    fflush(E.out);
    if (!E.served) _exit(status);
    return status;
}
// a path argument as the request's working directory sees it (messages print the argument as it was given)
static std::string at(const RunEnv &E, const char *path) {
    if (!E.cwd || !path || path[0] == '/') return path ? path : "";
    return std::string(E.cwd) + "/" + path;
}
// What a served request made and has to free, newest first; the one-shot frees nothing (the process ends and hands everything back at once).
struct Frees {
    bool on; std::vector<std::function<void()>> f; std::vector<std::function<void()>> *later;
    explicit Frees(const RunEnv &E) : on(E.served), later(E.after_answer) {}
    ~Frees() {
        if (!on) return;
        for (auto it = f.rbegin(); it != f.rend(); ++it) { if (later) later->push_back(std::move(*it)); else (*it)(); }
    }
    void add(std::function<void()> fn) { if (on) f.push_back(std::move(fn)); }
};

// The satisfiability check on the uploaded assignment.  0: satisfied; 1: not (the report is printed); -1: the call itself failed (reported).
constexpr size_t kCheckRows = 16;                              // failing constraints listed at most
static void print_hex32(const RunEnv &E, const uint8_t *le) { for (int i = 31; i >= 0; i--) fprintf(E.out, "%02x", le[i]); }   // canonical value, most significant digit first
static int run_check(const RunEnv &E, otti_instance *inst, otti_witness *wit, uint64_t num_cons) {
    uint64_t n_unsat = 0, rows[kCheckRows]; uint8_t abc[96 * kCheckRows]; float kernel_ms = 0;
    const double t0 = now_ms();
    const int rc = otti_witness_check_sat(inst, wit, &n_unsat, rows, kCheckRows, abc, &kernel_ms);
    if (rc) { fail(E, "check_sat", rc); return -1; }
    fprintf(E.out, "* check_sat %.3f ms\n  * kernel %.3f ms\n", now_ms() - t0, kernel_ms);
    if (!n_unsat) return 0;
    fprintf(E.out, "Unsatisfied: %llu of %llu constraints\n", (unsigned long long)n_unsat, (unsigned long long)num_cons);
    for (size_t i = 0; i < kCheckRows && i < n_unsat; i++) {
        fprintf(E.out, "  constraint %llu: A.z=", (unsigned long long)rows[i]); print_hex32(E, abc + 96 * i);
        fprintf(E.out, " B.z="); print_hex32(E, abc + 96 * i + 32); fprintf(E.out, " C.z="); print_hex32(E, abc + 96 * i + 64); fprintf(E.out, "\n");
    }
    return 1;
}

static bool read_file(const RunEnv &E, const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(at(E, path).c_str(), "rb");
    if (!f) { fprintf(E.err, "spzk: cannot read %s\n", path); return false; }
    fseek(f, 0, SEEK_END); const long len = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize(len > 0 ? (size_t)len : 0);
    const bool ok = fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    if (!ok) fprintf(E.err, "spzk: short read on %s\n", path);
    return ok;
}
static bool write_file(const RunEnv &E, const char *path, const uint8_t *p, size_t n) {
    FILE *f = fopen(at(E, path).c_str(), "wb");
    const bool ok = f && fwrite(p, 1, n, f) == n;
    if (f) fclose(f);
    if (!ok) fprintf(E.err, "spzk: cannot write %s\n", path);
    return ok;
}

// ---- SNARK mode, one role per process.  role 'e': encode, 'p': prove, 'v': verify.  Returns the exit status.
struct SnarkRoleArgs { char role; std::vector<const char *> files; const char *comm_in, *comm_out, *proof_in, *proof_out, *label; const uint8_t *seed; bool check, verify_comm; double t_main0; };
// A SERVED request, in NIZK and in SNARK mode alike, takes the files to a ready instance in one call (otti_instance_from_zkif, OTTI_INGEST_AUTO: on the
// device when the circuit's size allows — the worker's runtime is up).  SNARK encode / attach fill the decommitment from the entry lists the device
// ingest keeps in HBM (snark_encode.cpp decomm_fill_from_entries): no host lists are made for them.  The one-shot keeps the host path (it parses
// while its HIP runtime comes up).  After a device ingest the assignment's A, B, C are NULL: only their counts are set.
// SNARK requests take it from kServedSnarkMinMB MiB of circuit file on only: measured (profiles/snark_zkif_ingest.md, tools/snark_ingest_probe.py), a
// served `prove --comm-in` of the smallest probed circuit (2^16 uniform, 15.2 MiB) came out slower than the parent's host path at the median (39.7
// against 20.4 ms: a 22 - 28 ms wait in the ingest's first allocations behind the previous proof's frees, the one profiles/zkif_ingest.md describes),
// while from the next probed size (2^16 compiler-like, 43.9 MiB) on both requests beat it.  OTTI_INGEST_SNARK_MIN_MB (MiB, read per request)
// overrides it; with OTTI_INGEST_MIN_MB set and that one not, the general cut-over alone decides.
// Returns 1: taken; 0: not taken, or the FILES were refused (the three codes a loader gives a file: the
// caller then goes the host path, which words such a refusal stage by stage exactly as the one-shot does); any other failure — no device, no
// memory, a HIP error — is the request's failure and comes back as its negative code: nothing is parsed a second time behind it.
constexpr double kServedSnarkMinMB = 43.0;
static double served_snark_min_mb() {
    if (const char *e = getenv("OTTI_INGEST_SNARK_MIN_MB")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) return v; }
    return getenv("OTTI_INGEST_MIN_MB") ? 0.0 : kServedSnarkMinMB;
}
static int served_ingest(const RunEnv &E, bool nizk, const std::string &circuit, const std::string &inputs, const char *witness, otti_instance **inst, otti_r1cs **r,
                         otti_witness **wit = nullptr) {
    if (!E.served) return 0;
    struct stat st;
    if (!nizk && (stat(circuit.c_str(), &st) != 0 || (double)st.st_size < served_snark_min_mb() * 1048576.0)) return 0;
    // A prove request (wit given) whose witness file AUTO would read on the device: the circuit without the witness file — the call returns the public
    // inputs —, then the two files to a resident witness (otti_witness_from_zkif), which the proof is made from.  A refusal of the FILES by either call
    // — for the second also: files of other dimensions than the circuit's, and a worker without a device, which the host path words as the one-shot
    // does — leaves nothing behind and goes the host path.
    // A smaller witness file is parsed with the circuit and uploaded by the proof, as ever (profiles/zkif_witness_ingest.md: why the request looks itself).
    const bool resident = wit && stat(witness, &st) == 0 && (double)st.st_size >= otti_witness_ingest_min_mb() * 1048576.0;
    int rc = otti_instance_from_zkif(circuit.c_str(), inputs.c_str(), resident ? nullptr : witness, OTTI_INGEST_AUTO, inst, r);
    if (rc == OTTI_OK && resident) {
        rc = otti_witness_from_zkif(*inst, inputs.c_str(), witness, OTTI_INGEST_AUTO, wit, nullptr);
        if (rc != OTTI_OK) { otti_instance_free(*inst); otti_r1cs_free(*r); *inst = nullptr; *r = nullptr; if (rc == OTTI_ERR_BAD_ARG || rc == OTTI_ERR_NO_DEVICE) rc = OTTI_ERR_IO; }
    }
    if (rc == OTTI_OK) return 1;
    return rc == OTTI_ERR_IO || rc == OTTI_ERR_INVALID_INDEX || rc == OTTI_ERR_INVALID_SCALAR ? 0 : rc;
}
static const char *witness_word(const otti_witness *wit) {
    int32_t on_device = 0;
    return wit && otti_witness_ingest_info(wit, &on_device, nullptr, nullptr) == OTTI_OK && on_device ? "device" : "host";
}
static const char *ingest_word(const otti_instance *inst) {
    int32_t on_device = 0;
    return otti_instance_ingest_info(inst, &on_device, nullptr, nullptr, nullptr) == OTTI_OK && on_device ? "device" : "host";
}
// the one line in which a served request's stdout differs from the one-shot's: how the request was served / what the process's start cost
static void origin_line(const RunEnv &E, const otti_witness *wit, const otti_instance *inst, double t_main0) {
    if (E.served) fprintf(E.out, "* served: queue %.3f ms, generators %s, table %s, witness %s, ingest %s\n", E.queue_ms, E.gens->gens_word(), E.gens->table_word(), witness_word(wit),
                          ingest_word(inst));
    else fprintf(E.out, "* process start to main() %.0f ms (the dynamic loader mapping the HIP runtime), main() %.3f ms\n", E.t_before_main, now_ms() - t_main0);
}
static int snark_role(const RunEnv &E, const SnarkRoleArgs &a) {
    int rc; double t0 = now_ms(); Frees fr(E);
    if (a.role == 'v') {                                       // the commitment, the public inputs, the proof: nothing else, and no device
        std::vector<uint8_t> cb, proof;
        if (!read_file(E, a.comm_in, cb) || !read_file(E, a.proof_in, proof)) return 1;
        otti_comp_comm *cc = nullptr; rc = otti_comp_comm_from_bytes(cb.data(), cb.size(), &cc); if (rc) return fail(E, "commitment parse", rc);
        fr.add([=] { otti_comp_comm_free(cc); });
        otti_r1cs *r = nullptr; rc = otti_zkif_load_inputs(at(E, a.files[0]).c_str(), &r); if (rc) return fail(E, "zkif load (inputs)", rc);
        fr.add([=] { otti_r1cs_free(r); });
        uint64_t nc, nv, ni, nops; rc = otti_comp_comm_dims(cc, &nc, &nv, &ni, &nops, nullptr); if (rc) return fail(E, "commitment dimensions", rc);
        otti_snark_gens *sg = nullptr; rc = E.gens->snark_gens(nc, nv, ni, nops, &sg); if (rc) return fail(E, "SNARKGens::new", rc);
        const double t_setup = now_ms() - t0; t0 = now_ms();
        rc = otti_snark_verify(cc, r->inputs32, r->ninputs, sg, (const uint8_t *)a.label, strlen(a.label), proof.data(), proof.size());
        fprintf(E.out, "* commitment: %llu constraints, %llu variables, %llu inputs, %llu operations per matrix (%zu bytes)\n* setup (parse, SNARKGens::new) %.3f ms\n* SNARK::verify %.3f ms\n",
               (unsigned long long)nc, (unsigned long long)nv, (unsigned long long)ni, (unsigned long long)nops, cb.size(), t_setup, now_ms() - t0);
        if (rc) { char msg[512]; otti_last_error(msg, sizeof msg); fprintf(E.out, "Verification FAILED (%d%s%s)\n", rc, msg[0] ? ": " : "", msg); return 1; }
        fprintf(E.out, "Verification successful\n");
        return 0;
    }
    otti_r1cs *r = nullptr; otti_instance *inst = nullptr;
    otti_witness *wit = nullptr;                               // a served prove request whose witness file went straight to HBM; --check: uploaded below
    {
        const std::string f0 = at(E, a.files[0]), f1 = at(E, a.files.size() > 1 ? a.files[1] : nullptr), f2 = at(E, a.role == 'p' ? a.files[2] : nullptr);
        // (an encode request may name the circuit alone: the one-call ingest wants the inputs file as well, so that one goes the host path)
        const int took = a.files.size() > 1 ? served_ingest(E, false, f0, f1, a.role == 'p' ? f2.c_str() : nullptr, &inst, &r, a.role == 'p' ? &wit : nullptr) : 0;
        if (took < 0) return fail(E, "zkif ingest", took);
        if (!took) { rc = otti_zkif_load(f0.c_str(), a.files.size() > 1 ? f1.c_str() : nullptr, a.role == 'p' ? f2.c_str() : nullptr, &r); if (rc) return fail(E, "zkif load", rc); }
    }
    fr.add([=] { otti_r1cs_free(r); });
    const double t_load = now_ms() - t0; t0 = now_ms();
    if (!inst) { rc = otti_instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC, &inst); if (rc) return fail(E, "Instance::new", rc); }
    fr.add([=] { otti_instance_free(inst); });
    if (wit) fr.add([=] { otti_witness_free(wit); });
    const uint64_t nnz = std::max<uint64_t>({(uint64_t)r->nA, (uint64_t)r->nB, (uint64_t)r->nC});
    otti_snark_gens *sg = nullptr; rc = E.gens->snark_gens(r->num_cons, r->num_vars, r->num_inputs, nnz, &sg); if (rc) return fail(E, "SNARKGens::new", rc);
    const double t_setup = now_ms() - t0; t0 = now_ms();
    uint64_t nc, nv, ni; otti_instance_dims(inst, &nc, &nv, &ni);
    fprintf(E.out, "* instance: %llu constraints (padded %llu), %llu variables (padded %llu), %llu inputs, %llu non-zero entries in the largest matrix\n", (unsigned long long)r->num_cons,
           (unsigned long long)nc, (unsigned long long)r->num_vars, (unsigned long long)nv, (unsigned long long)ni, (unsigned long long)nnz);
    fprintf(E.out, "* zkif_load %.3f ms\n* setup (Instance::new, SNARKGens::new) %.3f ms\n", t_load, t_setup);
    otti_comp_comm *cc = nullptr;
    if (a.comm_in) {                                           // the stored commitment, completed from this process's own instance
        std::vector<uint8_t> cb;
        if (!read_file(E, a.comm_in, cb)) return 1;
        rc = otti_comp_comm_from_bytes(cb.data(), cb.size(), &cc); if (rc) return fail(E, "commitment parse", rc);
        fr.add([=] { otti_comp_comm_free(cc); });
        rc = otti_comp_comm_attach(cc, inst, sg, a.verify_comm ? OTTI_ATTACH_VERIFY : 0u); if (rc) return fail(E, "commitment attach", rc);
        fprintf(E.out, "* attach%s %.3f ms (computation commitment %zu bytes)\n", a.verify_comm ? " (commitments recomputed and compared)" : "", now_ms() - t0, cb.size());
    } else {
        rc = otti_snark_encode(inst, sg, &cc); if (rc) return fail(E, "SNARK::encode", rc);
        fr.add([=] { otti_comp_comm_free(cc); });
        uint8_t *cb = nullptr; size_t cb_len = 0; rc = otti_comp_comm_bytes(cc, &cb, &cb_len); if (rc) return fail(E, "commitment bytes", rc);
        fprintf(E.out, "* SNARK::encode %.3f ms (computation commitment %zu bytes)\n", now_ms() - t0, cb_len);
        if (a.role == 'e') origin_line(E, nullptr, inst, a.t_main0);
        if (a.comm_out && !write_file(E, a.comm_out, cb, cb_len)) { if (E.served) otti_buf_free(cb); return 1; }
        if (a.comm_out) fprintf(E.out, "Commitment written to %s (%zu bytes)\n", a.comm_out, cb_len);
        otti_buf_free(cb);
    }
    if (a.role == 'e') return done(E, 0);
    t0 = now_ms();
    if (a.check) {
        if (!wit) {
            rc = otti_witness_upload(inst, r->vars32, r->nvars, r->inputs32, r->ninputs, &wit); if (rc) return fail(E, "witness upload", rc);
            fr.add([=] { otti_witness_free(wit); });
        }
        const int sat = run_check(E, inst, wit, r->num_cons);
        if (sat < 0) return 1;
        if (sat) { fprintf(E.out, "Not proved (unsatisfied assignment)\n"); return 1; }
        t0 = now_ms();
    }
    uint8_t *proof = nullptr; size_t proof_len = 0; double st[10] = {0};
    if (wit) rc = otti_snark_prove_resident(inst, cc, wit, sg, (const uint8_t *)a.label, strlen(a.label), a.seed, &proof, &proof_len, st);
    else rc = otti_snark_prove(inst, cc, r->vars32, r->nvars, r->inputs32, r->ninputs, sg, (const uint8_t *)a.label, strlen(a.label), a.seed, OTTI_FLAG_GPU, &proof, &proof_len, st);
    if (rc) return fail(E, "SNARK::prove", rc);
    fr.add([=] { otti_buf_free(proof); });
    fprintf(E.out, "* SNARK::prove %.3f ms\n  * polycommit %.3f ms\n  * multiply_vec %.3f ms\n  * prove_sc_phase_one %.3f ms\n  * eval_table_sparse %.3f ms\n  * prove_sc_phase_two %.3f ms\n"
           "  * polyeval %.3f ms\n  * R1CSEvalProof: derefs commitment %.3f ms, product circuits %.3f ms, hash layer %.3f ms\n  * len_snark_proof %zu\n",
           now_ms() - t0, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], proof_len);
    origin_line(E, wit, inst, a.t_main0);
    if (!write_file(E, a.proof_out, proof, proof_len)) return 1;
    fprintf(E.out, "Proof written to %s (%zu bytes)\n", a.proof_out, proof_len);
    return done(E, 0);
}

int spzk_run(int argc, char **argv, const RunEnv &E) {
    const double t_main0 = now_ms();
    Frees fr(E);
    if (argc < 2) return usage(E);
    if (!strcmp(argv[1], "synth")) {
        if (argc < 4) return usage(E);
        uint64_t n = strtoull(argv[2], 0, 0), ni = argc > 4 ? strtoull(argv[4], 0, 0) : 10, seed = argc > 5 ? strtoull(argv[5], 0, 0) : 1;
        otti_r1cs *r = nullptr; int rc = otti_synth_r1cs(n, ni, seed, &r); if (rc) return fail(E, "synth", rc);
        std::string p = argv[3]; const std::string q = at(E, argv[3]);
        rc = otti_zkif_write(r, (q + ".zkif").c_str(), (q + ".inp.zkif").c_str(), (q + ".wit.zkif").c_str());
        otti_r1cs_free(r); if (rc) return fail(E, "zkif write", rc);
        fprintf(E.out, "wrote %s.zkif %s.inp.zkif %s.wit.zkif (%llu constraints)\n", p.c_str(), p.c_str(), p.c_str(), (unsigned long long)n);
        return 0;
    }
    const bool prove_only = !strcmp(argv[1], "prove"), check_only = !strcmp(argv[1], "check"), encode_only = !strcmp(argv[1], "encode");
    if (!prove_only && !check_only && !encode_only && strcmp(argv[1], "verify")) return usage(E);
    // one proof per process: the generator window table is built and used once, so a narrow window (small table, ~7 ms to build for
    // R = 1024) beats the wide one a long-lived prover process amortises (see prover.cpp device_window_bits); an explicit setting wins
    // (a server reads OTTI_MSM_WINDOW from its own environment, once: its table is used by many proofs)
    if (!E.served) setenv("OTTI_MSM_WINDOW", "10", 0);
    bool nizk = false, label_given = false, check = false, verify_comm = false; std::vector<const char *> files;
    const char *seed_hex = nullptr, *proof_out = nullptr, *proof_in = nullptr, *comm_in = nullptr, *comm_out = nullptr, *label = "nizk_example";
    for (int i = 2; i < argc; i++) {
        if (!strcmp(argv[i], "--nizk")) nizk = true;
        else if (!strcmp(argv[i], "--check")) check = true;
        else if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed_hex = argv[++i];
        else if (!strcmp(argv[i], "--proof-out") && i + 1 < argc) proof_out = argv[++i];
        else if (!strcmp(argv[i], "--proof-in") && i + 1 < argc) proof_in = argv[++i];
        else if (!strcmp(argv[i], "--comm-in") && i + 1 < argc) comm_in = argv[++i];
        else if (!strcmp(argv[i], "--comm-out") && i + 1 < argc) comm_out = argv[++i];
        else if (!strcmp(argv[i], "--verify-comm")) verify_comm = true;
        else if (!strcmp(argv[i], "--label") && i + 1 < argc) { label = argv[++i]; label_given = true; }
        else files.push_back(argv[i]);
    }
    const bool verify_only = proof_in != nullptr;
    if (check_only) {                                          // load, Instance::new, upload, check: no generators, no window table
        if (files.size() != 3 || verify_only || proof_out || comm_in || comm_out) return usage(E);
        otti_r1cs *r = nullptr; otti_instance *inst = nullptr; int rc = 0;
        const int took = served_ingest(E, nizk, at(E, files[0]), at(E, files[1]), at(E, files[2]).c_str(), &inst, &r);
        if (took < 0) return fail(E, "zkif ingest", took);
        if (!took) {
            rc = otti_zkif_load(at(E, files[0]).c_str(), at(E, files[1]).c_str(), at(E, files[2]).c_str(), &r); if (rc) return fail(E, "zkif load", rc);
            fr.add([=] { otti_r1cs_free(r); });
            rc = otti_instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC, &inst); if (rc) return fail(E, "Instance::new", rc);
        } else fr.add([=] { otti_r1cs_free(r); });
        fr.add([=] { otti_instance_free(inst); });
        rc = otti_prepare_device(inst, nullptr); if (rc) return fail(E, "device setup", rc);
        otti_witness *wit = nullptr;
        rc = otti_witness_upload(inst, r->vars32, r->nvars, r->inputs32, r->ninputs, &wit); if (rc) return fail(E, "witness upload", rc);
        fr.add([=] { otti_witness_free(wit); });
        const int sat = run_check(E, inst, wit, r->num_cons);
        if (sat == 0) fprintf(E.out, "Satisfied\n");
        return done(E, sat == 0 ? 0 : 1);
    }
    if (check && verify_only) return usage(E);                  // a separate verifier has no witness to check
    // the stored computation commitment belongs to SNARK mode; its roles: encode / prove / verify --comm-in --proof-in (snark_role)
    if (nizk && (encode_only || comm_in || comm_out || verify_comm)) return usage(E);
    const bool snark_split = !nizk && (encode_only || prove_only || verify_only);
    if (!nizk && !label_given) label = "snark_example";
    if (prove_only && (verify_only || !proof_out)) return usage(E);
    if (snark_split) {
        if (encode_only && (!comm_out || comm_in || proof_out || verify_only || check || verify_comm || (files.size() != 1 && files.size() != 2))) return usage(E);
        if (prove_only && (files.size() != 3 || comm_out || (verify_comm && !comm_in))) return usage(E);
        if (verify_only && (!comm_in || comm_out || proof_out || verify_comm || files.size() != 1)) {
            fprintf(E.err, "spzk: SNARK mode verifies a stored proof against a stored commitment: verify <inputs.inp.zkif> --comm-in FILE --proof-in FILE\n"); return usage(E);
        }
    } else {
        if (comm_in || comm_out || verify_comm) return usage(E);
        if (verify_only ? (files.size() != 2 && files.size() != 3) : files.size() != 3) return usage(E);
    }
    uint8_t seed[32]; const uint8_t *seedp = nullptr;
    if (seed_hex) {
        if (strlen(seed_hex) != 64) { fprintf(E.err, "spzk: --seed wants 64 hex digits\n"); return 2; }
        for (int i = 0; i < 32; i++) { unsigned v; if (sscanf(seed_hex + 2 * i, "%2x", &v) != 1) return usage(E); seed[i] = (uint8_t)v; }
        seedp = seed;
    }
    // the HIP runtime takes a noticeable fraction of a second to come up: let it do so while the files are being parsed
    // (a server's workers brought their contexts up when they started)
    std::thread warm;
    if (!E.served) warm = std::thread([&] { if (!verify_only && otti_device_count() > 0) (void)otti_prepare_device(nullptr, nullptr); });
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{warm};
    if (snark_split) {
        SnarkRoleArgs a{encode_only ? 'e' : prove_only ? 'p' : 'v', files, comm_in, comm_out, proof_in, proof_out, label, seedp, check, verify_comm, t_main0};
        const int status = snark_role(E, a);
        fflush(E.out);
        return status;
    }
    double t0 = now_ms();
    otti_r1cs *r = nullptr; int rc;
    otti_instance *inst = nullptr;
    otti_witness *wit = nullptr;                               // a served prove request: the witness file went straight to HBM; --check: uploaded below; proved from HBM
    {
        const std::string f0 = at(E, files[0]), f1 = at(E, files[1]), f2 = at(E, verify_only ? nullptr : files[2]);
        const int took = served_ingest(E, nizk, f0, f1, verify_only ? nullptr : f2.c_str(), &inst, &r, verify_only ? nullptr : &wit);
        if (took < 0) return fail(E, "zkif ingest", took);
        if (!took) {
            rc = otti_zkif_load(f0.c_str(), f1.c_str(), verify_only ? nullptr : f2.c_str(), &r); if (rc) return fail(E, "zkif load", rc);
        }
    }
    fr.add([=] { otti_r1cs_free(r); });
    double t_load = now_ms() - t0; t0 = now_ms();
    // NIZKGens::new (a thousand hash-to-group maps and the host window tables) depends on the sizes only: it runs next to Instance::new
    otti_gens *gens_early = nullptr; int gens_rc = 0;
    std::thread gens_thread;
    if (nizk) gens_thread = std::thread([&] { gens_rc = E.gens->nizk_gens(r->num_cons, r->num_vars, r->num_inputs, &gens_early); });
    auto gens_rc_wait = [&] { if (gens_thread.joinable()) gens_thread.join(); return gens_rc; };
    struct GensJoiner { std::thread &t; ~GensJoiner() { if (t.joinable()) t.join(); } } gens_joiner{gens_thread};
    if (!inst) { rc = otti_instance_new(r->num_cons, r->num_vars, r->num_inputs, r->A, r->nA, r->B, r->nB, r->C, r->nC, &inst); if (rc) return fail(E, "Instance::new", rc); }
    fr.add([=] { otti_instance_free(inst); });
    if (wit) fr.add([=] { otti_witness_free(wit); });
    if (check) {                                               // --check: the assignment is uploaded once, checked, and proved from HBM
        rc = otti_prepare_device(inst, nullptr); if (rc) return fail(E, "device setup", rc);
        if (!wit) {
            rc = otti_witness_upload(inst, r->vars32, r->nvars, r->inputs32, r->ninputs, &wit); if (rc) return fail(E, "witness upload", rc);
            fr.add([=] { otti_witness_free(wit); });
        }
        const int sat = run_check(E, inst, wit, r->num_cons);
        if (sat < 0) return 1;
        if (sat) { fprintf(E.out, "Verification FAILED (unsatisfied assignment)\n"); return 1; }
    }
    if (!nizk) {                                               // ---- SNARK mode: encode, prove, verify
        const uint64_t nnz = std::max<uint64_t>({(uint64_t)r->nA, (uint64_t)r->nB, (uint64_t)r->nC});
        otti_snark_gens *sg = nullptr; rc = E.gens->snark_gens(r->num_cons, r->num_vars, r->num_inputs, nnz, &sg); if (rc) return fail(E, "SNARKGens::new", rc);
        double t_setup = now_ms() - t0; t0 = now_ms();
        otti_comp_comm *cc = nullptr; rc = otti_snark_encode(inst, sg, &cc); if (rc) return fail(E, "SNARK::encode", rc);
        fr.add([=] { otti_comp_comm_free(cc); });
        double t_encode = now_ms() - t0; t0 = now_ms();
        uint8_t *proof = nullptr; size_t proof_len = 0; double st[10] = {0};
        if (wit) rc = otti_snark_prove_resident(inst, cc, wit, sg, (const uint8_t *)label, strlen(label), seedp, &proof, &proof_len, st);
        else rc = otti_snark_prove(inst, cc, r->vars32, r->nvars, r->inputs32, r->ninputs, sg, (const uint8_t *)label, strlen(label), seedp, OTTI_FLAG_GPU, &proof, &proof_len, st);
        if (rc) return fail(E, "SNARK::prove", rc);
        fr.add([=] { otti_buf_free(proof); });
        double t_prove = now_ms() - t0; t0 = now_ms();
        // the verifier's copy of the commitment: its bytes only
        uint8_t *cb = nullptr; size_t cb_len = 0; rc = otti_comp_comm_bytes(cc, &cb, &cb_len); if (rc) return fail(E, "commitment bytes", rc);
        fr.add([=] { otti_buf_free(cb); });
        otti_comp_comm *vc = nullptr; rc = otti_comp_comm_from_bytes(cb, cb_len, &vc); if (rc) return fail(E, "commitment parse", rc);
        fr.add([=] { otti_comp_comm_free(vc); });
        rc = otti_snark_verify(vc, r->inputs32, r->ninputs, sg, (const uint8_t *)label, strlen(label), proof, proof_len);
        double t_verify = now_ms() - t0;
        uint64_t nc, nv, ni; otti_instance_dims(inst, &nc, &nv, &ni);
        fprintf(E.out, "* instance: %llu constraints (padded %llu), %llu variables (padded %llu), %llu inputs, %llu non-zero entries in the largest matrix\n", (unsigned long long)r->num_cons,
               (unsigned long long)nc, (unsigned long long)r->num_vars, (unsigned long long)nv, (unsigned long long)ni, (unsigned long long)nnz);
        fprintf(E.out, "* zkif_load %.3f ms\n* setup (Instance::new, SNARKGens::new) %.3f ms\n* SNARK::encode %.3f ms (computation commitment %zu bytes)\n", t_load, t_setup, t_encode, cb_len);
        fprintf(E.out, "* SNARK::prove %.3f ms\n  * polycommit %.3f ms\n  * multiply_vec %.3f ms\n  * prove_sc_phase_one %.3f ms\n  * eval_table_sparse %.3f ms\n  * prove_sc_phase_two %.3f ms\n"
               "  * polyeval %.3f ms\n  * R1CSEvalProof: derefs commitment %.3f ms, product circuits %.3f ms, hash layer %.3f ms\n  * len_snark_proof %zu\n",
               t_prove, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], proof_len);
        fprintf(E.out, "* SNARK::verify %.3f ms\n", t_verify);
        origin_line(E, wit, inst, t_main0);
        int wrc = 0;
        if (proof_out && !rc) { FILE *f = fopen(at(E, proof_out).c_str(), "wb"); if (!f || fwrite(proof, 1, proof_len, f) != proof_len) { fprintf(E.err, "spzk: cannot write %s\n", proof_out); wrc = 1; } if (f) fclose(f); }
        if (!E.served) { otti_buf_free(proof); otti_buf_free(cb); otti_comp_comm_free(vc); otti_comp_comm_free(cc); otti_snark_gens_free(sg); otti_instance_free(inst); otti_r1cs_free(r); }   // served: `fr` does, and the generators are the cache's
        if (rc) { fprintf(E.out, "Verification FAILED (%d)\n", rc); return 1; }
        if (wrc) return 1;
        fprintf(E.out, "Verification successful\n");
        return 0;
    }
    otti_gens *gens = nullptr; rc = gens_rc_wait(); if (rc) return fail(E, "NIZKGens::new", rc);
    gens = gens_early;
    double t_objs = now_ms() - t0;
    if (!verify_only) { rc = E.gens->prepare(inst, gens); if (rc) return fail(E, "device setup", rc); }
    double t_setup = now_ms() - t0; t0 = now_ms();
    uint8_t *proof = nullptr; size_t proof_len = 0; double st[8] = {0}, t_prove = 0, t_verify = 0;
    if (verify_only) {
        FILE *f = fopen(at(E, proof_in).c_str(), "rb");
        if (!f) { fprintf(E.err, "spzk: cannot read %s\n", proof_in); return 1; }
        fseek(f, 0, SEEK_END); long len = ftell(f); fseek(f, 0, SEEK_SET);
        proof = (uint8_t *)malloc(len > 0 ? (size_t)len : 1); proof_len = len > 0 ? (size_t)len : 0;
        fr.add([=] { free(proof); });
        if (fread(proof, 1, proof_len, f) != proof_len) { fclose(f); fprintf(E.err, "spzk: short read on %s\n", proof_in); return 1; }
        fclose(f);
    } else {
        if (wit) rc = otti_nizk_prove_resident(inst, wit, gens, (const uint8_t *)label, strlen(label), seedp, &proof, &proof_len, st);
        else rc = otti_nizk_prove(inst, r->vars32, r->nvars, r->inputs32, r->ninputs, gens, (const uint8_t *)label, strlen(label), seedp, OTTI_FLAG_GPU, &proof,
                                  &proof_len, st);
        if (rc) return fail(E, "NIZK::prove", rc);
        fr.add([=] { otti_buf_free(proof); });
        t_prove = now_ms() - t0; t0 = now_ms();
    }
    if (!prove_only) {
        rc = otti_nizk_verify(inst, r->inputs32, r->ninputs, gens, (const uint8_t *)label, strlen(label), proof, proof_len);
        t_verify = now_ms() - t0;
    }
    uint64_t nc, nv, ni; otti_instance_dims(inst, &nc, &nv, &ni);
    fprintf(E.out, "* instance: %llu constraints (padded %llu), %llu variables (padded %llu), %llu inputs\n", (unsigned long long)r->num_cons, (unsigned long long)nc,
           (unsigned long long)r->num_vars, (unsigned long long)nv, (unsigned long long)ni);
    fprintf(E.out, "* zkif_load %.3f ms\n* setup (Instance::new, NIZKGens::new, device tables) %.3f ms\n  * host objects %.3f ms\n", t_load, t_setup, t_objs);
    if (!verify_only)
        fprintf(E.out, "* NIZK::prove %.3f ms\n  * polycommit %.3f ms\n  * multiply_vec %.3f ms\n  * prove_sc_phase_one %.3f ms\n  * eval_table_sparse %.3f ms\n"
               "  * prove_sc_phase_two %.3f ms\n  * polyeval %.3f ms\n  * len_r1cs_sat_proof %zu\n", t_prove, st[0], st[1], st[2], st[3], st[4], st[5], proof_len);
    if (!prove_only) fprintf(E.out, "* NIZK::verify %.3f ms\n", t_verify);
    int wrc = 0;
    if (proof_out && !rc) {
        FILE *f = fopen(at(E, proof_out).c_str(), "wb");
        if (!f || fwrite(proof, 1, proof_len, f) != proof_len) { fprintf(E.err, "spzk: cannot write %s\n", proof_out); wrc = 1; }
        if (f) fclose(f);
    }
    // (no frees: the process ends here and hands everything back at once — releasing the device tables one by one costs milliseconds)
    origin_line(E, wit, inst, t_main0);
    if (rc) { fprintf(E.out, "Verification FAILED (%d: %s)\n", rc, rc == OTTI_ERR_VERIFY_DECOMPRESS ? "DecompressionError" : rc == OTTI_ERR_VERIFY_INTERNAL ? "InternalError" : "malformed proof"); return 1; }
    if (wrc) return 1;
    if (prove_only) { fprintf(E.out, "Proof written to %s (%zu bytes)\n", proof_out, proof_len); return done(E, 0); }
    fprintf(E.out, "Verification successful\n");
    return done(E, 0);                                         // everything is printed and written
}
