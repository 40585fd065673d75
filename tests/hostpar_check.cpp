// fan_out (otti_amd/csrc/hostpar.h) on its own: own main, nothing linked beside it, built by tests/test_hostpar_host.py under
// -fsanitize=address,undefined and under -fsanitize=thread, each once as it is and once with -DOTTI_HOSTPAR_TEST_FAIL_AT=k: the start of share k's
// thread then throws std::system_error as a refused pthread_create (EAGAIN) makes std::thread's constructor throw.  Either way fan_out(nt, f)
// calls f with every share of 0 .. nt - 1 exactly once and returns normally; with the failure the shares from k on run on the caller's thread.
#include "../otti_amd/csrc/hostpar.h"
#include <stdio.h>
#include <atomic>
#include <thread>
#include <vector>

int main() {
    int bad = 0;
    for (unsigned nt : {1u, 2u, 16u, 64u}) {
        std::vector<std::atomic<int>> calls(nt);
        std::vector<int> on_caller(nt, 0);                   // each share writes its own slot: the join is what makes them readable here
        for (auto &c : calls) c.store(0);
        const std::thread::id me = std::this_thread::get_id();
        otti::fan_out(nt, [&](unsigned t) { calls[t].fetch_add(1); on_caller[t] = std::this_thread::get_id() == me; });
        for (unsigned t = 0; t < nt; t++) {
            if (calls[t].load() != 1) { bad++; printf("nt %u: share %u called %d times\n", nt, t, calls[t].load()); }
            bool want_caller = t == 0;
#ifdef OTTI_HOSTPAR_TEST_FAIL_AT
            want_caller = want_caller || t >= (OTTI_HOSTPAR_TEST_FAIL_AT);
#endif
            if ((bool)on_caller[t] != want_caller) { bad++; printf("nt %u: share %u ran on %s thread\n", nt, t, on_caller[t] ? "the caller's" : "another"); }
        }
    }
#ifdef OTTI_HOSTPAR_TEST_FAIL_AT
    printf("hostpar_check: thread start %d fails, nt 1 2 16 64, %d failures\n", (int)(OTTI_HOSTPAR_TEST_FAIL_AT), bad);
#else
    printf("hostpar_check: nt 1 2 16 64, %d failures\n", bad);
#endif
    return bad ? 4 : 0;
}
