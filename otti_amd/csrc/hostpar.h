// Fork-join over the host cores for work whose lifetime is one call: shares 1 .. nt - 1 on threads of their own, share 0 on the caller,
// all joined before the call returns.  The caller chooses nt (its own cut-over and cap) and how a share maps to its data.
#pragma once
#include <system_error>
#include <thread>
#include <vector>

namespace otti {

// run f(0 .. nt) on nt threads (the caller's included).  A thread that cannot be started (EAGAIN under a pids cgroup or
// RLIMIT_NPROC) must not unwind through joinable std::threads (std::terminate): the shares that found no thread run here instead.
// f must not throw on a thread it was given.
template <class F> void fan_out(unsigned nt, F &&f) {
    std::vector<std::thread> th; th.reserve(nt);
    unsigned started = 1;
    for (; started < nt; started++) {
        try {
#ifdef OTTI_HOSTPAR_TEST_FAIL_AT                             // tests/hostpar_check.cpp: the start of this share's thread fails as EAGAIN makes it
            if (started == (OTTI_HOSTPAR_TEST_FAIL_AT)) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
#endif
            th.emplace_back(f, started);
        } catch (const std::system_error &) { break; }
    }
    f(0u);
    for (unsigned t = started; t < nt; t++) f(t);
    for (auto &x : th) x.join();
}

}  // namespace otti
