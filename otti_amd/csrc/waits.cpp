// Host waits on device mail: the prover thread's spins on pinned memory (a round's flag, the persistent tail's lines, the small MSMs' chunk
// mails), each ending in "the mail is whole" or a clean failure, and the host sums built on them.  The formats and their one reader are in
// mail.h; the one guarded spin is DevCtx::spin_until below.  Allocation of the mailboxes and the armed-launch bookkeeping: k_context.hip.
#include "device.h"
#include "snark_dev.h"
#include "hostifma.h"
#include "pool.h"
#include <stdlib.h>

namespace otti {

using Clock = std::chrono::steady_clock;
// Everything the three guarded waits differ in, with today's values; a difference not marked deliberate is inherited and kept as found.
// One more difference is not a field: what fail() throws — Error, but TailTimeout from the tail's wait (deliberate: SNARK::prove catches
// that type, switches the tail off and proves again with a launch per round).
struct WaitLimits {
    unsigned go_mask, clock_mask;  // h_go->timed_out is read when (spins & go_mask) == go_mask, the clock when (spins & clock_mask) == clock_mask.
                                   // Deliberate: a spin of the MSM wait is up to 1000 looks at a mail, one of the other two a single load
    Clock::duration timeout;       // deliberate: 20 s is below the armed launches' own 30 s (kArmDeadlineTicks); the tail's is short (OTTI_TAIL_TIMEOUT_MS,
                                   // 5 s) because its caller has another way to prove
    bool drain_checked;            // at the limit with nothing armed: a failing stream drain throws its HIP error (surfaces a device fault), else it
                                   // is ignored.  Inherited; as it is, the tail's wait throws nothing but TailTimeout at its limit
    bool recheck;                  // the condition is looked at once more after release-or-drain and the wait returns if it holds.  Inherited
    bool reset_counters;           // reset_arrival_counters() follows the drain.  Inherited (the MSM wait's drain leaves the counters as they are)
    const char *gave_up;           // message when an armed launch gave up waiting for this thread (the tail names itself)
};
static const char kGaveUp[] = "an armed launch gave up waiting for the host (the proving thread was stalled beyond the launch's deadline)";
static const WaitLimits kRoundWait = {0x3ff, 0xffff, std::chrono::seconds(20), true, true, true, kGaveUp};
static const WaitLimits kMsmWait = {0x3f, 0x3ff, std::chrono::seconds(20), true, true, false, kGaveUp};
static const WaitLimits &tail_wait() {
    static const WaitLimits w = [] {
        const char *e = getenv("OTTI_TAIL_TIMEOUT_MS"); const long x = e ? atol(e) : 0;
        return WaitLimits{0x3ff, 0xffff, std::chrono::milliseconds(x > 0 ? x : 5000L), false, false, true,
                          "the persistent sum-check launch gave up waiting for the host (the proving thread was stalled beyond the launch's deadline)"};
    }();
    return w;
}
template <class Pred, class OnLimit> void DevCtx::spin_until(Pred arrived, const WaitLimits &lim, Clock::time_point t0, OnLimit fail) {
    for (unsigned spins = 0;; spins++) {
        if (arrived()) return;
        cpu_relax();
        if ((spins & lim.go_mask) == lim.go_mask && __atomic_load_n(&h_go->timed_out, __ATOMIC_ACQUIRE)) {
            // an armed launch gave up waiting for this thread (it was stopped for longer than the launch's deadline): its grid returned
            // without touching anything, the launches queued behind it are released the same way, and the proof fails cleanly
            go_abort();
            throw Error(OTTI_ERR_INTERNAL, lim.gave_up);
        }
        if ((spins & lim.clock_mask) == lim.clock_mask && Clock::now() - t0 > lim.timeout) {
            if (go_published < go_issued) go_abort();         // release whatever is still armed, drain, clear the arrival counters
            else {
                if (lim.drain_checked) OTTI_HIP(hipStreamSynchronize(stream)); else (void)hipStreamSynchronize(stream);
                if (lim.recheck && arrived()) return;
                if (lim.reset_counters) reset_arrival_counters();
            }
            if (lim.recheck && arrived()) return;
            fail();
        }
    }
}
void DevCtx::wait_ticket(unsigned long long ticket) {
    volatile unsigned long long *f = h_flag;
    spin_until([&] { return *f >= ticket; }, kRoundWait, Clock::now(), [] { throw Error(OTTI_ERR_INTERNAL, "sum-check round result never arrived"); });
    // a line mail (mail.h kLineMark): number and tag came in one 16-byte store, the sums' first half possibly not yet — read until the tag fits
    Fr s3[3];
    if (*f == ticket && ((f[1] ^ ticket ^ kLineMark) & 0xffffffffull) == 0 && !mail_wait<RoundLineFmt>(reinterpret_cast<const RoundLine *>(h_results), ticket, 50000000u, s3))
        throw Error(OTTI_ERR_INTERNAL, "a round's mailed line never became whole");
}
void DevCtx::wait_tail(int n_groups, unsigned long long want) {
    const TailMail *h_tail = tail_mail.host;
    int done = 0;                                             // lines [0, done) have arrived
    // a round of the persistent launch takes tens of microseconds; seconds without every line in mean that part of its grid is not
    // resident (the workgroups that are wait for the host, the host for all of them): give the launch up — the caller proves again without it
    spin_until([&] { while (done < n_groups && __atomic_load_n(&h_tail[done].seq, __ATOMIC_ACQUIRE) >= want) done++; return done == n_groups; }, tail_wait(), Clock::now(),
               [] { throw TailTimeout(OTTI_ERR_INTERNAL, "sum-check round result never arrived (persistent launch: its grid was not resident as a whole)"); });
}
static inline void prefetch_line(const void *p, int second_half) {
#if defined(__x86_64__)
    _mm_prefetch((const char *)p, _MM_HINT_T0); _mm_prefetch((const char *)p + second_half, _MM_HINT_T0);
#endif
}
// lines [i0, i1) of a round's mails: wait for each (bounded when `bounded`: a helper thread must not throw) and add the W partials of every
// instance up (lines a few ahead are prefetched: each is a fresh cache line the device has just written, and 144 dependent misses in a row
// would cost more than the round's arithmetic)
static bool tail_sum_range(const TailMail *h_tail, int i0, int i1, int W, unsigned long long want, Fr *sums, bool bounded) {
    for (int i = i0; i < i1 && i < i0 + 16; i++) prefetch_line(&h_tail[i], 64);
    for (int i = i0; i < i1; i++) {
        if (i + 16 < i1) prefetch_line(&h_tail[i + 16], 64);
        if (bounded) {
            unsigned spins = 0;
            while (__atomic_load_n(&h_tail[i].seq, __ATOMIC_ACQUIRE) < want) {
                if (++spins > 2000000u) return false;             // ~ a millisecond or more: the calling thread takes the slow path with its failure handling
                cpu_relax();
            }
        }
        Fr part[3];
        if (!mail_wait<TailMailFmt>(&h_tail[i], want, 4000000u, part)) { if (bounded) return false; throw Error(OTTI_ERR_INTERNAL, "a sum-check round's mail never became whole"); }
        Fr *acc = sums + 3 * (i / W);
        if (i % W == 0) { acc[0] = part[0]; acc[1] = part[1]; acc[2] = part[2]; }
        else { acc[0] = fr_add(acc[0], part[0]); acc[1] = fr_add(acc[1], part[1]); acc[2] = fr_add(acc[2], part[2]); }
    }
    return true;
}
void DevCtx::wait_tail_sums(int n_inst, int W, unsigned long long want, Fr *sums /* [n_inst][3] */) {
    const int n = n_inst * W;
    const TailMail *h_tail = tail_mail.host;
    // 128-144 lines of 3 partial sums: adding them up on one core cost 2.6 us of every round (profiles/r3_tail_stamps.txt); the instances are
    // independent, so the prover thread's helpers (pool.h: pinned next to it, ~55 ns hand-over) take a share each
    SpinPool &pool = SpinPool::get();
    const int nt = (n >= 48 && n_inst >= 2) ? std::min(std::min(4, pool.workers() + 1), n_inst) : 1;
    if (nt > 1) {
        bool ok[4] = {true, true, true, true};
        std::function<void()> tasks[4];
        for (int t = 0; t < nt; t++) {
            const int y0 = n_inst * t / nt, y1 = n_inst * (t + 1) / nt;
            tasks[t] = [h_tail, t, y0, y1, W, want, sums, &ok] { ok[t] = tail_sum_range(h_tail, y0 * W, y1 * W, W, want, sums, true); };
        }
        pool.parallel(tasks, nt);
        if (ok[0] && ok[1] && ok[2] && ok[3]) return;
    }
    wait_tail(n, want);                                       // (throws if the launch gave up or never answers)
    tail_sum_range(h_tail, 0, n, W, want, sums, false);
}
// ---- the small MSMs' chunk mails (mail.h MsmMail), summed on the host
void MsmMailbox::queue(unsigned long long seq, uint32_t rows, uint32_t nchunks) {
    if (pending_n == kMsmMailRegions) {                      // the launch just queued mails over the oldest entry's region: that one can no longer be read
        for (int i = 1; i < kMsmMailRegions; i++) pending[i - 1] = pending[i];
        pending_n--;
    }
    MsmPending &p = pending[pending_n++];
    p.seq = seq; p.order = ++order; p.region = (int)(launches++ % kMsmMailRegions); p.rows = rows; p.nchunks = nchunks;
}
bool msm_mails_whole(const MsmMail *m, int n, unsigned long long want) {   // (an idle stream: what has not come will not)
    Fp v[4];
    for (int i = 0; i < n; i++) if (mail_try<MsmMailFmt>(m + i, want, v) != MailState::whole) return false;
    return true;
}
bool msm_mail_sum(const MsmMail *m, int i0, int i1, unsigned long long want, PtFe &acc, unsigned max_spins, bool allow_ifma) {
    bool ok = true;
    Fp v[4];
    auto next = [&](int k) -> const Fp * {
        const MsmMail *line = m + i0 + k;
        if (i0 + k + 4 < i1) prefetch_line(line + 4, 128);
        if (!mail_wait<MsmMailFmt>(line, want, max_spins, v)) { ok = false; return nullptr; }
        return v;
    };
    host_sum_cached(acc, i1 - i0, next, allow_ifma);
    return ok;
}
// Every mail of the launch, summed per row.  A row's chunks are split between the prover thread and its helpers (pool.h: pinned next to
// it), rows side by side; a helper spins a bounded time only — if one gives up, this thread waits for the launch mail by mail under
// spin_until (an armed launch that gave up, a deadline for the launch as a whole) and sums everything itself.
void DevCtx::msm_host_sum(const MsmPending &p) {
    const MsmMail *m = msm_mail.region(p.region);
    const int rows = (int)p.rows, nch = (int)p.nchunks;
    SpinPool &pool = SpinPool::get();
    // >= 8 mails per thread (a hand-over costs ~50 ns, an addition ~60), at most kMaxSumThreads threads whatever OTTI_HOST_THREADS gives the pool
    constexpr int kMaxSumThreads = 8;
    const int per_row = std::max(1, std::min(std::min((pool.workers() + 1) / rows, nch / 8), kMaxSumThreads / rows));
    const int nt = rows * per_row;
    PtFe part[kMaxSumThreads];
    bool ok[kMaxSumThreads];
    if (nt > 1 && nt <= kMaxSumThreads) {
        std::function<void()> tasks[kMaxSumThreads];
        for (int t = 0; t < nt; t++) {
            const int r = t / per_row, k = t % per_row, i0 = r * nch + nch * k / per_row, i1 = r * nch + nch * (k + 1) / per_row;
            tasks[t] = [m, i0, i1, &p, &part, &ok, t] { part[t] = ptfe_identity(); ok[t] = msm_mail_sum(m, i0, i1, p.seq, part[t], 2000000u, true); };
        }
        pool.parallel(tasks, nt);
        bool all = true;
        for (int t = 0; t < nt; t++) all = all && ok[t];
        if (all) {
            for (int r = 0; r < rows; r++) {
                PtFe acc = part[r * per_row];
                for (int k = 1; k < per_row; k++) host_point_add(acc, part[r * per_row + k]);
                h_pts[r] = ptfe_to(acc);
            }
            return;
        }
    }
    const auto t0 = Clock::now();
    for (int r = 0; r < rows; r++) {
        PtFe acc = ptfe_identity();
        for (int i = r * nch; i < (r + 1) * nch; i++) {
            PtFe one;
            spin_until([&] { one = ptfe_identity(); return msm_mail_sum(m, i, i + 1, p.seq, one, 1000u, true); }, kMsmWait, t0,
                       [] { throw Error(OTTI_ERR_INTERNAL, "a small MSM's chunk sums never arrived"); });
            host_point_add(acc, one);
        }
        h_pts[r] = ptfe_to(acc);
    }
}
void DevCtx::wait_points(const MsmTicket &t) {
    if (!t.delivers_without_sync()) { sync(); return; }      // kept, raw, encoded on the device, or in h_pts for the host to encode: all behind the stream
    if (t.route == MsmRoute::mail) {
        MsmMailbox &mb = msm_mail;
        int i = 0;
        while (i < mb.pending_n && mb.pending[i].seq != t.seq) i++;
        if (i == mb.pending_n) {
            // the ticket's sums were read already — then this returns at once, as a flag wait on a delivered launch does — or they are
            // gone, and nothing will ever raise a flag for them
            for (unsigned long long r : mb.read) if (r == t.seq) return;
            throw Error(OTTI_ERR_INTERNAL, "a small MSM's chunk sums were overwritten or released before they were read");
        }
        const MsmPending p = mb.pending[i];
        for (int j = i + 1; j < mb.pending_n; j++) mb.pending[j - 1] = mb.pending[j];
        mb.pending_n--;
        msm_host_sum(p);
        mb.read[mb.read_next++ & 7] = t.seq;
    } else wait_ticket(t.seq);
    // the ticket's own rows: a launch queued ahead of this wait (an armed bullet round) has set the count for itself since
    pending_host_encode = t.rows;
    encode_pending();
}
void DevCtx::sync() {
    OTTI_HIP(hipStreamSynchronize(stream));
    MsmMailbox &mb = msm_mail;
    if (mb.pending_n) {
        // the stream is idle: the latest launch's mails are all in (unless it was an armed launch released without running: then nothing is);
        // its row sums are what h_pts holds after a sync, unless a later launch of another kind left its own there
        const MsmPending p = mb.pending[mb.pending_n - 1];
        mb.pending_n = 0;
        if (p.order > mb.h_pts_order && msm_mails_whole(mb.region(p.region), (int)(p.rows * p.nchunks), p.seq)) {
            msm_host_sum(p);
            mb.read[mb.read_next++ & 7] = p.seq;
            pending_host_encode = p.rows;
        }
    }
    encode_pending();
}
void DevCtx::encode_pending() {
    if (pending_host_encode >= 2) {
        SpinPool &pool = SpinPool::get(); const int nt = std::min<int>(pool.workers() + 1, (int)pending_host_encode);
        const size_t n = pending_host_encode;
        std::vector<std::function<void()>> tasks(nt);
        for (int t = 0; t < nt; t++) tasks[t] = [this, t, nt, n] { for (size_t i = t; i < n; i += nt) pt_encode(h_points + 32 * i, h_pts[i]); };
        pool.parallel(tasks.data(), nt);
    } else if (pending_host_encode == 1) pt_encode(h_points, h_pts[0]);
    pending_host_encode = 0;
}

}  // namespace otti
