// Device mail: the three lines a kernel writes to pinned host memory with ONE store instruction and no fence, and the one host reader of
// them.  Every format is K 32-byte words followed by (number, tag); nothing orders the 64-byte halves of a line on their way, so a line is
// whole when its number is the awaited one and tag == f(number, words) — the same function on both sides of the bus.
#pragma once
#include "point.h"
#include "cpu_relax.h"
#include <cstddef>

namespace otti {

// every 64-bit word of the n values, rotated by its position, folded into the sequence number (also the tag of a GoBox, device.h)
HD unsigned long long go_tag(unsigned long long seq, const Fr *v, int n) {
    unsigned long long h = seq * 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < n; k++)
        for (int j = 0; j < 4; j++) {
            const unsigned long long w = (unsigned long long)v[k].v[2 * j] | ((unsigned long long)v[k].v[2 * j + 1] << 32);
            const int rot = ((4 * k + j) * 5 + 1) & 63;
            h ^= (w << rot) | (w >> ((64 - rot) & 63));
        }
    return h;
}
// ---- the round line.  The completion flag lives in result slot 3 — with slots 0..2 one 128-byte line.  A launch whose K <= 3 totals go to
// slot 0 mails that line with ONE store instruction and no fence (Mailbox.line_mail): number and tag travel in one 16-byte store; the low 32
// bits of the tag are the number's xor kLineMark, which tells the host that the line's first half is covered by the tag (a fenced mail leaves
// an older tag behind, whose number does not fit) and must be checked.
struct RoundLine { Fr s[3]; unsigned long long seq, tag, pad[2]; };             // h_results[0 .. 4) seen by the host; h_flag = &seq
constexpr unsigned long long kLineMark = 0x5a5a5a5aull;
HD unsigned long long line_tag(unsigned long long seq, const Fr *s3) { return (go_tag(seq, s3, 3) & ~0xffffffffull) | ((seq ^ kLineMark) & 0xffffffffull); }
// ---- the persistent tail's line (k_pc_tail, snark_dev.h): 128 bytes per workgroup, written by ONE store instruction (eight lanes x 16 bytes,
// system scope) and not followed by a fence: the three sums, then (number, tag).  A release fence per mail is what a round of 128-144
// workgroups waited for: all mails in after 8.3 us with "96 bytes, __threadfence_system, number", 3.35 us with the whole line in one
// instruction (tools/pollprobe.hip, profiles/r4_pollprobe_mail.txt).  tag = go_tag(seq, s, 3).
// (Partial stores without a fence are no alternative: seven 16-byte stores nobody waited for reached the host 13 us later.)
struct TailMail { Fr s[3]; unsigned long long seq, tag, pad[2]; };
static_assert(sizeof(TailMail) == 128 && sizeof(RoundLine) == 128 && offsetof(RoundLine, seq) == 96, "one mail = one 128-byte line");
// ---- small fixed-base MSMs whose row sums go to the host (k_msm_small, rows <= 2): every workgroup mails its chunk's sum, in cached form
// (Y - X, Y + X, 2d T, 2 Z), to a line pair of its own, written by ONE store instruction (nine lanes x 16 bytes) with no fence; the host adds
// the chunk sums of a row as they arrive (DevCtx::wait_points).  tag = go_tag(seq, v, 4): a pair that is not whole yet, or is left over
// from an earlier launch, does not fit.
struct MsmMail { Fp v[4]; unsigned long long seq, tag, pad[14]; };
static_assert(sizeof(MsmMail) == 256 && offsetof(MsmMail, seq) == 128, "one mail = the cached point in one line, (number, tag) at the start of the next");
HD unsigned long long msm_mail_tag(unsigned long long seq, const Fp *v4) { return go_tag(seq, reinterpret_cast<const Fr *>(v4), 4); }

// what the reader needs to know of a format.  kPassedIsDone: the line is reused by the next launch, so a reader that finds ANOTHER number
// than the one it came for stops (its launch has delivered and been overwritten); the other two are read before their slot is reused.
struct RoundLineFmt { using Line = RoundLine; using Word = Fr; static constexpr int kWords = 3; static constexpr bool kPassedIsDone = true;
                      static HD const Fr *words(const Line *l) { return l->s; } static HD unsigned long long tag(unsigned long long q, const Fr *w) { return line_tag(q, w); } };
struct TailMailFmt { using Line = TailMail; using Word = Fr; static constexpr int kWords = 3; static constexpr bool kPassedIsDone = false;
                     static HD const Fr *words(const Line *l) { return l->s; } static HD unsigned long long tag(unsigned long long q, const Fr *w) { return go_tag(q, w, 3); } };
struct MsmMailFmt { using Line = MsmMail; using Word = Fp; static constexpr int kWords = 4; static constexpr bool kPassedIsDone = false;
                    static HD const Fp *words(const Line *l) { return l->v; } static HD unsigned long long tag(unsigned long long q, const Fp *w) { return msm_mail_tag(q, w); } };
// one look at a line (host): its words copied to out, and whether they are those of mail `want`
enum class MailState { whole, torn, other_number };
template <class F> __attribute__((always_inline)) inline MailState mail_try(const typename F::Line *line, unsigned long long want, typename F::Word *out) {
    const unsigned long long s = __atomic_load_n(&line->seq, __ATOMIC_ACQUIRE), tag = __atomic_load_n(&line->tag, __ATOMIC_ACQUIRE);
    if (s != want) return MailState::other_number;
    for (int k = 0; k < F::kWords; k++) out[k] = F::words(line)[k];
    return F::tag(s, out) == tag ? MailState::whole : MailState::torn;
}
// read, check the tag, read again until it fits (normally at once).  False after more than max_spins further looks (0: no limit).
template <class F> __attribute__((always_inline)) inline bool mail_wait(const typename F::Line *line, unsigned long long want, unsigned max_spins, typename F::Word *out) {
    for (unsigned spins = 0;; spins++) {
        const MailState st = mail_try<F>(line, want, out);
        if (st == MailState::whole || (F::kPassedIsDone && st == MailState::other_number)) return true;
        if (max_spins && spins > max_spins) return false;
        cpu_relax();
    }
}

}  // namespace otti
