// The field order of every wire object, each written once (wire.h): walk(codec, object) visits the fields in wire order, with a Writer over
// a const object or a Reader over one being filled.  serialize() and parse() of the three top-level objects are at the bottom.
#include "wire.h"
#include "snark.h"

namespace otti {
namespace wire {
namespace {

// a vector whose elements the walk visits itself: its count goes out, or comes in (bounded) and sizes the vector
template <class C, class V> void sized(C &c, V &v, size_t max) {
    const size_t k = c.len(v.size(), max);
    if constexpr (C::reading) v.resize(k);
}

template <class C, class T> void walk_sumcheck(C &c, T &s) {                     // ZKSumcheckProof, its proofs DotProductProof
    c.pts(s.comm_polys, kMaxRounds); c.pts(s.comm_evals, kMaxRounds);
    sized(c, s.proofs, kMaxRounds);
    for (auto &d : s.proofs) { c.pt(d.delta); c.pt(d.beta); c.frs(d.z, kMaxRoundScalars); c.fr(d.z_delta); c.fr(d.z_beta); }
}
// DotProductProofLog.  Whether L_vec and R_vec must be equally long is NOT decided here: the two parsers differ (SnarkProof::parse below)
template <class C, class T> void walk_dplog(C &c, T &d) {
    c.pts(d.L_vec, kMaxRounds); c.pts(d.R_vec, kMaxRounds); c.pt(d.delta); c.pt(d.beta); c.fr(d.z1); c.fr(d.z2);
}
template <class C, class T> void walk_r1cs(C &c, T &P) {                         // R1CSProof: NizkProof without rx, ry
    c.pts(P.comm_vars, kMaxVarRows); walk_sumcheck(c, P.sc1);
    for (auto &claim : P.claims_phase2) c.pt(claim);
    c.pt(P.pok.alpha); c.fr(P.pok.z1); c.fr(P.pok.z2);
    c.pt(P.prod.alpha); c.pt(P.prod.beta); c.pt(P.prod.delta); for (auto &z : P.prod.z) c.fr(z);
    c.pt(P.eq1.alpha); c.fr(P.eq1.z);
    walk_sumcheck(c, P.sc2);
    c.pt(P.comm_vars_at_ry);
    walk_dplog(c, P.polyeval);
    c.pt(P.eq2.alpha); c.fr(P.eq2.z);
}
template <class C, class T> void walk_nizk(C &c, T &P) { walk_r1cs(c, P); c.frs(P.rx, kMaxRounds); c.frs(P.ry, kMaxRounds); }

template <class C, class T> void walk_evals4(C &c, T &e) { c.fr(e.init); c.frs_fixed(e.read, 3); c.frs_fixed(e.write, 3); c.fr(e.audit); }
template <class C, class T> void walk_batch(C &c, T &p) {                        // ProductCircuitEvalProofBatched
    sized(c, p.layers, kMaxRounds);
    for (auto &L : p.layers) {
        const size_t rounds = c.len(L.coeffs.size() / 3, kMaxRounds);            // coeffs is flat: a CompressedUniPoly of three per round
        if constexpr (C::reading) L.coeffs.resize(3 * rounds);
        for (size_t j = 0; j < rounds; j++) c.frs_fixed(&L.coeffs[3 * j], 3);
        c.frs(L.left, kMaxRounds); c.frs(L.right, kMaxRounds);
        c.expect(L.left.size() == L.right.size(), "layer claims");
    }
    c.frs(p.dotp_left, kMaxRounds); c.frs(p.dotp_right, kMaxRounds); c.frs(p.dotp_weight, kMaxRounds);
    c.expect(p.dotp_left.size() == p.dotp_right.size() && p.dotp_left.size() == p.dotp_weight.size(), "dot-product claims");
}
template <class C, class T> void walk_evalproof(C &c, T &E) {                    // R1CSEvalProof
    c.pts(E.comm_derefs, kMaxCommRows);
    walk_evals4(c, E.eval_row); walk_evals4(c, E.eval_col); c.frs_fixed(E.dotp_left, 3); c.frs_fixed(E.dotp_right, 3);
    walk_batch(c, E.proof_mem); walk_batch(c, E.proof_ops);
    c.frs_fixed(E.h_row_addr, 3); c.frs_fixed(E.h_row_read_ts, 3); c.fr(E.h_row_audit);
    c.frs_fixed(E.h_col_addr, 3); c.frs_fixed(E.h_col_read_ts, 3); c.fr(E.h_col_audit);
    c.frs_fixed(E.h_val, 3); c.frs_fixed(E.h_deref_row, 3); c.frs_fixed(E.h_deref_col, 3);
    walk_dplog(c, E.pe_ops); walk_dplog(c, E.pe_mem); walk_dplog(c, E.pe_derefs);
}
template <class C, class T> void walk_snark(C &c, T &S) {
    walk_r1cs(c, S.r1cs);
    for (auto &e : S.inst_evals) c.fr(e);
    walk_evalproof(c, S.eval);
}
template <class C, class T> void walk_comm(C &c, T &m) {                         // ComputationCommitment
    c.u64(m.num_cons); c.u64(m.num_vars); c.u64(m.num_inputs); c.u64(m.batch_size); c.u64(m.num_ops); c.u64(m.num_mem_cells);
    c.pts(m.comm_ops, kMaxCommRows); c.pts(m.comm_mem, kMaxCommRows);
}

}  // namespace
}  // namespace wire

using namespace wire;

std::vector<uint8_t> NizkProof::serialize() const { Writer w; walk_nizk(w, *this); return std::move(w.b); }
NizkProof NizkProof::parse(const uint8_t *p, size_t n) {
    Reader r{p, n}; NizkProof P;
    walk_nizk(r, P);
    r.expect(r.at_end(), "trailing bytes after proof");
    return P;
}

std::vector<uint8_t> SnarkProof::serialize() const { Writer w; walk_snark(w, *this); return std::move(w.b); }
SnarkProof SnarkProof::parse(const uint8_t *p, size_t n) {
    Reader r{p, n}; SnarkProof S;
    walk_snark(r, S);
    // This parser alone refuses a log dot-product proof whose L_vec and R_vec differ in length.  NizkProof::parse lets such a polyeval
    // through, and the verifier then rejects it (dotproductlog_verify: OTTI_ERR_VERIFY_INTERNAL); callers see the two codes, so both stay.
    for (const DotProductProofLog *d : {&S.r1cs.polyeval, &S.eval.pe_ops, &S.eval.pe_mem, &S.eval.pe_derefs})
        r.expect(d->L_vec.size() == d->R_vec.size(), "bullet reduction vectors");
    r.expect(r.at_end(), "trailing bytes after proof");
    return S;
}

std::vector<uint8_t> CompComm::serialize() const { Writer w; walk_comm(w, *this); return std::move(w.b); }
std::unique_ptr<CompComm> CompComm::parse(const uint8_t *p, size_t n) {
    Reader r{p, n}; auto c = std::make_unique<CompComm>();
    walk_comm(r, *c);
    r.expect(r.at_end() && c->batch_size == 3, "malformed computation commitment");
    return c;
}

}  // namespace otti
