"""Every field of a proof tampered once, on the verifier routes that use the device, verdicts held to the oracle by the rule of
test_proof_fields_host.py (proof_fields.verdict_error).  The proofs come from the product's prover in this process — each test first asserts that
they are byte-identical to the oracle's for the same seed —, so the generator tables are resident and the verifier's fixed-base hook is live.

    NIZK 2^12   the smallest size at which instance_evaluate is queued on the device, fed rx and ry straight from the proof bytes: one mutant per
                field; the singles against the oracle, the list through verify_many (default threads and one), the singles on the host route
    NIZK 2^16   the smallest size with 256 row commitments, where RowSum goes to the device: the steering corpus, whose comm_vars substitutes are the
                point — a valid but wrong row must be rejected, the identity and an undecodable row must give what the host route gives
    SNARK 2^14  uniform; all three row sums have at least 256 points: steering over the proof and over the commitment; the list through
                snark_verify_many in chunks of four; a commitment with one wrong (valid) row in comm_ops and one in comm_mem, and a fresh handle after it
    SNARK 2^12  compiler-like; comm_mem stays on the host while the other two sums go to the device: steering through snark_verify_many only

Which route ran is read from the kernel launch counters of the calling thread's stream (spmv: the evaluation; decode and msm_var: a row sum).

Measured on the MI355X host (every test prints its mutant count and seconds), the whole file in 9.4 s:
    NIZK 2^12   398 mutants: proofs 0.3 s, oracle 0.2 s, singles 0.6 s, verify_many 0.4 s (default threads) and 0.6 s (one), host route 0.6 s
    NIZK 2^16   103 mutants: proofs 0.6 s, oracle 0.3 s, singles 0.1 s, host route 0.2 s; the test 1.2 s
    SNARK 2^14  180 + 30 mutants: commitment and proofs 1.4 s, oracle 0.2 s, singles 0.4 s, snark_verify_many 0.2 s, the wrong-rows commitment 0.1 s
    SNARK 2^12  180 mutants: commitment and proofs 1.9 s, singles 0.3 s, snark_verify_many 0.2 s; the test 2.5 s
(the oracle rejects most mutants at the first failed equation; the product walks on and reports at the end, so its share is the larger one)"""
import time

import pytest

import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc

pytestmark = pytest.mark.gpu
SEED2 = bytes([0x5f]) * 32


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


@pytest.fixture(scope="module", autouse=True)
def narrow_tables():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OTTI_MSM_WINDOW", "10")                     # narrow generator tables: tens of MB, built in milliseconds
        yield


def _nizk_run(n, pick, what):
    t0 = time.time()
    case = pc.NizkCase(oa.synth_r1cs(n, 10, 1))
    proof = case.device_proof()
    assert proof == case.oracle_proof(), "the device proof differs from the oracle's for the same seed"
    print("%s: proofs made and compared in %.1f s" % (what, time.time() - t0))
    return pc.Run(case, proof, pick(proof, pf.nizk(proof)), what, skip_percent=None if pick is pf.steering else 1)


def _snark_run(r, what, seeds=(pc.SEED,)):
    t0 = time.time()
    case = pc.SnarkCase(r)
    proofs = case.device_proofs(seeds)
    assert proofs[0] == case.oracle_proof(), "the device proof differs from the oracle's for the same seed"
    print("%s: commitment and proofs made and compared in %.1f s" % (what, time.time() - t0))
    return case, proofs


def _launches(call):
    """(what call() returns, {kernel class: launches} on the calling thread's stream while it ran): which route a verifier took"""
    oa.stats_enable(True)
    try:
        out = call()
        st = oa.stats_read()
    finally:
        oa.stats_enable(False)
    return out, {k: v[0] for k, v in st.items() if v[0]}


def _mutant(corpus, name, what):
    return next(m for n, w, m in corpus.mutants if (n, w) == (name, what))


def _no_differences(corpus, want, got):
    bad = pf.differences(corpus, want, got)
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ NIZK, 2^12: the queued instance_evaluate
@pytest.fixture(scope="module")
def nizk_4096():
    return _nizk_run(1 << 12, pf.one_per_field, "NIZK 2^12, one mutant per field")


def test_nizk_4096_singles_against_the_oracle(nizk_4096):
    run = nizk_4096
    assert run.case.inst.dims[0] >= 4096                                                  # the evaluation is queued on the device
    assert len(run.corpus) >= 300 and run.corpus.check_skips() == 0
    for blob, want_ok in ((run.proof, True), (_mutant(run.corpus, "rx[0]", "plus_one"), False), (_mutant(run.corpus, "ry[3]", "plus_one"), False)):
        code, ran = _launches(lambda: run.case.product(blob))
        assert (code == 0) == want_ok and ran.get("spmv", 0) >= 1 and "msm_var" not in ran, (code, ran)   # evaluated on the device at the PROOF's point; 64 rows: host sum
    bad = run.failures()
    assert not bad, "%d of %d mutants:\n%s" % (len(bad), len(run.corpus), "\n".join(bad[:40]))


@pytest.mark.parametrize("threads", [0, 1])
def test_nizk_4096_verify_many_gives_the_single_codes(nizk_4096, threads):
    """the whole list in one call: the batched device evaluation takes every parsed mutant's rx and ry"""
    blobs, _ = nizk_4096.with_good()
    t0 = time.time()
    got = nizk_4096.case.product_many(blobs, threads)
    print("verify_many, threads=%d: %d items in %.1f s" % (threads, len(blobs), time.time() - t0))
    bad = nizk_4096.many_differences(got)
    assert not bad, "\n".join(bad[:40])


def test_nizk_4096_host_route_gives_the_same_codes(nizk_4096, monkeypatch):
    monkeypatch.setenv("OTTI_VERIFY_HOST", "1")
    t0 = time.time()
    got = pc.codes(nizk_4096.case.product, nizk_4096.corpus)
    print("OTTI_VERIFY_HOST=1: %d mutants in %.1f s" % (len(got), time.time() - t0))
    _no_differences(nizk_4096.corpus, nizk_4096.product, got)
    assert nizk_4096.case.product(nizk_4096.proof) == 0


# ------------------------------------------------------------------------------------------------ NIZK, 2^16: the device row sum
def test_nizk_65536_row_commitments_on_the_device(monkeypatch):
    run = _nizk_run(1 << 16, pf.steering, "NIZK 2^16, steering")
    proof, fields = run.proof, pf.nizk(run.proof)
    assert pf.value(proof, fields, "comm_vars.len") == 256                                # RowSum's device threshold is met
    names = {(name, what) for name, what, _ in run.corpus.mutants}
    for i in (0, 1, 128, 255):
        for what in pf.SUBSTITUTES["pt"]:
            assert ("comm_vars[%d]" % i, what) in names
    bad = run.failures()
    assert not bad, "%d of %d mutants:\n%s" % (len(bad), len(run.corpus), "\n".join(bad[:40]))
    probes = [(run.proof, True)] + [(_mutant(run.corpus, "comm_vars[%d]" % i, what), False) for i, what in ((1, "other_point"), (128, "identity"), (255, "undecodable"))]
    for blob, want_ok in probes:                                                          # the 256 rows are decoded and summed on the device
        code, ran = _launches(lambda: run.case.product(blob))
        assert (code == 0) == want_ok and ran.get("decode", 0) >= 1 and (ran.get("msm_var", 0) >= 1 or not want_ok), (code, ran)
    monkeypatch.setenv("OTTI_VERIFY_HOST", "1")
    code, ran = _launches(lambda: run.case.product(run.proof))
    assert code == 0 and "msm_var" not in ran and "decode" not in ran, (code, ran)        # and on the host under the switch
    t0 = time.time()
    got = pc.codes(run.case.product, run.corpus)
    print("OTTI_VERIFY_HOST=1: %d mutants in %.1f s" % (len(got), time.time() - t0))
    _no_differences(run.corpus, run.product, got)


# ------------------------------------------------------------------------------------------------ SNARK, 2^14 uniform: three device row sums
@pytest.fixture(scope="module")
def snark_16384():
    case, proofs = _snark_run(oa.synth_r1cs(1 << 14, 10, 1), "SNARK 2^14 uniform", (pc.SEED, SEED2))
    proof, cfields = proofs[0], pf.commitment(case.comm_bytes)
    rows = (pf.value(proof, pf.snark(proof), "comm_derefs.len"), pf.value(case.comm_bytes, cfields, "comm_ops.len"), pf.value(case.comm_bytes, cfields, "comm_mem.len"))
    assert min(rows) >= 256, rows
    return pc.Run(case, proof, pf.steering(proof, pf.snark(proof)), "SNARK 2^14 uniform, steering", skip_percent=None), proofs


def test_snark_16384_singles_against_the_oracle(snark_16384):
    run, _ = snark_16384
    bad = run.failures()
    assert not bad, "%d of %d mutants:\n%s" % (len(bad), len(run.corpus), "\n".join(bad[:40]))
    code, ran = _launches(lambda: run.case.product(run.proof))
    assert code == 0 and ran.get("msm_var", 0) >= 3 and ran.get("decode", 0) >= 3, (code, ran)   # comm_derefs, comm_ops and comm_mem are summed on the device


def test_snark_16384_commitment_fields_against_the_oracle(snark_16384):
    """steering over the commitment's bytes, re-parsed on both sides: a changed count is refused at parse by both, a changed dimension is refused
    or makes both reject the good proof, a substituted row follows the rule for points"""
    run, _ = snark_16384
    case, proof = run.case, run.proof
    corpus = pf.steering(case.comm_bytes, pf.commitment(case.comm_bytes))
    # the last row of either vector is padding: a commitment to a zero row, the identity already, so its identity substitute changes nothing
    assert corpus.check_skips(None) <= 2 and len(corpus) + len(corpus.skipped) == 2 * 4 * 3 + 8
    t0 = time.time(); bad = []
    for name, what, blob in corpus.mutants:
        oc, comm = case.parse_both(blob)
        o = None if oc is None else case.oracle(proof, comm=oc)
        p = None if comm is None else case.product(proof, comm=comm)
        if what in pf.SUBSTITUTES["pt"]:
            err = "refused at parse" if o is None or p is None else pf.verdict_error(what, o, p)
        elif name.endswith(".len"):
            err = None if (o, p) == (None, None) else "a changed count must be refused at parse"
        else:
            err = "ACCEPTED" if o == 0 or p == 0 else None
        if err:
            bad.append("%s / %s: %s (oracle %s, product %s)" % (name, what, err, o, p))
    print("commitment steering: %d mutants in %.1f s" % (len(corpus), time.time() - t0))
    assert not bad, "\n".join(bad)


def test_snark_16384_verify_many_gives_the_single_codes(snark_16384, monkeypatch):
    run, _ = snark_16384
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    order = pc.interleaved(len(run.corpus))
    blobs, _ = run.with_good(order)
    t0 = time.time()
    got, ran = _launches(lambda: run.case.product_many(blobs))
    print("snark_verify_many, chunk 4: %d items in %.1f s" % (len(blobs), time.time() - t0), ran)
    assert ran.get("msm_var", 0) >= 3, ran                                                # the batched device passes ran (on the calling thread's stream)
    bad = run.many_differences(got, order)
    assert not bad, "\n".join(bad[:40])


def test_snark_16384_a_commitment_with_valid_but_wrong_rows(snark_16384, monkeypatch):
    """one other_point row in comm_ops and one in comm_mem: both decode, the sums are wrong (and the transcript is another).  Every good proof gets
    the single verifier's code, which is the oracle's; a fresh handle from the original bytes accepts afterwards: what one handle cached of its rows
    stays with that handle"""
    run, proofs = snark_16384
    case = run.case
    cfields = pf.commitment(case.comm_bytes)
    n_ops, n_mem = pf.value(case.comm_bytes, cfields, "comm_ops.len"), pf.value(case.comm_bytes, cfields, "comm_mem.len")
    bad_bytes = case.comm_bytes
    for name in ("comm_ops[%d]" % (n_ops // 2), "comm_mem[%d]" % (n_mem // 3)):
        field = next(f for f in cfields if f[0] == name)
        bad_bytes = pf.substitute(bad_bytes, cfields, field, "other_point")
    assert sum(1 for a, b in zip(bad_bytes, case.comm_bytes) if a != b) > 2 and len(bad_bytes) == len(case.comm_bytes)
    oc, bad_comm = case.parse_both(bad_bytes)
    assert oc is not None and bad_comm is not None
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    singles = [case.product(p, comm=bad_comm) for p in proofs]
    assert all(c != 0 for c in singles) and singles == [case.oracle(p, comm=oc) for p in proofs]
    assert case.product_many(proofs * 3, comm=bad_comm) == singles * 3                    # six items: a chunk of four and one of two
    assert case.product_many(proofs * 3, threads=1, comm=bad_comm) == singles * 3
    fresh = oa.ComputationCommitment.from_bytes(case.comm_bytes)
    assert case.product_many(proofs * 3, comm=fresh) == [0] * 6
    assert [case.product(p, comm=fresh) for p in proofs] == [0, 0]
    assert case.product_many(proofs, comm=bad_comm) == singles                            # and the wrong rows stay wrong on their handle


# ------------------------------------------------------------------------------------------------ SNARK, 2^12 compiler-like: host and device sums in one call
def test_snark_4096_compiler_like_verify_many_gives_the_single_codes(monkeypatch):
    case, proofs = _snark_run(oa.synth_r1cs_compiler_like(1 << 12, 10, 5), "SNARK 2^12 compiler-like")
    proof, cfields = proofs[0], pf.commitment(case.comm_bytes)
    rows = (pf.value(proof, pf.snark(proof), "comm_derefs.len"), pf.value(case.comm_bytes, cfields, "comm_ops.len"), pf.value(case.comm_bytes, cfields, "comm_mem.len"))
    assert rows[0] >= 256 and rows[1] >= 256 and rows[2] < 256, rows                       # comm_mem is summed on the host
    corpus = pf.steering(proof, pf.snark(proof))
    assert case.product(proof) == 0
    t0 = time.time()
    singles = pc.codes(case.product, corpus)
    t1 = time.time()
    assert all(c != 0 for c in singles), [m[:2] for m, c in zip(corpus.mutants, singles) if c == 0]
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    order = pc.interleaved(len(corpus))
    blobs = [proof] + [corpus.mutants[i][2] for i in order] + [proof]
    got, ran = _launches(lambda: case.product_many(blobs))
    assert ran.get("msm_var", 0) >= 2, ran                                                # the batched device passes over comm_derefs and comm_ops ran
    print("SNARK 2^12 compiler-like, steering: %d mutants, %d skipped, singles %.1f s, snark_verify_many %.1f s" % (len(corpus), corpus.check_skips(None), t1 - t0, time.time() - t1))
    assert got[0] == got[-1] == 0
    _no_differences(corpus, singles, [got[1 + order.index(i)] for i in range(len(corpus))])
