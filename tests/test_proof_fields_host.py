"""Every field of a proof tampered once, verdicts held to the oracle (no GPU): the field map of proof_fields.py against closed forms in the
dimensions, and the full corpus of substitutes — NIZK at n = 64, SNARK at n = 16, three inputs — through the oracle's verifier and the product's
host verifiers.

The rule the verdicts are held to (proof_fields.verdict_error): both implementations reject every mutant; a non-canonical scalar (plus_l) and a
changed vector count are MALFORMED (-12) to both; identity, other_point, plus_one and zero get the same code from both (here -10: a valid point or
scalar that is not the prover's can only be refused by an equation, directly or through the transcript).  An undecodable point is where the two
legitimately differ: the product decompresses the row commitments and the sum-check commitments ahead of the rounds and defers its group equations to
the end, so it reports DECOMPRESS (-11) for a point that the oracle, walking in the protocol's order, never decodes because an equation over the
changed transcript has already failed (-10).  On these two corpora that is the case for 37 NIZK and 25 SNARK point fields; the test asks that the
product say -11 or -10, and -11 wherever the oracle does.  Neither verifier is to be changed to make these agree.

The product's codes are taken three times — with the default background threads of verify.h Deferred, with none (OTTI_VERIFY_THREADS=0: every
deferred equation runs inside finish()) and with six — and once more through each batched verifier; all must be equal, code for code.  Each module
fixture prints its corpus size, the skipped substitutes (equal to the original: at most 1 %) and the seconds taken."""
import collections
import time

import pytest

import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc


def _lg(x):
    assert x >= 1 and x & (x - 1) == 0, x
    return x.bit_length() - 1


# ------------------------------------------------------------------------------------------------ field counts in closed form
def _sumcheck_counts(name, rounds, nz):
    return {name + ".comm_polys.len": 1, name + ".comm_polys[]": rounds, name + ".comm_evals.len": 1, name + ".comm_evals[]": rounds,
            name + ".proofs.len": 1, name + ".proofs[].delta": rounds, name + ".proofs[].beta": rounds, name + ".proofs[].z.len": rounds,
            name + ".proofs[].z[]": nz * rounds, name + ".proofs[].z_delta": rounds, name + ".proofs[].z_beta": rounds}


def _dplog_counts(name, lg_row):
    return {name + ".L.len": 1, name + ".L[]": lg_row, name + ".R.len": 1, name + ".R[]": lg_row, name + ".delta": 1, name + ".beta": 1,
            name + ".z1": 1, name + ".z2": 1}


def _r1cs_counts(N, V):
    """R1CSProof over N constraints and V variables (padded): 2^(ell / 2) row commitments of 2^(ell - ell / 2) scalars, ell = log2 V; log2 N rounds
    of the cubic sum-check with four answers each, log2 2V rounds of the quadratic one with three"""
    nrx, nry, ell = _lg(N), _lg(2 * V), _lg(V)
    want = {"comm_vars.len": 1, "comm_vars[]": 1 << (ell // 2), "claims_phase2[]": 4, "pok.alpha": 1, "pok.z1": 1, "pok.z2": 1,
            "prod.alpha": 1, "prod.beta": 1, "prod.delta": 1, "prod.z[]": 5, "eq1.alpha": 1, "eq1.z": 1, "comm_vars_at_ry": 1, "eq2.alpha": 1, "eq2.z": 1}
    want.update(_sumcheck_counts("sc1", nrx, 4)); want.update(_sumcheck_counts("sc2", nry, 3)); want.update(_dplog_counts("polyeval", ell - ell // 2))
    return want


def _batch_counts(name, length, n_prod, n_dotp):
    """ProductCircuitEvalProofBatched over circuits of `length` leaves: max(1, log2 length) layers, layer i with i rounds of three coefficients"""
    nl = max(1, _lg(length)); rounds = nl * (nl - 1) // 2
    want = {name + ".layers.len": 1, name + ".layers[].coeffs.len": nl, name + ".layers[].coeffs[].len": rounds, name + ".layers[].coeffs[][]": 3 * rounds,
            name + ".layers[].left.len": nl, name + ".layers[].left[]": n_prod * nl, name + ".layers[].right.len": nl, name + ".layers[].right[]": n_prod * nl}
    for v in ("dotp_left", "dotp_right", "dotp_weight"):
        want.update({"%s.%s.len" % (name, v): 1, "%s.%s[]" % (name, v): n_dotp})
    return {k: v for k, v in want.items() if v}


def _snark_counts(N, V, num_ops, num_mem_cells):
    """the R1CSProof, then R1CSEvalProof: a polynomial of m variables is committed in 2^(m / 2) rows and opened with m - m / 2 reduction rounds;
    derefs has m = log2 num_ops + 3 (six tables, padded to eight), ops + 4 (fifteen, to sixteen), mem log2 num_mem_cells + 1 (two)"""
    m_derefs, m_ops, m_mem = _lg(num_ops) + 3, _lg(num_ops) + 4, _lg(num_mem_cells) + 1
    want = _r1cs_counts(N, V)
    want.update({"inst_evals[]": 3, "comm_derefs.len": 1, "comm_derefs[]": 1 << (m_derefs // 2), "h_row_audit": 1, "h_col_audit": 1})
    for e in ("eval_row", "eval_col"):
        want.update({e + ".init": 1, e + ".read.len": 1, e + ".read[]": 3, e + ".write.len": 1, e + ".write[]": 3, e + ".audit": 1})
    for v in ("dotp_left", "dotp_right", "h_row_addr", "h_row_read_ts", "h_col_addr", "h_col_read_ts", "h_val", "h_deref_row", "h_deref_col"):
        want.update({v + ".len": 1, v + "[]": 3})
    want.update(_batch_counts("proof_mem", num_mem_cells, 4, 0)); want.update(_batch_counts("proof_ops", num_ops, 12, 6))
    want.update(_dplog_counts("pe_ops", m_ops - m_ops // 2)); want.update(_dplog_counts("pe_mem", m_mem - m_mem // 2))
    want.update(_dplog_counts("pe_derefs", m_derefs - m_derefs // 2))
    return want, (1 << (m_ops // 2), 1 << (m_mem // 2))


def _group_counts(fields):
    return dict(collections.Counter(pf.group(name) for name, _, _ in fields))


def _check_layout(blob, fields):
    """the fields tile the blob: in order, without gaps, each of its kind's size"""
    pos = 0
    for name, off, kind in fields:
        assert off == pos, name
        pos += 8 if kind in ("len", "u64") else 32
    assert pos == len(blob)
    assert len({name for name, _, _ in fields}) == len(fields)                            # names are unique


@pytest.mark.parametrize("n", [2, 64, 4096])
def test_nizk_field_counts(n):
    case = pc.NizkCase(oa.synth_r1cs(n, 3 if n > 2 else 1, 7))
    proof = case.oracle_proof()
    fields = pf.nizk(proof)                                                               # raises unless the walk ends at len(proof)
    _check_layout(proof, fields)
    want = _r1cs_counts(case.N, case.V)
    want.update({"rx.len": 1, "rx[]": _lg(case.N), "ry.len": 1, "ry[]": _lg(2 * case.V)})
    assert _group_counts(fields) == want
    assert pf.value(proof, fields, "comm_vars.len") == 1 << (_lg(case.V) // 2) and pf.value(proof, fields, "sc1.proofs[0].z.len") == 4
    with pytest.raises(ValueError):
        pf.nizk(proof[:-1])
    with pytest.raises(ValueError):
        pf.nizk(proof + b"\0")


@pytest.mark.parametrize("n", [2, 16, 256])
def test_snark_field_counts(n):
    case = pc.SnarkCase(oa.synth_r1cs(n, 3 if n > 2 else 1, 7))
    proof = case.oracle_proof()
    fields, cfields = pf.snark(proof), pf.commitment(case.comm_bytes)
    _check_layout(proof, fields); _check_layout(case.comm_bytes, cfields)
    dims = {k: pf.value(case.comm_bytes, cfields, k) for k in ("num_cons", "num_vars", "num_inputs", "batch_size", "num_ops", "num_mem_cells")}
    assert (dims["num_cons"], dims["num_vars"], dims["num_inputs"], dims["batch_size"]) == (case.N, case.V, case.r["num_inputs"], 3)
    assert dims["num_mem_cells"] == max(case.N, 2 * case.V)
    assert dims["num_ops"] >= max(2, case.nz) and (dims["num_ops"] == 2 or dims["num_ops"] // 2 < case.nz)       # the next power of two
    want, (rows_ops, rows_mem) = _snark_counts(case.N, case.V, dims["num_ops"], dims["num_mem_cells"])   # layers and rounds follow from num_ops, num_mem_cells
    assert _group_counts(fields) == want
    assert _group_counts(cfields) == {"num_cons": 1, "num_vars": 1, "num_inputs": 1, "batch_size": 1, "num_ops": 1, "num_mem_cells": 1,
                                      "comm_ops.len": 1, "comm_ops[]": rows_ops, "comm_mem.len": 1, "comm_mem[]": rows_mem}
    nl = max(1, _lg(dims["num_ops"]))
    for layer in range(nl):                                                               # layer i of the ops circuits has i rounds
        assert pf.value(proof, fields, "proof_ops.layers[%d].coeffs.len" % layer) == layer
    with pytest.raises(ValueError):
        pf.snark(proof[:-1])
    with pytest.raises(ValueError):
        pf.commitment(case.comm_bytes + b"\0")


def test_reduced_corpora_pick_what_they_say():
    case = pc.NizkCase(oa.synth_r1cs(64, 3, 7))
    proof = case.oracle_proof()
    fields = pf.nizk(proof)
    one = pf.one_per_field(proof, fields)
    assert [m[0] for m in one.mutants] == [f[0] for f in fields] and not one.skipped
    assert {m[1] for m in one.mutants} == {"other_point", "plus_one", "len_plus_one"}
    st = pf.steering(proof, fields)
    picked = collections.defaultdict(list)
    for name, what, _ in st.mutants:
        picked[name].append(what)
    rows = pf.value(proof, fields, "comm_vars.len")
    assert rows == 8
    for i in (0, 1, rows // 2, rows - 1):
        assert picked["comm_vars[%d]" % i] == ["identity", "other_point", "undecodable"]
    assert sum(1 for name in picked if name.startswith("comm_vars[")) == 4
    for name, _, _ in fields:
        if name.startswith(("rx[", "ry[")):
            assert picked[name] == ["plus_one"]
    nrx = _lg(case.N)
    for name in ("sc1.proofs[0].z[0]", "sc1.proofs[%d].z[0]" % (nrx - 1), "sc1.proofs[0].z.len", "sc1.proofs[%d].z.len" % (nrx - 1), "prod.z[0]", "pok.z2",
                 "polyeval.L[0]", "rx.len", "comm_vars.len", "eq2.z"):
        assert len(picked[name]) == 1, name
    for name in ("sc1.proofs[1].z[0]", "sc1.proofs[0].z[1]", "prod.z[4]", "polyeval.L[1]"):
        assert name not in picked, name
    assert {pf.group(name) for name in picked} == {pf.group(f[0]) for f in fields}      # no group is left out
    for name, what, blob in one.mutants[:40] + st.mutants:                                # one field changed, nothing else
        off, kind = next((o, k) for f, o, k in fields if f == name)
        size = 8 if kind == "len" else 32
        assert len(blob) == len(proof) and blob[:off] == proof[:off] and blob[off + size:] == proof[off + size:] and blob[off:off + size] != proof[off:off + size]


# ------------------------------------------------------------------------------------------------ the full corpora
@pytest.fixture(scope="module")
def nizk_run():
    case = pc.NizkCase(oa.synth_r1cs(64, 3, 7))
    proof = case.oracle_proof()
    return pc.Run(case, proof, pf.full(proof, pf.nizk(proof)), "NIZK n = 64, ni = 3")


@pytest.fixture(scope="module")
def snark_run():
    case = pc.SnarkCase(oa.synth_r1cs(16, 3, 7))
    proof = case.oracle_proof()
    return pc.Run(case, proof, pf.full(proof, pf.snark(proof)), "SNARK n = 16, ni = 3")


@pytest.fixture(params=["nizk", "snark"])
def run(request, nizk_run, snark_run):
    return nizk_run if request.param == "nizk" else snark_run


def test_every_mutant_is_rejected_with_the_oracles_code(run):
    """the rule of the module docstring, for every substitute of every field; a failure names the field and the substitute"""
    bad = run.failures()
    assert not bad, "%d of %d mutants:\n%s" % (len(bad), len(run.corpus), "\n".join(bad[:40]))
    assert len(run.corpus) >= 500
    hist = collections.Counter((what, o, p) for (_, what, _), o, p in zip(run.corpus.mutants, run.oracle, run.product))
    print(sorted(hist.items()))


@pytest.mark.parametrize("threads", ["0", "6"])
def test_deferred_equations_with_and_without_workers(run, threads, monkeypatch):
    """OTTI_VERIFY_THREADS is read when a Deferred is constructed: 0 runs every handed-over equation inside finish(), 6 on six background threads"""
    monkeypatch.setenv("OTTI_VERIFY_THREADS", threads)
    t0 = time.time()
    got = pc.codes(run.case.product, run.corpus)
    print("OTTI_VERIFY_THREADS=%s: %d mutants in %.1f s" % (threads, len(got), time.time() - t0))
    bad = pf.differences(run.corpus, run.product, got)
    assert not bad, "\n".join(bad[:40])
    assert run.case.product(run.proof) == 0


@pytest.mark.parametrize("threads", [0, 1])
def test_nizk_verify_many_gives_the_single_codes(nizk_run, threads):
    """the whole corpus in one otti_nizk_verify_many call, the good proof at both ends and in the middle"""
    blobs, _ = nizk_run.with_good()
    t0 = time.time()
    got = nizk_run.case.product_many(blobs, threads)
    print("verify_many, threads=%d: %d items in %.1f s" % (threads, len(blobs), time.time() - t0))
    bad = nizk_run.many_differences(got)
    assert not bad, "\n".join(bad[:40])


def test_snark_verify_many_gives_the_single_codes(snark_run, monkeypatch):
    """the whole corpus in one otti_snark_verify_many call in chunks of four, ordered so that a chunk's four proofs come from four stretches of the
    wire form: mutants that die at different steps of the staged verifier share a chunk with each other and with proofs that go on"""
    monkeypatch.setenv("OTTI_SNARK_VERIFY_CHUNK", "4")
    order = pc.interleaved(len(snark_run.corpus))
    blobs, _ = snark_run.with_good(order)
    t0 = time.time()
    got = snark_run.case.product_many(blobs)
    print("snark_verify_many, chunk 4: %d items in %.1f s" % (len(blobs), time.time() - t0))
    bad = snark_run.many_differences(got, order)
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ counts that disagree in well-framed bytes
# The product's code for every move of proof_fields.balanced, by the member the move is in — recorded from the verifiers as they stood before the
# wire code was gathered into wire.cpp, and the same since: a refusal either belongs to the parser (MALFORMED) or to the verifier (VERIFY_INTERNAL),
# and callers see which.  The two modes differ on polyeval: SnarkProof::parse refuses an L / R of different lengths, NizkProof::parse does not and
# the verifier rejects it.  The sum-checks' three vectors are the verifier's to compare in both modes; everything of the evaluation proof is refused
# at parse.  The oracle's parser is stricter (every one of these is MALFORMED to it), so only its refusal is asserted, not its code.
BALANCED_CODES = {
    "nizk": {"sc1": pf.VERIFY_INTERNAL, "sc2": pf.VERIFY_INTERNAL, "polyeval": pf.VERIFY_INTERNAL},
    "snark": {"sc1": pf.VERIFY_INTERNAL, "sc2": pf.VERIFY_INTERNAL, "polyeval": pf.MALFORMED, "pe_ops": pf.MALFORMED, "pe_mem": pf.MALFORMED,
              "pe_derefs": pf.MALFORMED, "proof_mem": pf.MALFORMED, "proof_ops": pf.MALFORMED},
}
# nizk: 2 sum-checks x 3 moves + 2 of polyeval.  snark (n = 16: five mem layers, four ops layers; proof_mem has no dot-product claims to move):
# 6 + 2 x 4 log dot-product proofs + 2 x (5 + 4) layers + 3 of proof_ops' dot-product claims
BALANCED_MOVES = {"nizk": 8, "snark": 35}


def test_balanced_counts_get_the_recorded_codes(run, request, monkeypatch):
    """one vector shorter and its neighbour longer, bytes well framed (proof_fields.balanced): the single verifier with its default threads, with
    OTTI_VERIFY_THREADS 0 and 6, and the batched verifier all give the table's code; the oracle refuses every one"""
    mode = request.node.callspec.params["run"]
    case, table = run.case, BALANCED_CODES[mode]
    moves = pf.balanced(run.proof, case.fields(run.proof))
    assert len(moves) == BALANCED_MOVES[mode] and {name.split(".")[0] for name, _ in moves} == set(table)
    for name, blob in moves:
        case.fields(blob)                                                                 # raises unless the walk ends at len(blob): well framed
    want = [table[name.split(".")[0]] for name, _ in moves]
    names = [name for name, _ in moves]
    blobs = [blob for _, blob in moves]
    assert list(zip(names, [case.product(b) for b in blobs])) == list(zip(names, want))
    for threads in ("0", "6"):
        monkeypatch.setenv("OTTI_VERIFY_THREADS", threads)
        assert list(zip(names, [case.product(b) for b in blobs])) == list(zip(names, want)), threads
    monkeypatch.delenv("OTTI_VERIFY_THREADS")
    for threads in (0, 1):
        got = case.product_many([run.proof] + blobs + [run.proof], threads)
        assert list(zip(names, got[1:-1])) == list(zip(names, want)) and got[0] == got[-1] == 0, threads
    refused = [case.oracle(b) for b in blobs]
    assert all(refused), list(zip(names, refused))


# ------------------------------------------------------------------------------------------------ the statement outside the proof
def test_a_changed_or_missing_input_is_rejected(run):
    case, proof = run.case, run.proof
    ni = case.inputs.shape[0]
    assert ni == 3
    for k in range(ni):
        changed = pc.inputs_plus_one(case.inputs, k)
        o, p = case.oracle(proof, changed), case.product(proof, changed)
        assert o != 0 and p != 0 and o == p, ("input %d plus_one" % k, o, p)
    short = case.inputs[:-1]
    assert case.oracle(proof, short) == case.product(proof, short) == pf.INVALID_NUM_INPUTS


def test_every_field_of_the_commitment_binds(snark_run):
    """one_per_field over the commitment's bytes (its six u64, both counts, every point of comm_ops and comm_mem), re-parsed on both sides: each side
    refuses the bytes or rejects the good proof"""
    case, proof = snark_run.case, snark_run.proof
    corpus = pf.one_per_field(case.comm_bytes, pf.commitment(case.comm_bytes))
    assert corpus.check_skips() == 0 and len(corpus) == 8 + sum(pf.value(case.comm_bytes, pf.commitment(case.comm_bytes), v) for v in ("comm_ops.len", "comm_mem.len"))
    t0 = time.time(); bad = []
    for name, what, blob in corpus.mutants:
        oc, comm = case.parse_both(blob)
        o = None if oc is None else case.oracle(proof, comm=oc)
        p = None if comm is None else case.product(proof, comm=comm)
        if o == 0 or p == 0 or (name.endswith(".len") and (oc, comm) != (None, None)):
            bad.append("%s / %s: oracle %s, product %s" % (name, what, o, p))
    print("commitment: %d mutants in %.1f s" % (len(corpus), time.time() - t0))
    assert not bad, "\n".join(bad)
