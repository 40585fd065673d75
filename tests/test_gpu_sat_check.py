"""The satisfiability check on the GPU (otti_witness_check_sat / otti_kd_check_sat, `spzk check`) against the CPU oracle.

The expected failing set never comes from the code under test: the oracle's multiply_vec gives <A_r,z>, <B_r,z>, <C_r,z> for every row
(Montgomery form: each is multiplied by 2^-256 mod l here), and a row is expected to fail when a*b % l != c.  Expected values are those
integers as canonical little-endian bytes.  Bit-exact throughout: the arithmetic is in GF(l)."""
import hashlib
import json
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import otti_amd as oa
import orc

pytestmark = pytest.mark.gpu
L = orc.L_ORDER
R_INV = pow(1 << 256, -1, L)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPZK = os.path.join(ROOT, "otti_amd", "spzk")


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


# ------------------------------------------------------------------------------------------------ helpers
def _ints(a32):
    a = np.ascontiguousarray(a32, dtype=np.uint8).reshape(-1, 32)
    return [int.from_bytes(a[k].tobytes(), "little") for k in range(a.shape[0])]


def _bytes32(xs):
    return np.array([np.frombuffer((x % L).to_bytes(32, "little"), dtype=np.uint8) for x in xs], dtype=np.uint8).reshape(-1, 32)


class Case:
    """an R1CS with its assignment, the product's instance and the oracle's"""

    def __init__(self, nc, nv, ni, A, B, C, vars32, inputs32):
        self.nc, self.nv, self.ni, self.A, self.B, self.C = nc, nv, ni, A, B, C
        self.vars32, self.inputs32 = np.ascontiguousarray(vars32, dtype=np.uint8).reshape(-1, 32), np.ascontiguousarray(inputs32, dtype=np.uint8).reshape(-1, 32)
        self.inst, self.oinst = oa.Instance.new(nc, nv, ni, A, B, C), orc.OInstance(nc, nv, ni, A, B, C)
        self.ncp, self.nvp, _ = self.inst.dims
        assert (self.ncp, self.nvp) == (self.oinst.num_cons, self.oinst.num_vars)

    @classmethod
    def of(cls, r):
        return cls(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"], r["vars"], r["inputs"])

    def z_mont(self, vars32, inputs32):
        """z = vars || 0.. || 1 || inputs || 0..  (2 * padded num_vars elements) in Montgomery form, as the oracle's kernels read it"""
        v, i = _ints(vars32), _ints(inputs32)
        z = v + [0] * (self.nvp - len(v)) + [1] + i
        return orc.fr_from_ints(z + [0] * (2 * self.nvp - len(z)))

    def expected(self, vars32, inputs32):
        """(failing rows ascending, {row: (a, b, c)}) by the oracle"""
        mont = orc.multiply_vec(self.oinst, self.z_mont(vars32, inputs32))
        a, b, c = ([x * R_INV % L for x in _ints(m)] for m in mont)              # out of Montgomery form: times 2^-256 mod l
        rows = [r for r in range(self.ncp) if a[r] * b[r] % L != c[r]]
        return rows, {r: (a[r], b[r], c[r]) for r in rows}

    def witness(self, vars32, inputs32):
        return oa.Witness(self.inst, oa.VarsAssignment.new(vars32), oa.InputsAssignment.new(inputs32))

    def rows_reading(self, col):
        """constraint rows with an entry in column `col` (the caller's column numbering)"""
        return sorted(set(int(r) for M in (self.A, self.B, self.C) for r in M["row"][M["col"] == col]))

    def long_rows(self, more_than=64):
        out = set()
        for M in (self.A, self.B, self.C):
            counts = np.bincount(M["row"].astype(np.int64), minlength=self.nc)
            out |= set(int(r) for r in np.nonzero(counts > more_than)[0])
        return sorted(out)


def _check_report(case, vars32, inputs32, max_rows=64):
    """check_sat on the uploaded assignment equals the oracle's verdict: count, rows (lowest max_rows, ascending), values"""
    want_rows, want_abc = case.expected(vars32, inputs32)
    rep = case.witness(vars32, inputs32).check_sat(case.inst, max_rows=max_rows)
    print(f"n_unsat={rep.n_unsat} (oracle {len(want_rows)}) rows={rep.rows.tolist()[:8]} kernel_ms={rep.kernel_ms:.4f}")
    assert rep.n_unsat == len(want_rows)
    assert rep.rows.dtype == np.uint64 and rep.rows.tolist() == want_rows[:max_rows]
    assert bool(rep) == (not want_rows)
    assert rep.values.shape == (len(rep.rows), 3, 32)
    for k, r in enumerate(rep.rows.tolist()):
        assert [int.from_bytes(rep.values[k, j].tobytes(), "little") for j in range(3)] == list(want_abc[r]), r
    return rep, want_rows


def _bump(a32, k):
    """a copy with element k replaced by (element + 1) mod l"""
    out = np.array(a32, dtype=np.uint8, copy=True).reshape(-1, 32)
    out[k] = _bytes32([_ints(out[k:k + 1])[0] + 1])[0]
    return out


def _wide_r1cs(rng, n=1 << 12, ni=4, per_row=4):
    """hand-built: `per_row` entries per row and matrix, every coefficient a uniform 252-bit value (no small-integer codes), satisfiable
    by solving one coefficient of C per row"""
    size_z = n + 1 + ni
    z = [int.from_bytes(rng.bytes(40), "little") % L or 1 for _ in range(size_z)]
    z[n] = 1
    ents = {k: [] for k in "ABC"}
    for row in range(n):
        sums = {}
        for name in "ABC":
            cols = [int(c) for c in rng.choice(size_z, size=per_row, replace=False)]
            vals = [int.from_bytes(rng.bytes(32), "little") >> 4 for _ in cols]    # uniform below 2^252 < l
            sums[name] = (cols, vals)
        a = sum(v * z[c] for c, v in zip(*sums["A"])) % L
        b = sum(v * z[c] for c, v in zip(*sums["B"])) % L
        cc, cv = sums["C"]
        rest = sum(v * z[c] for c, v in zip(cc[1:], cv[1:])) % L
        cv[0] = (a * b - rest) * pow(z[cc[0]], -1, L) % L
        for name in "ABC":
            ents[name] += [(row, c, v) for c, v in zip(*sums[name])]
    mats = []
    for name in "ABC":
        e = np.zeros(len(ents[name]), dtype=oa.ENTRY_DTYPE)
        e["row"] = [t[0] for t in ents[name]]; e["col"] = [t[1] for t in ents[name]]
        e["val"] = _bytes32([t[2] for t in ents[name]])
        mats.append(e)
    return dict(num_cons=n, num_vars=n, num_inputs=ni, A=mats[0], B=mats[1], C=mats[2], vars=_bytes32(z[:n]), inputs=_bytes32(z[n + 1:]))


def _nonpow2_case():
    # num_vars not a power of two, fewer constraints than variables (padding and the column shift of Instance::new)
    r = oa.synth_r1cs(24, 5, 3)
    nv = 40
    vars_pad = np.zeros((nv, 32), dtype=np.uint8); vars_pad[:24] = r["vars"]
    A, B, C = r["A"].copy(), r["B"].copy(), r["C"].copy()
    for m in (A, B, C):
        m["col"] = np.where(m["col"] >= 24, m["col"] + (nv - 24), m["col"])
    return Case(24, nv, 5, A, B, C, vars_pad, r["inputs"])


def _rect_case(shape):
    n, ni = 64, 3
    r = oa.synth_r1cs(n, ni, 21)
    A, B, C, vars_, inputs = r["A"].copy(), r["B"].copy(), r["C"].copy(), r["vars"], r["inputs"]
    if shape == "many_vars":
        extra = 2048
        for M in (A, B, C):
            M["col"] = np.where(M["col"] >= n, M["col"] + extra, M["col"])
        canon = np.random.default_rng(5).integers(0, 256, size=(extra, 32), dtype=np.uint8); canon[:, 31] &= 0x0f
        return Case(n, n + extra, ni, A, B, C, np.concatenate([vars_, canon]), inputs)
    reps = 64                                                  # many_cons: every constraint 64 times over 64 variables

    def rep(M):
        out = np.tile(M, reps); out["row"] = np.concatenate([M["row"] + k * n for k in range(reps)]); return out
    return Case(n * reps, n, ni, rep(A), rep(B), rep(C), vars_, inputs)


# The three instances of "both lane layouts and both coefficient paths": the uniform synthetic instance has one entry per row, two in three of
# them small integers (row per lane, coefficient codes), the compiler-like one ~4.6 small-integer entries per row (row per quad, coefficient
# codes) and rows of more than 64 entries (the segmented path), the hand-built one 4 entries per row with 252-bit coefficients (row per quad,
# no codes).  That each reaches its kernels is asserted below, through device_info; row per lane without codes is test_gpu_sparse_edges.py's.
_cache = {}
_VARIANT = {"uniform": dict(quad=False, use_small=True, heavy=False), "compiler": dict(quad=True, use_small=True, heavy=True),
            "wide": dict(quad=True, use_small=False, heavy=False)}


def _layout_case(name):
    if name not in _cache:
        if name == "uniform":
            _cache[name] = Case.of(oa.synth_r1cs(1 << 16, 10, 1))
        elif name == "compiler":
            _cache[name] = Case.of(oa.synth_r1cs_compiler_like(1 << 16, 10, 5))
        else:
            _cache[name] = Case.of(_wide_r1cs(np.random.default_rng(777)))
        info, want = _cache[name].inst.device_info(), _VARIANT[name]
        assert (info["quad"], info["use_small"], info["n_heavy"] > 0) == (want["quad"], want["use_small"], want["heavy"]), (name, info)
    return _cache[name]


LAYOUTS = ["uniform", "compiler", "wide"]


# ------------------------------------------------------------------------------------------------ 1. satisfied instances report zero
@pytest.mark.parametrize("name", LAYOUTS + ["uniform_2p10", "nonpow2", "many_vars", "many_cons"])
def test_satisfied_instances_report_zero(name):
    case = (_layout_case(name) if name in LAYOUTS else Case.of(oa.synth_r1cs(1 << 10, 10, 1)) if name == "uniform_2p10"
            else _nonpow2_case() if name == "nonpow2" else _rect_case(name))
    if name == "compiler":
        assert case.long_rows(), "the compiler-like instance has no row of more than 64 entries: the segmented path would not run"
    rep, want_rows = _check_report(case, case.vars32, case.inputs32)
    assert rep.n_unsat == 0 and want_rows == [] and rep.rows.size == 0 and bool(rep)
    assert case.inst.is_sat(oa.VarsAssignment.new(case.vars32), oa.InputsAssignment.new(case.inputs32))
    assert case.oinst.is_sat(case.vars32, case.inputs32)


# ------------------------------------------------------------------------------------------------ 2. one corrupted variable
@pytest.mark.parametrize("name", LAYOUTS)
def test_one_corrupted_variable(name):
    case = _layout_case(name)
    targets = [0, case.nc - 1] + (case.long_rows()[:1] if name == "compiler" else [])
    if name == "compiler":
        assert len(targets) == 3, "no long row in the compiler-like instance"
    for row in targets:
        cols = [int(c) for c in case.A["col"][case.A["row"] == row] if c < case.nv]            # a variable this row's A reads
        assert cols, row
        bad = _bump(case.vars32, cols[0])
        rep, want_rows = _check_report(case, bad, case.inputs32)
        assert row in want_rows, (row, want_rows[:10])                                         # the case cannot pass vacuously
        assert set(want_rows) <= set(case.rows_reading(cols[0]))
        assert not case.inst.is_sat(oa.VarsAssignment.new(bad), oa.InputsAssignment.new(case.inputs32))


# ------------------------------------------------------------------------------------------------ 3. a corrupted public input
@pytest.mark.parametrize("name", ["uniform", "compiler"])
def test_corrupted_public_input(name):
    case = _layout_case(name)
    k = next(k for k in range(case.ni) if case.rows_reading(case.nv + 1 + k))                  # an input some row reads
    bad_inputs = _bump(case.inputs32, k)
    rep, want_rows = _check_report(case, case.vars32, bad_inputs)
    assert want_rows and set(want_rows) <= set(case.rows_reading(case.nv + 1 + k))


# ------------------------------------------------------------------------------------------------ 4. everything fails
@pytest.mark.parametrize("name", ["uniform", "compiler"])
def test_everything_fails(name):
    case = _layout_case(name)
    # every variable off by one: each row's product a*b moves away from what its C row gives
    bad = _bytes32([x + 1 for x in _ints(case.vars32)])
    want_rows, _ = case.expected(bad, case.inputs32)
    assert len(want_rows) >= case.ncp // 2
    rep, _ = _check_report(case, bad, case.inputs32, max_rows=64)
    assert rep.n_unsat == len(want_rows) and rep.rows.tolist() == want_rows[:64] and rep.rows.tolist() == sorted(rep.rows.tolist())
    wit = case.witness(bad, case.inputs32)
    alone = wit.check_sat(case.inst, max_rows=0)                                              # rows_cap = 0: the count alone
    assert alone.n_unsat == len(want_rows) and alone.rows.size == 0
    no_values = wit.check_sat(case.inst, max_rows=5, values=False)
    assert no_values.n_unsat == len(want_rows) and no_values.rows.tolist() == want_rows[:5] and no_values.values is None
    many = wit.check_sat(case.inst, max_rows=200)                                             # more rows than one launch of the report kernel takes
    assert many.rows.tolist() == want_rows[:200]
    _, abc = case.expected(bad, case.inputs32)
    assert [int.from_bytes(many.values[199, j].tobytes(), "little") for j in range(3)] == list(abc[want_rows[199]])


# ------------------------------------------------------------------------------------------------ 5. the check is read-only
def test_check_leaves_witness_and_proof_unchanged():
    golden = [g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "proofs.json"))) if g["n"] == 65536]
    assert golden
    g = golden[0]
    r = oa.synth_r1cs(g["n"], g["num_inputs"], g["instance_seed"])
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(r["inputs"]))
    assert wit.check_sat(inst).n_unsat == 0
    p = oa.NIZK.prove(inst, wit, None, gens, g["label"].encode(), bytes.fromhex(g["tape_seed"]))
    assert len(p.bytes) == g["proof_len"] and hashlib.sha256(p.bytes).hexdigest() == g["proof_sha256"]
    assert wit.check_sat(inst).n_unsat == 0                                                   # and after a proof on the same context
    p2 = oa.NIZK.prove(inst, wit, None, gens, g["label"].encode(), bytes.fromhex(g["tape_seed"]))
    assert p2.bytes == p.bytes


# ------------------------------------------------------------------------------------------------ 7. device pointers, caller's stream
@pytest.mark.parametrize("name", LAYOUTS)
def test_kd_check_sat_bitmap(name):
    case = _layout_case(name)
    row = case.long_rows()[0] if name == "compiler" else 77
    col = next(int(c) for c in case.A["col"][case.A["row"] == row] if c < case.nv)
    words = (case.ncp + 63) // 64
    KD = oa.kernels_dev
    stream = KD.stream_create()
    try:
        for vars32 in (case.vars32, _bump(case.vars32, col), _bytes32([x + 1 for x in _ints(case.vars32)])):
            want_rows, _ = case.expected(vars32, case.inputs32)
            want_bits = np.zeros(words, dtype=np.uint64)
            for r in want_rows:
                want_bits[r >> 6] |= np.uint64(1 << (r & 63))
            z = oa.DeviceArray.from_host(case.z_mont(vars32, case.inputs32))
            for st in (None, stream):
                bits = oa.DeviceArray(words, 8)
                oa.lib.otti_dev_upload(bits.ptr, np.full(words, 0xa5a5a5a5a5a5a5a5, dtype=np.uint64).ctypes.data_as(oa.api._vp), words * 8)   # every word must be written
                n = KD.check_sat(case.inst, z, bits, st)
                if st is not None:
                    KD.stream_sync(st)
                got = bits.to_host().reshape(-1).view(np.uint64)
                assert n == len(want_rows)
                assert np.array_equal(got, want_bits)
            # what the report of the resident form implies is the same bitmap
            rep = case.witness(vars32, case.inputs32).check_sat(case.inst, max_rows=64, values=False)
            assert rep.n_unsat == n and rep.rows.tolist() == want_rows[:64]
    finally:
        KD.stream_destroy(stream)


# ------------------------------------------------------------------------------------------------ 8. four threads, one witness
def test_four_threads_check_the_same_witness():
    case = _layout_case("compiler")
    row = case.long_rows()[0]
    col = next(int(c) for c in case.A["col"][case.A["row"] == row] if c < case.nv)
    bad = _bump(case.vars32, col)
    want_rows, want_abc = case.expected(bad, case.inputs32)
    assert row in want_rows
    case.inst.prepare_device()
    wit_bad, wit_ok = case.witness(bad, case.inputs32), case.witness(case.vars32, case.inputs32)
    results, errors = [], []

    def run():
        try:
            for _ in range(5):
                a, b = wit_bad.check_sat(case.inst), wit_ok.check_sat(case.inst)
                results.append((a.n_unsat, a.rows.tolist(), a.values.tobytes(), b.n_unsat))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run) for _ in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    want_values = b"".join(int(x).to_bytes(32, "little") for r in want_rows[:64] for x in want_abc[r])
    assert len(results) == 20 and all(res == (len(want_rows), want_rows[:64], want_values, 0) for res in results)


def test_witness_of_other_dimensions_is_refused():
    small, big = Case.of(oa.synth_r1cs(64, 4, 2)), Case.of(oa.synth_r1cs(256, 4, 2))
    wit = small.witness(small.vars32, small.inputs32)
    with pytest.raises(oa.R1CSError) as e:
        wit.check_sat(big.inst)
    assert e.value.code == -4                                                                  # OTTI_ERR_INVALID_NUM_VARS


def test_sat_check_kernel_class_is_timed():
    case = Case.of(oa.synth_r1cs(1 << 12, 4, 2))
    wit = case.witness(case.vars32, case.inputs32)
    oa.stats_enable(True)
    try:
        rep = wit.check_sat(case.inst)
        st = oa.stats_read()
    finally:
        oa.stats_enable(False)
    assert rep.n_unsat == 0 and rep.kernel_ms > 0
    assert st["sat_check"][0] == 1 and st["sat_check"][1] > 0 and st["spmv"][0] == 0


# ------------------------------------------------------------------------------------------------ 9. command line
def test_spzk_check_and_check_option(tmp_path):
    pre, bad_pre = str(tmp_path / "syn"), str(tmp_path / "bad")
    files = lambda p: [p + ".zkif", p + ".inp.zkif", p + ".wit.zkif"]
    assert subprocess.run([SPZK, "synth", "300", pre, "7", "4"], capture_output=True).returncode == 0
    res = subprocess.run([SPZK, "check"] + files(pre), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert re.search(r"^\* check_sat [0-9.]+ ms$", res.stdout, re.M) and res.stdout.rstrip().endswith("Satisfied")
    # one witness value flipped, written back as a zkif triple
    r = oa.zkif_load(*files(pre))
    r["vars"] = _bump(r["vars"], 5)
    oa.zkif_write(r, *files(bad_pre))
    case = Case.of(oa.zkif_load(*files(bad_pre)))
    want_rows, want_abc = case.expected(case.vars32, case.inputs32)
    assert 0 < len(want_rows) <= 16
    res = subprocess.run([SPZK, "check"] + files(bad_pre), capture_output=True, text=True)
    assert res.returncode == 1, res.stdout + res.stderr
    assert f"Unsatisfied: {len(want_rows)} of 300 constraints" in res.stdout and "Satisfied\n" not in res.stdout
    named = re.findall(r"^  constraint (\d+): A\.z=([0-9a-f]{64}) B\.z=([0-9a-f]{64}) C\.z=([0-9a-f]{64})$", res.stdout, re.M)
    assert [int(m[0]) for m in named] == want_rows
    for m in named:
        assert tuple(int(h, 16) for h in m[1:]) == want_abc[int(m[0])]
    # --check stops before proving; without it the behaviour is the old one
    res = subprocess.run([SPZK, "verify", "--nizk", "--check"] + files(bad_pre), capture_output=True, text=True)
    assert res.returncode == 1 and "* NIZK::prove" not in res.stdout, res.stdout + res.stderr
    assert res.stdout.rstrip().endswith("Verification FAILED (unsatisfied assignment)") and f"Unsatisfied: {len(want_rows)} of 300" in res.stdout
    res = subprocess.run([SPZK, "verify", "--nizk"] + files(bad_pre), capture_output=True, text=True)
    assert res.returncode == 1 and "* NIZK::prove" in res.stdout and "check_sat" not in res.stdout
    assert res.stdout.rstrip().splitlines()[-1].startswith("Verification FAILED (-10")
    # on the good triple --check changes nothing but the added lines, in both modes, and the proof is the same
    for mode in (["--nizk"], []):
        outs = []
        for extra in ([], ["--check"]):
            out = str(tmp_path / ("p" + "".join(mode + extra)))
            res = subprocess.run([SPZK, "verify"] + mode + extra + files(pre) + ["--seed", "2a" * 32, "--proof-out", out], capture_output=True, text=True)
            assert res.returncode == 0 and res.stdout.rstrip().endswith("Verification successful"), res.stdout + res.stderr
            assert ("* check_sat" in res.stdout) == bool(extra)
            outs.append(open(out, "rb").read())
        assert outs[0] == outs[1]
