"""prove_many's front half alone (otti_k_prove_front) on staged vectors: the joint row job of K witnesses and their tiles of four against the
single launches — the rows against otti_k_msm_job's kept sums of each vector's variables, the products against otti_k_multiply_vec, byte for byte.
Witness counts of 15 and 16 at V = 2^12 (L = R = 64) sit on either side of msm_plan's 2^16-scalar threshold: 15 * 4096 scalars are a small launch,
16 * 4096 the chip-filling one, while each single job (4096 scalars) is a small one.  At V = 2^13 eight small-valued vectors (64-bit integers) and
eight uniform ones give one job per MSM variant."""
import numpy as np
import pytest

import otti_amd as oa
import orc

pytestmark = pytest.mark.gpu
K = oa.kernels
L = 2 ** 252 + 27742317777372353535851937790883648493


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def _setup(n, compiler_like=False):
    r = oa.synth_r1cs_compiler_like(n, 10, 5) if compiler_like else oa.synth_r1cs(n, 10, 3)
    inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
    return r, inst, gens


def _vector(rng, r, V, small):
    """2V Montgomery words as a resident witness holds them: V variables (uniform below l, or 64-bit integers of either sign), 1, the inputs, zeros"""
    if small:
        ints = [int(x) % L for x in rng.integers(-2 ** 62, 2 ** 62, size=V)]
    else:
        ints = [int.from_bytes(rng.bytes(40), "little") % L for _ in range(V)]
    tail = [1] + [int.from_bytes(bytes(x), "little") for x in np.asarray(r["inputs"], dtype=np.uint8).reshape(-1, 32)]
    return orc.fr_from_ints(ints + tail + [0] * (V - len(tail)))


def _check(n, smalls, want_kernels, compiler_like=False, joint_products=False):
    r, inst, gens = _setup(n, compiler_like)
    V = inst.dims[1]
    assert V == n
    ell = V.bit_length() - 1
    Lrows = 1 << (ell // 2)
    rng = np.random.default_rng(20261020 + n + len(smalls))
    zs = [_vector(rng, r, V, s) for s in smalls]
    rows, Az, Bz, Cz, info, _ = K.prove_front(inst, gens, zs, smalls)
    print(n, len(smalls), info)
    nk = len(smalls)
    # the products are formed jointly where the front-half rule (prove_many.cpp front_rule) says so: in the row-per-quad layout, or with the rule aside
    assert inst.device_info()["quad"] == compiler_like
    assert info["chunks"] == 1 and info["front_failed"] == 0 and info["product_tiles"] == ((nk + 3) // 4 if joint_products else 0)
    assert info["rows_from_front"] == nk and info["products_from_front"] == (nk if joint_products else 0)
    assert info["row_jobs"] == len(want_kernels) and info["row_kernel"] == list(want_kernels), info
    for k, z in enumerate(zs):
        want_rows, plan, _ = K.msm_job(gens, Lrows, dense=z[:V], mode="keep", sparse=int(smalls[k]))
        assert plan["kernel"] == "small", plan                                       # each single job is a latency-bound launch
        assert np.array_equal(rows[k], want_rows), ("rows of vector", k)
        a, b, c, _ = K.multiply_vec(inst, z)
        assert np.array_equal(Az[k], a) and np.array_equal(Bz[k], b) and np.array_equal(Cz[k], c), ("products of vector", k)


@pytest.fixture(autouse=True)
def narrow_table(monkeypatch):
    monkeypatch.setenv("OTTI_MSM_WINDOW", "10")                                      # a narrow generator table: tens of MB, built in milliseconds


def test_fifteen_witnesses_are_a_small_joint_job():
    _check(1 << 12, [False] * 15, ("small",))


def test_sixteen_witnesses_cross_into_the_bulk_kernel():
    _check(1 << 12, [False] * 16, ("bulk",))


def test_two_variants_are_two_jobs():
    """V = 2^13 (L = 64, R = 128): eight uniform and eight small-valued vectors, 8 * 8192 = 2^16 scalars each: the bulk kernel and its work-list twin"""
    _check(1 << 13, [True] * 8 + [False] * 8, ("bulk", "bulk_sparse"))


def test_products_are_joint_in_the_quad_layout():
    """a compiler-like instance (row per quad, coefficient codes, a long row): five small-valued vectors, a tile of four and a tile of one"""
    _check(1 << 12, [True] * 5, ("small",), compiler_like=True, joint_products=True)


def test_with_the_rule_set_aside_the_uniform_instance_has_tiles_too(monkeypatch):
    monkeypatch.setenv("OTTI_PROVE_MANY_RULE", "0")
    _check(1 << 12, [False] * 6, ("small",), joint_products=True)
