"""tests/msm_cases.py proved on the host, by brute force over its own restatement of the recoding: every scalar is below l and is the sum of its
digits; the digit cases look up exactly the reachable (window, magnitude, sign) entries at the narrow widths and every listed magnitude at the
wide ones, at every base; the seam cases sit where they claim and fill the work list to its cap; the plan restated in Python agrees with the
launches tests/msm_plan_check.cpp pins.  A case that does not meet its claim fails here, not on the GPU."""
import pytest

import msm_cases as mc

WIDTHS = (4, 7, 8, 9, 11, 12, 13, 15, 16, 17)


@pytest.mark.parametrize("c", range(4, 18))
def test_digits_reconstruct_the_scalar(c):
    E = 1 << (c - 1)
    for s in mc.digit_scalars(c) + mc.family(c, mc.magnitudes(c))[:: 7 if c == 8 else 1]:
        ds = mc.digits(s, c)
        assert 0 <= s < mc.L and len(ds) == mc.windows(c) and all(-E <= d < E for d in ds)
        assert sum(d * (1 << (c * w)) for w, d in enumerate(ds)) == s


@pytest.mark.parametrize("c", range(4, 18))
def test_the_chain_is_minus_E_everywhere_but_the_top(c):
    s, E = mc.chain(c), 1 << (c - 1)
    assert s < mc.L and mc.digits(s, c) == [-E] * (mc.windows(c) - 1) + [1]


def test_reachable_entries_per_base_of_the_two_families():
    for c, want in ((4, 946), (8, 7921), (9, 14309)):
        got = set()
        for s in mc.family(c, range(1, (1 << (c - 1)) + 1)):
            got |= mc.entries(s, c)
        assert len(got) == want, c
        assert mc.reachable(c) == got, c                          # the chain and the top-window scalars add nothing to them


@pytest.mark.parametrize("c", WIDTHS)
def test_digit_cases_cover_what_they_claim_at_every_base(c):
    R = 16
    rows = mc.digit_rows(c, R)
    got = mc.looked_up(rows, c)
    per_base = {e[1:] for e in got}
    assert got == {(b,) + e for b in range(R + 2) for e in per_base}              # every base meets the same entries
    if c <= mc.NARROW_MAX:
        reach = mc.reachable(c)
        assert per_base == reach                                                  # the share of reachable entries left out is zero
    else:
        E, T = 1 << (c - 1), mc.table_block(c)
        listed = {m for m in (1, 2, T - 1, T, T + 1, 2 * T, E - 1, E) if 1 <= m <= E}
        assert set(mc.magnitudes(c)) == listed
        assert mc.reachable(c, listed) <= per_base
        for w in range(mc.windows(c) - 2):                                         # below the two top windows nothing is out of reach
            assert {(w, m, -1) for m in listed} | {(w, m, 1) for m in listed if m < E} <= per_base
    scal = set(mc.digit_scalars(c))
    assert {mc.chain(c), mc.L - 1, 0, 1, 1 << 252} <= scal
    top = mc.digits(mc.L - 1, c)[-1]                               # the top window's digit grows with the scalar
    assert top >= max(mc.digits(s, c)[-1] for s in scal)
    assert any(mc.digits(s, c)[-1] == top for s in scal)
    assert len(rows) <= 300


def test_the_top_digit_that_is_only_a_carry():
    c = 11                                                         # 253 = 11 * 23: the top window starts above every scalar
    S = mc.digit_scalars(c)
    assert mc.windows(c) == 24 and all(mc.digits(s, c)[-1] in (0, 1) for s in S)
    assert all(mc.digits(s, c)[-1] == 1 for s in S if s >= 1 << 252) and not any(mc.digits(s, c)[-1] for s in S if s < 1 << 251)
    assert any(s >= 1 << 252 for s in S) and (23, 1, 1) in mc.reachable(c, mc.magnitudes(c))


def test_seams_and_the_work_list_cap():
    assert [mc.sub_cap(c) for c in (8, 9, 13, 16, 17)] == [260, 286, 416, 512, 512]
    assert 260 * 32 == mc.K_MSM_LIST_CAP == 8320
    for kind, c, R in (("bulk", 4, 4096), ("bulk", 8, 4096), ("sparse", 8, 2048), ("sparse", 9, 2048), ("sparse", 13, 2048), ("scatter", 8, 2048)):
        S, jobs = mc.seam_rows(kind, c, R)
        n_all = [j["n_dense"] + len(j["extra_base"]) for j in jobs]
        assert {S - 1, S, S + 1, 2 * S + 3, 4 * S} <= set(n_all)
        whole_zero = 0
        if kind != "scatter":
            assert any(j["n_dense"] == S and len(j["extra_base"]) == 1 for j in jobs)                 # one extra alone behind the seam
            assert any(j["n_dense"] == S - 4 and len(j["extra_base"]) == 8 for j in jobs)             # four and four
            assert any(j["n_dense"] + len(j["extra_base"]) == S and j["extra_base"] for j in jobs)    # wholly before it
        for j in jobs:
            assert j["n_dense"] <= R and all(b < R + 2 for b in j["extra_base"])
            p = mc.plan(c, j["rows"], j["n_dense"], len(j["extra_base"]), sparse=j["sparse"], force_bulk=True, bulk_workgroups=1)
            if kind != "scatter":
                assert (p["chunk"], p["nchunks"], p["fuse"]) == (j["n_dense"], 1, 0)
            for r in range(j["rows"]):
                row = j["dense"][r] + j["extra"][r]
                assert all(0 <= s < mc.L for s in row) and all(j["extra"][r])
                subs = [row[k: k + S] for k in range(0, len(row), S)]
                kinds = [mc.KINDS[(k + r) % 4] for k in range(len(subs))]
                for sub, what in zip(subs, kinds):
                    pairs = sum(1 for s in sub for d in mc.digits(s, c) if d)
                    if what == "full":
                        assert pairs == len(sub) * mc.windows(c)
                    if kind == "sparse":
                        assert pairs <= mc.K_MSM_LIST_CAP
                if kind == "sparse" and c == 8 and len(row) >= S and r == 0:
                    assert sum(1 for s in subs[0] for d in mc.digits(s, c) if d) == mc.K_MSM_LIST_CAP        # the list exactly at its cap
                for k, what in enumerate(kinds):
                    if what == "zero":                                                                   # a sub-chunk all zero: an empty list
                        assert not any(row[k * S: min((k + 1) * S, j["n_dense"])])
                        whole_zero += (k + 1) * S <= j["n_dense"]
        assert whole_zero >= 3


def test_shape_jobs_fold_onto_the_points():
    R = 128
    jobs = mc.shape_jobs(R, 8)
    names = [j["name"] for j in jobs]
    assert len(set(names)) == len(names)
    assert {(j["rows"], len(j["extra_base"]), j["mode"]) for j in jobs if not j["n_dense"]} == {(r, e, m) for r in (1, 2, 3, 9, 164) for e in (1, 6, 8) for m in ("raw", "compressed")}
    assert {1, 2, 63, 64, 65} <= {j["n_dense"] for j in jobs}
    for j in jobs:
        vs = mc.job_vectors(j, R)
        assert len(vs) == j["rows"] and all(len(v) == R + 2 and all(0 <= s < mc.L for s in v) for v in vs)
        if j.get("identity"):
            assert not any(any(v) for v in vs)
    assert any(j["mode"] == "keep" for j in jobs) and any(j["force_bulk"] and j["rows"] == 3 for j in jobs)
    assert any(len(set(j["extra_base"])) < len(j["extra_base"]) for j in jobs)                         # two extras on one base


def test_the_plan_restated_agrees_with_the_pinned_launches():
    """rows of tests/msm_plan_check.cpp (no bullet round, no addend)"""
    P = mc.plan
    assert P(17, 1024, 1024, 0, "keep") == dict(kernel="bulk", chunk=1024, nchunks=1, fuse=0, route="keep")
    assert P(17, 1024, 1024, 0, "keep", sparse=True)["kernel"] == "bulk_sparse" and P(7, 1024, 1024, 0, "keep", sparse=True)["kernel"] == "bulk"
    assert P(16, 512, 8192, 0) == dict(kernel="bulk", chunk=4096, nchunks=2, fuse=0, route="device_encode")
    assert P(8, 256, 256, 0, "keep") == dict(kernel="bulk", chunk=64, nchunks=4, fuse=0, route="keep")
    assert P(8, 64, 64, 0, "keep") == dict(kernel="small", chunk=8, nchunks=8, fuse=0, route="keep")
    assert P(8, 3, 64, 0, "keep", force_bulk=True) == dict(kernel="bulk", chunk=8, nchunks=8, fuse=0, route="keep")
    assert P(8, 2, 64, 0, "keep") == dict(kernel="small", chunk=6, nchunks=11, fuse=0, route="keep")
    assert P(17, 164, 0, 6, "raw") == dict(kernel="small", chunk=1, nchunks=1, fuse=0, route="raw")
    assert P(17, 1, 1024, 0, "raw") == dict(kernel="small", chunk=12, nchunks=86, fuse=0, route="raw")
    assert P(17, 1, 1024, 1) == dict(kernel="small", chunk=11, nchunks=94, fuse=2, route="mail")
    assert P(17, 1, 1024, 1, host_sum=False) == dict(kernel="small", chunk=11, nchunks=94, fuse=1, route="flag")
    assert P(8, 2, 16, 1) == dict(kernel="small", chunk=4, nchunks=4, fuse=2, route="mail")
    assert P(8, 3, 16, 1) == dict(kernel="small", chunk=6, nchunks=3, fuse=0, route="host_encode")
    assert P(8, 9, 16, 1) == dict(kernel="small", chunk=6, nchunks=3, fuse=0, route="device_encode")
    assert P(4, 2, 32767, 1) == dict(kernel="small", chunk=64, nchunks=512, fuse=0, route="host_encode")
    assert P(8, 3, 2048, 8, force_bulk=True, bulk_workgroups=1) == dict(kernel="bulk", chunk=2048, nchunks=1, fuse=0, route="host_encode")
    assert P(13, 1, 2048, 1, sparse=True, force_bulk=True, bulk_workgroups=1) == dict(kernel="bulk_sparse", chunk=2048, nchunks=1, fuse=0, route="host_encode")


def test_the_job_entry_judges_its_arguments_before_it_touches_a_device():
    """otti_k_msm_job: a base beyond the table, more than 8 extras, more raw rows than the host's point buffer, more dense terms than generators and no
    terms at all are OTTI_ERR_BAD_ARG (-21) with or without a GPU — the kernels take table columns from these numbers"""
    import numpy as np
    import otti_amd as oa
    import orc
    gens = oa.NIZKGens.new(256, 256, 1)                            # R = 16: 18 points
    one = orc.fr_from_ints([1] * 17)
    bad = [dict(rows=1, dense=one[:16], extra_s=one[:1], extra_base=[18]), dict(rows=1, dense=one[:16], extra_s=one[:9], extra_base=[0] * 9),
           dict(rows=513, dense=np.repeat(one[:1], 513, axis=0), mode="raw"), dict(rows=1, dense=one[:17]), dict(rows=1)]
    for kw in bad:
        with pytest.raises(oa.SpartanError) as e:
            oa.kernels.msm_job(gens, **kw)
        assert e.value.code == -21, (kw.get("extra_base"), e.value.args)
    with pytest.raises(KeyError):
        mc.seam("other", 8)
