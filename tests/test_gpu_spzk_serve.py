"""`spzk serve` on the GPU: served proofs are the one-shot's and the CPU oracle's byte for byte, generators are cached, one window table
serves circuits of several sizes (built for the larger, adopted by the smaller), SNARK mode and `check` are served, two workers prove at
once, and the server ends with status 0.

One server process for the whole module (two workers, OTTI_MSM_WINDOW=10 and a 1 GiB table budget: tables of tens of MB); the clients open
no GPU.  Every subprocess has a time limit.  If the server ever ends by a signal, with a non-zero status or at a time limit, the test that
saw it fails and the remaining ones skip: no second server is started behind a fault."""
import os
import re
import shutil
import subprocess
import tempfile
import threading

import pytest

import otti_amd as oa
import orc
from otti_amd.serve import SPZK, SpzkServer

pytestmark = pytest.mark.gpu
ENV = dict(os.environ, OTTI_MSM_WINDOW="10", OTTI_MSM_TABLE_GB="1")
ENV.pop("SPZK_SERVER", None)
T = 120
SEED = "2a" * 32
_state = {"srv": None, "dead": None}


def setup_module(module):
    assert oa.device_count() >= 1, "no MI355X visible"


def teardown_module(module):
    srv = _state["srv"]
    if srv is not None and srv.proc is not None:
        srv.close()


def one_shot(argv, cwd):
    return subprocess.run([SPZK] + argv, cwd=cwd, env=ENV, capture_output=True, text=True, timeout=T)


def normal(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith("* process start to main()") or line.startswith("* served:"):
            line = "<start or served>"
        out.append(re.sub(r"[0-9.]+ ms", "N ms", line))
    return out


def oracle_nizk(pre):
    r = oa.zkif_load(pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif")
    oi, og = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"]), orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    return orc.nizk_prove(oi, r["vars"], r["inputs"], og, b"nizk_example", b"\x2a" * 32)[0]


@pytest.fixture(scope="module")
def work():
    """circuits of 300, 5000 and 1024 constraints as zkif files, and the oracle's NIZK proofs of the first two — made once, left alone"""
    d = tempfile.mkdtemp(prefix="spzk-g-")
    want = {}
    for name, n, ni, seed in (("a", 300, 7, 4), ("b", 5000, 5, 9), ("s", 1024, 3, 2)):
        assert subprocess.run([SPZK, "synth", str(n), os.path.join(d, name), str(ni), str(seed)], capture_output=True, timeout=T).returncode == 0
        if name != "s":
            want[name] = oracle_nizk(os.path.join(d, name))
    yield d, want
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def server(work):
    if _state["dead"]:
        pytest.skip("the module's server ended abnormally earlier (%s): no other one is started" % _state["dead"])
    if _state["srv"] is None:
        _state["srv"] = SpzkServer(socket_path=os.path.join(work[0], "s"), jobs=2, idle_exit=300, env=ENV, start_timeout=T)
        try:
            _state["srv"].start()
        except Exception:
            _state["dead"] = _state["srv"].abnormal_end or "did not start"
            raise
    srv = _state["srv"]
    try:
        yield srv
    finally:
        if srv.abnormal_end:
            _state["dead"] = srv.abnormal_end


def nizk_argv(name, out):
    return ["verify", "--nizk", name + ".zkif", name + ".inp.zkif", name + ".wit.zkif", "--seed", SEED, "--proof-out", out]


def read(d, f):
    return open(os.path.join(d, f), "rb").read()


def test_served_proofs_are_the_one_shots_and_one_table_serves_two_sizes(work, server):
    d, want = work
    one = one_shot(nizk_argv("a", "a.one"), d)
    assert one.returncode == 0, one.stderr
    first = server.run(nizk_argv("a", "a.1"), cwd=d, timeout=T)
    assert first.returncode == 0 and first.stderr == one.stderr, first.stdout + first.stderr
    assert normal(first.stdout) == normal(one.stdout) and first.stdout.splitlines()[-1] == "Verification successful"
    assert "generators built, table built" in first.stdout
    assert read(d, "a.1") == read(d, "a.one") == want["a"]
    again = server.run(nizk_argv("a", "a.2"), cwd=d, timeout=T)
    assert again.returncode == 0 and "generators cached, table own" in again.stdout and read(d, "a.2") == want["a"]
    st = server.status()
    assert st["tables_built"] == 1 and st["adoptions"] == 0 and st["table"]["c"] == 10 and st["table"]["bases"] == 34 and st["handles_cached"] == 1
    small_bytes = st["table"]["bytes"]
    # a larger circuit: its table replaces the first, whose handle adopts it
    larger = server.run(nizk_argv("b", "b.1"), cwd=d, timeout=T)
    assert larger.returncode == 0 and "generators built, table built" in larger.stdout, larger.stdout + larger.stderr
    assert read(d, "b.1") == want["b"]
    back = server.run(nizk_argv("a", "a.3"), cwd=d, timeout=T)
    assert back.returncode == 0 and "generators cached, table adopted" in back.stdout and read(d, "a.3") == want["a"]
    assert normal(back.stdout) == normal(one.stdout)
    st = server.status()
    assert st["tables_built"] == 2 and st["adoptions"] >= 1 and st["handles_cached"] == 2
    assert st["table"]["c"] == 10 and st["table"]["bases"] == 130 and st["table"]["bytes"] * 34 == small_bytes * 130      # ONE table: the larger handle's
    # prove and verify as separate requests, the verifier without the witness
    p = server.run(["prove", "--nizk", "b.zkif", "b.inp.zkif", "b.wit.zkif", "--seed", SEED, "--proof-out", "b.2"], cwd=d, timeout=T)
    assert p.returncode == 0 and p.stdout.splitlines()[-1].startswith("Proof written to b.2") and read(d, "b.2") == want["b"]
    v = server.run(["verify", "--nizk", "b.zkif", "b.inp.zkif", "--proof-in", "b.2"], cwd=d, timeout=T)
    assert v.returncode == 0 and v.stdout.splitlines()[-1] == "Verification successful"


def test_snark_mode_is_served(work, server):
    d, _ = work
    argv = ["verify", "s.zkif", "s.inp.zkif", "s.wit.zkif", "--seed", SEED, "--proof-out"]
    one, via = one_shot(argv + ["s.one"], d), server.run(argv + ["s.via"], cwd=d, timeout=T)
    assert one.returncode == 0 and via.returncode == 0, one.stderr + via.stderr
    assert normal(via.stdout) == normal(one.stdout) and via.stdout.splitlines()[-1] == "Verification successful"
    assert read(d, "s.via") == read(d, "s.one")


def test_check_of_a_corrupted_witness_reports_as_the_one_shot(work, server):
    d, _ = work
    wit = bytearray(read(d, "a.wit.zkif")); wit[-40] ^= 1
    open(os.path.join(d, "bad.wit.zkif"), "wb").write(bytes(wit))
    for argv in (["check", "a.zkif", "a.inp.zkif", "bad.wit.zkif"], ["check", "a.zkif", "a.inp.zkif", "a.wit.zkif"],
                 ["verify", "--nizk", "a.zkif", "a.inp.zkif", "bad.wit.zkif", "--check"]):
        one, via = one_shot(argv, d), server.run(argv, cwd=d, timeout=T)
        assert (via.returncode, via.stderr, normal(via.stdout)) == (one.returncode, one.stderr, normal(one.stdout)), argv
        assert via.returncode == (0 if argv[3] == "a.wit.zkif" else 1)


def test_two_workers_prove_at_once(work, server):
    d, want = work
    res = [None] * 4
    def client(k):
        name = "ab"[k % 2]
        res[k] = (name, "%s.j%d" % (name, k), server.run(nizk_argv(name, "%s.j%d" % (name, k)), cwd=d, timeout=T))
    th = [threading.Thread(target=client, args=(k,)) for k in range(len(res))]
    [t.start() for t in th]; [t.join() for t in th]
    for name, out, r in res:
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "Verification successful", r.stdout + r.stderr
        assert read(d, out) == want[name], out
    assert server.status()["tables_built"] == 2                  # nothing was rebuilt for them


def test_shutdown_ends_the_server_with_status_0(work, server):
    assert server.close(timeout=T) == 0 and server.abnormal_end is None
    assert not os.path.exists(server.socket_path)
