"""`spzk serve` and `spzk-client` where no GPU is needed: the client's fallback, a server that verifies stored proofs and answers proving
requests with the one-shot's own failure, the request's working directory, malformed input on the socket, and the server's lifetime.

Server and one-shot run with no device visible (HIP_VISIBLE_DEVICES empty), so both sides of every comparison behave alike on any machine.
A served request's stdout is compared with the one-shot's line by line after replacing the numbers of milliseconds, the one line that
differs by design (`* process start to main()` / `* served:`) and the CODE in a last line `Verification FAILED (<code>: <name>)`: the verifier hands
its group equations to background threads and reports whichever failed first in time (verify.h Deferred), so a damaged proof is rejected as -10 or
as -11 from one run of the same process to the next; that the line is there, and the status, are compared."""
import os
import re
import shutil
import socket
import struct
import subprocess
import tempfile
import threading

import pytest

import otti_amd as oa
import orc
from otti_amd.serve import SPZK, SPZK_CLIENT, SpzkServer

ENV = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
ENV.pop("SPZK_SERVER", None)
T = 60                                                            # seconds: the limit of every subprocess here


def run(argv, cwd=None, env=ENV):
    return subprocess.run(argv, cwd=cwd, env=env, capture_output=True, text=True, timeout=T)


def normal(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith("* process start to main()") or line.startswith("* served:"):
            line = "<start or served>"
        out.append(re.sub(r"[0-9.]+ ms", "N ms", line))
    if out:
        out[-1] = re.sub(r"^Verification FAILED \(-1[01]: \w+\)$", "Verification FAILED (<the check that failed first>)", out[-1])
    return out


@pytest.fixture(scope="module")
def work():
    """a circuit of 300 constraints as zkif files, the oracle's proof of it and damaged copies; a short path, for the socket's sake"""
    d = tempfile.mkdtemp(prefix="spzk-t-")
    pre = os.path.join(d, "syn")
    assert run([SPZK, "synth", "300", pre, "7", "4"]).returncode == 0
    r = oa.zkif_load(pre + ".zkif", pre + ".inp.zkif", pre + ".wit.zkif")
    oi = orc.OInstance(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
    og = orc.OGens(r["num_cons"], r["num_vars"], r["num_inputs"])
    proof, _ = orc.nizk_prove(oi, r["vars"], r["inputs"], og, b"nizk_example", b"\x2a" * 32)
    open(pre + ".proof", "wb").write(proof)
    bad = bytearray(proof); bad[len(bad) // 2] ^= 4
    open(pre + ".flipped", "wb").write(bytes(bad))
    open(pre + ".short", "wb").write(proof[:-5])
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def server(work):
    srv = SpzkServer(socket_path=os.path.join(work, "s"), idle_exit=300, env=ENV).start()
    yield srv
    assert srv.close() == 0 and srv.abnormal_end is None
    assert not os.path.exists(srv.socket_path)


# ------------------------------------------------------------------------------------------------ the client alone
def test_client_links_neither_the_library_nor_the_hip_runtime():
    libs = subprocess.check_output(["ldd", SPZK_CLIENT], text=True)
    assert "libamdhip64" not in libs and "libottispartan" not in libs and "libstdc++" not in libs, libs


@pytest.mark.parametrize("argv,status", [(["synth", "16", "P", "2", "5"], 0), ([], 2), (["verify", "P.zkif"], 2)], ids=["synth", "no arguments", "verify with one file"])
def test_without_a_server_the_client_is_the_one_shot(tmp_path, argv, status):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    one, via = run([SPZK] + argv, cwd=a), run([SPZK_CLIENT] + argv, cwd=b)
    assert (via.returncode, via.stdout, via.stderr) == (one.returncode, one.stdout, one.stderr) and one.returncode == status
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        assert (a / f).read_bytes() == (b / f).read_bytes()
    # a socket path nobody listens on: the same
    dead = run([SPZK_CLIENT] + argv, cwd=b, env=dict(ENV, SPZK_SERVER=str(tmp_path / "nobody")))
    assert (dead.returncode, dead.stdout, dead.stderr) == (one.returncode, one.stdout, one.stderr)


def test_status_and_shutdown_talk_to_a_server_only(tmp_path):
    for flag in ("--server-status", "--server-shutdown"):
        for env in (ENV, dict(ENV, SPZK_SERVER=str(tmp_path / "nobody"))):
            r = run([SPZK_CLIENT, flag], env=env)
            assert r.returncode == 1 and r.stdout == "" and "no server answers" in r.stderr


# ------------------------------------------------------------------------------------------------ served requests
VERIFY = ["verify", "--nizk", "syn.zkif", "syn.inp.zkif", "--proof-in"]


@pytest.mark.parametrize("tail,ok", [(["syn.proof"], True), (["syn.flipped"], False), (["syn.short"], False), (["syn.proof", "--label", "other"], False)],
                         ids=["the proof", "a flipped byte", "truncated", "another label"])
def test_served_verifier_answers_as_the_one_shot(work, server, tail, ok):
    one, via = run([SPZK] + VERIFY + tail, cwd=work), server.run(VERIFY + tail, cwd=work, timeout=T)
    assert normal(via.stdout) == normal(one.stdout) and via.stderr == one.stderr and via.returncode == one.returncode
    assert any(line.startswith("* served: queue ") and "generators" in line and "table" in line for line in via.stdout.splitlines())
    if ok:
        assert via.returncode == 0 and via.stdout.splitlines()[-1] == "Verification successful"
    else:
        assert via.returncode != 0 and "Verification successful" not in via.stdout and via.stdout.splitlines()[-1].startswith("Verification FAILED")


def test_second_request_of_a_size_finds_its_generators_cached(work, server):
    server.run(VERIFY + ["syn.proof"], cwd=work, timeout=T)
    again = server.run(VERIFY + ["syn.proof"], cwd=work, timeout=T)
    assert "generators cached" in again.stdout and again.returncode == 0
    st = server.status()
    assert st["handles_cached"] >= 1 and st["requests_served"] >= 2 and st["tables_built"] == 0 and st["table"] == {"c": 0, "bytes": 0, "bases": 0}


@pytest.mark.parametrize("argv", [["verify", "--nizk", "syn.zkif", "syn.inp.zkif", "syn.wit.zkif"], ["prove", "--nizk", "syn.zkif", "syn.inp.zkif", "syn.wit.zkif", "--proof-out", "x.proof"],
                                  ["verify", "syn.zkif", "syn.inp.zkif", "syn.wit.zkif"], ["check", "syn.zkif", "syn.inp.zkif", "syn.wit.zkif"]],
                         ids=["nizk", "nizk prove", "snark", "check"])
def test_served_proving_request_without_a_device_fails_as_the_one_shot(work, server, argv):
    one, via = run([SPZK] + argv, cwd=work), server.run(argv, cwd=work, timeout=T)
    assert one.returncode == 1 and "(-20)" in one.stderr
    assert (via.returncode, via.stderr, normal(via.stdout)) == (one.returncode, one.stderr, normal(one.stdout))
    assert not os.path.exists(os.path.join(work, "x.proof"))


def test_other_subcommands_are_served(work, server, tmp_path):
    via = server.run(["synth", "16", "P", "2", "5"], cwd=str(tmp_path), timeout=T)
    one_dir = tmp_path / "one"; one_dir.mkdir()
    one = run([SPZK, "synth", "16", "P", "2", "5"], cwd=one_dir)
    assert (via.returncode, via.stdout, via.stderr) == (0, one.stdout, one.stderr)
    for f in ("P.zkif", "P.inp.zkif", "P.wit.zkif"):
        assert (tmp_path / f).read_bytes() == (one_dir / f).read_bytes()
    for argv in ([], ["verify", "P.zkif"], ["frobnicate"], ["serve", "--socket", "x"]):
        r = server.run(argv, cwd=str(tmp_path), timeout=T)
        assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("usage: spzk" if argv[:1] != ["serve"] else "spzk serve:")


def test_relative_paths_resolve_from_the_clients_directory(work, server, tmp_path):
    here = server.run(VERIFY + ["syn.proof"], cwd=work, timeout=T)
    assert here.returncode == 0
    elsewhere, one = server.run(VERIFY + ["syn.proof"], cwd=str(tmp_path), timeout=T), run([SPZK] + VERIFY + ["syn.proof"], cwd=tmp_path)
    assert elsewhere.returncode == one.returncode != 0 and elsewhere.stderr == one.stderr and "Verification successful" not in elsewhere.stdout
    absolute = [a if a.startswith("-") or a == "verify" else os.path.join(work, a) for a in VERIFY + ["syn.proof"]]
    assert server.run(absolute, cwd=str(tmp_path), timeout=T).returncode == 0
    sub = os.path.join(work, "sub"); os.makedirs(sub, exist_ok=True)
    up = ["verify", "--nizk", "../syn.zkif", "../syn.inp.zkif", "--proof-in", "../syn.proof"]
    assert server.run(up, cwd=sub, timeout=T).returncode == 0


# ------------------------------------------------------------------------------------------------ what the socket may be sent
def _request(argv, cwd):
    body = struct.pack("<I", len(cwd)) + cwd + struct.pack("<I", len(argv)) + b"".join(struct.pack("<I", len(a)) + a for a in argv)
    return struct.pack("<IHHI", 0x4b5a5053, 1, 1, len(body)) + body


def _exchange(path, data):
    """sends data, ends the sending side, returns everything the server answers before it closes"""
    with socket.socket(socket.AF_UNIX, socket.SOCK_STREAM) as s:
        s.settimeout(T)
        s.connect(path)
        try:
            s.sendall(data)
            s.shutdown(socket.SHUT_WR)
        except OSError:
            pass                                                   # the server may have hung up on the header already
        got = b""
        while True:
            try:
                chunk = s.recv(65536)
            except ConnectionResetError:
                break
            if not chunk:
                break
            got += chunk
        return got


def test_malformed_requests_close_their_connection_and_the_server_lives_on(work, server):
    good = _request([b"verify", b"--nizk", b"syn.zkif", b"syn.inp.zkif", b"--proof-in", b"syn.proof"], work.encode())
    answer = _exchange(server.socket_path, good)
    assert answer.endswith(b"\x03\x04\x00\x00\x00" + struct.pack("<i", 0)) and b"Verification successful\n" in answer
    bad = {"garbage": os.urandom(64), "nothing": b"", "half a header": good[:7], "truncated body": good[:-9], "a byte behind the last argument": good[:8] + struct.pack("<I", len(good) - 12 + 1) + good[12:] + b"x",
           "another version": good[:4] + b"\x02\x00" + good[6:], "another kind": good[:6] + b"\x09\x00" + good[8:],
           "oversized": struct.pack("<IHHI", 0x4b5a5053, 1, 1, 65536) + b"\0" * 65536,
           "65 arguments": _request([b"x"] * 65, b"/"), "a string of 4097 bytes": _request([b"y" * 4097], b"/"), "a NUL in an argument": _request([b"a\0b"], b"/"),
           "a length beyond the body": good[:12] + struct.pack("<I", 0xfffffff0) + good[16:]}
    for name, data in bad.items():
        assert _exchange(server.socket_path, data) == b"", name
        assert server.run(VERIFY + ["syn.proof"], cwd=work, timeout=T).returncode == 0, name


# ------------------------------------------------------------------------------------------------ lifetime
def _serve(path, *more):
    return subprocess.Popen([SPZK, "serve", "--socket", path, "--with-parent", *more], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_idle_exit_ends_the_server_with_status_0_and_removes_the_socket(work):
    path = os.path.join(work, "idle")
    p = _serve(path, "--idle-exit", "1")
    out, err = p.communicate(timeout=T)
    assert p.returncode == 0 and out == "spzk serve: ready %s\n" % path and not os.path.exists(path), err


def test_shutdown_live_socket_and_stale_socket(work):
    path = os.path.join(work, "life")
    stale = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM); stale.bind(path); stale.close()       # a socket file nobody listens on
    assert os.path.exists(path)
    with SpzkServer(socket_path=path, idle_exit=120, env=ENV) as srv:                               # replaced
        assert oct(os.stat(path).st_mode & 0o777) == "0o600"
        second = _serve(path, "--idle-exit", "5")
        out, err = second.communicate(timeout=T)
        assert second.returncode == 1 and out == "" and "live server" in err
        assert srv.status()["requests_served"] == 0                                                # the first one was not disturbed
        r = run([SPZK_CLIENT, "--server-shutdown"], env=dict(ENV, SPZK_SERVER=path))
        assert r.returncode == 0
        assert srv.close() == 0
    assert srv.abnormal_end is None and not os.path.exists(path)
    # not a socket: not ours to replace
    open(path, "w").close()
    third = _serve(path)
    out, err = third.communicate(timeout=T)
    assert third.returncode == 1 and "not a socket" in err and os.path.exists(path)
    os.unlink(path)
    for bad in (["--jobs", "9"], ["--jobs", "0"], ["--frob"]):
        p = _serve(path, *bad)
        assert p.communicate(timeout=T) and p.returncode == 2


def test_sigterm_ends_the_server_like_a_shutdown_request(work):
    path = os.path.join(work, "term")
    srv = SpzkServer(socket_path=path, idle_exit=120, env=ENV).start()
    srv.proc.terminate()
    srv._end(kill=False, why=None, timeout=T)
    assert srv.returncode == 0 and srv.abnormal_end is None and not os.path.exists(path)


def test_two_jobs_serve_two_clients_at_once(work):
    with SpzkServer(socket_path=os.path.join(work, "j2"), jobs=2, idle_exit=120, env=ENV) as srv:
        res = [None] * 6
        def client(k):
            res[k] = srv.run(VERIFY + (["syn.proof"] if k % 2 == 0 else ["syn.flipped"]), cwd=work, timeout=T)
        th = [threading.Thread(target=client, args=(k,)) for k in range(len(res))]
        [t.start() for t in th]; [t.join() for t in th]
        for k, r in enumerate(res):
            assert (r.returncode == 0) == (k % 2 == 0) and ("Verification successful" in r.stdout) == (k % 2 == 0), (k, r.stdout, r.stderr)
        st = srv.status()
        assert st["jobs"] == 2 and st["requests_served"] == len(res) and st["handles_cached"] == 1
    assert srv.returncode == 0 and srv.abnormal_end is None
