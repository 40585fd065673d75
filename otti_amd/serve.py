"""SpzkServer — a resident ``spzk serve`` process as a context manager.

    with SpzkServer(jobs=1) as srv:
        res = srv.run(["verify", "--nizk", "c.zkif", "c.inp.zkif", "c.wit.zkif"], cwd=workdir)     # a CompletedProcess
        info = srv.status()                                                                         # the status line, parsed

The server is started with ``--with-parent`` (it ends when this process does) and ``--idle-exit``; requests go through the
``spzk-client`` binary with ``SPZK_SERVER`` set, so what a caller gets is what a caller of ``spzk`` gets: stdout, stderr and the exit
status.  Every wait has a time limit.  A server that ended by a signal, with a non-zero status or at a time limit is recorded in
``abnormal_end`` (None otherwise) and refuses further requests.
"""
import json
import os
import select
import shutil
import subprocess
import tempfile
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
SPZK = os.path.join(_HERE, "spzk")
SPZK_CLIENT = os.path.join(_HERE, "spzk-client")


class SpzkServerError(RuntimeError):
    pass


class SpzkServer:
    def __init__(self, socket_path=None, jobs=1, idle_exit=60, env=None, start_timeout=60.0):
        self._own_dir = None
        if socket_path is None:                                    # a short path: sun_path holds 107 bytes
            self._own_dir = tempfile.mkdtemp(prefix="spzk-")
            socket_path = os.path.join(self._own_dir, "s")
        self.socket_path, self.jobs, self.idle_exit = socket_path, jobs, idle_exit
        self.env = dict(os.environ if env is None else env)
        self.start_timeout = start_timeout
        self.proc, self.abnormal_end, self.returncode, self.stderr_text = None, None, None, ""

    # ---- lifetime
    def start(self):
        argv = [SPZK, "serve", "--socket", self.socket_path, "--jobs", str(self.jobs), "--idle-exit", str(self.idle_exit), "--with-parent"]
        self.proc = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=self.env)
        deadline, line = time.monotonic() + self.start_timeout, b""
        fd = self.proc.stdout.fileno()
        while not line.endswith(b"\n"):
            left = deadline - time.monotonic()
            if left <= 0 or not select.select([fd], [], [], left)[0]:
                self._end(kill=True, why="no ready line within %.0f s" % self.start_timeout)
                raise SpzkServerError(self.abnormal_end)
            chunk = os.read(fd, 1)
            if not chunk:                                          # it ended before it was ready
                self._end(kill=False, why=None)
                raise SpzkServerError("spzk serve ended at start (status %s): %s" % (self.returncode, self.stderr_text.strip()))
            line += chunk
        if line.decode().strip() != "spzk serve: ready " + self.socket_path:
            self._end(kill=True, why="unexpected first line %r" % line)
            raise SpzkServerError(self.abnormal_end)
        return self

    def _end(self, kill, why, timeout=30.0):
        """collects the process; an end by a signal, a non-zero status or a time limit is recorded"""
        if self.proc is None:
            return
        if kill:
            self.proc.kill()
        try:
            _, err = self.proc.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            self.proc.kill()
            _, err = self.proc.communicate()
            why = why or "did not end within %.0f s" % timeout
        self.stderr_text = (err or b"").decode(errors="replace")
        self.returncode, self.proc = self.proc.returncode, None
        if why is None and self.returncode != 0:
            why = "ended by signal %d" % -self.returncode if self.returncode < 0 else "exit status %d" % self.returncode
        if why is not None:
            self.abnormal_end = "spzk serve: " + why
        if self._own_dir:
            shutil.rmtree(self._own_dir, ignore_errors=True)
            self._own_dir = None

    def _alive(self):
        if self.proc is not None and self.proc.poll() is not None:
            self._end(kill=False, why=None)
            if self.abnormal_end is None:
                self.abnormal_end = "spzk serve: ended by itself (status 0) while in use"
        if self.proc is None:
            raise SpzkServerError(self.abnormal_end or "spzk serve is not running")

    def _client(self, argv, cwd, timeout):
        self._alive()
        env = dict(self.env, SPZK_SERVER=self.socket_path)
        try:
            return subprocess.run([SPZK_CLIENT] + list(argv), cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self._end(kill=True, why="a request was not answered within %.0f s" % timeout)
            raise SpzkServerError(self.abnormal_end)

    # ---- requests
    def run(self, argv, cwd=None, timeout=120.0):
        """one spzk command line (without argv[0]) through the server; relative paths resolve against cwd"""
        return self._client(argv, cwd, timeout)

    def status(self, timeout=30.0):
        res = self._client(["--server-status"], None, timeout)
        if res.returncode != 0:
            raise SpzkServerError("status request failed: " + res.stderr.strip())
        return json.loads(res.stdout)

    def close(self, timeout=60.0):
        """asks the server to finish and exit; returns its exit status"""
        if self.proc is None:
            return self.returncode
        if self.proc.poll() is None:
            try:
                subprocess.run([SPZK_CLIENT, "--server-shutdown"], env=dict(self.env, SPZK_SERVER=self.socket_path), capture_output=True, timeout=timeout)
            except subprocess.TimeoutExpired:
                self._end(kill=True, why="the shutdown request was not answered within %.0f s" % timeout)
                return self.returncode
        self._end(kill=False, why=None, timeout=timeout)
        return self.returncode

    def __enter__(self):
        return self.start()

    def __exit__(self, *exc):
        self.close()
        return False
