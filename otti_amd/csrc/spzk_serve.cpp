// spzk serve — one process that keeps the HIP context and the generators' device table alive and runs `spzk` requests that arrive on a
// Unix stream socket (wire format: serve_proto.h; the client: spzk_client.c).  A request is the one-shot's argv and the client's working
// directory; the answer is what the one-shot would have printed and its exit status (spzk_run.h).
//
// Generators.  NIZK handles are cached by padded sizes, at most kMaxHandles, least recently used first out.  There is ONE resident window
// table: every NIZKGens takes its points from one stream, so the table of the handle with the most points serves them all
// (otti_gens_adopt_table).  A request that needs no more points than the table has adopts it; one that needs more lets every cached handle
// drop its reference (the small table is freed first: two wide tables do not fit one card), builds its own and has the others adopt that.
// Replacement runs with no proof in flight: requests hold the table gate shared from the moment they get their handle to their end, and
// whoever changes which table a handle holds has it exclusively.  SNARK generators share nothing: the most recent set is kept.
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <stdlib.h>
#include <string.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "serve_proto.h"
#include "spzk_run.h"
#include "spzk_serve.h"

namespace {

constexpr size_t kMaxHandles = 8;
constexpr int kMaxJobs = 8;
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// readers and one writer, not tied to threads (a request takes it on the thread that fetches its generators and gives it back on its worker);
// a waiting writer holds new readers back
struct Gate {
    std::mutex m; std::condition_variable cv; int readers = 0, writers_waiting = 0; bool writer = false;
    void lock_shared() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !writer && !writers_waiting; }); readers++; }
    void unlock_shared() { std::lock_guard<std::mutex> l(m); if (--readers == 0) cv.notify_all(); }
    void lock() { std::unique_lock<std::mutex> l(m); writers_waiting++; cv.wait(l, [&] { return !writer && readers == 0; }); writers_waiting--; writer = true; }
    void unlock() { std::lock_guard<std::mutex> l(m); writer = false; cv.notify_all(); }
};

uint64_t next_pow2(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }
// stream points a NIZKGens of these sizes has: R + 2, at least 5, R = 2^ceil(log2(padded vars) / 2) (spartan_host.cpp gens_new).  Only ranks
// handles: otti_gens_adopt_table compares the real numbers and refuses a donor that is too short.
size_t gens_points(uint64_t nv, uint64_t ni) {
    const uint64_t nvp = next_pow2(std::max<uint64_t>(nv, ni + 1)); int ell = 0; while (((uint64_t)1 << ell) < nvp) ell++;
    return std::max<size_t>(((size_t)1 << (ell - ell / 2)) + 2, 5);
}
struct GensEntry {
    uint64_t key[3]; otti_gens *g = nullptr; size_t points = 0;
    uint64_t table_gen = 0;                                       // which resident table it holds (0: none); written with the gate held exclusively
    ~GensEntry() { otti_gens_free(g); }
};
struct SnarkEntry { uint64_t key[4]; otti_snark_gens *g = nullptr; ~SnarkEntry() { otti_snark_gens_free(g); } };

struct Server {
    std::mutex mu;                                                // the lists below
    std::list<std::shared_ptr<GensEntry>> lru;                    // most recently used first
    std::shared_ptr<SnarkEntry> snark;
    Gate gate;
    std::shared_ptr<GensEntry> resident; uint64_t table_gen = 0;  // whose table everyone holds; written with the gate held exclusively
    std::atomic<uint64_t> served{0}, tables_built{0}, adoptions{0};
    // connections
    struct Conn { int fd; double t_accept; };
    std::mutex qm; std::condition_variable qcv; std::deque<Conn> queue; bool stopping = false; int in_flight = 0; double last_activity = 0;
    int jobs = 1, warmed = 0;
};

// One request's view of the cache: lends handles that live until it is destroyed
struct RequestGens : GensProvider {
    Server &S; std::shared_ptr<GensEntry> entry; std::shared_ptr<SnarkEntry> snark; bool holding = false, cached = false; const char *table = "none";
    explicit RequestGens(Server &s) : S(s) {}
    ~RequestGens() override { if (holding) S.gate.unlock_shared(); }
    const char *gens_word() const override { return cached ? "cached" : "built"; }
    const char *table_word() const override { return table; }

    std::shared_ptr<GensEntry> find(const uint64_t key[3]) {     // S.mu held
        for (auto it = S.lru.begin(); it != S.lru.end(); ++it)
            if (!memcmp((*it)->key, key, sizeof (*it)->key)) { S.lru.splice(S.lru.begin(), S.lru, it); return S.lru.front(); }
        return nullptr;
    }
    int nizk_gens(uint64_t nc, uint64_t nv, uint64_t ni, otti_gens **out) override {
        const uint64_t key[3] = {next_pow2(nc), next_pow2(std::max<uint64_t>(nv, ni + 1)), ni};
        { std::lock_guard<std::mutex> l(S.mu); entry = find(key); }
        cached = entry != nullptr;
        if (!entry) {
            auto e = std::make_shared<GensEntry>(); memcpy(e->key, key, sizeof key); e->points = gens_points(nv, ni);
            const int rc = otti_gens_new(nc, nv, ni, &e->g); if (rc) return rc;
            std::lock_guard<std::mutex> l(S.mu);
            entry = find(key);                                    // another worker made the same meanwhile: that one stays
            if (!entry) { S.lru.push_front(e); entry = e; while (S.lru.size() > kMaxHandles) S.lru.pop_back(); }
        }
        S.gate.lock_shared(); holding = true;
        if (entry->table_gen) table = entry == S.resident ? "own" : "adopted";
        *out = entry->g;
        return OTTI_OK;
    }
    // gate held exclusively
    int make_table() {
        if (S.resident && S.resident->points >= entry->points) {
            if (entry->table_gen != S.table_gen) {
                const int rc = otti_gens_adopt_table(entry->g, S.resident->g); if (rc) return rc;
                entry->table_gen = S.table_gen; S.adoptions++;
            }
            table = entry == S.resident ? "own" : "adopted";
            return OTTI_OK;
        }
        std::vector<std::shared_ptr<GensEntry>> all;
        { std::lock_guard<std::mutex> l(S.mu); all.assign(S.lru.begin(), S.lru.end()); }
        if (S.resident && std::find(all.begin(), all.end(), S.resident) == all.end()) all.push_back(S.resident);
        if (std::find(all.begin(), all.end(), entry) == all.end()) all.push_back(entry);
        for (auto &e : all) { (void)otti_gens_release_device(e->g); e->table_gen = 0; }
        S.resident = nullptr;
        const int rc = otti_prepare_device(nullptr, entry->g); if (rc) return rc;
        S.resident = entry; entry->table_gen = ++S.table_gen; S.tables_built++;
        for (auto &e : all)                                       // a handle with MORE points (cached by a request that needed no table) keeps none: it becomes the next resident when it proves
            if (e != entry && e->points <= entry->points && otti_gens_adopt_table(e->g, entry->g) == OTTI_OK) { e->table_gen = S.table_gen; S.adoptions++; }
        table = "built";
        return OTTI_OK;
    }
    int prepare(otti_instance *inst, otti_gens *) override {
        int rc = otti_prepare_device(inst, nullptr); if (rc) return rc;      // without a device: the one-shot's own failure
        if (S.resident && entry->table_gen == S.table_gen && S.resident->points >= entry->points) { table = entry == S.resident ? "own" : "adopted"; return OTTI_OK; }
        S.gate.unlock_shared(); holding = false;
        S.gate.lock(); rc = make_table(); S.gate.unlock();
        S.gate.lock_shared(); holding = true;                     // (a replacement in between re-adopts every cached handle: the handle's table is valid either way)
        return rc;
    }
    int snark_gens(uint64_t nc, uint64_t nv, uint64_t ni, uint64_t nops, otti_snark_gens **out) override {
        const uint64_t key[4] = {nc, nv, ni, nops};
        { std::lock_guard<std::mutex> l(S.mu); if (S.snark && !memcmp(S.snark->key, key, sizeof key)) snark = S.snark; }
        if (!snark) {
            auto e = std::make_shared<SnarkEntry>(); memcpy(e->key, key, sizeof key);
            const int rc = otti_snark_gens_new(nc, nv, ni, nops, &e->g); if (rc) return rc;
            std::lock_guard<std::mutex> l(S.mu); S.snark = e; snark = e;      // the set it replaces goes with its last user
        }
        *out = snark->g;
        return OTTI_OK;
    }
};

// ---- socket helpers
bool read_all(int fd, uint8_t *p, size_t n) { while (n) { const ssize_t r = recv(fd, p, n, 0); if (r <= 0) { if (r < 0 && errno == EINTR) continue; return false; } p += r; n -= (size_t)r; } return true; }
bool write_all(int fd, const uint8_t *p, size_t n) { while (n) { const ssize_t r = send(fd, p, n, MSG_NOSIGNAL); if (r <= 0) { if (r < 0 && errno == EINTR) continue; return false; } p += r; n -= (size_t)r; } return true; }
bool send_stream(int fd, uint8_t tag, const char *p, size_t n) {
    while (n) {
        const uint32_t len = (uint32_t)std::min<size_t>(n, SPZK_MAX_FRAME); uint8_t h[SPZK_FRAME_HEADER_BYTES];
        if (spzk_frame_header_encode(h, tag, len) != SPZK_OK || !write_all(fd, h, sizeof h) || !write_all(fd, (const uint8_t *)p, len)) return false;
        p += len; n -= len;
    }
    return true;
}
bool send_answer(int fd, const char *out, size_t nout, const char *err, size_t nerr, int status) {
    uint8_t ef[SPZK_FRAME_HEADER_BYTES + 4]; spzk_exit_frame(ef, status);
    return send_stream(fd, SPZK_TAG_STDOUT, out, nout) && send_stream(fd, SPZK_TAG_STDERR, err, nerr) && write_all(fd, ef, sizeof ef);
}

int g_wake[2] = {-1, -1};
void on_signal(int) { const char c = 's'; (void)!write(g_wake[1], &c, 1); }
void request_stop() { const char c = 'q'; (void)!write(g_wake[1], &c, 1); }

std::string status_json(Server &S) {
    size_t handles; { std::lock_guard<std::mutex> l(S.mu); handles = S.lru.size(); }
    uint32_t c = 0; uint64_t bytes = 0; size_t bases = 0;
    S.gate.lock_shared();
    if (S.resident) { (void)otti_gens_table_info(S.resident->g, &c, &bytes); bases = S.resident->points; }
    S.gate.unlock_shared();
    char buf[512];
    snprintf(buf, sizeof buf, "{\"requests_served\": %llu, \"handles_cached\": %zu, \"table\": {\"c\": %u, \"bytes\": %llu, \"bases\": %zu}, \"tables_built\": %llu, \"adoptions\": %llu, "
             "\"jobs\": %d, \"devices\": %d}\n", (unsigned long long)S.served.load(), handles, c, (unsigned long long)bytes, bases, (unsigned long long)S.tables_built.load(),
             (unsigned long long)S.adoptions.load(), S.jobs, (int)otti_device_count());
    return buf;
}

void handle(Server &S, const Server::Conn &conn) {
    const int fd = conn.fd;
    struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
    struct ucred cred; socklen_t cl = sizeof cred;
    if (getsockopt(fd, SOL_SOCKET, SO_PEERCRED, &cred, &cl) != 0 || cred.uid != geteuid()) return;       // another user's process: not served
    const struct timeval rt = {10, 0}, st = {60, 0};             // a client that stops talking does not hold a worker
    (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &rt, sizeof rt); (void)setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &st, sizeof st);
    uint8_t hdr[SPZK_HEADER_BYTES]; uint16_t kind; uint32_t body_len;
    if (!read_all(fd, hdr, sizeof hdr) || spzk_header_parse(hdr, sizeof hdr, &kind, &body_len) != SPZK_OK) return;   // malformed: nothing is answered
    std::vector<uint8_t> body(body_len ? body_len : 1);
    if (body_len && !read_all(fd, body.data(), body_len)) return;
    spzk_request rq;
    if (spzk_body_parse(kind, body.data(), body_len, &rq) != SPZK_OK) return;
    if (kind == SPZK_KIND_STATUS) { const std::string j = status_json(S); (void)send_answer(fd, j.data(), j.size(), "", 0, 0); return; }
    if (kind == SPZK_KIND_SHUTDOWN) { const char *m = "spzk serve: shutting down\n"; (void)send_answer(fd, m, strlen(m), "", 0, 0); request_stop(); return; }
    std::vector<std::string> args; args.emplace_back("spzk");
    for (uint32_t i = 0; i < rq.argc; i++) args.emplace_back((const char *)rq.argv[i].p, rq.argv[i].len);
    const std::string cwd((const char *)rq.cwd.p, rq.cwd.len);
    std::vector<char *> argv; for (auto &a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    char *obuf = nullptr, *ebuf = nullptr; size_t on = 0, en = 0;
    FILE *out = open_memstream(&obuf, &on), *err = open_memstream(&ebuf, &en);
    int status = 1;
    auto answer = [&] {                                          // once: when the request's last line is printed, ahead of its frees
        if (out) fclose(out);
        if (err) fclose(err);
        out = err = nullptr;
        S.served++;
        (void)send_answer(fd, obuf ? obuf : "", obuf ? on : 0, ebuf ? ebuf : "", ebuf ? en : 0, status);
        free(obuf); free(ebuf);
    };
    if (!out || !err) { answer(); return; }
    if (args.size() > 1 && args[1] == "serve") { fprintf(err, "spzk serve: a server does not start servers\n"); status = 2; answer(); return; }
    std::vector<std::function<void()>> frees;
    {
        RequestGens gens(S);                                     // gives the table gate back at the end of this block
        const RunEnv E{out, err, cwd.empty() ? nullptr : cwd.c_str(), &gens, true, now_ms() - conn.t_accept, &frees, 0.0};
        try { status = spzk_run((int)args.size(), argv.data(), E); }
        catch (const std::exception &e) { fprintf(err, "spzk serve: request failed: %s\n", e.what()); status = 1; }
    }
    answer();
    // what the request made is handed back behind its answer (spzk_run.h RunEnv::after_answer): the client does not wait for it, the worker's next
    // request does (its `queue` time).  Measured and not kept: a thread of its own for this — the frees then ran beside the next request's file
    // parsing and device allocations and slowed both by what they saved (profiles/spzk_serve.md).
    for (auto &f : frees) f();
}

void worker(Server &S) {
    if (otti_device_count() > 0) (void)otti_prepare_device(nullptr, nullptr);      // this thread's device context, ahead of its first request
    { std::lock_guard<std::mutex> l(S.qm); S.warmed++; }
    S.qcv.notify_all();
    for (;;) {
        Server::Conn c;
        {
            std::unique_lock<std::mutex> l(S.qm);
            S.qcv.wait(l, [&] { return S.stopping || !S.queue.empty(); });
            if (S.queue.empty()) return;                         // stopping, and nothing accepted is left unanswered
            c = S.queue.front(); S.queue.pop_front(); S.in_flight++;
        }
        handle(S, c);
        { std::lock_guard<std::mutex> l(S.qm); S.in_flight--; S.last_activity = now_ms(); }
    }
}

int serve_usage() {
    fprintf(stderr, "usage: spzk serve --socket PATH [--jobs N (1 .. %d, default 1)] [--idle-exit SECONDS (default 300; 0: never)] [--with-parent]\n", kMaxJobs);
    return 2;
}

}  // namespace

int spzk_serve_main(int argc, char **argv) {
    const char *path = nullptr; int jobs = 1; double idle_s = 300; bool with_parent = false;
    for (int i = 2; i < argc; i++) {
        if (!strcmp(argv[i], "--socket") && i + 1 < argc) path = argv[++i];
        else if (!strcmp(argv[i], "--jobs") && i + 1 < argc) jobs = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--idle-exit") && i + 1 < argc) idle_s = atof(argv[++i]);
        else if (!strcmp(argv[i], "--with-parent")) with_parent = true;
        else return serve_usage();
    }
    struct sockaddr_un addr; memset(&addr, 0, sizeof addr); addr.sun_family = AF_UNIX;
    if (!path || !*path || jobs < 1 || jobs > kMaxJobs || idle_s < 0) return serve_usage();
    if (strlen(path) >= sizeof addr.sun_path) { fprintf(stderr, "spzk serve: socket path longer than %zu bytes\n", sizeof addr.sun_path - 1); return 1; }
    strcpy(addr.sun_path, path);
    if (with_parent) { prctl(PR_SET_PDEATHSIG, SIGTERM); if (getppid() == 1) return 0; }       // the parent is gone already
    signal(SIGPIPE, SIG_IGN);
    // a live server's socket is left alone; a stale socket file is replaced; anything else under that name is not ours to remove
    struct stat sb;
    if (lstat(path, &sb) == 0) {
        if (!S_ISSOCK(sb.st_mode)) { fprintf(stderr, "spzk serve: %s exists and is not a socket\n", path); return 1; }
        const int probe = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
        const bool live = probe >= 0 && connect(probe, (struct sockaddr *)&addr, sizeof addr) == 0;
        if (probe >= 0) close(probe);
        if (live) { fprintf(stderr, "spzk serve: %s is served by a live server\n", path); return 1; }
        unlink(path);
    }
    const int lfd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    const mode_t old_mask = umask(0177);
    const bool bound = lfd >= 0 && bind(lfd, (struct sockaddr *)&addr, sizeof addr) == 0;
    umask(old_mask);
    if (!bound || chmod(path, 0600) != 0 || listen(lfd, 64) != 0) { fprintf(stderr, "spzk serve: cannot listen on %s: %s\n", path, strerror(errno)); if (bound) unlink(path); return 1; }
    if (pipe2(g_wake, O_CLOEXEC | O_NONBLOCK) != 0) { unlink(path); return 1; }
    struct sigaction sa; memset(&sa, 0, sizeof sa); sa.sa_handler = on_signal; sigaction(SIGTERM, &sa, nullptr); sigaction(SIGINT, &sa, nullptr);

    Server S; S.jobs = jobs; S.last_activity = now_ms();
    std::vector<std::thread> workers;
    for (int i = 0; i < jobs; i++) workers.emplace_back(worker, std::ref(S));
    { std::unique_lock<std::mutex> l(S.qm); S.qcv.wait(l, [&] { return S.warmed == jobs; }); S.last_activity = now_ms(); }
    printf("spzk serve: ready %s\n", path); fflush(stdout);

    for (;;) {
        struct pollfd pf[2] = {{lfd, POLLIN, 0}, {g_wake[0], POLLIN, 0}};
        const int pr = poll(pf, 2, 200);
        if (pr < 0 && errno != EINTR) break;
        if (pr > 0 && (pf[1].revents & POLLIN)) break;           // a signal or a shutdown request
        if (pr > 0 && (pf[0].revents & POLLIN)) {
            const int fd = accept4(lfd, nullptr, nullptr, SOCK_CLOEXEC);
            if (fd >= 0) { { std::lock_guard<std::mutex> l(S.qm); S.queue.push_back({fd, now_ms()}); S.last_activity = now_ms(); } S.qcv.notify_one(); }
            continue;
        }
        if (idle_s > 0) {
            std::lock_guard<std::mutex> l(S.qm);
            if (!S.in_flight && S.queue.empty() && now_ms() - S.last_activity >= idle_s * 1e3) break;
        }
    }
    // the end, whatever began it: no new connections, the accepted ones answered, tables and handles freed, the socket removed
    close(lfd); unlink(path);
    { std::lock_guard<std::mutex> l(S.qm); S.stopping = true; }
    S.qcv.notify_all();
    for (auto &t : workers) t.join();
    { std::lock_guard<std::mutex> l(S.mu); S.lru.clear(); S.snark.reset(); }
    S.resident.reset();
    fflush(stdout); fflush(stderr);
    _exit(0);                                                     // as the one-shot: the HIP runtime's own teardown is skipped, everything of ours is freed
}
