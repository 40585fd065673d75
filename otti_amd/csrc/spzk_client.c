/* spzk-client — `spzk`'s command line in front of a resident `spzk serve` process.
 *
 * Takes spzk's argv unchanged, sends it with the working directory to the server whose socket SPZK_SERVER names (wire format:
 * serve_proto.h), copies the answer's stdout and stderr to its own and exits with the answer's status.  Plain C, and linked against
 * neither libottispartan nor the HIP runtime: the dynamic loader has nothing to map, which is the point — a one-shot `spzk` spends most of
 * its life there.
 *
 * Fallback: SPZK_SERVER unset, nothing accepting there, or a command line beyond the wire format's bounds — the real binary next to this
 * one (spzk-mi355x, else spzk) is started as a CHILD process with the same argv, waited for, and its status returned.  The client never
 * replaces itself.  Once a request has been sent, a server that goes away is an error (status 1): the request may have been half done.
 *
 *   spzk-client --server-status      one JSON line about the server      (these two talk to the server only:
 *   spzk-client --server-shutdown    ask it to finish and exit            status 1 when none answers) */
#define _GNU_SOURCE
#include <errno.h>
#include <limits.h>
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <sys/wait.h>
#include <unistd.h>
#include "serve_proto.h"

extern char **environ;

static int read_all(int fd, uint8_t *p, size_t n) { while (n) { const ssize_t r = recv(fd, p, n, 0); if (r <= 0) { if (r < 0 && errno == EINTR) continue; return 0; } p += r; n -= (size_t)r; } return 1; }
static int write_all(int fd, const uint8_t *p, size_t n) { while (n) { const ssize_t r = send(fd, p, n, MSG_NOSIGNAL); if (r <= 0) { if (r < 0 && errno == EINTR) continue; return 0; } p += r; n -= (size_t)r; } return 1; }
static int write_fd(int fd, const uint8_t *p, size_t n) { while (n) { const ssize_t r = write(fd, p, n); if (r <= 0) { if (r < 0 && errno == EINTR) continue; return 0; } p += r; n -= (size_t)r; } return 1; }

static int connect_server(void) {
    const char *path = getenv("SPZK_SERVER");
    struct sockaddr_un addr; int fd;
    if (!path || !*path || strlen(path) >= sizeof addr.sun_path) return -1;
    memset(&addr, 0, sizeof addr); addr.sun_family = AF_UNIX; strcpy(addr.sun_path, path);
    fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (fd < 0) return -1;
    if (connect(fd, (struct sockaddr *)&addr, sizeof addr) != 0) { close(fd); return -1; }
    return fd;
}

/* the real binary beside this one, started as a child */
static int run_child(char **argv) {
    char self[PATH_MAX], cand[PATH_MAX + 16]; struct stat me, st; const char *names[2] = {"spzk-mi355x", "spzk"}; char *slash; int i, status; pid_t pid;
    const ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
    if (n <= 0) { fprintf(stderr, "spzk-client: cannot find its own path\n"); return 1; }
    self[n] = 0;
    if (stat(self, &me) != 0) memset(&me, 0, sizeof me);
    slash = strrchr(self, '/'); if (!slash) return 1;
    slash[1] = 0;
    for (i = 0; i < 2; i++) {
        snprintf(cand, sizeof cand, "%s%s", self, names[i]);
        if (stat(cand, &st) != 0 || !S_ISREG(st.st_mode) || access(cand, X_OK) != 0) continue;
        if (st.st_dev == me.st_dev && st.st_ino == me.st_ino) continue;       /* installed under that name: this is the client itself */
        if (posix_spawn(&pid, cand, NULL, NULL, argv, environ) != 0) { fprintf(stderr, "spzk-client: cannot start %s: %s\n", cand, strerror(errno)); return 1; }
        while (waitpid(pid, &status, 0) < 0) if (errno != EINTR) return 1;
        return WIFEXITED(status) ? WEXITSTATUS(status) : 128 + (WIFSIGNALED(status) ? WTERMSIG(status) : 0);
    }
    fprintf(stderr, "spzk-client: no server at SPZK_SERVER and no spzk-mi355x or spzk beside %s\n", self);
    return 1;
}

/* copies the answer's frames to stdout and stderr; returns the status of its last frame */
static int relay(int fd) {
    static uint8_t payload[SPZK_MAX_FRAME];
    for (;;) {
        uint8_t h[SPZK_FRAME_HEADER_BYTES], tag; uint32_t len;
        if (!read_all(fd, h, sizeof h) || spzk_frame_header_parse(h, sizeof h, &tag, &len) != SPZK_OK || (len && !read_all(fd, payload, len))) {
            fprintf(stderr, "spzk-client: the server went away before the request was answered\n"); return 1;
        }
        if (tag == SPZK_TAG_EXIT) return (int)spzk_exit_status(payload);
        (void)write_fd(tag == SPZK_TAG_STDOUT ? 1 : 2, payload, len);
    }
}

int main(int argc, char **argv) {
    static uint8_t req[SPZK_MAX_REQUEST];
    char cwd[PATH_MAX]; size_t n = 0; int fd, status; uint16_t kind = SPZK_KIND_RUN;
    if (argc == 2 && !strcmp(argv[1], "--server-status")) kind = SPZK_KIND_STATUS;
    else if (argc == 2 && !strcmp(argv[1], "--server-shutdown")) kind = SPZK_KIND_SHUTDOWN;
    if (kind != SPZK_KIND_RUN) {
        fd = connect_server();
        if (fd < 0) { fprintf(stderr, "spzk-client: no server answers at SPZK_SERVER%s\n", getenv("SPZK_SERVER") ? "" : " (unset)"); return 1; }
        if (spzk_request_encode(req, sizeof req, kind, "", 0, NULL, &n) != SPZK_OK || !write_all(fd, req, n)) { close(fd); return 1; }
        status = relay(fd); close(fd);
        return status;
    }
    if (!getcwd(cwd, sizeof cwd) || strlen(cwd) > SPZK_MAX_STR) return run_child(argv);
    if (spzk_request_encode(req, sizeof req, SPZK_KIND_RUN, cwd, argc - 1, (const char *const *)(argv + 1), &n) != SPZK_OK) return run_child(argv);
    fd = connect_server();
    if (fd < 0) return run_child(argv);
    if (!write_all(fd, req, n)) { close(fd); fprintf(stderr, "spzk-client: the server went away while the request was sent\n"); return 1; }
    status = relay(fd); close(fd);
    return status & 0xff;
}
