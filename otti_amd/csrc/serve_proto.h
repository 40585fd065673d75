/* Wire format of `spzk serve` (spzk_serve.cpp) and `spzk-client` (spzk_client.c), as pure functions over byte buffers: standard library
 * only, valid as C99 and as C++, no I/O, no allocation — so the parser that faces the socket is checked as a host program
 * (tests/serve_proto_check.cpp, plain and under the address and undefined-behaviour sanitizers).  All integers little-endian.
 *
 * Request (client -> server), one per connection:
 *     header, 12 bytes:  magic u32 = "SPZK" | version u16 = 1 | kind u16 | body_len u32
 *     body, body_len bytes, for kind RUN:       cwd string | argc u32 | argc strings      (argv as `spzk` takes it, argv[0] left out)
 *                           for STATUS, SHUTDOWN: empty
 *     string:            len u32 | len bytes, no NUL among them, no terminator
 *   Bounds: argc <= 64; every string <= 4096 bytes; header + body <= 64 KiB; the body is consumed exactly (trailing bytes are an error).
 * Response (server -> client): frames  tag u8 | len u32 | len bytes,  len <= 64 KiB:
 *     tag 1: a piece of the request's stdout;  tag 2: of its stderr;  tag 3: the exit status, len = 4, an i32 — always the last frame.
 * A server that cannot parse a request sends nothing and closes the connection.
 *
 * Every parser reads a byte only after comparing its offset with the length it was given; lengths taken from the wire are validated
 * against the bounds above before they are added to an offset (no sum can wrap: all are far below 2^32). */
#ifndef OTTI_SERVE_PROTO_H
#define OTTI_SERVE_PROTO_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SPZK_MAGIC 0x4b5a5053u /* "SPZK" */
enum { SPZK_PROTO_VERSION = 1 };
enum { SPZK_KIND_RUN = 1, SPZK_KIND_STATUS = 2, SPZK_KIND_SHUTDOWN = 3 };
enum { SPZK_HEADER_BYTES = 12, SPZK_MAX_ARGS = 64, SPZK_MAX_STR = 4096, SPZK_MAX_REQUEST = 65536 };
enum { SPZK_TAG_STDOUT = 1, SPZK_TAG_STDERR = 2, SPZK_TAG_EXIT = 3 };
enum { SPZK_FRAME_HEADER_BYTES = 5, SPZK_MAX_FRAME = 65536 };
enum {
    SPZK_OK = 0,
    SPZK_E_MAGIC = -1,      /* not this protocol */
    SPZK_E_VERSION = -2,
    SPZK_E_KIND = -3,
    SPZK_E_TOO_LONG = -4,   /* a length beyond its bound */
    SPZK_E_TRUNCATED = -5,  /* the buffer ends inside a field */
    SPZK_E_TRAILING = -6,   /* bytes after the last field */
    SPZK_E_NUL = -7,        /* a NUL inside a string */
    SPZK_E_TAG = -8,
    SPZK_E_ROOM = -9        /* encode: the output buffer is too small */
};

/* a string inside the parsed buffer: not terminated, valid as long as the buffer is */
typedef struct spzk_str { const uint8_t *p; uint32_t len; } spzk_str;
typedef struct spzk_request { uint16_t kind; spzk_str cwd; uint32_t argc; spzk_str argv[SPZK_MAX_ARGS]; } spzk_request;

static inline uint32_t spzk_get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline void spzk_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* the 12 header bytes: what kind of request follows and how long its body is */
static inline int spzk_header_parse(const uint8_t *hdr, size_t n, uint16_t *kind, uint32_t *body_len) {
    uint32_t version, k, len;
    if (n < SPZK_HEADER_BYTES) return SPZK_E_TRUNCATED;
    if (spzk_get32(hdr) != SPZK_MAGIC) return SPZK_E_MAGIC;
    version = (uint32_t)hdr[4] | (uint32_t)hdr[5] << 8; k = (uint32_t)hdr[6] | (uint32_t)hdr[7] << 8; len = spzk_get32(hdr + 8);
    if (version != SPZK_PROTO_VERSION) return SPZK_E_VERSION;
    if (k != SPZK_KIND_RUN && k != SPZK_KIND_STATUS && k != SPZK_KIND_SHUTDOWN) return SPZK_E_KIND;
    if (len > SPZK_MAX_REQUEST - SPZK_HEADER_BYTES) return SPZK_E_TOO_LONG;
    *kind = (uint16_t)k; *body_len = len;
    return SPZK_OK;
}

/* one string at body[*off ..): advances *off behind it */
static inline int spzk_str_parse(const uint8_t *body, uint32_t body_len, uint32_t *off, spzk_str *out) {
    uint32_t len;
    if (body_len - *off < 4) return SPZK_E_TRUNCATED;           /* *off <= body_len always holds */
    len = spzk_get32(body + *off); *off += 4;
    if (len > SPZK_MAX_STR) return SPZK_E_TOO_LONG;
    if (body_len - *off < len) return SPZK_E_TRUNCATED;
    if (len && memchr(body + *off, 0, len)) return SPZK_E_NUL;
    out->p = body + *off; out->len = len; *off += len;
    return SPZK_OK;
}

/* the body that goes with a parsed header.  rq's strings point into body. */
static inline int spzk_body_parse(uint16_t kind, const uint8_t *body, uint32_t body_len, spzk_request *rq) {
    uint32_t off = 0, i; int rc;
    if (body_len > SPZK_MAX_REQUEST - SPZK_HEADER_BYTES) return SPZK_E_TOO_LONG;
    rq->kind = kind; rq->cwd.p = 0; rq->cwd.len = 0; rq->argc = 0;
    if (kind == SPZK_KIND_STATUS || kind == SPZK_KIND_SHUTDOWN) return body_len ? SPZK_E_TRAILING : SPZK_OK;
    if (kind != SPZK_KIND_RUN) return SPZK_E_KIND;
    if ((rc = spzk_str_parse(body, body_len, &off, &rq->cwd)) != SPZK_OK) return rc;
    if (body_len - off < 4) return SPZK_E_TRUNCATED;
    i = spzk_get32(body + off); off += 4;
    if (i > SPZK_MAX_ARGS) return SPZK_E_TOO_LONG;
    rq->argc = i;
    for (i = 0; i < rq->argc; i++) if ((rc = spzk_str_parse(body, body_len, &off, &rq->argv[i])) != SPZK_OK) { rq->argc = 0; return rc; }
    if (off != body_len) { rq->argc = 0; return SPZK_E_TRAILING; }
    return SPZK_OK;
}

/* a whole request (header and body) in one buffer of exactly n bytes */
static inline int spzk_request_parse(const uint8_t *buf, size_t n, spzk_request *rq) {
    uint16_t kind; uint32_t body_len; int rc = spzk_header_parse(buf, n, &kind, &body_len);
    if (rc != SPZK_OK) return rc;
    if (n - SPZK_HEADER_BYTES < body_len) return SPZK_E_TRUNCATED;
    if (n - SPZK_HEADER_BYTES > body_len) return SPZK_E_TRAILING;
    return spzk_body_parse(kind, buf + SPZK_HEADER_BYTES, body_len, rq);
}

/* Encodes a request into out[0 .. cap).  argv: argc NUL-terminated strings; cwd: NUL-terminated (both ignored unless kind is RUN).
 * Returns SPZK_OK with *written set, or the bound that was broken (nothing useful is in out then). */
static inline int spzk_request_encode(uint8_t *out, size_t cap, uint16_t kind, const char *cwd, int argc, const char *const *argv, size_t *written) {
    size_t off = SPZK_HEADER_BYTES; int i;
    if (kind != SPZK_KIND_RUN && kind != SPZK_KIND_STATUS && kind != SPZK_KIND_SHUTDOWN) return SPZK_E_KIND;
    if (cap < SPZK_HEADER_BYTES) return SPZK_E_ROOM;
    if (kind == SPZK_KIND_RUN) {
        if (argc < 0 || argc > SPZK_MAX_ARGS) return SPZK_E_TOO_LONG;
        for (i = -1; i < argc; i++) {                            /* -1: the cwd, followed by the count */
            const char *s = i < 0 ? cwd : argv[i]; const size_t len = s ? strlen(s) : 0;
            if (len > SPZK_MAX_STR) return SPZK_E_TOO_LONG;
            if (off + 4 + len + (i < 0 ? 4u : 0u) > SPZK_MAX_REQUEST) return SPZK_E_TOO_LONG;
            if (off + 4 + len + (i < 0 ? 4u : 0u) > cap) return SPZK_E_ROOM;
            spzk_put32(out + off, (uint32_t)len); off += 4;
            if (len) memcpy(out + off, s, len);
            off += len;
            if (i < 0) { spzk_put32(out + off, (uint32_t)argc); off += 4; }
        }
    }
    spzk_put32(out, SPZK_MAGIC);
    out[4] = (uint8_t)SPZK_PROTO_VERSION; out[5] = 0; out[6] = (uint8_t)kind; out[7] = (uint8_t)(kind >> 8);
    spzk_put32(out + 8, (uint32_t)(off - SPZK_HEADER_BYTES));
    *written = off;
    return SPZK_OK;
}

/* response frames */
static inline int spzk_frame_header_encode(uint8_t out[SPZK_FRAME_HEADER_BYTES], uint8_t tag, uint32_t len) {
    if (tag != SPZK_TAG_STDOUT && tag != SPZK_TAG_STDERR && tag != SPZK_TAG_EXIT) return SPZK_E_TAG;
    if (len > SPZK_MAX_FRAME || (tag == SPZK_TAG_EXIT && len != 4)) return SPZK_E_TOO_LONG;
    out[0] = tag; spzk_put32(out + 1, len);
    return SPZK_OK;
}
static inline int spzk_frame_header_parse(const uint8_t *in, size_t n, uint8_t *tag, uint32_t *len) {
    uint32_t l;
    if (n < SPZK_FRAME_HEADER_BYTES) return SPZK_E_TRUNCATED;
    if (in[0] != SPZK_TAG_STDOUT && in[0] != SPZK_TAG_STDERR && in[0] != SPZK_TAG_EXIT) return SPZK_E_TAG;
    l = spzk_get32(in + 1);
    if (l > SPZK_MAX_FRAME || (in[0] == SPZK_TAG_EXIT && l != 4)) return SPZK_E_TOO_LONG;
    *tag = in[0]; *len = l;
    return SPZK_OK;
}
static inline void spzk_exit_frame(uint8_t out[SPZK_FRAME_HEADER_BYTES + 4], int32_t status) {
    out[0] = SPZK_TAG_EXIT; spzk_put32(out + 1, 4); spzk_put32(out + SPZK_FRAME_HEADER_BYTES, (uint32_t)status);
}
static inline int32_t spzk_exit_status(const uint8_t payload[4]) { return (int32_t)spzk_get32(payload); }

#endif
