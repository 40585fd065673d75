// Host check of otti_amd/csrc/serve_proto.h (the wire format of `spzk serve`): round trips, every bound at its edge and one past it,
// truncation at every byte of a valid request, and 10,000 seeded mutations.  Every buffer handed to a parser is a heap block of exactly
// the length announced, so a read past it is what the address sanitizer build of this program reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "serve_proto.h"

static int failures = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { failures++; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// parses a copy of exactly n bytes (the sanitizer's red zone begins right behind it)
static int parse_exact(const uint8_t *p, size_t n, spzk_request *rq, std::vector<std::string> *args = nullptr, std::string *cwd = nullptr) {
    uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(copy, p, n);
    spzk_request local; if (!rq) rq = &local;
    const int rc = spzk_request_parse(copy, n, rq);
    if (rc == SPZK_OK) {
        if (cwd) cwd->assign((const char *)rq->cwd.p, rq->cwd.len);
        if (args) { args->clear(); for (uint32_t i = 0; i < rq->argc; i++) args->emplace_back((const char *)rq->argv[i].p, rq->argv[i].len); }
    }
    free(copy);
    return rc;
}
static std::vector<uint8_t> encode(uint16_t kind, const std::string &cwd, const std::vector<std::string> &args, int *rc_out = nullptr) {
    std::vector<const char *> av; for (auto &a : args) av.push_back(a.c_str());
    std::vector<uint8_t> buf(SPZK_MAX_REQUEST); size_t n = 0;
    const int rc = spzk_request_encode(buf.data(), buf.size(), kind, cwd.c_str(), (int)av.size(), av.data(), &n);
    if (rc_out) *rc_out = rc;
    buf.resize(rc == SPZK_OK ? n : 0);
    return buf;
}
static void put32(std::vector<uint8_t> &b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }
static void put_str(std::vector<uint8_t> &b, const std::string &s) { put32(b, (uint32_t)s.size()); b.insert(b.end(), s.begin(), s.end()); }
// a request written by hand, so that bounds the encoder refuses can still be put on the wire
static std::vector<uint8_t> raw_request(uint16_t kind, const std::string &cwd, uint32_t argc_field, const std::vector<std::string> &args, int32_t body_len_override = -1) {
    std::vector<uint8_t> body; put_str(body, cwd); put32(body, argc_field); for (auto &a : args) put_str(body, a);
    std::vector<uint8_t> b; put32(b, SPZK_MAGIC); b.push_back(SPZK_PROTO_VERSION); b.push_back(0); b.push_back((uint8_t)kind); b.push_back((uint8_t)(kind >> 8));
    put32(b, body_len_override >= 0 ? (uint32_t)body_len_override : (uint32_t)body.size());
    b.insert(b.end(), body.begin(), body.end());
    return b;
}

int main() {
    // ---- round trips
    const std::vector<std::string> argv = {"verify", "--nizk", "c.zkif", "i.inp.zkif", "w.wit.zkif", "--seed", std::string(64, 'a'), "", "--label", "caf\xc3\xa9"};
    {
        int rc; std::vector<uint8_t> b = encode(SPZK_KIND_RUN, "/work/dir", argv, &rc); CHECK(rc == SPZK_OK);
        spzk_request rq; std::vector<std::string> got; std::string cwd;
        CHECK(parse_exact(b.data(), b.size(), &rq, &got, &cwd) == SPZK_OK);
        CHECK(rq.kind == SPZK_KIND_RUN && cwd == "/work/dir" && got == argv);
        b = encode(SPZK_KIND_RUN, "", {}, &rc); CHECK(rc == SPZK_OK && b.size() == SPZK_HEADER_BYTES + 8);
        CHECK(parse_exact(b.data(), b.size(), &rq, &got, &cwd) == SPZK_OK && got.empty() && cwd.empty());
        for (uint16_t kind : {(uint16_t)SPZK_KIND_STATUS, (uint16_t)SPZK_KIND_SHUTDOWN}) {
            b = encode(kind, "ignored", argv, &rc); CHECK(rc == SPZK_OK && b.size() == SPZK_HEADER_BYTES);
            CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_OK && rq.kind == kind && rq.argc == 0);
            b.push_back(0); b[8] = 1; CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_E_TRAILING);      // a body where none belongs
        }
        // frames
        uint8_t fh[SPZK_FRAME_HEADER_BYTES] = {0}; uint8_t tag = 0; uint32_t len = 0;
        for (uint8_t t : {(uint8_t)SPZK_TAG_STDOUT, (uint8_t)SPZK_TAG_STDERR})
            for (uint32_t l : {0u, 1u, (uint32_t)SPZK_MAX_FRAME}) { CHECK(spzk_frame_header_encode(fh, t, l) == SPZK_OK); CHECK(spzk_frame_header_parse(fh, sizeof fh, &tag, &len) == SPZK_OK && tag == t && len == l); }
        CHECK(spzk_frame_header_encode(fh, SPZK_TAG_STDOUT, SPZK_MAX_FRAME + 1) == SPZK_E_TOO_LONG);
        CHECK(spzk_frame_header_encode(fh, 0, 0) == SPZK_E_TAG && spzk_frame_header_encode(fh, 4, 0) == SPZK_E_TAG);
        CHECK(spzk_frame_header_encode(fh, SPZK_TAG_EXIT, 5) == SPZK_E_TOO_LONG);
        for (int32_t st : {0, 1, 2, 255, -20, INT32_MIN, INT32_MAX}) {
            uint8_t ef[SPZK_FRAME_HEADER_BYTES + 4]; spzk_exit_frame(ef, st);
            CHECK(spzk_frame_header_parse(ef, SPZK_FRAME_HEADER_BYTES, &tag, &len) == SPZK_OK && tag == SPZK_TAG_EXIT && len == 4 && spzk_exit_status(ef + SPZK_FRAME_HEADER_BYTES) == st);
        }
        uint8_t bad[SPZK_FRAME_HEADER_BYTES] = {SPZK_TAG_STDOUT, 1, 0, 1, 0};                              // 65537 bytes
        CHECK(spzk_frame_header_parse(bad, sizeof bad, &tag, &len) == SPZK_E_TOO_LONG);
        bad[0] = 9; CHECK(spzk_frame_header_parse(bad, sizeof bad, &tag, &len) == SPZK_E_TAG);
        bad[0] = SPZK_TAG_EXIT; bad[1] = 3; bad[3] = 0; CHECK(spzk_frame_header_parse(bad, sizeof bad, &tag, &len) == SPZK_E_TOO_LONG);
        for (size_t n = 0; n < SPZK_FRAME_HEADER_BYTES; n++) CHECK(spzk_frame_header_parse(fh, n, &tag, &len) == SPZK_E_TRUNCATED);
    }
    // ---- bounds, at the edge and one past it
    {
        int rc; spzk_request rq; std::vector<std::string> got;
        std::vector<std::string> a64(SPZK_MAX_ARGS, "x"), a65(SPZK_MAX_ARGS + 1, "x");
        std::vector<uint8_t> b = encode(SPZK_KIND_RUN, "/", a64, &rc); CHECK(rc == SPZK_OK);
        CHECK(parse_exact(b.data(), b.size(), &rq, &got) == SPZK_OK && got == a64);
        encode(SPZK_KIND_RUN, "/", a65, &rc); CHECK(rc == SPZK_E_TOO_LONG);
        b = raw_request(SPZK_KIND_RUN, "/", SPZK_MAX_ARGS + 1, a65); CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_E_TOO_LONG);
        b = raw_request(SPZK_KIND_RUN, "/", 0xffffffffu, {}); CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_E_TOO_LONG);
        const std::string s4096(SPZK_MAX_STR, 'p'), s4097(SPZK_MAX_STR + 1, 'p');
        b = encode(SPZK_KIND_RUN, s4096, {s4096}, &rc); CHECK(rc == SPZK_OK);
        CHECK(parse_exact(b.data(), b.size(), &rq, &got) == SPZK_OK && got.size() == 1 && got[0] == s4096 && rq.cwd.len == SPZK_MAX_STR);
        encode(SPZK_KIND_RUN, "/", {s4097}, &rc); CHECK(rc == SPZK_E_TOO_LONG);
        encode(SPZK_KIND_RUN, s4097, {}, &rc); CHECK(rc == SPZK_E_TOO_LONG);
        b = raw_request(SPZK_KIND_RUN, "/", 1, {s4097}); CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_E_TOO_LONG);
        b = raw_request(SPZK_KIND_RUN, s4097, 0, {}); CHECK(parse_exact(b.data(), b.size(), &rq) == SPZK_E_TOO_LONG);
        // the request as a whole: 64 KiB exactly, then one byte more.  15 strings of 4096 and a last one that fills the rest
        const size_t fixed = SPZK_HEADER_BYTES + 4 + 1 + 4 + 16 * 4;                                     // header, cwd "/", argc, 16 length words
        std::vector<std::string> big(15, s4096); big.push_back(std::string(SPZK_MAX_REQUEST - fixed - 15 * SPZK_MAX_STR, 'q'));
        b = encode(SPZK_KIND_RUN, "/", big, &rc); CHECK(rc == SPZK_OK && b.size() == SPZK_MAX_REQUEST);
        CHECK(parse_exact(b.data(), b.size(), &rq, &got) == SPZK_OK && got == big);
        big.back() += 'q';
        encode(SPZK_KIND_RUN, "/", big, &rc); CHECK(rc == SPZK_E_TOO_LONG);
        b = raw_request(SPZK_KIND_RUN, "/", 16, big); CHECK(b.size() == SPZK_MAX_REQUEST + 1 && parse_exact(b.data(), b.size(), &rq) == SPZK_E_TOO_LONG);
        { uint16_t kind; uint32_t bl; CHECK(spzk_header_parse(b.data(), SPZK_HEADER_BYTES, &kind, &bl) == SPZK_E_TOO_LONG); }     // the server stops at the header
        // the encoder's own room
        std::vector<const char *> av = {"verify"}; uint8_t small[SPZK_HEADER_BYTES + 8 + 4 + 6]; size_t n = 0;
        CHECK(spzk_request_encode(small, sizeof small, SPZK_KIND_RUN, "", 1, av.data(), &n) == SPZK_OK && n == sizeof small);
        CHECK(spzk_request_encode(small, sizeof small - 1, SPZK_KIND_RUN, "", 1, av.data(), &n) == SPZK_E_ROOM);
        CHECK(spzk_request_encode(small, SPZK_HEADER_BYTES - 1, SPZK_KIND_STATUS, "", 0, nullptr, &n) == SPZK_E_ROOM);
        // header fields
        b = encode(SPZK_KIND_RUN, "/w", argv, &rc);
        std::vector<uint8_t> m = b; m[0] ^= 1; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_MAGIC);
        m = b; m[4] = 2; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_VERSION);
        m = b; m[5] = 1; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_VERSION);
        m = b; m[6] = 0; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_KIND);
        m = b; m[6] = 4; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_KIND);
        m = b; m[7] = 1; CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_KIND);
        m = b; m.push_back('x'); CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_TRAILING);
        m = raw_request(SPZK_KIND_RUN, "/w", 1, {"a", "b"}); CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_TRAILING);          // a string more than argc says
        m = raw_request(SPZK_KIND_RUN, "/w", 3, {"a", "b"}); CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_TRUNCATED);         // a string fewer
        m = raw_request(SPZK_KIND_RUN, "/w", 1, {std::string("a\0b", 3)}); CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_NUL);
        m = raw_request(SPZK_KIND_RUN, std::string("\0", 1), 0, {}); CHECK(parse_exact(m.data(), m.size(), &rq) == SPZK_E_NUL);
    }
    // ---- truncation at every byte of a valid request: never OK, never a read past the end
    {
        int rc; const std::vector<uint8_t> b = encode(SPZK_KIND_RUN, "/some/where", argv, &rc); CHECK(rc == SPZK_OK);
        int ok = 0;
        for (size_t n = 0; n < b.size(); n++) {
            const int r = parse_exact(b.data(), n, nullptr); if (r == SPZK_OK) ok++;
            if (n >= SPZK_HEADER_BYTES) {                          // as the server reads: the header's own length, then a body cut short
                uint16_t kind = 0; uint32_t bl = 0; CHECK(spzk_header_parse(b.data(), SPZK_HEADER_BYTES, &kind, &bl) == SPZK_OK);
                const size_t bn = n - SPZK_HEADER_BYTES; uint8_t *body = (uint8_t *)malloc(bn ? bn : 1); if (bn) memcpy(body, b.data() + SPZK_HEADER_BYTES, bn);
                spzk_request rq; if (spzk_body_parse(kind, body, (uint32_t)(n - SPZK_HEADER_BYTES), &rq) == SPZK_OK) ok++;
                free(body);
            }
        }
        CHECK(ok == 0);
        CHECK(parse_exact(b.data(), b.size(), nullptr) == SPZK_OK);
    }
    // ---- 10,000 seeded mutations of valid requests: any answer but a crash; an accepted one re-encodes to the same bytes
    {
        uint64_t s = 0x9e3779b97f4a7c15ull; auto rnd = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        int rc; const std::vector<uint8_t> base = encode(SPZK_KIND_RUN, "/some/where", argv, &rc);
        int accepted = 0, refused = 0;
        for (int it = 0; it < 10000; it++) {
            std::vector<uint8_t> m = base;
            const int kind = (int)(rnd() % 5), edits = 1 + (int)(rnd() % 4);
            for (int e = 0; e < edits; e++) {
                const size_t pos = rnd() % m.size();
                if (kind == 0) m[pos] ^= (uint8_t)(1u << (rnd() % 8));
                else if (kind == 1) m[pos] = (uint8_t)rnd();
                else if (kind == 2) m.resize(pos);                                              // cut
                else if (kind == 3) m.insert(m.begin() + pos, (uint8_t)rnd());                  // grow
                else { const size_t at = pos & ~(size_t)3; if (at + 4 <= m.size()) { const uint32_t v = (rnd() & 1) ? 0xffffffffu - (uint32_t)(rnd() % 8) : (uint32_t)(rnd() % 70000); for (int k = 0; k < 4; k++) m[at + k] = (uint8_t)(v >> (8 * k)); } }
                if (m.empty()) break;
            }
            spzk_request rq; std::vector<std::string> got; std::string cwd;
            const int r = parse_exact(m.data(), m.size(), &rq, &got, &cwd);
            if (r == SPZK_OK) {
                accepted++;
                int rc2; const std::vector<uint8_t> again = encode(rq.kind, cwd, got, &rc2);
                CHECK(rc2 == SPZK_OK && again == m);
            } else { refused++; CHECK(r <= SPZK_E_MAGIC && r >= SPZK_E_NUL); }
        }
        CHECK(accepted + refused == 10000 && refused > 5000);
        printf("mutations: %d accepted, %d refused\n", accepted, refused);
    }
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
