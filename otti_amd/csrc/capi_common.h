// Shared by the translation units of the extern "C" surface (capi.cpp, capi_host.cpp, capi_kernels.cpp).  Private: not installed, not part of the ABI.
#pragma once
#include "device.h"
#include "shard.h"
#include "snark.h"
#include "snark_dev.h"
#include "hosttail.h"
#include "hostifma.h"
#include <atomic>
#include <chrono>
#include "pool.h"

using namespace otti;

struct otti_instance { std::unique_ptr<Instance> I; };
struct otti_gens { std::unique_ptr<Gens> g; };
struct otti_witness { std::unique_ptr<DeviceWitness> w; };
struct otti_snark_gens { std::unique_ptr<SnarkGens> g; };
struct otti_comp_comm { std::unique_ptr<CompComm> c; };

extern thread_local std::string g_last_error;               // ONE object (capi.cpp): otti_last_error reads what an entry of any of the three files wrote
template <class F> int32_t guarded(F &&f) {
    try { g_last_error.clear(); return f(); }
    catch (const Error &e) { g_last_error = e.what(); return e.code; }
    catch (const std::bad_alloc &) { g_last_error = "out of memory"; return OTTI_ERR_INTERNAL; }
    catch (const std::exception &e) { g_last_error = e.what(); return OTTI_ERR_INTERNAL; }
    catch (...) { g_last_error = "unknown error"; return OTTI_ERR_INTERNAL; }
}
inline std::vector<Fr> scalars_from_bytes(const uint8_t *b, size_t n) {
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; i++) if (!fr_from_bytes(v[i], b + 32 * i)) throw Error(OTTI_ERR_INVALID_SCALAR, "non-canonical scalar in assignment");
    return v;
}
inline uint8_t *to_malloc(const std::vector<uint8_t> &v, size_t *len) {
    uint8_t *p = (uint8_t *)malloc(std::max<size_t>(1, v.size())); memcpy(p, v.data(), v.size()); *len = v.size(); return p;
}
inline Fr fr_load(const uint8_t *p) { Fr x; memcpy(x.v, p, 32); return x; }
// the end of every prove entry: the stage timings, if asked for, and the proof in a buffer the caller frees with otti_buf_free
template <class T> int32_t emit_proof(const std::vector<uint8_t> &pf, const T &tm, uint8_t **proof, size_t *proof_len, double *stage_ms) {
    if (stage_ms) memcpy(stage_ms, tm.ms, sizeof tm.ms);
    *proof = to_malloc(pf, proof_len); return OTTI_OK;
}
// a new handle around a freshly made object (every handle struct holds exactly one owning pointer)
template <class H, class T> int32_t adopt(H **out, std::unique_ptr<T> obj) { *out = new H{std::move(obj)}; return OTTI_OK; }
inline void need_shard() { if (!shard_comm()) throw Error(OTTI_ERR_BAD_ARG, "otti_shard_init has not been called"); }
inline void check_witness_dims(const otti_witness *wit, const Instance &I) {
    if (wit->w->z.n != 2 * I.num_vars) throw Error(OTTI_ERR_INVALID_NUM_VARS, "the witness was uploaded for an instance of other dimensions");
}
