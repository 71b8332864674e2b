// p2_host.h — host API of the specialised two-state engine (p2_host.hip), used by the C-ABI (sg_engine.hip).
// As in gen_host.h: a call reports a caller's error as (return code, msg) and throws on a HIP failure.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/siddhi_gpu.h"

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_OK(x)                                                                                       \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess)                                                                           \
            throw HipError(std::string(#x) + ": " + hipGetErrorString(e_));                             \
    } while (0)

// a caller's error: (return code, msg)
inline int refuse(std::string& msg, int code, const char* text) { return msg = text, code; }

// the query is not a two-state pattern (p2_create, p2_jit_check): it runs on the general engine
struct P2NotTwoState : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// sg_config's sizes with their defaults
inline uint32_t sg_cfg_keys(const sg_config& c) { return c.n_keys ? c.n_keys : 1; }
inline uint32_t sg_cfg_cap(const sg_config& c) { return c.partial_capacity ? c.partial_capacity : 64; }
inline uint32_t sg_cfg_batch(const sg_config& c) { return c.max_batch ? c.max_batch : (1u << 20); }
inline uint64_t sg_cfg_matches(const sg_config& c) {
    return c.match_capacity ? c.match_capacity : (uint64_t)sg_cfg_batch(c) * 4;
}

// the environment's knobs of the advance kernel
struct P2Settings {
    uint32_t reg_slots = 14;  // SGD_REG_SLOTS: partials per key held in registers by the advance kernel (14 against
                              // 12: staged pass 4.5 % faster, fewer keys stopped for the HBM pass, same occupancy —
                              // LDS-bound at three workgroups per CU, where 168 VGPRs are free; 16: slower)
    uint32_t reg_slots_hbm = 16;  // SGD_REG_SLOTS_HBM: the HBM pass's window (the keys the staged pass stopped;
                                  // 24 walks C2_walk 10 % faster but compiles 3.5x slower per query)
    uint32_t stage_override = 0;  // SGD_STAGE_CHUNKS: fixed LDS staging per wave (tests force the HBM path)
};
P2Settings p2_settings_from_env();  // throws std::invalid_argument for a value out of range

struct P2Engine;
// on the calling thread's device (range-checked by the caller); throws P2NotTwoState (before any HIP call or engine
// object), std::invalid_argument, HipError
P2Engine* p2_create(const void* ir, size_t ir_len, const sg_config& cfg, P2Settings set);
void p2_destroy(P2Engine* e);
// the query-specialised kernel source of an IR blob, compiled for one null variant (no device, no engine)
int p2_jit_check(const void* ir, size_t ir_len, uint32_t variant_flags, std::string& text, std::string& msg);
int p2_push(P2Engine* e, const sg_batch* b, std::string& msg);
int p2_poll(P2Engine* e, uint32_t memflags, sg_match_batch* out, std::string& msg);
void p2_release(P2Engine* e);
bool p2_held(const P2Engine* e);
int p2_set_projection(P2Engine* e, const uint32_t* code, uint32_t words, const uint32_t* pc, const uint32_t* len,
                      const uint32_t* types, uint32_t n, const int32_t* part_attr, uint32_t n_streams, std::string& msg);
int p2_get_projection(P2Engine* e, uint32_t mem, sg_projection* out, std::string& msg);
void p2_synchronize(P2Engine* e);  // every queued batch done (both streams), their status blocks taken
void p2_stats(P2Engine* e, sg_stats* out);
std::string p2_describe(const P2Engine* e);
uint64_t p2_min_seq(P2Engine* e);
hipStream_t p2_stream(const P2Engine* e);  // the main stream (a push's reads of its batch join it before the advance)
uint32_t p2_n_keys(const P2Engine* e);
void p2_wait_stream(P2Engine* e, hipStream_t s);
// keys: a device array of n ids already range-checked by the caller
int p2_reset_keys(P2Engine* e, const uint32_t* keys, uint32_t n, std::string& msg);
struct SdDoc;
int p2_state_export(P2Engine* e, SdDoc& d, std::string& msg);
int p2_state_import(P2Engine* e, const SdDoc& d, std::string& msg);

// ---- snapshot / restore: the slab image (p2_host.hip) behind the two-state fields of the C-ABI's SnapHeader --------
struct P2SnapRef {
    uint32_t &K, &cap, &rows, &n_capw, &nullable, &have_base, &n_agg;
    uint64_t &next_seq, &body_bytes;
};
int p2_snapshot(P2Engine* e, P2SnapRef h, std::vector<uint64_t>& body, std::string& msg);  // body_bytes bytes of it
int p2_restore(P2Engine* e, P2SnapRef h, const uint8_t* body, std::string& msg);
