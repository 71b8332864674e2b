// sg_engine.hip — the C-ABI (include/siddhi_gpu.h) of the MI355X engine: argument checks, the error channel and the
// dispatch of every entry point over the three backends behind an sg_engine handle:
//   shard  the multi-device fan-out (sg_sharded.cpp), n_devices > 1
//   p2     the specialised two-state engine (p2_host.hip): `[every] e1 -> e2` and `every (e1 -> e2)`
//   gen    the general device engine (gen_host.hip): count, logical, SEQUENCE, absent states, longer chains
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/siddhi_gpu.h"
#include "../../include/siddhi_gpu_ir.h"
#include "gen_engine.h"
#include "gen_host.h"
#include "p2_host.h"
#include "sg_sharded.h"
#include "state_doc.h"
#include "sg_engine.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace

struct sg_engine {
    ShardEngine* shard = nullptr;
    P2Engine* p2 = nullptr;
    GenEngine* gen = nullptr;
    int device = 0;
    sg_config cfg{};
    uint64_t ir_hash = 0;  // FNV-1a of the IR words: a snapshot restores only into the same query
    hipStream_t stream = nullptr;   // the general engine's stream
    hipEvent_t wait_ev = nullptr;   // ... and the event of its sg_wait_stream

    hipStream_t main_stream() const { return gen ? stream : p2_stream(p2); }
    uint32_t n_keys() const { return gen ? sg_cfg_keys(cfg) : p2_n_keys(p2); }

    ~sg_engine() {
        if (!p2 && !stream) return;  // a shard handle, or a creation that failed before its device was checked
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (gen) gen_destroy(gen);
        if (p2) p2_destroy(p2);
        if (wait_ev) (void)hipEventDestroy(wait_ev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// The body of an entry point of a single-device engine, past its argument checks: the calling thread on the engine's
// device, the body's (return code, msg) into sg_last_error, any exception into SG_ERR_DEVICE.
// sg_release_matches and sg_engine_describe do not come through here (they touch no device).
template <class F> int guarded(sg_engine* e, F&& body) {
    try {
        HIP_OK(hipSetDevice(e->device));
        std::string msg;
        const int rc = body(msg);
        return rc == SG_OK ? rc : fail(rc, msg);
    } catch (const std::exception& ex) {
        return fail(SG_ERR_DEVICE, ex.what());
    }
}

}  // namespace

// the other host-side translation units (sg_dict.cpp) report through the same sg_last_error
int sg_set_error(int code, const char* msg) { return fail(code, msg); }

// the multi-device engine (sg_sharded.cpp): the smallest event seq a live partial references (UINT64_MAX: none),
// after every queued batch; and an event recorded behind everything queued so far (its reads of a pushed device
// batch included: the two-state engine's grouping stream joins the main stream before the advance)
uint64_t sg_internal_min_seq(sg_engine* e) {
    HIP_OK(hipSetDevice(e->device));
    return e->gen ? gen_min_seq(e->gen) : p2_min_seq(e->p2);
}
void sg_internal_record(sg_engine* e, hipEvent_t ev) {
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipEventRecord(ev, e->main_stream()));
}

bool sg_internal_keep_heads(sg_engine* e) { return e && e->gen ? gen_keep_timer_heads(e->gen, true) : false; }
void sg_internal_heads(sg_engine* e, std::vector<uint32_t>& keys, std::vector<int64_t>& heads) {
    keys.clear();
    heads.clear();
    if (e && e->gen) gen_timer_heads(e->gen, keys, heads);
}

extern "C" {

const char* sg_last_error(void) { return g_err.c_str(); }
int sg_abi_version(void) { return SG_ABI_VERSION; }

int sg_engine_create(const void* ir, size_t ir_len, const sg_config* cfg, sg_engine** out) {
    if (!ir || !out || !cfg) return fail(SG_ERR_INVALID, "null argument");
    // (the fields before n_devices are the round-2 sg_config: such a caller gets one device)
    if (cfg->struct_size < offsetof(sg_config, n_devices)) return fail(SG_ERR_INVALID, "sg_config too small");
    sg_config full{};
    memcpy(&full, cfg, std::min<size_t>(cfg->struct_size, sizeof(sg_config)));
    full.struct_size = sizeof(sg_config);
    if (cfg->struct_size < sizeof(sg_config)) {
        full.n_devices = 1;
        full.devices = nullptr;
    }
    if (full.n_devices > 1) {
        if (!full.devices) return fail(SG_ERR_INVALID, "n_devices > 1 needs the devices list");
        int rc = SG_OK;
        ShardEngine* sh = shd_create(ir, ir_len, &full, &rc);
        if (!sh) return rc;
        *out = new sg_engine();
        (*out)->cfg = full;
        (*out)->shard = sh;
        return SG_OK;
    }
    try {
        std::unique_ptr<sg_engine> e(new sg_engine());  // (owns no backend yet: its destructor makes no HIP call)
        e->cfg = full;
        e->device = full.device;
        const P2Settings set = p2_settings_from_env();
        if (sg_cfg_cap(full) > SGD_MAX_CAP) throw std::invalid_argument("partial_capacity above 4095");
        if (sg_cfg_matches(full) >= (1ull << 31)) throw std::invalid_argument("match_capacity must be < 2^31");
        if (ir_len < SG_IR_HDR_WORDS * 4 || ir_len % 4) throw std::invalid_argument("IR too short");
        const uint32_t* w = (const uint32_t*)ir;
        if (w[0] != SG_IR_MAGIC || w[1] != SG_IR_VERSION) throw std::invalid_argument("bad IR magic/version");
        // every shape must lower onto the general engine (validates the IR); the specialised
        // two-state kernel takes the shapes it covers
        delete gen_build_program(w, ir_len / 4, sg_cfg_cap(full));
        e->ir_hash = 1469598103934665603ull;
        for (size_t i = 0; i < ir_len / 4; i++) e->ir_hash = (e->ir_hash ^ w[i]) * 1099511628211ull;
        int ndev = 0;  // the one device-range check: either engine is created on the device set here
        HIP_OK(hipGetDeviceCount(&ndev));
        if (full.device < 0 || full.device >= ndev) throw HipError("no such HIP device");
        HIP_OK(hipSetDevice(full.device));
        if (!getenv("SG_FORCE_GENERAL")) {
            try {
                e->p2 = p2_create(ir, ir_len, full, set);
            } catch (const P2NotTwoState&) {
            }
        }
        if (!e->p2) {
            HIP_OK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
            e->gen = gen_create(w, ir_len / 4, full, e->stream);
        }
        *out = e.release();
        return SG_OK;
    } catch (const HipError& ex) {
        return fail(SG_ERR_DEVICE, ex.what());
    } catch (const std::invalid_argument& ex) {
        return fail(SG_ERR_INVALID, ex.what());
    } catch (const std::exception& ex) {
        return fail(SG_ERR_UNSUPPORTED, ex.what());
    }
}

void sg_engine_destroy(sg_engine* e) {
    if (e && e->shard) {
        shd_destroy(e->shard);
        e->shard = nullptr;
    }
    delete e;
}

int sg_push_batch(sg_engine* e, const sg_batch* b) {
    if (!e || !b) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_push(e->shard, b);
    return guarded(e, [&](std::string& msg) { return e->gen ? gen_push(e->gen, b, msg) : p2_push(e->p2, b, msg); });
}

int sg_advance_time(sg_engine* e, int64_t now_ms) {
    if (!e) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_advance(e->shard, now_ms);
    if (!e->gen) return SG_OK;  // the two-state kernel's shapes have no timers
    return guarded(e, [&](std::string& msg) { return gen_advance(e->gen, now_ms, msg); });
}

int sg_set_projection(sg_engine* e, const uint32_t* code, uint32_t code_words, const uint32_t* item_pc,
                      const uint32_t* item_len, const uint32_t* item_type, uint32_t n_items, const int32_t* part_attr,
                      uint32_t n_streams) {
    if (!e || !code || !item_pc || !item_len || !item_type) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard)
        return shd_set_projection(e->shard, code, code_words, item_pc, item_len, item_type, n_items, part_attr, n_streams);
    return guarded(e, [&](std::string& msg) {
        return e->gen ? gen_set_projection(e->gen, code, code_words, item_pc, item_len, item_type, n_items, msg)
                      : p2_set_projection(e->p2, code, code_words, item_pc, item_len, item_type, n_items, part_attr,
                                          n_streams, msg);
    });
}

int sg_get_projection(sg_engine* e, uint32_t mem, sg_projection* out) {
    if (!e || !out) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_get_projection(e->shard, mem, out);
    return guarded(e, [&](std::string& msg) {
        return e->gen ? gen_get_projection(e->gen, mem, out, msg) : p2_get_projection(e->p2, mem, out, msg);
    });
}

int sg_wait_stream(sg_engine* e, void* stream) {
    if (!e) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_wait_stream(e->shard, stream);
    return guarded(e, [&](std::string&) {
        if (e->p2) {
            p2_wait_stream(e->p2, (hipStream_t)stream);
            return SG_OK;
        }
        if (!e->wait_ev && hipEventCreate(&e->wait_ev) != hipSuccess) throw std::runtime_error("hipEventCreate failed");
        HIP_OK(hipEventRecord(e->wait_ev, (hipStream_t)stream));  // (a wait captures the recorded work: reusable)
        HIP_OK(hipStreamWaitEvent(e->stream, e->wait_ev, 0));
        return SG_OK;
    });
}

int sg_poll_matches(sg_engine* e, uint32_t mem, sg_match_batch* out) {
    if (!e || !out) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_poll(e->shard, mem, out);
    return guarded(e, [&](std::string& msg) {  // (the general engine's polls always wait for every pushed batch)
        return e->gen ? gen_poll(e->gen, mem & ~(uint32_t)SG_POLL_READY, out, msg) : p2_poll(e->p2, mem, out, msg);
    });
}

int sg_release_matches(sg_engine* e, sg_match_batch* m) {
    if (!e) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_release(e->shard, m);
    if (e->gen) gen_release(e->gen);
    else p2_release(e->p2);
    if (m) memset(m, 0, sizeof(*m));
    return SG_OK;
}

int sg_synchronize(sg_engine* e) {
    if (!e) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_synchronize(e->shard);
    return guarded(e, [&](std::string&) {
        if (e->gen) HIP_OK(hipStreamSynchronize(e->stream));
        else p2_synchronize(e->p2);
        return SG_OK;
    });
}

int sg_get_stats_sized(sg_engine* e, sg_stats* out, size_t out_size) {
    if (!out || out_size == 0) return fail(SG_ERR_INVALID, "null stats or zero size");
    sg_stats full{};
    const int rc = sg_get_stats(e, &full);
    if (rc == SG_OK) memcpy(out, &full, std::min(out_size, sizeof(sg_stats)));
    return rc;
}

int sg_get_stats(sg_engine* e, sg_stats* out) {
    if (!e || !out) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_stats(e->shard, out);
    return guarded(e, [&](std::string&) {
        if (e->gen) gen_stats(e->gen, out);
        else p2_stats(e->p2, out);
        return SG_OK;
    });
}

int sg_engine_describe(sg_engine* e, char* out, size_t out_len) {
    if (!e || (!out && out_len)) return fail(SG_ERR_INVALID, "null argument");
    const sg_engine* one = e->shard ? shd_first(e->shard) : e;
    std::string d = one->gen ? gen_describe(one->gen) : p2_describe(one->p2);
    if (e->shard) d = std::to_string(shd_count(e->shard)) + " shards, each " + d;
    if (out_len) {
        const size_t n = std::min(out_len - 1, d.size());
        memcpy(out, d.data(), n);
        out[n] = 0;
    }
    return SG_OK;
}

// ---- partition purge (PartitionRuntimeImpl.java:368-401) ----------------------------------------
int sg_reset_keys(sg_engine* e, const uint32_t* keys, uint64_t n, uint32_t mem) {
    if (!e || (!keys && n)) return fail(SG_ERR_INVALID, "null argument");
    if (n == 0) return SG_OK;
    if (e->shard) return shd_reset_keys(e->shard, keys, n, mem);
    if (n >= (1ull << 32)) return fail(SG_ERR_INVALID, "too many keys in one reset");
    return guarded(e, [&](std::string& msg) {
        if (e->p2 && p2_held(e->p2)) return refuse(msg, SG_ERR_STATE, "release the polled matches before resetting keys");
        const uint32_t K = e->n_keys();
        const hipStream_t st = e->main_stream();
        const uint32_t* dk = keys;
        uint32_t* tmp = nullptr;
        if (mem == SG_MEM_HOST) {
            for (uint64_t i = 0; i < n; i++)
                if (keys[i] >= K) return refuse(msg, SG_ERR_INVALID, "key id outside [0, n_keys)");
            HIP_OK(hipMalloc(&tmp, n * 4 + 4));
            HIP_OK(hipMemcpyAsync(tmp, keys, n * 4, hipMemcpyHostToDevice, st));
            dk = tmp;
        } else {
            // device ids: validated before any state changes (all or nothing, as for host ids)
            HIP_OK(hipMalloc(&tmp, 4));
            if (sgd_launch_check_keys(dk, (uint32_t)n, K, tmp, st) != 0) throw HipError("k_check_keys launch failed");
            uint32_t bad = 0;
            HIP_OK(hipMemcpyAsync(&bad, tmp, 4, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            if (bad) {
                HIP_OK(hipFree(tmp));
                return refuse(msg, SG_ERR_INVALID, "key id outside [0, n_keys)");
            }
        }
        const int rc = e->gen ? gen_reset_keys(e->gen, dk, (uint32_t)n, msg) : p2_reset_keys(e->p2, dk, (uint32_t)n, msg);
        HIP_OK(hipStreamSynchronize(st));
        if (tmp) HIP_OK(hipFree(tmp));
        return rc;
    });
}

// ---- persistence -------------------------------------------------------------
// The reference snapshots, per partition key, each pre-state processor's pending and newAndEvery lists
// (StreamPreStateProcessor.StreamPreState.snapshot/restore, StreamPreStateProcessor.java:450-469) through
// PartitionStateHolder (util/snapshot/state/PartitionStateHolder.java:43-80).  The device keeps exactly
// that state in HBM, so the image is a header plus the state buffers:
//   two-state kernel: the slab image (p2_host.h)
//   general kernel:  the interleaved per-key state blocks and the engine clock (gen_snapshot).
// Matches are output, not state: a snapshot or restore with matches waiting to be polled fails with
// SG_ERR_STATE (the reference has delivered its callbacks by the time a snapshot completes).  A
// restore needs an engine created from the same IR with the same n_keys; the two-state image needs
// partial_capacity >= rows, the general one the same partial_capacity (block layout).
struct SnapHeader {
    uint32_t magic;       // SG_SNAP_MAGIC
    uint32_t version;
    uint32_t kind;        // 1 = two-state kernel, 2 = general kernel
    uint32_t K;
    uint64_t ir_hash;
    uint32_t cap;         // partial_capacity of the source engine
    uint32_t rows;        // two-state: slab rows in the image
    uint32_t n_capw;
    uint32_t nullable;
    uint64_t next_seq;    // two-state: sequence numbers must keep increasing across a restore (general: 0)
    uint32_t have_base;
    uint32_t n_agg;       // two-state: per-key aggregator states in the image (selector aggregators)
    GenClock clk;
    uint64_t body_bytes;
};
#define SG_SNAP_MAGIC 0x4e534753u  // "SGSN"
#define SG_SNAP_VERSION 2u
static P2SnapRef p2_fields(SnapHeader& h) {
    return {h.K, h.cap, h.rows, h.n_capw, h.nullable, h.have_base, h.n_agg, h.next_seq, h.body_bytes};
}

int sg_snapshot(sg_engine* e, void** buf, size_t* len) {
    if (!e || !buf || !len) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_snapshot(e->shard, buf, len);
    return guarded(e, [&](std::string& msg) {
        SnapHeader h{};
        h.magic = SG_SNAP_MAGIC;
        h.version = SG_SNAP_VERSION;
        h.ir_hash = e->ir_hash;
        h.kind = e->gen ? 2 : 1;
        std::vector<uint64_t> body;  // (8-byte units: the images hold 64-bit planes)
        if (e->gen) {
            h.K = sg_cfg_keys(e->cfg);
            h.cap = sg_cfg_cap(e->cfg);
            h.body_bytes = gen_state_words(e->gen) * 4;
            body.resize((h.body_bytes + 7) / 8);
        }
        const int rc = e->gen ? gen_snapshot(e->gen, (uint32_t*)body.data(), &h.clk, msg) : p2_snapshot(e->p2, p2_fields(h), body, msg);
        if (rc != SG_OK) return rc;
        uint8_t* out = (uint8_t*)malloc(sizeof(h) + h.body_bytes);
        if (!out) return refuse(msg, SG_ERR_CAPACITY, "snapshot buffer allocation failed");
        memcpy(out, &h, sizeof(h));
        memcpy(out + sizeof(h), body.data(), h.body_bytes);
        *buf = out;
        *len = sizeof(h) + h.body_bytes;
        return SG_OK;
    });
}

int sg_restore(sg_engine* e, const void* buf, size_t len) {
    if (!e || !buf) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_restore(e->shard, buf, len);
    SnapHeader h;
    if (len < sizeof(h)) return fail(SG_ERR_INVALID, "snapshot too short");
    memcpy(&h, buf, sizeof(h));
    if (h.magic != SG_SNAP_MAGIC || h.version != SG_SNAP_VERSION) return fail(SG_ERR_INVALID, "not a snapshot of this engine version");
    if (len != sizeof(h) + h.body_bytes) return fail(SG_ERR_INVALID, "snapshot length does not match its header");
    if (h.ir_hash != e->ir_hash) return fail(SG_ERR_INVALID, "snapshot of a different query");
    if (h.kind != (e->gen ? 2u : 1u)) return fail(SG_ERR_INVALID, "snapshot of a different engine kind");
    const uint8_t* body = (const uint8_t*)buf + sizeof(h);
    return guarded(e, [&](std::string& msg) {
        if (e->gen) {
            if (h.K != sg_cfg_keys(e->cfg) || h.body_bytes != gen_state_words(e->gen) * 4)
                return refuse(msg, SG_ERR_INVALID, "snapshot taken with a different n_keys / partial_capacity");
            return gen_restore(e->gen, (const uint32_t*)body, h.clk, msg);
        }
        return p2_restore(e->p2, p2_fields(h), body, msg);
    });
}
int sg_free_buffer(void* buf) {
    free(buf);
    return SG_OK;
}

// ---- the per-key state in the reference's per-state-processor form (state_doc.h) -----------------------
int sg_state_export(sg_engine* e, void** buf, size_t* len) {
    if (!e || !buf || !len) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_state_export(e->shard, buf, len);
    return guarded(e, [&](std::string& msg) {
        SdDoc d;
        if (const int rc = e->gen ? gen_state_export(e->gen, d, msg) : p2_state_export(e->p2, d, msg); rc != SG_OK) return rc;
        const std::vector<uint8_t> bytes = sd_write(d);
        void* out = malloc(bytes.size());
        if (!out) return refuse(msg, SG_ERR_CAPACITY, "state document allocation failed");
        memcpy(out, bytes.data(), bytes.size());
        *buf = out;
        *len = bytes.size();
        return SG_OK;
    });
}

int sg_state_import(sg_engine* e, const void* buf, size_t len) {
    if (!e || !buf) return fail(SG_ERR_INVALID, "null argument");
    if (e->shard) return shd_state_import(e->shard, buf, len);
    SdDoc d;
    try {
        d = sd_read(buf, len);
    } catch (const std::exception& ex) {
        return fail(SG_ERR_INVALID, ex.what());
    }
    return guarded(e, [&](std::string& msg) {
        return e->gen ? gen_state_import(e->gen, d, msg) : p2_state_import(e->p2, d, msg);
    });
}

int sg_jit_check(const void* ir, size_t ir_len, uint32_t variant_flags, char* out, size_t out_len) {
    if (!ir) return fail(SG_ERR_INVALID, "null argument");
    std::string text, msg;
    const int rc = p2_jit_check(ir, ir_len, variant_flags, text, msg);
    if (out && out_len) {
        const size_t m = std::min(out_len - 1, text.size());
        memcpy(out, text.data(), m);
        out[m] = 0;
    }
    return rc == SG_OK ? rc : fail(rc, msg);
}

}  // extern "C"
