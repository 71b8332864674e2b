// seq_kernels.hip — stencil kernels for sequences of stream states, partitioned or not
//
//     every e1=S[f0], e2=S[f1], ..., en=S[f(n-1)] [within W]          (SEQUENCE, one stream, 2 <= n <= 4)
//
// The general kernel (gen_kernels.hip) runs this query through the processor graph, one lane per key.  Under
// SEQUENCE semantics the graph does very little per event (paths under
// modules/siddhi-core/src/main/java/io/siddhi/core/query/input/stream/state/ of the reference):
//   receiver/SequenceMultiProcessStreamReceiver.java:39-50 stabilizeStates -> StateStreamRuntime.java:81-88
//       resetAndUpdate: every pending list is cleared before every event and what the last event staged is promoted
//   StreamPreStateProcessor.java:214-227 addState (SEQUENCE): a partial is staged only into an empty newAndEvery list
//   StreamPreStateProcessor.java:371-397 processAndReturn (SEQUENCE): a pending partial the event does not advance
//       is dropped
//   StreamPreStateProcessor.java:118-129 isExpired: |ts(e1) - ts(event)| > W, checked by expireEvents (:325-361)
//       at every event before the reset
//   StreamPostStateProcessor.java:64-83: a passing partial moves to the next state's addState; state 0 under
//       `every` stages a blank clone of it into its own newAndEvery list (:229-247)
// So a key holds at most one partial per state, a partial lives for exactly one event per state, and the partial
// waiting at state i is the key's previous i events.  With A_i(j) = "after event j of the key a partial of i events
// (e[j-i+1] .. e[j]) is staged at state i":
//   A_1(j)     = f0(e[j])
//   A_{i+1}(j) = A_i(j-1) and |ts(e[j-i]) - ts(e[j])| <= W and f_i(e[j]; e1 = e[j-i], .., e_i = e[j-1])
//   match(j)   = the same with i = n - 1
// — a stencil of width n over each key's run of the key-sorted batch, the halo being the key's last n - 1 events of
// earlier batches.  Nothing is sequential per key, so the kernel is one thread per EVENT:
//   k_seq_keys_<NW>      one lane per key: a key whose state arrives in its general block is adopted (the block
//                        validated as the canonical form and turned into a carry record) or handed to the general
//                        kernel; the batch's per-element tag (key, record to read, rank in the run) written
//   k_seq_batch_<n>_<NW> a workgroup of 256 threads takes 256 - (n - 1) elements plus the n - 1 before them, stages
//                        the decoded events in LDS (SoA), and each thread assembles its window of n events in
//                        registers: from LDS where the predecessor is in the batch, from the key's carry record
//                        where its rank in the run is smaller.  A_1 .. A_{n-1} go through LDS from neighbour to
//                        neighbour, one filter per phase, so every event evaluates each filter once and the work
//                        counters (all closed-form in these bits) come for free.  Matches are compacted with a wave
//                        ballot into a reserved range of the raw records.
//   k_seq_flush_<NW>     the records written back to the general blocks in a canonical layout
// The carry of a key is a pair of records: the thread of a run's last event writes the record the batch does NOT
// read (GEN_W0_SEQP, flipped by k_seq_keys before the batch kernel), so threads of the same run in other workgroups
// that still read the old carry never race with it, and untouched keys cost nothing.
//
// The unpartitioned query is one key whose run is the whole batch in arrival order, so it needs no grouping, no
// payload and no tags:
//   k_seq_head_<NW>      one wave, before the batch kernel: what k_seq_keys does for key 0 (adopt or hand over, flip
//                        GEN_W0_SEQP), and the record to read published in one device word (GenBatch.ekey[0])
//   k_seq_flat_<n>_<NW>  the same tile, phases and emission over the columns themselves: a thread's element is its
//                        global index, its rank that index clipped to n - 1, the element count a launch argument; the
//                        thread of the batch's last event writes the other record
// With a select list set (gen_host.hip gen_set_projection: no aggregators, every item at most two entries deep) the
// `_p` instantiations of both batch kernels evaluate the items from the emitting thread's window and write them to
// the raw record where the general kernel's projectSelect puts them.
#include <hip/hip_runtime.h>

#include "../../include/siddhi_gpu.h"
#include "../../include/siddhi_gpu_ir.h"
#include "gen_engine.h"
#include "java_ops.h"
#include "sg_engine.h"
#include "reg_common.h"

namespace {

constexpr uint32_t SEQ_TB = 256;   // threads of a batch workgroup

// one key's pair of carry records (gen_engine.h seq_rec_rows)
template <int NW> struct SeqRec {
    gu32* R;
    uint32_t K, k, rows;
    __device__ SeqRec(const GenArgs& a, uint32_t n, uint32_t key) : R(gp(a.rec)), K(a.K), k(key), rows(seq_rec_rows(NW, n)) {}
    __device__ __forceinline__ gu32& at(uint32_t c, uint32_t r) const { return R[(size_t)(c * rows + r) * K + k]; }
    __device__ __forceinline__ uint32_t ev(uint32_t j, uint32_t f) const { return 1u + j * (5u + NW) + f; }
    __device__ __forceinline__ void load(uint32_t c, uint32_t j, AbsEv<NW>& e) const {
        e.seq = (uint64_t)at(c, ev(j, 0)) | ((uint64_t)at(c, ev(j, 1)) << 32);
        e.ts = (int64_t)((uint64_t)at(c, ev(j, 2)) | ((uint64_t)at(c, ev(j, 3)) << 32));
        e.nb = at(c, ev(j, 4));
#pragma unroll
        for (int q = 0; q < NW; ++q) e.w[q] = at(c, ev(j, 5u + (uint32_t)q));
    }
    __device__ __forceinline__ void store(uint32_t c, uint32_t j, const AbsEv<NW>& e) const {
        at(c, ev(j, 0)) = (uint32_t)e.seq;
        at(c, ev(j, 1)) = (uint32_t)(e.seq >> 32);
        at(c, ev(j, 2)) = (uint32_t)(uint64_t)e.ts;
        at(c, ev(j, 3)) = (uint32_t)((uint64_t)e.ts >> 32);
        at(c, ev(j, 4)) = e.nb;
#pragma unroll
        for (int q = 0; q < NW; ++q) at(c, ev(j, 5u + (uint32_t)q)) = e.w[q];
    }
};

// one key's general block
struct SeqBlock {
    const cGenProgram& G;
    gu32* S;
    uint32_t K, k;
    __device__ SeqBlock(const GenArgs& a, uint32_t key) : G(*(cGenProgram*)a.G), S(gp(a.state)), K(a.K), k(key) {}
    __device__ __forceinline__ gu32& W(uint32_t w) const { return S[gen_il(K, k, w)]; }
    __device__ __forceinline__ int64_t R64(uint32_t w) const { return (int64_t)((uint64_t)W(w) | ((uint64_t)W(w + 1) << 32)); }
    __device__ __forceinline__ void W64(uint32_t w, int64_t v) const {
        W(w) = (uint32_t)(uint64_t)v;
        W(w + 1) = (uint32_t)((uint64_t)v >> 32);
    }
    __device__ __forceinline__ uint32_t ks(int i) const { return G.offKS + (uint32_t)G.seqP[i] * G.ksWords; }
    __device__ __forceinline__ uint32_t slotOf(int i) const { return (uint32_t)G.pre[G.seqP[i]].stateId; }
    __device__ __forceinline__ uint32_t stw(uint32_t se, uint32_t f) const { return G.offST + se * G.stWords + f; }
    __device__ __forceinline__ uint32_t sew(uint32_t e, uint32_t f) const { return G.offSE + e * G.seWords + f; }
};

// ---- adopt: a key whose state is in its block (first touched by the general kernel, imported, restored) ----
// The canonical form: every pending list empty; state i's newAndEvery list holds at most one partial, of exactly the
// events e1 .. e_i (single, unshared), stamped with its last event's time; the partials agree on the events they
// share counted from the newest (they are suffixes of one run); state 0 holds its blank clone exactly when state 1
// holds a partial.  Anything else: false, and the general kernel walks the key's run.
template <int NW> __device__ bool seq_adopt(const GenArgs& a, uint32_t key) {
    const SeqBlock B(a, key);
    const cGenProgram& G = B.G;
    const int n = G.seqN;
    uint32_t se[4] = {GEN_NIL, GEN_NIL, GEN_NIL, GEN_NIL};
    uint32_t bits = 0, cnt = 0;
    for (int i = 0; i < n; i++) {
        if (B.W(B.ks(i) + KS_PLEN) != 0u) return false;
        const uint32_t nl = B.W(B.ks(i) + KS_NLEN);
        if (nl > 1u) return false;
        if (!nl) continue;
        const uint32_t s = B.W(B.ks(i) + KS_LISTS + G.L);
        if (s >= G.STCAP || B.W(B.stw(s, ST_TYPE)) != 0u || B.W(B.stw(s, ST_RC)) != 1u) return false;
        for (int t = 0; t < n; t++) {
            const uint32_t e = B.W(B.stw(s, ST_SLOTS + B.slotOf(t)));
            if ((t < i) != (e != GEN_NIL)) return false;
            if (e != GEN_NIL && (e >= G.SECAP || B.W(B.sew(e, SE_NEXT)) != GEN_NIL)) return false;
        }
        se[i] = s;
        if (i > 0) {
            bits |= 1u << (i - 1);
            cnt = (uint32_t)i;
        }
    }
    if ((se[0] != GEN_NIL) != ((bits & 1u) != 0u)) return false;
    const SeqRec<NW> rec(a, (uint32_t)n, key);
    if (cnt) {
        // the longest partial's events are the carry (newest first); the others must be its suffixes
        const uint32_t sl = se[cnt];
        const uint32_t last = B.W(B.stw(sl, ST_SLOTS + B.slotOf((int)cnt - 1)));
        const int64_t tl = B.R64(B.sew(last, SE_TS));
        if (se[0] != GEN_NIL && B.R64(B.stw(se[0], ST_TS)) != tl) return false;
        for (uint32_t i = 1; i <= cnt; i++) {
            if (se[i] == GEN_NIL) continue;
            if (B.R64(B.stw(se[i], ST_TS)) != tl) return false;
            for (uint32_t d = 0; d < i; d++) {
                const uint32_t x = B.W(B.stw(se[i], ST_SLOTS + B.slotOf((int)(i - 1 - d))));
                const uint32_t y = B.W(B.stw(sl, ST_SLOTS + B.slotOf((int)(cnt - 1 - d))));
                if (B.R64(B.sew(x, SE_SEQ)) != B.R64(B.sew(y, SE_SEQ)) || B.R64(B.sew(x, SE_TS)) != B.R64(B.sew(y, SE_TS)))
                    return false;
            }
        }
        for (uint32_t d = 0; d < cnt; d++) {
            const uint32_t y = B.W(B.stw(sl, ST_SLOTS + B.slotOf((int)(cnt - 1 - d))));
            AbsEv<NW> ev;
            ev.seq = (uint64_t)B.R64(B.sew(y, SE_SEQ));
            ev.ts = B.R64(B.sew(y, SE_TS));
            ev.nb = B.W(B.sew(y, SE_NULL));
#pragma unroll
            for (int q = 0; q < NW; ++q) ev.w[q] = B.W(B.sew(y, G.absWordAt[q]));
            rec.store(0u, d, ev);
        }
    }
    rec.at(0u, 0u) = cnt | (bits << 4);
    return true;
}

// the record a batch reads of a key it touches, the key's other record made current (GEN_W0_SEQP flipped); a key whose
// state arrives in its block is adopted first.  false: the general kernel walks the key's run
template <int NW> __device__ __forceinline__ bool seq_claim(const GenArgs& a, const cGenProgram& G, uint32_t key, uint32_t& rd) {
    gu32& w0r = gp(a.state)[gen_il(a.K, key, 0)];
    const uint32_t w0 = w0r;
    rd = 0;
    if (w0 & GEN_W0_REG) {
        rd = (w0 & GEN_W0_SEQP) ? 1u : 0u;
        w0r = w0 ^ GEN_W0_SEQP;
    } else if (!(w0 & 1u)) {   // PartitionRuntimeImpl.initPartition: the seed state 0 stages dies at the first event
        SeqRec<NW>(a, (uint32_t)G.seqN, key).at(0u, 0u) = 0u;
        w0r = 1u | GEN_W0_REG | GEN_W0_SEQP;
    } else if (seq_adopt<NW>(a, key)) {
        w0r = 1u | GEN_W0_REG | GEN_W0_SEQP;
    } else {
        return false;
    }
    return true;
}

// ---- keys: one lane per key, before the batch kernel ----
template <int NW> __device__ void seq_keys(const GenArgs& a) {
    const uint32_t key = blockIdx.x * 64u + threadIdx.x, lane = threadIdx.x & 63u;
    const cGenProgram& G = *(cGenProgram*)a.G;
    uint32_t b = 0, e = 0;
    if (key < a.K) {
        b = gp(a.b.seg_begin)[key];
        e = gp(a.b.seg_end)[key];
    }
    bool fb = false;
    uint32_t tag = SEQ_NOKEY;
    if (b < e) {
        uint32_t rd;
        fb = !seq_claim<NW>(a, G, key, rd);
        if (!fb) tag = key | (rd << 29);
    }
    gu32* ek = gp(a.b.ekey);
    const uint32_t hd = e - b < 8u ? e : b + 8u;
    for (uint32_t i = b; i < hd; i++) ek[i] = fb ? SEQ_NOKEY : tag | ((i - b < 3u ? i - b : 3u) << 30);
    // the rest of a long run by the whole wave
    unsigned long long m = __ballot(e > hd);
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        const uint32_t lb = (uint32_t)__shfl((int)hd, l, 64), le = (uint32_t)__shfl((int)e, l, 64);
        const uint32_t lt = (uint32_t)__shfl((int)tag, l, 64);
        for (uint32_t i = lb + lane; i < le; i += 64u) ek[i] = lt == SEQ_NOKEY ? SEQ_NOKEY : lt | (3u << 30);
    }
    abs_fallback(a, fb, key, b);
    const unsigned long long fm = __ballot(fb);   // (sg_stats.window_spills: keys handed to the general kernel)
    if (fm && lane == 0) atomicAdd(&a.o.stats[GST_SPILLS], (unsigned long long)__popcll(fm));
}

// ---- head: the unpartitioned query's one key, one wave before the flat kernel ----
// GenBatch.ekey[0]: the record the batch reads, or SEQ_NOKEY when key 0 went to the hand-over list
template <int NW> __device__ void seq_head(const GenArgs& a) {
    const cGenProgram& G = *(cGenProgram*)a.G;
    bool fb = false;
    if ((threadIdx.x & 63u) == 0u) {
        uint32_t rd;
        fb = !seq_claim<NW>(a, G, 0u, rd);
        gp(a.b.ekey)[0] = fb ? SEQ_NOKEY : rd;
        if (fb) atomicAdd(&a.o.stats[GST_SPILLS], 1ull);   // (sg_stats.window_spills)
    }
    abs_fallback(a, fb, 0u, 0u);
}

// ---- batch: one thread per event of the key-sorted batch ----
// the event at batch position `pos` from the columns (a batch without the payload: more than four words with the
// null bits); reg_common.h abs_gather, inlined so that the window stays in registers
template <int NW> __device__ __forceinline__ void seq_gather(const GenArgs& a, const cGenProgram& G, uint32_t pos,
                                                             AbsEv<NW>& ev) {
    const int na = G.nattr[0];
    for (int at = 0; at < na; at++) {
        const int ty = G.attrType[0][at];
        const void* c = a.b.col[at];
        uint32_t lo = 0, hi = 0;
        if (ty == SG_T_LONG || ty == SG_T_DOUBLE) {
            const uint64_t v = gp((const uint64_t*)c)[pos];
            lo = (uint32_t)v;
            hi = (uint32_t)(v >> 32);
        } else if (ty == SG_T_BOOL) {
            lo = gp((const uint8_t*)c)[pos] ? 1u : 0u;
        } else {
            lo = gp((const uint32_t*)c)[pos];
        }
        const uint32_t o = G.absOff[at];
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            if ((uint32_t)q == o) ev.w[q] = lo;
            if ((ty == SG_T_LONG || ty == SG_T_DOUBLE) && (uint32_t)q == o + 1) ev.w[q] = hi;
        }
        if (a.b.nul[at] && gp(a.b.nul[at])[pos]) ev.nb |= 1u << at;
    }
}

template <int NW> __device__ __forceinline__ GVal seq_word(const cGenProgram& G, const uint32_t (&w)[NW], uint32_t nb,
                                                           uint32_t at) {
    const int ty = G.attrType[0][at];
    const uint32_t o = G.absOff[at];
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) {
        if ((uint32_t)q == o) lo = w[q];
        if ((uint32_t)q == o + 1) hi = w[q];
    }
    const uint64_t v = (ty == SG_T_LONG || ty == SG_T_DOUBLE) ? ((uint64_t)lo | ((uint64_t)hi << 32)) : (uint64_t)lo;
    return GVal{v, ((nb >> at) & 1u) != 0};
}

// filter M on a partial of M events and this event: win[N - 1] is the event, win[N - 1 - d] the key's event d back
// slot s of a partial of M events and this event: the state whose event it holds, -1: an empty slot
template <int M> __device__ __forceinline__ int seq_state_of(const cGenProgram& G, uint32_t s, int32_t c) {
    const int t = s < (uint32_t)GEN_MAXSLOT ? G.seqSlotEv[s] : -1;
    return (t < 0 || t > M || !(c == 0 || c == -1)) ? -1 : t;   // (single-event slots: index 0 or `last`)
}
// attribute `at` of that slot's event: win[N - 1] is this event, win[N - 1 - d] the key's event d back
template <int N, int NW, int M> __device__ __forceinline__ GVal seq_var(const cGenProgram& G, const AbsEv<NW> (&win)[N],
                                                                      uint32_t s, uint32_t at, int32_t c) {
    const int t = seq_state_of<M>(G, s, c);
    if (t < 0) return GVal{0, true};
    uint32_t w[NW], nb = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) w[q] = 0;
#pragma unroll
    for (int j = N - 1 - M; j < N; ++j) {   // (selects: no indexing of the register window)
        const bool here = j == N - 1 - M + t;
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = here ? win[j].w[q] : w[q];
        nb = here ? win[j].nb : nb;
    }
    return seq_word<NW>(G, w, nb, at);
}

template <int N, int NW, int M> __device__ __forceinline__ bool seq_filter(const cGenProgram& G, const AbsEv<NW> (&win)[N],
                                                                         uint32_t& err) {
    auto stateOf = [&](uint32_t s, int32_t c) -> int { return seq_state_of<M>(G, s, c); };
    auto var_ = [&](uint32_t s, uint32_t at, int32_t c) -> GVal { return seq_var<N, NW, M>(G, win, s, at, c); };
    const int nt = G.seqNT[M];
    for (int q = 0; q < nt; ++q) {   // (a run-time loop: one copy of the interpreter per filter)
        bool ok;
        if (G.seqFF[M][q].on) {
            ok = jo_fast(G.seqFF[M][q], var_);
        } else {
            const GVal v = jo_eval<false>(G.code, G.seqTpc[M][q], G.seqTlen[M][q], err, var_,
                                          [&](uint32_t s, int32_t c) -> bool { return stateOf(s, c) < 0; });
            ok = !v.null && (v.b & 1);
        }
        if (!ok) return false;
    }
    return true;
}

// the select list and `having` of a match from its window, laid out as gen_kernels.hip projectSelect lays them out:
// 3 words per item (value lo, hi, null) from pv; `having` reads the items just written (SG_PROJ_SLOT_OUT).  No
// aggregators, every item at most two entries deep (gen_host.hip gen_set_projection checked it)
template <int N, int NW> __device__ __forceinline__ void seq_project(const cGenProgram& G, const AbsEv<NW> (&win)[N], gu32* pv,
                                                                     uint32_t& err) {
    for (uint32_t i = 0; i < G.projN; i++) {   // (a run-time loop: one copy of the interpreter)
        const GVal v = jo_eval<false>(G.code, G.projPc[i], G.projLen[i], err,
                                      [&](uint32_t s, uint32_t at, int32_t c) -> GVal {
                                          if (s == SG_PROJ_SLOT_OUT)
                                              return GVal{(uint64_t)pv[3 * at] | ((uint64_t)pv[3 * at + 1] << 32),
                                                          pv[3 * at + 2] != 0};
                                          return seq_var<N, NW, N - 1>(G, win, s, at, c);
                                      },
                                      [&](uint32_t s, int32_t c) -> bool { return seq_state_of<N - 1>(G, s, c) < 0; });
        pv[3 * i] = (uint32_t)v.b;
        pv[3 * i + 1] = (uint32_t)(v.b >> 32);
        pv[3 * i + 2] = v.null ? 1u : 0u;
    }
}

struct SeqOut {
    uint32_t abits, scanned, err;   // A_1 .. A_{n-1} of this event, the pending partials it visited, error bits
    bool match;
};
template <int N, int NW> struct SeqPhase {
    // phases M .. N - 1 of one thread: `live` = a partial of M events is pending at this event (M = 0: the seed or
    // the clone state 0 always holds)
    template <int M> static __device__ __forceinline__ SeqOut run(const cGenProgram& G, const AbsEv<NW> (&win)[N], bool mine,
                                                                  bool first, uint32_t cbits, uint32_t (*sA)[SEQ_TB],
                                                                  SeqOut o) {
        const uint32_t tid = threadIdx.x;
        bool live = mine;
        if constexpr (M > 0) {
            __syncthreads();
            const bool prev = first ? ((cbits >> (M - 1)) & 1u) != 0u : (tid > 0u && sA[M - 1][tid - 1u] != 0u);
            bool expired = false;
            if (G.within != -1) {
                const int64_t d = win[N - 1 - M].ts - win[N - 1].ts;
                expired = (d < 0 ? -d : d) > G.within;
            }
            live = mine && prev && !expired;
            o.scanned += live ? 1u : 0u;
        }
        bool pass = false;
        uint32_t err = 0;
        if (live) pass = seq_filter<N, NW, M>(G, win, err);
        o.err |= err;
        if constexpr (M < N - 1) {
            sA[M][tid] = pass ? 1u : 0u;
            o.abits |= pass ? 1u << M : 0u;
            return run<M + 1>(G, win, mine, first, cbits, sA, o);
        } else {
            o.match = pass;
            return o;
        }
    }
};

// ---- the tail both batch kernels share: the match record, the carry record, the counter row ----
// the match: one raw record, reserved per wave (StreamPostStateProcessor -> QuerySelector input); PROJ: with the
// select list's items behind it
template <int N, int NW, bool PROJ>
__device__ __forceinline__ void seq_emit(const GenArgs& a, const cGenProgram& G, const AbsEv<NW> (&win)[N], bool match,
                                         uint32_t pos, uint32_t key, uint32_t& err) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long mm = __ballot(match);
    if (!mm) return;
    const int leader = __ffsll((long long)mm) - 1;
    const uint32_t sg = (blockIdx.x * (SEQ_TB / 64u) + wv) % a.o.nseg;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(&a.o.raw_count[sg], (unsigned long long)__popcll(mm));
    base = __shfl(base, leader, 64);
    if (!match) return;
    const unsigned long long r = (unsigned long long)sg * a.o.seg_cap + base + __popcll(mm & ((1ull << lane) - 1ull));
    if (r >= (unsigned long long)(sg + 1) * a.o.seg_cap) {
        err |= GERR_MATCHCAP;
        return;
    }
    gu32* out = gp(a.o.raw) + r * a.o.recWords;
    const AbsEv<NW>& ev = win[N - 1];
    out[0] = pos;
    out[1] = 0u;
    out[2] = (uint32_t)ev.seq;
    out[3] = (uint32_t)(ev.seq >> 32);
    out[4] = (uint32_t)(uint64_t)ev.ts;
    out[5] = (uint32_t)((uint64_t)ev.ts >> 32);
    out[6] = key;
    gu32* lens = out + 7;
    gu32* seqs = lens + G.nslots;
    for (int s = 0; s < G.nslots; s++) {   // (n slots, one event each: slot s at s * MC, MC = 1)
        const int t = G.seqSlotEv[s];
        uint64_t q = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) q = j == t ? win[j].seq : q;
        lens[s] = 1u;
        seqs[2 * s] = (uint32_t)q;
        seqs[2 * s + 1] = (uint32_t)(q >> 32);
    }
    if constexpr (PROJ) seq_project<N, NW>(G, win, out + G.projOff, err);
    gp(a.o.t_cnt)[pos] = 1u;
    if (a.mode & GEN_M_TFIRST) gp(a.o.t_first)[pos] = (uint32_t)r;
}

// the carry after a run's last event (rank rk, cnt events read from the old record): the newest n - 1 of them
template <int N, int NW>
__device__ __forceinline__ void seq_carry(const SeqRec<NW>& rec, uint32_t c, uint32_t rk, uint32_t cnt, uint32_t abits,
                                          const AbsEv<NW> (&win)[N]) {
    constexpr uint32_t H = N - 1;
    const uint32_t have = rk + 1u + cnt;
    const uint32_t nc = have < H ? have : H;
    rec.at(c, 0u) = nc | (abits << 4);
#pragma unroll
    for (uint32_t j = 0; j < H; ++j)
        if (j < nc) rec.store(c, j, win[N - 1 - j]);
}

// the work counters of the general kernel, one row per workgroup (every thread calls this)
__device__ __forceinline__ void seq_stats(const GenArgs& a, unsigned long long sc, unsigned long long cr, unsigned long long ma,
                                          unsigned long long ky, uint32_t err, unsigned long long (*sStat)[4]) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        sc += __shfl_xor(sc, off, 64);
        cr += __shfl_xor(cr, off, 64);
        ma += __shfl_xor(ma, off, 64);
        ky += __shfl_xor(ky, off, 64);
        err |= (uint32_t)__shfl_xor((int)err, off, 64);
    }
    if (lane == 0) {
        if (err) atomicOr(a.o.err, err);
        sStat[wv][0] = sc;
        sStat[wv][1] = cr;
        sStat[wv][2] = ma;
        sStat[wv][3] = ky;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long t[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t w = 0; w < SEQ_TB / 64u; w++)
#pragma unroll
            for (int c = 0; c < 4; c++) t[c] += sStat[w][c];
        auto row = gp(a.o.wstats) + (size_t)blockIdx.x * GST_N;
        row[GST_SCANNED] = t[0];
        row[GST_CREATED] = t[1];
        row[GST_MATCHES] = t[2];
        row[GST_KEYS] = t[3];
        row[GST_LIVE0] = 0;
        row[GST_SPILLS] = 0;
    }
}

template <int N, int NW, bool PROJ> __device__ __forceinline__ void seq_batch(const GenArgs& a) {
    constexpr uint32_t H = N - 1, T = SEQ_TB - H;
    __shared__ uint32_t sE[4 + NW][SEQ_TB];   // the decoded events: batch position, ts lo, hi, null bits, words
    __shared__ uint32_t sK[SEQ_TB + 1];       // their tags, and the tag of the element after the tile
    __shared__ uint32_t sA[H][SEQ_TB];        // A_1 .. A_{n-1} of each element
    __shared__ unsigned long long sStat[SEQ_TB / 64][4];
    const cGenProgram& G = *(cGenProgram*)a.G;
    const uint32_t tid = threadIdx.x;
    const uint32_t nv = gp(a.b.seg_end)[a.K - 1];   // elements of the key-sorted batch (null keys dropped)
    const int64_t g = (int64_t)blockIdx.x * T + tid - H;
    const bool valid = g >= 0 && g < (int64_t)nv;
    const uint32_t tag = valid ? gp(a.b.ekey)[g] : SEQ_NOKEY;
    sK[tid] = tag;
    if (tid == 0) {
        const uint64_t g1 = (uint64_t)blockIdx.x * T + T;
        sK[SEQ_TB] = g1 < nv ? gp(a.b.ekey)[g1] : SEQ_NOKEY;
    }
    const bool mine = tag != SEQ_NOKEY;
    const uint32_t key = tag & SEQ_KEYMASK, rd = (tag >> 29) & 1u, rk = tag >> 30;
    AbsEv<NW> win[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        win[j].ts = 0;
        win[j].seq = 0;
        win[j].nb = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) win[j].w[q] = 0;
    }
    uint32_t pos = 0;
    if (mine) {
        if (a.b.pay) {
            abs_pay<NW>(a, (uint32_t)g, gp(a.b.ts)[0], win[N - 1]);
            pos = (uint32_t)(win[N - 1].seq - a.b.seq_base);
        } else {
            pos = a.b.sidx ? gp(a.b.sidx)[(size_t)g * (a.b.sidxStride ? a.b.sidxStride : 1u)] : (uint32_t)g;
            win[N - 1].ts = gp(a.b.ts)[pos];
            win[N - 1].seq = a.b.seq_base + pos;
            seq_gather<NW>(a, G, pos, win[N - 1]);
        }
    }
    sE[0][tid] = pos;
    sE[1][tid] = (uint32_t)(uint64_t)win[N - 1].ts;
    sE[2][tid] = (uint32_t)((uint64_t)win[N - 1].ts >> 32);
    sE[3][tid] = win[N - 1].nb;
#pragma unroll
    for (int q = 0; q < NW; ++q) sE[4 + q][tid] = win[N - 1].w[q];
    __syncthreads();
    // the window: the event d back from the tile where this run has it, else from the key's carry record (the
    // first n - 1 threads only serve as the halo: what they cannot reach is never used)
    const SeqRec<NW> rec(a, (uint32_t)N, mine ? key : 0u);
    uint32_t cnt = 0, cbits = 0;
    if (mine && rk < H) {
        const uint32_t h = rec.at(rd, 0u);
        cnt = h & 15u;
        cbits = (h >> 4) & 7u;
    }
#pragma unroll
    for (uint32_t d = 1; d <= H; ++d) {
        AbsEv<NW>& w = win[N - 1 - d];
        if (mine && rk >= d) {
            if (tid >= d) {
                const uint32_t s = tid - d;
                w.seq = a.b.seq_base + sE[0][s];
                w.ts = (int64_t)((uint64_t)sE[1][s] | ((uint64_t)sE[2][s] << 32));
                w.nb = sE[3][s];
#pragma unroll
                for (int q = 0; q < NW; ++q) w.w[q] = sE[4 + q][s];
            }
        } else if (mine && d - rk - 1u < cnt) {
            rec.load(rd, d - rk - 1u, w);
        }
    }
    const SeqOut o = SeqPhase<N, NW>::template run<0>(G, win, mine, rk == 0u, cbits, sA, SeqOut{0u, mine ? 1u : 0u, 0u, false});
    const uint32_t abits = o.abits;
    uint32_t err = o.err;
    const bool own = mine && tid >= H;   // (the halo threads' elements belong to the workgroup before)
    const bool match = o.match && own;
    seq_emit<N, NW, PROJ>(a, G, win, match, pos, key, err);
    // the carry: the thread of the run's last event writes the record this batch does not read
    const uint32_t nxt = sK[tid + 1];
    if (own && !(nxt != SEQ_NOKEY && (nxt & SEQ_KEYMASK) == key)) seq_carry<N, NW>(rec, rd ^ 1u, rk, cnt, abits, win);
    seq_stats(a, own ? o.scanned : 0u, (own && (abits & 1u)) ? 1u : 0u, match ? 1u : 0u, (own && rk == 0u) ? 1u : 0u, err,
              sStat);
}

// ---- flat: one thread per event of the unpartitioned batch, in arrival order ----
// The batch is key 0's run: element g is batch position g, its rank min(g, n - 1), the events before it the tile's or
// (the first n - 1 elements of the batch) the carry record k_seq_head published.  Consecutive threads read consecutive
// positions of ts and of every column.
template <int N, int NW, bool PROJ> __device__ __forceinline__ void seq_flat(const GenArgs& a) {
    constexpr uint32_t H = N - 1, T = SEQ_TB - H;
    __shared__ uint32_t sE[3 + NW][SEQ_TB];   // the decoded events: ts lo, hi, null bits, words
    __shared__ uint32_t sA[H][SEQ_TB];        // A_1 .. A_{n-1} of each element
    __shared__ unsigned long long sStat[SEQ_TB / 64][4];
    const cGenProgram& G = *(cGenProgram*)a.G;
    const uint32_t tid = threadIdx.x;
    const uint32_t rd = gp(a.b.ekey)[0];   // (one word, the same for every workgroup)
    if (rd == SEQ_NOKEY) {   // key 0 is on the hand-over list: the general kernel walks the batch
        seq_stats(a, 0u, 0u, 0u, 0u, 0u, sStat);
        return;
    }
    const uint32_t n = a.b.n;
    const int64_t g = (int64_t)blockIdx.x * T + tid - H;
    const bool mine = g >= 0 && g < (int64_t)n;
    const uint32_t pos = mine ? (uint32_t)g : 0u, rk = pos < H ? pos : H;
    AbsEv<NW> win[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        win[j].ts = 0;
        win[j].seq = 0;
        win[j].nb = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) win[j].w[q] = 0;
    }
    if (mine) {
        win[N - 1].ts = gp(a.b.ts)[pos];
        win[N - 1].seq = a.b.seq_base + pos;
        seq_gather<NW>(a, G, pos, win[N - 1]);
    }
    sE[0][tid] = (uint32_t)(uint64_t)win[N - 1].ts;
    sE[1][tid] = (uint32_t)((uint64_t)win[N - 1].ts >> 32);
    sE[2][tid] = win[N - 1].nb;
#pragma unroll
    for (int q = 0; q < NW; ++q) sE[3 + q][tid] = win[N - 1].w[q];
    __syncthreads();
    // the window: the event d back from the tile, else (the batch's first n - 1 elements) from the carry record;
    // what the halo threads cannot reach is never used
    const SeqRec<NW> rec(a, (uint32_t)N, 0u);
    uint32_t cnt = 0, cbits = 0;
    if (mine && rk < H) {
        const uint32_t h = rec.at(rd, 0u);
        cnt = h & 15u;
        cbits = (h >> 4) & 7u;
    }
#pragma unroll
    for (uint32_t d = 1; d <= H; ++d) {
        AbsEv<NW>& w = win[N - 1 - d];
        if (mine && rk >= d) {
            if (tid >= d) {
                const uint32_t s = tid - d;
                w.seq = a.b.seq_base + (pos - d);
                w.ts = (int64_t)((uint64_t)sE[0][s] | ((uint64_t)sE[1][s] << 32));
                w.nb = sE[2][s];
#pragma unroll
                for (int q = 0; q < NW; ++q) w.w[q] = sE[3 + q][s];
            }
        } else if (mine && d - rk - 1u < cnt) {
            rec.load(rd, d - rk - 1u, w);
        }
    }
    const SeqOut o = SeqPhase<N, NW>::template run<0>(G, win, mine, rk == 0u, cbits, sA, SeqOut{0u, mine ? 1u : 0u, 0u, false});
    const uint32_t abits = o.abits;
    uint32_t err = o.err;
    const bool own = mine && tid >= H;
    const bool match = o.match && own;
    seq_emit<N, NW, PROJ>(a, G, win, match, pos, 0u, err);
    if (own && pos == n - 1u) seq_carry<N, NW>(rec, rd ^ 1u, rk, cnt, abits, win);   // the batch's last event
    seq_stats(a, own ? o.scanned : 0u, (own && (abits & 1u)) ? 1u : 0u, match ? 1u : 0u, (own && pos == 0u) ? 1u : 0u, err,
              sStat);
}

// ---- the records written back to the blocks (before a snapshot, a state export, the min-seq scan, a purge) ----
// Canonical layout: state i's partial = StateEvent i - 1 over StreamEvents i (i - 1) / 2 .. + i - 1 (its own copies,
// as the reference clones the event per pending partial), state 0's clone = StateEvent n - 1.
template <int NW> __device__ void seq_flush(const GenArgs& a) {
    const uint32_t key = blockIdx.x * 64u + threadIdx.x;
    if (key >= a.K || !a.rec) return;
    const SeqBlock B(a, key);
    const cGenProgram& G = B.G;
    const uint32_t w0 = B.W(0);
    if (!(w0 & GEN_W0_REG)) return;
    const int n = G.seqN;
    const SeqRec<NW> rec(a, (uint32_t)n, key);
    const uint32_t c = (w0 & GEN_W0_SEQP) ? 1u : 0u;
    const uint32_t h = rec.at(c, 0u), cnt = h & 15u, bits = (h >> 4) & 7u;
    AbsEv<NW> ev[3];
    for (uint32_t j = 0; j < 3u; j++) {
        ev[j].seq = 0;
        ev[j].ts = 0;
        ev[j].nb = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) ev[j].w[q] = 0;
        if (j < cnt) rec.load(c, j, ev[j]);
    }
    uint32_t stMask = 0, seMask = 0;
    B.W(B.ks(0) + KS_FLAGS) = GF_INIT;
    B.W(B.ks(0) + KS_PLEN) = 0u;
    B.W(B.ks(0) + KS_NLEN) = bits & 1u;
    if (bits & 1u) {   // the blank clone `every` staged when the last event passed f0, stamped with its time
        const uint32_t s = (uint32_t)n - 1u;
        B.W(B.ks(0) + KS_LISTS + G.L) = s;
        B.W64(B.stw(s, ST_TS), ev[0].ts);
        B.W(B.stw(s, ST_TYPE)) = 0u;
        B.W(B.stw(s, ST_RC)) = 1u;
        for (int sl = 0; sl < G.nslots; sl++) B.W(B.stw(s, ST_SLOTS + (uint32_t)sl)) = GEN_NIL;
        stMask |= 1u << s;
    }
    for (int i = 1; i < n; i++) {
        const bool on = ((bits >> (i - 1)) & 1u) != 0u;
        B.W(B.ks(i) + KS_FLAGS) = 0u;
        B.W(B.ks(i) + KS_PLEN) = 0u;
        B.W(B.ks(i) + KS_NLEN) = on ? 1u : 0u;
        if (!on) continue;
        const uint32_t s = (uint32_t)i - 1u, e0 = (uint32_t)(i * (i - 1) / 2);
        B.W(B.ks(i) + KS_LISTS + G.L) = s;
        B.W64(B.stw(s, ST_TS), ev[0].ts);
        B.W(B.stw(s, ST_TYPE)) = 0u;
        B.W(B.stw(s, ST_RC)) = 1u;
        for (int sl = 0; sl < G.nslots; sl++) {
            const int t = G.seqSlotEv[sl];
            B.W(B.stw(s, ST_SLOTS + (uint32_t)sl)) = (t >= 0 && t < i) ? e0 + (uint32_t)t : GEN_NIL;
        }
        stMask |= 1u << s;
        for (int t = 0; t < i; t++) {   // state t's event: i - 1 - t back from the newest
            const AbsEv<NW>& x = ev[i - 1 - t];
            const uint32_t eb = e0 + (uint32_t)t;
            B.W64(B.sew(eb, SE_SEQ), (int64_t)x.seq);
            B.W64(B.sew(eb, SE_TS), x.ts);
            B.W(B.sew(eb, SE_NEXT)) = GEN_NIL;
            B.W(B.sew(eb, SE_RC)) = 1u;
            B.W(B.sew(eb, SE_NULL)) = x.nb;
#pragma unroll
            for (int q = 0; q < NW; ++q) B.W(B.sew(eb, G.absWordAt[q])) = x.w[q];
            seMask |= 1u << eb;
        }
    }
    for (uint32_t q = 0; q < (G.STCAP + 31) / 32; q++) B.W(G.offSTfree + q) = q == 0 ? stMask : 0u;
    for (uint32_t q = 0; q < (G.SECAP + 31) / 32; q++) B.W(G.offSEfree + q) = q == 0 ? seMask : 0u;
    B.W(G.offDef) = 0u;
    B.W(0) = 1u;   // (the block is the key's state again)
}

}  // namespace

// One batch kernel per (states, attribute words of the event) and variant (partitioned / flat, bare / projecting: the
// projecting code is in instantiations of its own, so a launch without a select list pays nothing for it); the
// per-key kernels per word count.  The batch kernels read their GenArgs through the kernarg segment (gen_kernels.hip
// gen_kernarg: the column arrays are indexed at run time, and the by-value parameter would be copied into every
// lane's scratch for that).
#define SEQ_BATCH(N, NW)                                                                                    \
    extern "C" __global__ void __launch_bounds__(256) k_seq_batch_##N##_##NW(const GenArgs ap) {           \
        seq_batch<N, NW, false>(*(const GenArgs*)(const void*)__builtin_amdgcn_kernarg_segment_ptr());      \
    }                                                                                                       \
    extern "C" __global__ void __launch_bounds__(256) k_seq_batch_##N##_##NW##_p(const GenArgs ap) {          \
        seq_batch<N, NW, true>(*(const GenArgs*)(const void*)__builtin_amdgcn_kernarg_segment_ptr());       \
    }                                                                                                       \
    extern "C" __global__ void __launch_bounds__(256) k_seq_flat_##N##_##NW(const GenArgs ap) {            \
        seq_flat<N, NW, false>(*(const GenArgs*)(const void*)__builtin_amdgcn_kernarg_segment_ptr());       \
    }                                                                                                       \
    extern "C" __global__ void __launch_bounds__(256) k_seq_flat_##N##_##NW##_p(const GenArgs ap) {           \
        seq_flat<N, NW, true>(*(const GenArgs*)(const void*)__builtin_amdgcn_kernarg_segment_ptr());        \
    }
#define SEQ_KERNELS(NW)                                                                                     \
    SEQ_BATCH(2, NW) SEQ_BATCH(3, NW) SEQ_BATCH(4, NW)                                                      \
    extern "C" __global__ void __launch_bounds__(64) k_seq_keys_##NW(const GenArgs ap) { seq_keys<NW>(ap); } \
    extern "C" __global__ void __launch_bounds__(64) k_seq_head_##NW(const GenArgs ap) { seq_head<NW>(ap); } \
    extern "C" __global__ void __launch_bounds__(64) k_seq_flush_##NW(const GenArgs ap) { seq_flush<NW>(ap); }
SEQ_KERNELS(1)
SEQ_KERNELS(2)
SEQ_KERNELS(3)
SEQ_KERNELS(4)
