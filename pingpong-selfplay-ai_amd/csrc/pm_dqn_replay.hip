// K11 — the stand-alone learner fed from a device replay (pm_dqn_replay_update), and memory.push for a
// caller's own transitions (pm_replay_push).
//
// pm_dqn_replay_update(d, rp, U) is U times three launches on the stream, each one workgroup, nothing
// read back by the host:
//   k_dqr_sample   256 threads. frame = stats.steps + 1 and beta on the device; ceil(batch / 64) rounds of
//                  pm_per.h's per_sample_block over the tree in rp.per_work (fill rp.size, no pending push);
//                  the weights (size P(i))^-beta by per_is_weight, their maximum (wave_max, then the four
//                  waves' in LDS: a maximum has no order to keep) and k_per_normalize's float32 division;
//                  then four lanes per sample copy its 64-byte row, one 16-byte load each, into the
//                  learner's own batch buffers. A tree without mass, or a slot outside [0, size), makes
//                  the update void: idx <- -1, a status bit, nothing gathered.
//   k_dqr_update   pm_dqn.hip: k_dqn_update's two bodies, skipped when idx[0] < 0 (pm_dqn_replay_update_opt:
//                  k_dqr_update_opt, the same with a pm_dqn_opt's loss and clip).
//   k_dqr_scatter  1024 threads. (1) thread j < batch: the last duplicate of a slot in batch order wins
//                  (k_per_update's rule) and stores prios[i] = td[j] + 1e-6f and leaf[i] = prio_pow(..);
//                  every wave drains its stores, barrier. (2) four lanes per sample recompute the level-1
//                  node over its leaf (per_quarter's 16-leaf sequential fp64 sums, per_combine); drain,
//                  barrier. (3) the winners recompute their level-2 node (per_chunk_sum's order). Samples
//                  that share a node write the same value: every input of a node was stored before the
//                  barrier in front of it. The leaves and level-1 nodes this launch stored are read back
//                  around L1 (nontemporal loads through a plain pointer, as k_learn_multi's multi_quarter:
//                  per_quarter takes them const __restrict__, which may not be mixed with stores to them).
//   A recomputed node is the same additions in the same order as a rebuild's, so the workspace equals
//   pm_per_build(prios) bit for bit after every update, and the next one draws from it as it is.
//   k_dqp_sample / k_dqp_scatter are the population learner's (pm_dqn_pop_replay_update, pm_dqn_pop.hip): a grid
//   of n workgroups, workgroup p running the same body on the p-th record of a device table (pm_dqn_pop.h).
#include "pm_dev.h"
#include "pm_dqn_pop.h"
#include "pm_host.h"
#include "pm_per.h"

using namespace pm;

namespace {

constexpr int kScatter = 1024;
static_assert(kScatter == 4 * PM_MAX_BATCH, "four lanes per sampled level-1 node");

enum : int { DQR_NO_MASS = 1, DQR_NAN_PRIO = 2, DQR_BAD_SLOT = 4 };  // pm_dqn_stats.status

struct DqrSampleSmem {
    PerSampleSmem per;
    int64_t sidx[PM_MAX_BATCH];
    float w[PM_MAX_BATCH];
    float red[4];
};

#define PM_DQR_HORIZON(j, bits)
__global__ __launch_bounds__(256) void k_dqr_sample(const pm_dqn d, const pm_dqn_replay rp, int upd) {
    __shared__ DqrSampleSmem sm;
#include "pm_dqr_sample_body.inc"
}

// The population's draw + gather: workgroup p draws from member p's own tree into member p's own batch buffers.
__global__ __launch_bounds__(256) void k_dqp_sample(const pm_dqn_member* tab, int upd) {
    __shared__ DqrSampleSmem sm;
    const pm_dqn_member m = pop_member(tab, blockIdx.x);
    const pm_dqn& d = m.d;
    const pm_dqn_replay& rp = m.rp;
#include "pm_dqr_sample_body.inc"
}

// The two with a horizon buffer (pm_dqn_replay_update_n, pm_dqn_nstep_pop_set): the gather also decodes bits 16..18
// of the row's last word into hz[j] = 1..PM_NSTEP_MAX, next to act and done.
#undef PM_DQR_HORIZON
#define PM_DQR_HORIZON(j, bits) \
    if (hz) hz[j] = (uint8_t)((((bits) >> 16) & 7) + 1)
__global__ __launch_bounds__(256) void k_dqr_sample_n(const pm_dqn d, const pm_dqn_replay rp, int upd, uint8_t* hz) {
    __shared__ DqrSampleSmem sm;
#include "pm_dqr_sample_body.inc"
}

__global__ __launch_bounds__(256) void k_dqp_sample_n(const pm_dqn_member* tab, uint8_t* const* hzt, int upd) {
    __shared__ DqrSampleSmem sm;
    const pm_dqn_member m = pop_member(tab, blockIdx.x);
    const pm_dqn& d = m.d;
    const pm_dqn_replay& rp = m.rp;
    uint8_t* const hz = hzt[blockIdx.x];
#include "pm_dqr_sample_body.inc"
}
#undef PM_DQR_HORIZON

typedef float f32x4n __attribute__((ext_vector_type(4)));

// per_quarter with no pending push, the leaves loaded around L1 through a plain pointer.
__device__ __forceinline__ double dqr_quarter(const float* leaf, int64_t sb, int k, int64_t cap) {
    const int64_t lo = sb * PER_SUB + 16 * k;
    float v[16];
    if (lo + 16 <= cap) {
        const f32x4n* p4 = reinterpret_cast<const f32x4n*>(leaf + lo);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4n x = __builtin_nontemporal_load(p4 + q);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = lo + i < cap ? __builtin_nontemporal_load(leaf + lo + i) : 0.f;
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += lo + i < cap ? (double)v[i] : 0.0;
    return acc;
}
// per_chunk_sum, the level-1 nodes loaded around L1.
__device__ __forceinline__ double dqr_chunk_sum(const PerTree& t, int64_t c) {
    double v[PER_FAN];
#pragma unroll
    for (int k = 0; k < PER_FAN; ++k) v[k] = c * PER_FAN + k < t.nsub ? __builtin_nontemporal_load(t.sub + c * PER_FAN + k) : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PER_FAN; ++k) acc += v[k];
    return acc;
}

// k_dqr_scatter's body, block-wide (kScatter threads); sidx: PM_MAX_BATCH slots of LDS.
__device__ __forceinline__ void dqr_scatter_body(const pm_dqn& d, const pm_dqn_replay& rp, int64_t* sidx) {
    const int t = threadIdx.x, B = d.batch;
    if (rp.idx[0] < 0) return;  // a void update (block-uniform)
    const PerTree tr = per_tree(rp.per_work, rp.cap);
    const int64_t i = t < B ? rp.idx[t] : 0;
    if (t < B) sidx[t] = i;
    if (__syncthreads_or(i < 0 || i >= rp.size)) return;  // never: k_dqr_sample checked every slot
    // ---- (1) priorities and leaves
    bool win = t < B;
    if (t < B) {
        for (int k = t + 1; k < B; ++k)
            if (sidx[k] == i) { win = false; break; }  // a later duplicate wins (sequential update order)
        const float prio = fabsf(d.td[t]) + 1e-6f;
        if (prio != prio) atomicOr(&d.stats->status, DQR_NAN_PRIO);
        if (win) {
            rp.prios[i] = prio;
            tr.leaf[i] = prio_pow(prio, (float)rp.alpha);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the leaves are in L2 before the L1-bypassing loads
    __syncthreads();
    // ---- (2) level-1 nodes, four lanes each (lanes past the batch repeat its last sample's node)
    {
        const int64_t sb = sidx[min(t >> 2, B - 1)] / PER_SUB;
        const double q = dqr_quarter(tr.leaf, sb, t & 3, rp.cap);
        const double v = per_combine(quad_f64<0>(q), quad_f64<1>(q), quad_f64<2>(q), quad_f64<3>(q));
        if ((t & 3) == 0) tr.sub[sb] = v;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // ---- (3) level-2 nodes
    if (win) {
        const int64_t c = i / PER_CHUNK;
        tr.chunk[c] = dqr_chunk_sum(tr, c);
    }
}

__global__ __launch_bounds__(kScatter) void k_dqr_scatter(const pm_dqn d, const pm_dqn_replay rp) {
    __shared__ int64_t sidx[PM_MAX_BATCH];
    dqr_scatter_body(d, rp, sidx);
}

// The population's scatter + tree refresh: member p's priorities and member p's tree only.
__global__ __launch_bounds__(kScatter) void k_dqp_scatter(const pm_dqn_member* tab) {
    __shared__ int64_t sidx[PM_MAX_BATCH];
    const pm_dqn_member m = pop_member(tab, blockIdx.x);
    dqr_scatter_body(m.d, m.rp, sidx);
}

// ----------------------------------------------------------------------------- pm_replay_push
// k_push_rows' and k_push_rows_n's body. kHz: a horizon per row, (horizon - 1) & 7 into bits 16..18 of the last word.
template <bool kHz>
__device__ __forceinline__ void push_rows_body(float* __restrict__ trans, float* __restrict__ prios,
                                               float* __restrict__ leaf, int64_t cap, int64_t pos, float alpha, float prio,
                                               const float* __restrict__ s, const int32_t* __restrict__ act,
                                               const float* __restrict__ rew, const float* __restrict__ ns,
                                               const uint8_t* __restrict__ done, const uint8_t* __restrict__ hz, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t slot = pos + i;
    if (slot >= cap) slot -= cap;  // pos < cap and i < n <= cap
    const float* a = s + (size_t)i * 7;
    const float* b = ns + (size_t)i * 7;
    int bits = (act[i] & 0xff) | ((done[i] ? 1 : 0) << 8);
    if (kHz) bits |= ((hz[i] - 1) & 7) << 16;
    float4* row = reinterpret_cast<float4*>(trans + slot * PM_TRANS_F);
    row[0] = make_float4(a[0], a[1], a[2], a[3]);
    row[1] = make_float4(a[4], a[5], a[6], rew[i]);
    row[2] = make_float4(b[0], b[1], b[2], b[3]);
    row[3] = make_float4(b[4], b[5], b[6], __int_as_float(bits));
    prios[slot] = prio;
    leaf[slot] = prio_pow(prio, alpha);
}

__global__ __launch_bounds__(256) void k_push_rows(float* __restrict__ trans, float* __restrict__ prios,
                                                   float* __restrict__ leaf, int64_t cap, int64_t pos, float alpha,
                                                   float prio, const float* __restrict__ s, const int32_t* __restrict__ act,
                                                   const float* __restrict__ rew, const float* __restrict__ ns,
                                                   const uint8_t* __restrict__ done, int n) {
    push_rows_body<false>(trans, prios, leaf, cap, pos, alpha, prio, s, act, rew, ns, done, nullptr, n);
}

// pm_replay_push_n
__global__ __launch_bounds__(256) void k_push_rows_n(float* __restrict__ trans, float* __restrict__ prios,
                                                     float* __restrict__ leaf, int64_t cap, int64_t pos, float alpha,
                                                     float prio, const float* __restrict__ s, const int32_t* __restrict__ act,
                                                     const float* __restrict__ rew, const float* __restrict__ ns,
                                                     const uint8_t* __restrict__ done, const uint8_t* __restrict__ hz,
                                                     int n) {
    push_rows_body<true>(trans, prios, leaf, cap, pos, alpha, prio, s, act, rew, ns, done, hz, n);
}

// The level-1 nodes overlapping the pushed ring range, four lanes each (k_per_subs's form).
__global__ __launch_bounds__(256) void k_push_subs(int64_t cap, int64_t pos, int64_t n, PerTree tr) {
    const RingNodes rn = ring_nodes(PushRange{pos, n, cap, 0.f}, PER_SUB);
    const PushRange none{0, 0, cap, 0.f};
    const int64_t cnt = rn.count();
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < cnt * 4; t0 += (int64_t)gridDim.x * 256) {
        const int64_t t = t0 + threadIdx.x, k = t >> 2;
        const int64_t sb = rn.at(k < cnt ? k : cnt - 1);
        const double v = per_sub_sum4(tr.leaf, sb, none);
        if ((t & 3) == 0 && k < cnt) tr.sub[sb] = v;
    }
}

__global__ __launch_bounds__(256) void k_push_chunks(int64_t cap, int64_t pos, int64_t n, PerTree tr) {
    const RingNodes rn = ring_nodes(PushRange{pos, n, cap, 0.f}, PER_CHUNK);
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < rn.count(); k += (int64_t)gridDim.x * 256) {
        const int64_t c = rn.at(k);
        tr.chunk[c] = per_chunk_sum(tr, c);
    }
}

}  // namespace

extern "C" size_t pm_dqn_replay_sizeof(void) { return sizeof(pm_dqn_replay); }

// The replay side of pm_dqn_replay_update's checks (pm_dqn_pop_create runs them per member, updates = 1).
int pm::dqn_replay_check(const pm_dqn* d, const pm_dqn_replay* rp, int32_t updates) {
    PM_REQUIRE(rp, PM_E_ARG, "pm_dqn_replay_update: null replay descriptor");
    PM_REQUIRE(d->isw, PM_E_ARG, "pm_dqn_replay_update: null isw (the draw's weights are written there)");
    PM_REQUIRE(rp->trans && rp->prios && rp->per_work && rp->idx, PM_E_ARG, "pm_dqn_replay_update: null replay buffer");
    PM_REQUIRE(((uintptr_t)rp->trans & 15) == 0 && ((uintptr_t)rp->per_work & 15) == 0, PM_E_ARG,
               "pm_dqn_replay_update: trans and per_work must be 16-byte aligned");
    PM_REQUIRE(rp->size > 0 && rp->size <= rp->cap, PM_E_SIZE, "pm_dqn_replay_update: size=%lld cap=%lld",
               (long long)rp->size, (long long)rp->cap);
    PM_REQUIRE(updates > 0, PM_E_SIZE, "pm_dqn_replay_update: updates=%d", updates);
    PM_REQUIRE(rp->beta_frames > 0, PM_E_SIZE, "pm_dqn_replay_update: beta_frames=%lld", (long long)rp->beta_frames);
    return PM_OK;
}

int pm::dqp_launch_sample(const pm_dqn_member* tab, uint8_t* const* hzt, int n, int upd, hipStream_t st) {
    if (hzt)
        hipLaunchKernelGGL(k_dqp_sample_n, dim3(n), dim3(256), 0, st, tab, hzt, upd);
    else
        hipLaunchKernelGGL(k_dqp_sample, dim3(n), dim3(256), 0, st, tab, upd);
    PM_LAUNCHED(hzt ? "k_dqp_sample_n" : "k_dqp_sample");
    return PM_OK;
}

int pm::dqp_launch_scatter(const pm_dqn_member* tab, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_dqp_scatter, dim3(n), dim3(kScatter), 0, st, tab);
    PM_LAUNCHED("k_dqp_scatter");
    return PM_OK;
}

// pm_dqn_replay_update (with_opt false), pm_dqn_replay_update_opt and pm_dqn_replay_update_n (hz: k_dqr_sample_n); the
// middle launch's kernel is dqn_launch's choice from the same three.
static int replay_update(const pm_dqn* d, bool with_opt, const pm_dqn_opt* o, const pm_dqn_replay* rp, int32_t updates,
                         void* stream, uint8_t* hz = nullptr) {
    if (int rc = dqn_check(d, o)) return rc;
    if (int rc = dqn_replay_check(d, rp, updates)) return rc;
    hipStream_t st = pm_stream(stream);
    for (int k = 0; k < updates; ++k) {
        if (hz)
            hipLaunchKernelGGL(k_dqr_sample_n, dim3(1), dim3(256), 0, st, *d, *rp, k, hz);
        else
            hipLaunchKernelGGL(k_dqr_sample, dim3(1), dim3(256), 0, st, *d, *rp, k);
        PM_LAUNCHED(hz ? "k_dqr_sample_n" : "k_dqr_sample");
        if (int rc = dqn_launch(DQN_UPDATE_GATED, d, with_opt, o, hz, rp->idx, st)) return rc;
        hipLaunchKernelGGL(k_dqr_scatter, dim3(1), dim3(kScatter), 0, st, *d, *rp);
        PM_LAUNCHED("k_dqr_scatter");
    }
    return PM_OK;
}

extern "C" int pm_dqn_replay_update(const pm_dqn* d, const pm_dqn_replay* rp, int32_t updates, void* stream) {
    return replay_update(d, false, nullptr, rp, updates, stream);
}

extern "C" int pm_dqn_replay_update_opt(const pm_dqn* d, const pm_dqn_opt* o, const pm_dqn_replay* rp, int32_t updates,
                                        void* stream) {
    return replay_update(d, true, o, rp, updates, stream);
}

extern "C" int pm_dqn_replay_update_n(const pm_dqn* d, const pm_dqn_opt* o, const pm_dqn_nstep* ns,
                                      const pm_dqn_replay* rp, int32_t updates, void* stream) {
    PM_REQUIRE(ns && ns->horizon, PM_E_ARG, "pm_dqn_replay_update_n: null horizon (the gather writes the rows' horizons there)");
    return replay_update(d, true, o, rp, updates, stream, ns->horizon);
}

// pm_replay_push (hz null) and pm_replay_push_n.
static int replay_push(float* trans, float* prios, void* per_work, int64_t cap, int64_t pos, float alpha, float prio,
                       const float* s, const int32_t* act, const float* rew, const float* ns, const uint8_t* done,
                       const uint8_t* hz, int32_t n, void* stream) {
    PM_REQUIRE(trans && prios && per_work, PM_E_ARG, "pm_replay_push: null replay buffer");
    PM_REQUIRE(s && act && rew && ns && done, PM_E_ARG, "pm_replay_push: null transition buffer");
    PM_REQUIRE(((uintptr_t)trans & 15) == 0 && ((uintptr_t)per_work & 15) == 0, PM_E_ARG,
               "pm_replay_push: trans and per_work must be 16-byte aligned");
    PM_REQUIRE(cap > 0, PM_E_SIZE, "pm_replay_push: cap=%lld", (long long)cap);
    PM_REQUIRE(n > 0 && n <= cap, PM_E_SIZE, "pm_replay_push: n=%d (1..cap=%lld)", n, (long long)cap);
    PM_REQUIRE(pos >= 0 && pos < cap, PM_E_SIZE, "pm_replay_push: pos=%lld (0..cap-1)", (long long)pos);
    hipStream_t st = pm_stream(stream);
    const PerTree tr = per_tree(per_work, cap);
    const auto grid = [](int64_t items) {
        const int64_t b = (items + 255) / 256;
        return (unsigned)(b < 4096 ? (b > 0 ? b : 1) : 4096);
    };
    // the leaves land (one launch) before the nodes over them are summed (the next), level 1 before level 2
    if (hz)
        hipLaunchKernelGGL(k_push_rows_n, dim3(pm_blocks(n, 256)), dim3(256), 0, st, trans, prios, tr.leaf, cap, pos, alpha,
                           prio, s, act, rew, ns, done, hz, (int)n);
    else
        hipLaunchKernelGGL(k_push_rows, dim3(pm_blocks(n, 256)), dim3(256), 0, st, trans, prios, tr.leaf, cap, pos, alpha,
                           prio, s, act, rew, ns, done, (int)n);
    PM_LAUNCHED(hz ? "k_push_rows_n" : "k_push_rows");
    hipLaunchKernelGGL(k_push_subs, dim3(grid(((int64_t)n / PER_SUB + 2) * 4)), dim3(256), 0, st, cap, pos, (int64_t)n, tr);
    PM_LAUNCHED("k_push_subs");
    hipLaunchKernelGGL(k_push_chunks, dim3(grid((int64_t)n / PER_CHUNK + 2)), dim3(256), 0, st, cap, pos, (int64_t)n, tr);
    PM_LAUNCHED("k_push_chunks");
    return PM_OK;
}

extern "C" int pm_replay_push(float* trans, float* prios, void* per_work, int64_t cap, int64_t pos, float alpha, float prio,
                              const float* s, const int32_t* act, const float* rew, const float* ns, const uint8_t* done,
                              int32_t n, void* stream) {
    return replay_push(trans, prios, per_work, cap, pos, alpha, prio, s, act, rew, ns, done, nullptr, n, stream);
}

extern "C" int pm_replay_push_n(float* trans, float* prios, void* per_work, int64_t cap, int64_t pos, float alpha,
                                float prio, const float* s, const int32_t* act, const float* rew, const float* ns,
                                const uint8_t* done, const uint8_t* horizon, int32_t n, void* stream) {
    return replay_push(trans, prios, per_work, cap, pos, alpha, prio, s, act, rew, ns, done, horizon, n, stream);
}
