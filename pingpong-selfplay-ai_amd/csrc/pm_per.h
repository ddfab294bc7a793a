// PER pieces shared between pm_replay.hip and the self-play learner's units (pm_sp_rollout.hip, pm_sp_learn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pongmi.h"
#include "pm_dev.h"

namespace pm {

// Sum tree over the leaves prio^alpha (fp32 leaf array, fp64 nodes), two node levels:
//   leaf[e]  = powf(prio[e], alpha), kept next to the priorities (push and scatter write both)
//   sub[s]   = ((q0 + q1) + q2) + q3, q_k = sequential fp64 sum of leaves [64 s + 16 k, +16)  (level 1)
//   chunk[c] = sequential fp64 sum of sub[16 c .. 16 c + 16)                                  (level 2)
// Every node is always computed by the same functions in the same order, so a node recomputed
// after an incremental change is bit-identical to a full rebuild. The stored leaves mean a node
// refresh is loads + adds (no pow), and 4 threads share a level-1 node (one quarter each).
constexpr int PER_SUB = 64;
constexpr int PER_FAN = 16;
constexpr int PER_CHUNK = PER_SUB * PER_FAN;

__host__ __device__ inline int64_t per_pad(int64_t n_doubles) { return ((n_doubles * 8 + 255) / 256) * 256; }

struct PerTree {
    double* chunk;  // [nchunk]
    double* sub;    // [nsub]
    float* leaf;    // [cap]
    int64_t nchunk, nsub;
};

__host__ __device__ inline PerTree per_tree(void* work, int64_t cap) {
    PerTree t;
    t.nsub = (cap + PER_SUB - 1) / PER_SUB;
    t.nchunk = (cap + PER_CHUNK - 1) / PER_CHUNK;
    char* w = reinterpret_cast<char*>(work);
    t.chunk = reinterpret_cast<double*>(w);
    t.sub = reinterpret_cast<double*>(w + per_pad(t.nchunk));
    t.leaf = reinterpret_cast<float*>(w + per_pad(t.nchunk) + per_pad(t.nsub));
    return t;
}

inline int64_t per_work_bytes(int64_t cap) {
    return per_pad((cap + PER_CHUNK - 1) / PER_CHUNK) + per_pad((cap + PER_SUB - 1) / PER_SUB) +
           ((cap * 4 + 255) / 256) * 256;
}

// The replay push that is about to land (or landing concurrently): entries [pos, pos + n) mod cap
// hold leaf value `pval` = powf(max(prios), alpha) (memory.push stores max(prios),
// train_iterative.py:57) as far as the tree and the sampler are concerned. n = 0: none.
struct PushRange {
    int64_t pos, n, cap;
    float pval;
    __device__ __forceinline__ int64_t dist(int64_t e) const {
        const int64_t d = e - pos;
        return d < 0 ? d + cap : d;
    }
    __device__ __forceinline__ bool covers(int64_t e) const { return dist(e) < n; }
};

__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// wave_incl_scan without the LDS crossbar (each __shfl_up of a double is two ds_bpermute round trips,
// twelve on the chain): the same Hillis-Steele steps, at step o lane L adds the value lane L - o held
// before the step, so every lane's sum has the same association and the same bits. Offsets 1, 2, 4, 8
// are o DPP wave_shr:1 moves (a whole-wave shift, zeros shifted in: row_shr cannot cross a 16-lane
// row); 16 and 32 are the gfx950 row / half swaps. Lanes below o add the +0.0 shifted in where the
// loop adds nothing: the same bits for every value but -0.0, which a sum that starts at +0.0 never
// is. Full waves only. Used by per_round_prefix alone (multi_update keeps wave_incl_scan).
__device__ __forceinline__ double wave_shr1_f64(double v) {
    const unsigned long long x = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)x, 0x138, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(x >> 32), 0x138, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double wave_incl_scan_dpp(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        double u = v;
#pragma unroll
        for (int s = 0; s < o; ++s) u = wave_shr1_f64(u);
        v += u;
    }
    const int row = lane >> 4;
    {   // o = 16: rows (r0, r1, r2, r3) -> (0, r0, r1, r2)
        const unsigned long long x = (unsigned long long)__double_as_longlong(v);
        unsigned w[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned d = (unsigned)(x >> (32 * h));
            const auto p = __builtin_amdgcn_permlane16_swap(d, d, false, false);  // [0] = (r0, r0, r2, r2), [1] = (r1, r1, r3, r3)
            const auto m = __builtin_amdgcn_permlane32_swap(p[1], p[1], false, false);  // [0] = (r1, r1, r1, r1)
            w[h] = row == 0 ? 0u : (row == 2 ? m[0] : p[0]);
        }
        v += __longlong_as_double((long long)(((unsigned long long)w[1] << 32) | w[0]));
    }
    {   // o = 32: (r0, r1, r2, r3) -> (0, 0, r0, r1)
        const unsigned long long x = (unsigned long long)__double_as_longlong(v);
        unsigned w[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned d = (unsigned)(x >> (32 * h));
            const auto p = __builtin_amdgcn_permlane32_swap(d, d, false, false);  // [0] = (r0, r1, r0, r1)
            w[h] = row < 2 ? 0u : p[0];
        }
        v += __longlong_as_double((long long)(((unsigned long long)w[1] << 32) | w[0]));
    }
    return v;
}

// Tree nodes of granularity g (entries per node) overlapping the ring range [pos, pos + n) mod cap:
// ids a0 .. a0 + na - 1 (the part up to cap) then 0 .. nb - 1 (the wrapped part). Overlaps between
// the two segments only repeat a node (same value written twice).
struct RingNodes {
    int64_t a0, na, nb;
    __device__ __forceinline__ int64_t count() const { return na + nb; }
    __device__ __forceinline__ int64_t at(int64_t k) const { return k < na ? a0 + k : k - na; }
};
__device__ __forceinline__ RingNodes ring_nodes(const PushRange& pr, int64_t g) {
    RingNodes r{pr.pos / g, 0, 0};
    if (pr.n <= 0) return r;
    const int64_t end1 = pr.pos + pr.n < pr.cap ? pr.pos + pr.n : pr.cap;
    r.na = (end1 - 1) / g - r.a0 + 1;
    const int64_t end2 = pr.pos + pr.n - pr.cap;
    r.nb = end2 > 0 ? (end2 - 1) / g + 1 : 0;
    return r;
}

// prio ** alpha, PrioritizedReplay's leaf (train_iterative.py:67: prios ** alpha in float32). Formed
// in double from +, -, *, / and exact scalings only — ln p by the atanh series on m in
// [sqrt(1/2), sqrt(2)), exp by a Cody-Waite split and its Taylor series — then rounded once to float:
// within an ulp of numpy's powf (the reference's arithmetic), and a fixed sequence of correctly
// rounded operations, so the oracle (oracle.det_pow_f32) restates every leaf bit for bit; equal to
// the correctly rounded pow on every input and within 1 ulp of numpy's float32 power
// (tests/test_oracle_golden.py::test_det_pow_within_one_ulp_of_numpy_power). Non-positive and NaN
// priorities give a 0 leaf (never sampled); the learner latches pm_ctrl.status bit 1 for a NaN one,
// where the reference's numpy would carry the NaN into np.random.choice (which raises).
__device__ __forceinline__ float prio_pow(float p, float alpha) {
    if (!(p > 0.f)) return 0.f;
    int e;
    double m = 2.0 * frexp((double)p, &e);  // p = m 2^(e - 1), m in [1, 2): exact
    e = e - 1;
    if (m > 1.4142135623730951) { m = m * 0.5; e = e + 1; }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    const double q = s2 * (0.66666666666666663 + s2 * (0.40000000000000002 + s2 * (0.28571428571428570 +
                     s2 * (0.22222222222222221 + s2 * (0.18181818181818182 + s2 * (0.15384615384615385 +
                     s2 * (0.13333333333333333 + s2 * (0.11764705882352941 + s2 * (0.10526315789473684 +
                     s2 * 0.09523809523809523)))))))));
    const double y = (double)alpha * ((double)e * 0.69314718055994531 + (2.0 * s + s * q));
    const double k = floor(y * 1.4426950408889634 + 0.5);
    const double r = (y - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;  // |r| <= ln2 / 2
    const double ex = 1.0 + r * (1.0 + r * (0.5 + r * (0.16666666666666666 + r * (0.041666666666666664 +
                      r * (0.008333333333333333 + r * (0.001388888888888889 + r * (0.0001984126984126984 +
                      r * (2.48015873015873e-05 + r * (2.7557319223985893e-06 + r * (2.755731922398589e-07 +
                      r * (2.505210838544172e-08 + r * (2.08767569878681e-09 + r * 1.6059043836821613e-10))))))))))));
    return (float)ldexp(ex, (int)k);
}

// Leaf e as the tree sees it: pushed value inside the pending push range, 0 past cap.
__device__ __forceinline__ float per_leaf(const float* __restrict__ leaf, int64_t e, const PushRange& pr) {
    return pr.covers(e) ? pr.pval : (e < pr.cap ? leaf[e] : 0.f);
}

// Quarter k of level-1 node sb: sequential fp64 sum of its 16 leaves (loads issued together).
__device__ __forceinline__ double per_quarter(const float* __restrict__ leaf, int64_t sb, int k, const PushRange pr) {
    const int64_t lo = sb * PER_SUB + 16 * k;
    float v[16];
    if (lo + 16 <= pr.cap) {
        const float4* p4 = reinterpret_cast<const float4*>(leaf + lo);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 x = p4[q];
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = lo + i < pr.cap ? leaf[lo + i] : 0.f;
    }
    const int64_t d0 = pr.dist(lo);  // covers(lo + i) without a 64-bit op per leaf
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int64_t d = d0 + i;
        if (d >= pr.cap) d -= pr.cap;
        acc += lo + i < pr.cap ? (double)(d < pr.n ? pr.pval : v[i]) : 0.0;  // past cap: no leaf
    }
    return acc;
}
__device__ __forceinline__ double per_combine(double q0, double q1, double q2, double q3) {
    return ((q0 + q1) + q2) + q3;
}
// Level-1 node, one thread (rebuilds and rare paths).
__device__ __forceinline__ double per_sub_sum(const float* __restrict__ leaf, int64_t sb, const PushRange pr) {
    const double q0 = per_quarter(leaf, sb, 0, pr), q1 = per_quarter(leaf, sb, 1, pr);
    const double q2 = per_quarter(leaf, sb, 2, pr), q3 = per_quarter(leaf, sb, 3, pr);
    return per_combine(q0, q1, q2, q3);
}
// Level-1 node by 4 consecutive lanes (lane & 3 = quarter); the node lands in every lane of the group.
__device__ __forceinline__ double per_sub_sum4(const float* __restrict__ leaf, int64_t sb, const PushRange pr) {
    const int lane = threadIdx.x & 63;
    const double q = per_quarter(leaf, sb, lane & 3, pr);
    return per_combine(quad_f64<0>(q), quad_f64<1>(q), quad_f64<2>(q), quad_f64<3>(q));
}

// A level-1 node wholly inside the push range: the same sums over 16 copies of the pushed leaf.
__device__ __forceinline__ bool per_sub_pushed(int64_t sb, const PushRange pr) {
    const int64_t lo = sb * PER_SUB;
    return lo + PER_SUB <= pr.cap && pr.dist(lo) + PER_SUB <= pr.n;
}
__device__ __forceinline__ double per_sub_pushed_sum(const PushRange pr) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) q += (double)pr.pval;
    return per_combine(q, q, q, q);
}

// Level-2 node c from its 16 level-1 nodes. One thread.
__device__ __forceinline__ double per_chunk_sum(const PerTree& t, int64_t c) {
    double v[PER_FAN];
#pragma unroll
    for (int k = 0; k < PER_FAN; ++k) v[k] = c * PER_FAN + k < t.nsub ? t.sub[c * PER_FAN + k] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PER_FAN; ++k) acc += v[k];
    return acc;
}

// Both node levels for one 256-thread block (blockIdx.x: its 64 level-1 nodes; subl: 64 doubles of LDS): the block
// computes the nodes (four lanes each, per_sub_sum4) into HBM and LDS, then four of its threads sum their 16-node
// groups into the level-2 nodes in per_chunk_sum's order (same values: the 16 loads per_chunk_sum would issue come
// from LDS). Every thread of the block calls it.
__device__ __forceinline__ void per_nodes_block(const PerTree& tr, const PushRange& pr, double* subl) {
    const int64_t sb = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const double v = per_sub_sum4(tr.leaf, sb < tr.nsub ? sb : tr.nsub - 1, pr);
    if ((threadIdx.x & 3) == 0) {
        subl[threadIdx.x >> 2] = sb < tr.nsub ? v : 0.0;
        if (sb < tr.nsub) tr.sub[sb] = v;
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 4 + threadIdx.x;
    if (threadIdx.x < 4 && c < tr.nchunk) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < PER_FAN; ++k) acc += subl[threadIdx.x * PER_FAN + k];
        tr.chunk[c] = acc;
    }
}

// ----------------------------------------------------------------------------- block sampler
// PrioritizedReplay.sample (scripts/train_iterative.py:64-73): np.random.choice(p) picks the first
// index whose running sum of p exceeds u (searchsorted 'right'). Here a 256-thread block draws
// PER_BS = 64 samples at once, descending the tree in three dependent load round trips:
//   level 2: the block loads every chunk sum once (4 per thread), forms their inclusive prefix in LDS
//            (one block scan) and each sample searches it for t = u * total (per_lds_search);
//   level 1: 4 lanes per sample read the chosen chunk's 16 sub sums (4 each), a 4-lane scan finds
//            the sub-block;
//   level 0: the same 4 lanes read its 64 leaves (16 each, one float4 x4 load) and find the entry.
// Compared with one wave per sample, the block does the top-level scan once for 64 samples: the
// wave-wide scans of <= 1024 chunk sums per sample were VALU work that starved beside the act's MFMA
// streams. Every sum has a fixed order, so a sample is a pure function of (tree, u). When rounding
// leaves the target at or past a node's running total, the last nonzero child is taken (as before).
constexpr int PER_BS = 64;       // samples per 256-thread block
constexpr int PER_ROUND = 1024;  // chunk sums per prefix round (capacities <= 1M: one round)

struct PerSampleSmem {
    double incl[PER_ROUND];  // inclusive prefix of the round's chunk sums (plus the earlier rounds)
    double wsum[4];
};

// The round's inclusive prefix of chunk sums [c0, c0 + 1024) into sm.incl, offset by base; returns
// the running total after the round. v: this thread's 4 chunk sums (chunks c0 + 4t .. 4t + 3).
__device__ inline double per_round_prefix(const double (&v)[4], double base, PerSampleSmem& sm) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    double run[4], acc = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc += v[e]; run[e] = acc; }
    const double incl = wave_incl_scan_dpp(acc, lane);
    const double excl = wave_shr1_f64(incl);  // lane 0: 0.0
    if (lane == 63) sm.wsum[wv] = incl;
    __syncthreads();
    double wb = base;
    for (int w = 0; w < wv; ++w) wb += sm.wsum[w];
    const double ex = wb + excl;
#pragma unroll
    for (int e = 0; e < 4; ++e) sm.incl[4 * t + e] = ex + run[e];
    const double tot = ((base + sm.wsum[0]) + sm.wsum[1]) + sm.wsum[2] + sm.wsum[3];
    __syncthreads();
    return tot;
}

// First k in [0, n) with sm.incl[k] > x (n if none). Like the binary search it replaced, this is
// that k only where sm.incl is non-decreasing over [0, n). per_round_prefix does not prove it: a
// thread's values are (wb + excl) + run[e] while the next thread starts from the wave scan's sum of
// the same terms in another association, so two neighbours across a thread boundary can invert by
// an ulp of the running total (priorities spanning more than 2^53 make that ulp larger than a chunk
// sum). x then has to fall inside that one-ulp gap for any search to depend on its probe positions;
// base-4 and binary probes may then pick different chunks, each with a prefix value above x.
__device__ __forceinline__ int per_lds_search(const PerSampleSmem& sm, int n, double x) {
    // Five rounds of three independent probes (strides 256, 64, 16, 4, 1) instead of ten dependent
    // ones: the prefix is non-decreasing, so the probes that are not above x are a prefix of each
    // round's and their count is the round's base-4 digit of k. An index at or past n counts as above
    // x (its read is clamped), which leaves k = n when no value is.
    static_assert(PER_ROUND == 1024, "per_lds_search's five base-4 digits");
    int base = 0;
#pragma unroll
    for (int stride = 256; stride >= 1; stride >>= 2) {
        const int np = stride == 256 ? 4 : 3;  // the first round also probes the last value: k = n when none is above x
        double v[4];
#pragma unroll
        for (int i = 0; i < np; ++i) v[i] = sm.incl[min(base + stride * (i + 1) - 1, n - 1)];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < np; ++i) cnt += (base + stride * (i + 1) - 1 < n && !(v[i] > x)) ? 1 : 0;
        base += stride * cnt;
    }
    return base;
}

// 4-lane group search over the group's 4 x NV values (lane q of the group holds values
// [NV q, NV q + NV) in v, in order): the first value whose running sum exceeds x, else the last
// nonzero one. Returns its index in [0, 4 NV) (every lane of the group), `before` = running sum in
// front of it, `val` = the value.
template <int NV>
__device__ __forceinline__ int per_group_find(const double (&v)[NV], double x, double& before, double& val) {
    const int lane = threadIdx.x & 63, q = lane & 3, g0 = lane & ~3;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < NV; ++e) acc += v[e];
    const double s0 = quad_f64<0>(acc), s1 = quad_f64<1>(acc), s2 = quad_f64<2>(acc);
    const double ex = q == 0 ? 0.0 : (q == 1 ? s0 : (q == 2 ? s0 + s1 : (s0 + s1) + s2));
    // Compare-and-select code, no branch per value. pre[e]: the running sum in front of v[e] (the same
    // additions in the same order). The first hit is found walking down from the last value, so the
    // earliest one is left standing; the last nonzero value is only looked for when the group has no
    // hit (rounding left x at or past the group's total).
    double pre[NV + 1];
    pre[0] = ex;
#pragma unroll
    for (int e = 0; e < NV; ++e) pre[e + 1] = pre[e] + v[e];
    int k = -1;
    double hb = 0.0, hv = 0.0;
#pragma unroll
    for (int e = NV - 1; e >= 0; --e) {
        const bool h = pre[e + 1] > x;
        k = h ? e : k;
        hb = h ? pre[e] : hb;
        hv = h ? v[e] : hv;
    }
    const unsigned gh = (unsigned)(__ballot(k >= 0) >> g0) & 15u;
    int src;
    if (gh) {
        src = __ffs(gh) - 1;
    } else {  // group-uniform
        hb = ex;
        hv = 0.0;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const bool z = v[e] > 0.0;
            k = z ? e : k;
            hb = z ? pre[e] : hb;
            hv = z ? v[e] : hv;
        }
        const unsigned gn = (unsigned)(__ballot(k >= 0) >> g0) & 15u;
        src = gn ? 31 - __clz(gn) : 0;
        k = k < 0 ? 0 : k;
    }
    // every lane computed its candidate; take lane src's (the branch above is group-uniform)
    const int kk = quad_sel_i32(k, src);
    before = quad_sel_f64(hb, src);
    val = quad_sel_f64(hv, src);
    return src * NV + kk;
}

// Block-wide (256 threads, block-uniform arguments): samples j0 .. j0 + 63 (those < bs) with uniforms
// ufn(j), un-normalised IS weights (size * P(i))^-beta. Leaves inside the pending push range read as
// pr.pval (the push kernel may be writing them). out(j, idx, w) is called once per sample. For
// capacities <= 1M the chunk sums are loaded before `active` is tested (the caller's control-block
// read and these loads share one round trip); !active returns with nothing written.
struct NoHook {
    __device__ void operator()() const {}
};
// l1issued() / l0issued(): called by every thread right behind the issue of the level-1 (sub sum) and
// of the level-0 (leaf) loads, where a caller issues loads of its own that must delay neither the
// chunk-sum round trip nor the descent: vmcnt retires in issue order, so a load issued in front of the
// sub sums is waited for with them. Plain loads go into l1issued (the sub sums' wait then counts them
// out); LDS DMA goes into l0issued, behind the last loads of the descent (with LDS DMA in flight hipcc
// waits vmcnt(0) at the next use of a plain load, and the leaves are the last such use). Nothing may
// be consumed inside a hook.
// RAW: out(j, idx, pa, total) instead, the leaf and the total the weight is formed from: the fp64 pow
// (~300 instructions and two divisions) then no longer stands between the leaf search and whatever
// the caller does with idx. The caller evaluates per_is_weight(size, pa, total, beta) itself.
__device__ __forceinline__ float per_is_weight(int64_t size, double pa, double total, double beta) {
    return (float)pow((double)size * (pa / total), -beta);
}
template <bool RAW = false, class UFn, class OutFn, class Hook1 = NoHook, class Hook0 = NoHook>
__device__ inline void per_sample_block(bool active, int64_t size, const PerTree& tr, const PushRange& pr, double beta,
                                        int j0, int bs, PerSampleSmem& sm, UFn ufn, OutFn out, Hook1 l1issued = Hook1(),
                                        Hook0 l0issued = Hook0()) {
    const int t = threadIdx.x, q = t & 3;
    const int j = j0 + (t >> 2);
    const bool one_round = tr.nchunk <= PER_ROUND;  // kernel-argument uniform
    double vc[4] = {0.0, 0.0, 0.0, 0.0};
    if (one_round) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t c = 4 * t + e;
            vc[e] = c < tr.nchunk ? tr.chunk[c] : 0.0;
        }
        asm volatile("" ::"v"(vc[0]), "v"(vc[1]), "v"(vc[2]), "v"(vc[3]));
    }
    if (!active) return;  // block-uniform
    const int64_t nb = (size + PER_CHUNK - 1) / PER_CHUNK;
    const double u = j < bs ? ufn(j) : 0.0;
    // level 2
    double total = 0.0;
    if (nb > PER_ROUND) {  // capacities > 1M: the total first, one pass over the rounds
        for (int64_t c0 = 0; c0 < nb; c0 += PER_ROUND) {
            double v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t c = c0 + 4 * t + e;
                v[e] = c < nb ? tr.chunk[c] : 0.0;
            }
            total = per_round_prefix(v, total, sm);
        }
    }
    int64_t blk = -1, lastnz = 0;
    double before = 0.0, lastbef = 0.0, x = 0.0, run = 0.0;
    for (int64_t c0 = 0; c0 < nb; c0 += PER_ROUND) {
        double v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t c = c0 + 4 * t + e;
            v[e] = c < nb ? (one_round ? vc[e] : tr.chunk[c]) : 0.0;
        }
        const double end = per_round_prefix(v, run, sm);
        if (nb <= PER_ROUND) total = end;
        x = u * total;
        const int n = (int)(nb - c0 < PER_ROUND ? nb - c0 : PER_ROUND);
        if (blk < 0 && end > run) {
            const int k = per_lds_search(sm, n, x);
            if (k < n) {
                blk = c0 + k;
                before = k ? sm.incl[k - 1] : run;
            } else {  // last nonzero chunk of the round: the first to reach the round's end value
                int lo = 0, hi = n - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sm.incl[mid] >= sm.incl[n - 1]) hi = mid;
                    else lo = mid + 1;
                }
                lastnz = c0 + lo;
                lastbef = lo ? sm.incl[lo - 1] : run;
            }
        }
        run = end;
        __syncthreads();  // sm.incl is rewritten by the next round
    }
    if (blk < 0) { blk = lastnz; before = lastbef; }
    PM_BLK(4);
    // level 1: the chunk's 16 sub sums, 4 per lane of the sample's group
    double sv[4];
    const int64_t s0 = blk * PER_FAN + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) sv[e] = s0 + e < tr.nsub ? tr.sub[s0 + e] : 0.0;
    __builtin_amdgcn_sched_barrier(0);
    l1issued();
    __builtin_amdgcn_sched_barrier(0);
    double b1, v1;
    const int64_t sb = blk * PER_FAN + per_group_find<4>(sv, x - before, b1, v1);
    PM_BLK(5);
    // level 0: the sub-block's 64 leaves, 16 per lane
    double lv[16];
    {
        const int64_t lo = sb * PER_SUB + 16 * q;
        float f[16];
        if (lo + 16 <= pr.cap) {
            const float4* p4 = reinterpret_cast<const float4*>(tr.leaf + lo);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 a = p4[k];
                f[4 * k] = a.x; f[4 * k + 1] = a.y; f[4 * k + 2] = a.z; f[4 * k + 3] = a.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) f[k] = lo + k < pr.cap ? tr.leaf[lo + k] : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
        l0issued();
        __builtin_amdgcn_sched_barrier(0);
        // covers(lo + k) and lo + k < size as ranges of k, one set per lane, instead of a ring distance
        // and a 64-bit compare per leaf: leaf k lies d0 + k into the ring from pos while k < kw (the
        // ring's wrap), k - kw after it, and is in the push range when that is below n.
        const int64_t d0 = pr.dist(lo);
        const int64_t wrap = pr.cap - d0;
        const int kw = (int)(wrap < 0 ? 0 : (wrap < 16 ? wrap : 16));
        const int ka = min(kw, (int)(pr.n - d0 < 0 ? 0 : (pr.n - d0 < 16 ? pr.n - d0 : 16)));
        const int kb = (int)(wrap + pr.n < 0 ? 0 : (wrap + pr.n < 16 ? wrap + pr.n : 16));
        const int ks = (int)(size - lo < 0 ? 0 : (size - lo < 16 ? size - lo : 16));
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool cov = k < ka || (k >= kw && k < kb);
            const double lf = (double)(cov ? pr.pval : f[k]);
            lv[k] = k < ks ? lf : 0.0;
        }
    }
    double b0, pa;
    const int k = per_group_find<16>(lv, x - before - b1, b0, pa);
    PM_BLK(6);
    if (q == 0 && j < bs) {
        if constexpr (RAW) out(j, sb * PER_SUB + k, pa, total);
        else out(j, sb * PER_SUB + k, per_is_weight(size, pa, total, beta));
    }
    PM_BLK(7);
}

// Full rebuild over prios[0, cap): leaves, then level-1 and level-2 nodes with the pending push
// range substituted (from ctrl when non-null, else none).
int per_launch_build(const float* prios, int64_t cap, float alpha, const pm_ctrl* ctrl, int64_t n_push, void* work,
                     hipStream_t st);
int per_launch_update(float* prios, const int64_t* idx, const float* err, int bs, hipStream_t st);
// Level-1 and level-2 nodes over leaves already written (no pending push range).
int per_launch_nodes(void* work, int64_t cap, hipStream_t st);

}  // namespace pm
