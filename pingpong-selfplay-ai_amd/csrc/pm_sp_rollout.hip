// The self-play learner's rollout unit: the kernels that act, tick the environments, push to the
// replay and draw the update's PER sample, and the entry points that launch only them.
//
//   k_actenv (pm_selfplay_actenv)   the fused step's first launch: sampler blocks (sample_fwd_block16)
//                                   + modelB's act and the env tick of 256 arenas per block (env_block)
//   k_act_sp + k_env                the plain step's two launches (pm_selfplay_rollout)
//   k_sp_init                       serves, opponents and first observations (pm_selfplay_init)
//   k_resample + k_batch_fwd        updates 1..U-1 without k_learn_multi (pm_selfplay_resample)
//
// k_resample shares sample_block's per_sample_block instantiation with k_act_sp: its code changes when
// the two are compiled apart (DESIGN.md "The self-play learner's units").
#include "pm_sp.h"

#ifdef PM_DIAG
// k_env phase timeline (diagnostic build only): wave 0 of each env block. A stamp records when the
// wave's instruction stream reaches it (no drain: stores still in flight are not waited for);
// PM_ENV_STAMP_DRAIN first waits for every outstanding memory operation of the wave.
static __device__ unsigned long long pm_diag_env[8][1024];
#define PM_ENV_STAMP(k, blk)                                                                   \
    do {                                                                                       \
        asm volatile("" ::: "memory");                                                         \
        if (threadIdx.x == 0 && (blk) < 1024) pm_diag_env[(k)][(blk)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define PM_ENV_STAMP_DRAIN(k, blk)                                                             \
    do {                                                                                       \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                            \
        if (threadIdx.x == 0 && (blk) < 1024) pm_diag_env[(k)][(blk)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
// where the env block runs, as PM_BLK_END's slot 3: CU id (__smid) | XCC id << 16, read at the block's start
static __device__ unsigned long long pm_diag_env_place[1024];
#define PM_ENV_PLACE(blk)                                                                      \
    do {                                                                                       \
        if (threadIdx.x == 0 && (blk) < 1024)                                                  \
            pm_diag_env_place[(blk)] =                                                         \
                (unsigned long long)__smid() | ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 15) << 16); \
    } while (0)
#else
#define PM_ENV_PLACE(blk) \
    do {                  \
    } while (0)
#define PM_ENV_STAMP(k, blk) \
    do {                     \
    } while (0)
#define PM_ENV_STAMP_DRAIN(k, blk) \
    do {                           \
    } while (0)
#endif

namespace {
__device__ __forceinline__ bool learner_active(const pm_selfplay& sp) {
    const int64_t s = sp.ctrl->size + sp.n;
    return (s < sp.cap ? s : sp.cap) >= sp.batch;
}
}  // namespace

// ------------------------------------------------------------------------------------ rollout
// PrioritizedReplay.sample (:64-73) for update samples [64 b, 64 b + 64): proportional draw + un-normalised
// IS weight, one 256-thread block per 64 samples (pm_per.h: per_sample_block). pending: the step's
// push has not landed yet (update 0, drawn beside k_env: the tree accounts for it and its leaves read
// as the pushed value); otherwise (updates 1..U-1) the replay is as k_env left it. The fill is the
// post-push one either way: pos/size advance only when the step commits.
__device__ __forceinline__ void sample_block(const pm_selfplay& sp, int b, bool pending, PerSampleSmem& sm) {
    const pm_ctrl* c = sp.ctrl;
    const int64_t s = c->size + sp.n;
    const int64_t size = s < sp.cap ? s : sp.cap;
    const int64_t frame = c->frame_idx + 1;  // frame_idx += 1 before sampling (:136)
    const PushRange pr = pending ? push_of(sp, c->pos, c->size, c->max_prio) : PushRange{0, 0, sp.cap, 0.f};
    const uint64_t key = sp.seed_env;
    per_sample_block(
        size >= sp.batch, size, per_tree(sp.per_work, sp.cap), pr, beta_of(sp, frame), b * PER_BS,
        min(sp.batch, b * PER_BS + PER_BS), sm,
        [&](int j) {
            const U4 r = philox64((uint32_t)j, TAG_PER, (uint64_t)frame, key);
            return u53(r.x, r.y);
        },
        [&](int j, int64_t idx, float w) {
            sp.idx[j] = idx;
            sp.isw[j] = w;
        });
}

// The env blocks' replay rows, state and observation rows go out write-through (pm_dev.h st_out):
// none of it is re-read from this L2 before the kernel boundary. PM_ENV_WT=0 builds plain stores.
#ifndef PM_ENV_WT
#define PM_ENV_WT 7
#endif
constexpr bool kEnvWTRows = (PM_ENV_WT & 1) != 0, kEnvWTState = (PM_ENV_WT & 2) != 0, kEnvWTObs = (PM_ENV_WT & 4) != 0;
constexpr bool kEnvWTPrio = (PM_ENV_WT & 8) != 0;  // prios and the PER leaf of the pushed rows
// frow (the U > 1 path's feature rows): eight 16-byte pieces per lane at a 32-byte stride, the narrow
// pattern that write-through makes slower; plain stores, as they were while bit 1 was off
constexpr bool kEnvWTFrow = (PM_ENV_WT & 16) != 0;

// Actions ahead (pm_sp_learn.hip, feat_tiles_ahead): sp.gB holds modelB's greedy actions for this step.
__device__ __forceinline__ bool gb_current(const pm_selfplay& sp) {
    return sp.featB && sp.gB && sp.gB_ready && !sp.frow;
}

// k_env's last ceil(2B/128) blocks (plain step): rows f * 128 .. of the batch (s rows, then s').
// pending = false (updates 1..U-1, k_batch_fwd): no push is in flight, this block computes every row.
__device__ __forceinline__ void env_fwd_block(const pm_selfplay& sp, int f, bool pending = true) {
    __shared__ __attribute__((aligned(16))) float lw[kLwFloats];
    __shared__ __attribute__((aligned(16))) float hf[2][264];
    if (!learner_active(sp)) return;  // block-uniform
    stage_frags_lds(sp.w_B, lw, f * 5);
    for (int k = threadIdx.x; k < 2 * 264; k += blockDim.x) hf[k / 264][k % 264] = sp.learn_heads[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, B = sp.batch;
    const int r0 = f * 128 + (int)(threadIdx.x >> 6) * 32;
    if (r0 >= 2 * B) return;  // wave-uniform
    const int r = min(r0 + (lane & 31), 2 * B - 1);
    const bool nxt = r >= B;
    const int j = nxt ? r - B : r;
    const int64_t id = sp.idx[j];
    const pm_ctrl* c = sp.ctrl;
    const bool mine = r0 + (lane & 31) < 2 * B && !(pending && push_of(sp, c->pos, c->size, c->max_prio).covers(id));
    f32x16 c2[2];
    float qb[3], qt[3];
    float rb[2];
    batch_row_fwd(sp, lw, hf[0], hf[1], id, nxt, lane, c2, qb, qt, rb);
    if (mine) store_hfeat(sp.hfeat, j, nxt, lane, c2, qb, qt, rb);
}

// Both players act (train_iterative.py:240-241) on the matrix cores: ActGrid blocks, modelB tiles
// with epsilon-greedy, opponent tiles grouped by net (modelA / pool) so weights are tile-uniform.
// Blocks [0, ceil(batch/64)) sample the update's batch instead (latency-bound, hidden under the act).
// part: PM_ACT_ALL (sample + side B + side A), PM_ACT_B (sample + side B), PM_ACT_A (side A only:
// the opponents' greedy actions depend on nothing the learner writes, so the overlapped step runs
// them for the next vector step beside k_learn).
union ActSpShared {
    ActShared act;
    PerSampleSmem per;
};
__global__ __launch_bounds__(kActBlock, 4) void k_act_sp(const pm_selfplay sp, int part) {
    __shared__ __attribute__((aligned(16))) ActSpShared sh;
    PM_BLK(0);
    const int nsb = part == PM_ACT_A ? 0 : (sp.batch + PER_BS - 1) / PER_BS;
    {   // parts A / ALL with featB: modelB's features for these observations, blocks after the act grid
        const ActGrid g{sp.n, sp.n_pool + 1, sp.chunk_A, sp.chunk_P, part == PM_ACT_A ? 0 : 1};
        const int fb = (int)blockIdx.x - nsb - g.blocks();
        if (fb >= 0) {  // block-uniform
            const int t0 = fb * kFeatTilesAct;
            feat_tiles(sh.act.lw, sp.w_B, sp.obsB, sp.n, t0, min(t0 + kFeatTilesAct, feat_ntiles(sp.n)), sp.featB);
            return;
        }
    }
    if ((int)blockIdx.x < nsb) {
        PM_STAMP(64);
        sample_block(sp, (int)blockIdx.x, true, sh.per);
        PM_STAMP(65);
        PM_BLK_END();
        return;
    }
    if ((int)blockIdx.x == nsb) PM_STAMP_ANY(70);
    const ActGrid g{sp.n, sp.n_pool + 1, sp.chunk_A, sp.chunk_P, part == PM_ACT_A ? 0 : 1};
    const TileOut outA{sp.aA, nullptr, -1.0, 0, 0};
    const TileOut outB{sp.aB, nullptr, -1.0, 0, 0};  // greedy here; k_env applies the epsilon draw
    act_block(sh.act, g, sp.w_opp, sp.n_pool > 0 ? sp.opp : nullptr, sp.w_B, sp.obsA, sp.obsB, outA, outB,
              (int)blockIdx.x - nsb, sp.n_pool + 1 <= kListNets ? sp.opp_list : nullptr, sp.opp_cnt);
    PM_BLK_END();
}

// The fused step's sampler blocks: block b draws samples [8 b, 8 b + 8) (per_sample_block) and then
// computes their stable rows' forward itself, as one 16-column tile on v_mfma_f32_16x16x4_f32 in
// k_rollout16's layout (pm_mfma.h "16-column tiles"): columns 0-7 are the samples' s rows, columns 8-15
// their s' rows, so no other block waits for the sample and no descent runs twice. Wave rt owns units
// 16 rt .. 16 rt + 15 of both layers: layer 1 is 2 MFMAs, layer 2 is 16, each handed on through LDS in
// the next stage's k order; wave 0 then runs both head sets (learn_heads: Q_B on every column, Q_T for
// the s' columns) as one chain of 32 v_mfma_f32_4x4x1_f32. Every accumulator chain has tile_hidden's /
// tile_heads' k order, so every stored value is bit-identical to batch_row_fwd's (a wave's layer chain
// is 18 MFMAs of 32 cycles, where the 32-row tiles split by layer-2 tile ran 40 of 64).
constexpr int kSampBlock = 8;  // samples per sampler block: half a 16-column tile
struct SampleFwd16Smem {
    PerSampleSmem per;
    int64_t sidx[kSampBlock];
    __attribute__((aligned(16))) float h1s[4][4][16][4];  // [g][s >> 2][col][s & 3]: layer-2 B of instruction s
    __attribute__((aligned(16))) float c2s[2][8][16][4];  // [h][q >> 2][col][q & 3]: ReLU(layer 2), chain order
    __attribute__((aligned(16))) float hf[pad256(2 * 264)];  // learn_heads: set 0 = Q_B's heads, set 1 = Q_T's
    __attribute__((aligned(16))) float opw[2][2][4][32];     // [set]: heads_to_opw of hf[264 set ..]
};
__device__ __forceinline__ void sample_fwd_block16(const pm_selfplay& sp, int b, SampleFwd16Smem& sm) {
    constexpr int NS = kSampBlock;
    // The control block is read once, here, in the chunk sums' round trip (sample_block's fields, with
    // the pending push): `active`, the push range of `mine` and beta all come from these values. A
    // second read after the descent is a dependent round trip in front of the row loads. pm_ctrl is
    // written by the learner launches (k_learn / k_adam: apply_finish and max_prio; k_commit;
    // k_learn_multi) and k_tree_repaired; the stream orders every one of them before or after this
    // launch, none runs beside it.
    const pm_ctrl* c = sp.ctrl;
    const int64_t csize = c->size, cpos = c->pos, cframe = c->frame_idx;
    const float cmaxp = c->max_prio;
    const int64_t s = csize + sp.n;
    const int64_t size = s < sp.cap ? s : sp.cap;
    const int64_t frame = cframe + 1;  // frame_idx += 1 before sampling (:136)
    const bool active = size >= sp.batch;  // learner_active(sp)
    const PushRange pr = push_of(sp, cpos, csize, cmaxp);
    const double beta = beta_of(sp, frame);
    const uint64_t key = sp.seed_env;
    const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int rt = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // this lane's sample (q == 0 lanes of wave 0's first half) as the descent leaves it: the leaf and
    // the total of its IS weight, which is formed behind the row loads below (only k_learn reads isw)
    int wj = -1;
    double wpa = 0.0, wtot = 1.0;
    // The wave's A operands come from w_B's fragment image (pm_mfma.h F_W1 / F_W2, the 32-row tiles'
    // operand order: the same floats as the plain weights). A 16 x 16 x 4 lane (row 16 rt + col, k group g)
    // finds its operands there as whole float4s: layer 1's two (input k' = g and 4 + g) are elements
    // g >> 1 and 2 + (g >> 1) of the row's F_W1 quad in lane half g & 1; layer 2's instruction i
    // multiplies unit l2_unit(4 i + g), which is element 2 (i & 1) + (g >> 1) of F_W2 quad
    // (t = i >> 3, rq = (i & 7) >> 1) of the same row and lane half. So a wave loads 9 float4s whose
    // lanes form two 256-byte runs each (36 cache lines; gathering the 18 floats from the plain weights
    // touched 16 lines per load and held the level-1 loads behind it back by 1.3 us), plus the b2 quad
    // its accumulator starts from. They are issued right behind the level-1 (sub sum) loads and the LDS
    // DMA of the two head sets right behind the leaf loads (pm_per.h l1issued / l0issued): in front of
    // the chunk sums they would stand in that round trip, and in front of the sub sums, where they stood
    // before, the sub sums' wait counted all ten of them (vmcnt retires in issue order; level 2 -> level 1
    // 1.08 -> 0.76 us). With LDS DMA in flight hipcc waits vmcnt(0) at the next use of a plain load, so
    // the DMA goes behind the descent's last loads. Nothing here is consumed inside a hook: a load used
    // there would hold its wave for a round trip of its own.
    float4 f1 = make_float4(0.f, 0.f, 0.f, 0.f), f2[8], b2r = f1;
#pragma unroll
    for (int m = 0; m < 8; ++m) f2[m] = f1;
    per_sample_block<true>(
        active, size, per_tree(sp.per_work, sp.cap), pr, beta, b * NS, min(sp.batch, b * NS + NS), sm.per,
        [&](int j) {
            const U4 r = philox64((uint32_t)j, TAG_PER, (uint64_t)frame, key);
            return u53(r.x, r.y);
        },
        [&](int j, int64_t idx, double pa, double total) {
            sp.idx[j] = idx;
            sm.sidx[j - b * NS] = idx;
            wj = j;
            wpa = pa;
            wtot = total;
        },
        [&] {
            const float* w = sp.w_B;
            const int jt = rt >> 1, fl = 32 * (g & 1) + 16 * (rt & 1) + col;  // the row's tile and fragment lane
            f1 = reinterpret_cast<const float4*>(w + PLAIN + F_W1)[jt * 64 + fl];
            const float4* q2 = reinterpret_cast<const float4*>(w + PLAIN + F_W2) + jt * 8 * 64 + fl;
#pragma unroll
            for (int m = 0; m < 8; ++m) f2[m] = q2[m * 64];
            b2r = *reinterpret_cast<const float4*>(w + B2 + 16 * rt + 4 * g);
        },
        [&] { copy_lds_f32x4<2 * 264>(sp.learn_heads, sm.hf); });
    if (!active) return;  // block-uniform
    __syncthreads();  // sidx, the staged heads
    PM_BLK(1);
    const int B = sp.batch;
    const bool nxt = col >= NS;  // columns 0-7: s rows, 8-15: s' rows of the same samples
    const int j = b * NS + (col & (NS - 1));
    const int64_t id = sm.sidx[min(j, B - 1) - b * NS];
    const bool mine = j < B && !pr.covers(id);
    // The row's loads (the lane's two layer-1 inputs, then reward and action|done bits, which only wave
    // 0 stores: behind a wave-uniform branch they cost every wave a vmcnt(0) at its second input), then
    // the weight: in this order hipcc issues the loads back to back and starts the weight's fp64 code
    // after the last. The weight is stored at the block's end: vmcnt counts stores, and a store between
    // the loads and layer 1 would have its acknowledgement waited for there.
    const float* tr = sp.trans + id * PM_TRANS_F;
    const float* o = tr + (nxt ? 8 : 0);
    const float o0 = o[g == 0 ? 0 : g - 1];
    const float x1 = o[3 + g];
    const float rb0 = tr[7], rb1 = tr[15];
    // waves 2-3 (their lanes hold no sample) rearrange one head set each by output, under the row loads
    if (rt >= 2) heads_to_opw(sm.opw, rt - 2, sm.hf + (rt - 2) * 264);
    float wisw = 0.f;
    if (wj >= 0) wisw = per_is_weight(size, wpa, wtot, beta);
    // this lane's elements of the quads (selects, under the row loads)
    const bool odd = (g >> 1) != 0;
    const float w1r[2] = {odd ? f1.y : f1.x, odd ? f1.w : f1.z};
    float w2r[16];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        w2r[2 * m] = odd ? f2[m].y : f2[m].x;
        w2r[2 * m + 1] = odd ? f2[m].w : f2[m].z;
    }
    // layer 1, the wave's row tile (K 8: bias + 7 inputs, input k' = 4 s + g) -> ReLU -> LDS
    {
        const float x0 = g == 0 ? 1.0f : o0;
        const f32x4v16 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4v16 c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[0], x0, zero, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r[1], x1, c1, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // unit 16 rt + 4 g + r -> its slot in layer 2's k order
            const int q = l2_pos(16 * rt + 4 * g + r), sq = q >> 2;
            sm.h1s[q & 3][sq >> 2][col][sq & 3] = relu(c1[r]);
        }
    }
    __syncthreads();  // layer 1, opw
    // lane 32 set + 16 h + 4 cg + j's head A operands, the weights of output j of the set's half h, and
    // the set's biases: wave 0's, read here so that they retire under layer 2 (every wave reads them: a
    // wave-uniform branch costs the other waves 36 register clears at its join)
    float hw4[32];
    {
        const float* src = sm.opw[lane >> 5][(lane >> 4) & 1][lane & 3];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 w = *reinterpret_cast<const float4*>(src + 4 * k);
            hw4[4 * k] = w.x; hw4[4 * k + 1] = w.y; hw4[4 * k + 2] = w.z; hw4[4 * k + 3] = w.w;
        }
    }
    const float4 bhr = *reinterpret_cast<const float4*>(sm.hf + (lane >> 5) * 264 + 256);
    float bs[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(sm.h1s[g][k][col]);
        bs[4 * k] = v.x; bs[4 * k + 1] = v.y; bs[4 * k + 2] = v.z; bs[4 * k + 3] = v.w;
    }
    f32x4v16 c2 = {b2r.x, b2r.y, b2r.z, b2r.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2r[i], bs[i], c2, 0, 0, 0);
    float* row = sp.hfeat + (size_t)j * 80;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int u = 16 * rt + 4 * g + r, q = head_pos(u);
        c2[r] = relu(c2[r]);
        sm.c2s[(u >> 2) & 1][q >> 2][col][q & 3] = c2[r];
    }
    // the features of s, by unit index: units 16 rt + 4 g .. + 3 of the row are this lane's accumulator
    if (mine && !nxt) *reinterpret_cast<float4*>(row + 16 * rt + 4 * g) = make_float4(c2[0], c2[1], c2[2], c2[3]);
    __syncthreads();  // layer 2
    if (rt != 0) return;
    if (wj >= 0) sp.isw[wj] = wisw;  // wave 0's lanes
    // Heads on the matrix cores, as k_rollout16's wave 0: lane block (set, h, column group) multiplies
    // the 4 outputs' weights by 4 columns' ReLU(layer 2), so lane 32 set + 16 h + col ends with the four
    // partial sums of tile_heads' half chains of its column, in tile_heads' fmaf order.
    const int set = lane >> 5, hh = (lane >> 4) & 1;
    float xb[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(sm.c2s[hh][k][col]);
        xb[4 * k] = x.x; xb[4 * k + 1] = x.y; xb[4 * k + 2] = x.z; xb[4 * k + 3] = x.w;
    }
    f32x4v16 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 32; ++q) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(hw4[q], xb[q], acc, 0, 0, 0);
    // + the other half (both lanes get the same bits), the biases, Q = V + (A - mean(A))
    float v = xor16_sum(acc[0]), a0 = xor16_sum(acc[1]), a1 = xor16_sum(acc[2]), a2 = xor16_sum(acc[3]);
    v += bhr.x;
    a0 += bhr.y;
    a1 += bhr.z;
    a2 += bhr.w;
    const float mean = ((a0 + a1) + a2) / 3.0f;  // A.mean(dim=1)
    const float q0 = v + (a0 - mean), q1 = v + (a1 - mean), q2 = v + (a2 - mean);
    if (mine && hh == 0) {
        if (set == 0) {  // Q_B
            float* qd = row + (nxt ? 68 : 64);
            qd[0] = q0; qd[1] = q1; qd[2] = q2;
            if (!nxt) {
                row[67] = rb0;  // reward
                row[71] = rb1;  // action | done << 8 (float bits)
            }
        } else if (nxt) {  // Q_T, stored for s' only
            row[72] = q0; row[73] = q1; row[74] = q2;
        }
    }
}

__device__ __forceinline__ void write_opp_lists(const pm_selfplay& sp, OppListSmem& sm, int blk, int i, bool valid,
                                                int net) {
    write_opp_lists(sp.n_pool + 1, sp.opp_list, sp.opp_cnt, sm, blk, i, valid, net);
}

struct EnvSmem {
    float lds[2][kBlock][7];
    float4 rows[kBlock][4];  // the replay rows' way to whole-line stores, 4 KB per wave (wave-private)
    long long red[kBlock / 64][6];
    OppListSmem ol;
};
struct ActEnvSmem {
    EnvSmem e;
    float lw[kLwFloats];  // modelB's acting fragment image
};

// env.step (:242) + memory.push (:243) + episode bookkeeping (:245-249) + next opponent (:235-236)
// and env.reset (:238) for finished arenas of env block blk; writes next step's observations.
// ACT (the fused step, k_actenv): modelB's greedy action for the block's 256 arenas is computed here
// first (select_action_B, :126-130, the argmax side), on the matrix cores: wave w takes the two
// 32-row tiles of its own 64 arenas, so lane l's action sits in lane l (tile 0 holds rows 0-31 in
// both lane halves, tile 1 rows 32-63), with no LDS exchange. The env's state loads are issued with
// the weight staging and land under it. Without ACT (k_env) the argmax comes from k_act_sp via aB.
template <bool ACT>
__device__ __forceinline__ void env_block(const pm_selfplay& sp, int blk, EnvSmem& sm, float* lw) {
    const int i0 = blk * kBlock;
    const int i = i0 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool valid = i < sp.n;
    const int ii = valid ? i : sp.n - 1;
    const pm_ctrl* c = sp.ctrl;
    if (blk == 0) PM_STAMP_ANY(72);
    PM_ENV_STAMP(0, blk);
    PM_ENV_PLACE(blk);
    float xs[2][4];
    f32x16 fc2[2][2];  // featB: this wave's two tiles of modelB's features (computed ahead)
    // actions ahead: gB holds the greedy action (or, tile-wise, the sentinel). Nothing is staged and
    // there is no barrier; a kernel-argument condition, so block-uniform
    const bool ahead = ACT && gb_current(sp);
    if (ahead) {
    } else if (ACT && sp.featB) {
        // heads only: F_H .. F_BH of the acting image (65 float4) -> LDS; the features from featB
        if (threadIdx.x < 65)
            reinterpret_cast<float4*>(lw + F_H)[threadIdx.x] =
                reinterpret_cast<const float4*>(sp.w_B + PLAIN + F_H)[threadIdx.x];
        // featB holds feat_ntiles(n) tiles: in a ragged last block the waves past n take the last tile
        // again (their rows are stored nowhere) instead of reading up to 6 tiles past its end
        const int tlast = feat_ntiles(sp.n) - 1;
#pragma unroll
        for (int k = 0; k < 2; ++k) feat_load(sp.featB, min(blk * 8 + 2 * wv + k, tlast), lane, fc2[k]);
    } else if (ACT) {
        stage_frags_lds(sp.w_B, lw, blk);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int row = min(i0 + 64 * wv + 32 * k + (lane & 31), sp.n - 1);
            tile_inputs(sp.obsB + (size_t)row * 7, lane >> 5, xs[k]);
        }
    }
    // Every per-arena load is issued here, in one basic block, before any branch (loads placed after
    // a branch were issued only after it, one more HBM round trip). The serve counter goes first:
    // the next episode's opponent and serve are drawn for every lane while the state loads are in
    // flight (lanes that finish use them; see k_env_step).
    // The control block is read before them (vmcnt retires in issue order: what only needs ns and
    // the control words can then run while the state is still in flight).
    const uint32_t ns = (uint32_t)__builtin_nontemporal_load(&sp.st.serves[ii]);
    const int64_t pos = c->pos, size = c->size;
    const float cmaxp = c->max_prio;
    const uint64_t cstep = c->step;
    const double ceps = c->epsilon;
    const int o = sp.opp[ii];
    const float er0 = sp.ep_reward[ii];
    Arena a = load_arena(sp.st, ii);
    const int aA = sp.aA[ii];
    int aB = ACT ? (ahead ? (int)sp.gB[ii] : 0) : sp.aB[ii];
    __builtin_amdgcn_sched_barrier(0);
    const float maxp = push_prio(size, cmaxp);  // max(prios) if buffer else 1.0 (:57)
    float* leaf = per_tree(sp.per_work, sp.cap).leaf;
    const float pval = prio_pow(maxp, (float)sp.alpha);  // its PER leaf

    // Draws that need only the serve counter and the control block, pinned ahead of everything that
    // waits for the state loads:
    //   select_action_B (:126-130): random.random() < eps ? randint(0, 2) : argmax (the argmax is
    //   the act's; the draw is per-arena VALU work, cheaper here than beside the MFMAs);
    //   the next episode's opponent (:235-236) and serve (env.reset(), :238), used if this one ends.
    int onext, eps_a;
    bool eps_hit;
    double svx, svy, sspn;
    {
        const U4 rr = philox64((uint32_t)ii, TAG_ACT, cstep, sp.seed_env);
        eps_hit = u53(rr.x, rr.y) < ceps;
        eps_a = (int)below(rr.z, 3u);
        const U4 q = philox((uint32_t)ii, TAG_OPP, ns, 0u, sp.seed_env);
        onext = (sp.n_pool > 0 && u53(q.x, q.y) < sp.pool_ratio) ? 1 + below(q.z, (uint32_t)sp.n_pool) : 0;
        philox_serve(sp.env, (uint32_t)ii, ns, sp.seed_env, svx, svy, sspn);
        asm volatile("" ::"v"(onext), "v"(svx), "v"(svy), "v"(sspn), "v"(eps_hit), "v"(eps_a));
        __builtin_amdgcn_sched_barrier(0);
    }
    if (ahead) {
        // a tile whose hand-off timed out in the learner launch (all 32 arenas hold the sentinel): its
        // features are in featB; heads straight from the acting image in global memory (the same
        // values in the same order as the staged copy). Wave-uniform, no barrier.
        const unsigned long long fb = __ballot(valid && aB == PM_GB_NONE);
        if (fb) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (!(uint32_t)(fb >> (32 * k))) continue;  // wave-uniform
                float q[3];
                feat_load(sp.featB, blk * 8 + 2 * wv + k, lane, fc2[k]);
                tile_heads(sp.w_B + PLAIN + F_H, fc2[k], lane, q);
                if ((lane >> 5) == k) aB = argmax3(q);
            }
        }
        if (!valid) aB = 0;  // lanes past n read arena n - 1's byte (possibly the sentinel); nothing of theirs is stored
        PM_ENV_STAMP(7, blk);
    } else if (ACT) {
        __syncthreads();  // the fragment image is staged (every load of the block has landed)
        PM_ENV_STAMP(7, blk);
        int act[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float q[3];
            if (sp.featB) {
                tile_heads(lw + F_H, fc2[k], lane, q);
            } else {
                f32x16 c2[2];
                tile_hidden(lw, xs[k], lane, c2);
                tile_heads(lw + F_H, c2, lane, q);
            }
            act[k] = argmax3(q);
            if (sp.featB && sp.frow) {  // k_learn_multi's features of s: ReLU(layer 2) of this push's rows
                const int ar = i0 + 64 * wv + 32 * k + (lane & 31);
                if (ar < sp.n) {
                    int64_t slot = pos + ar;
                    if (slot >= sp.cap) slot -= sp.cap;
                    float4* fr = reinterpret_cast<float4*>(sp.frow + slot * 64) + (lane >> 5);
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4)  // units 32 jt + 8 q4 + 4 h + 0..3
                            st_f4<kEnvWTFrow>(fr + 8 * jt + 2 * q4,
                                              make_float4(relu(fc2[k][jt][4 * q4]), relu(fc2[k][jt][4 * q4 + 1]),
                                                          relu(fc2[k][jt][4 * q4 + 2]), relu(fc2[k][jt][4 * q4 + 3])));
                }
            }
        }
        aB = lane < 32 ? act[0] : act[1];
    }
    PM_ENV_STAMP(1, blk);
    if (eps_hit) aB = eps_a;
    float oA[7], oB[7];
    observe(a, oA, oB);  // the state the actions were chosen on (= obs of the previous env kernel)
    float rA, rB;
    const int d = tick(sp.env, a, aA, aB, rA, rB);
    float nA[7], nB[7];
    observe(a, nA, nB);
#ifdef PM_DIAG
    asm volatile("" ::"v"(nA[0]), "v"(nB[1]), "v"(d));
#endif
    PM_ENV_STAMP(2, blk);
    const float er = er0 + rB;  // ep_reward += rB (:245)
    const bool fin = valid && d;
    {   // per-block partials, no atomics (:247-249)
        const bool win = er > 0.f;
        const unsigned long long mf = __ballot(fin), mA = __ballot(fin && o == 0), mwA = __ballot(fin && o == 0 && win);
        const unsigned long long mP = __ballot(fin && o != 0), mwP = __ballot(fin && o != 0 && win);
        const int rs = wave_sum(fin ? (int)er : 0);
        if (lane == 0) {
            sm.red[wv][0] = __popcll(mf); sm.red[wv][1] = __popcll(mA); sm.red[wv][2] = __popcll(mwA);
            sm.red[wv][3] = __popcll(mP); sm.red[wv][4] = __popcll(mwP); sm.red[wv][5] = rs;
        }
    }
    int onew = o;
    {
        // memory.push((oB, aB, rB, nB, done)) (:243, :56-63): the wave's 64 rows as whole lines, every
        // lane taking part (pm_dev.h store_ring_rows16; a lane past n holds arena n - 1's values, which
        // are stored nowhere).
        // write-through (pm_dev.h st_out): the ring is re-read only by later samples, and the state and
        // observation rows only by later launches, so none of it stays dirty in L2 for the boundary
        static_assert(PM_TRANS_F == 16, "store_ring_rows16 writes 64-byte rows");
        const float4 piece[4] = {make_float4(oB[0], oB[1], oB[2], oB[3]), make_float4(oB[4], oB[5], oB[6], rB),
                                 make_float4(nB[0], nB[1], nB[2], nB[3]),
                                 make_float4(nB[4], nB[5], nB[6], __int_as_float(aB | (d << 8)))};
        store_ring_rows16<kEnvWTRows>(sp.trans, pos, sp.cap, i0 + 64 * wv, sp.n, sm.rows + 64 * wv, piece);
    }
    if (valid) {
        int64_t slot = pos + i;  // pos < cap and i < n <= cap: one conditional subtract is the modulo
        if (slot >= sp.cap) slot -= sp.cap;  // (a per-lane 64-bit % is a ~100-instruction expansion)
        st_out<kEnvWTPrio>(&sp.prios[slot], maxp);
        st_out<kEnvWTPrio>(&leaf[slot], pval);
        float ernew = er;
        if (d) {  // next episode: the opponent and serve drawn above
            onew = onext;
            serve(a, svx, svy, sspn);
            sp.st.serves[i] = (int32_t)ns + 1;
            ernew = 0.f;
            observe(a, nA, nB);
        }
        store_arena<kEnvWTState>(sp.st, i, a);
        sp.opp[i] = onew;
        sp.aB[i] = (int8_t)aB;  // the action taken
        sp.ep_reward[i] = ernew;
    }
    PM_ENV_STAMP(3, blk);
#pragma unroll
    for (int k = 0; k < 7; ++k) { sm.lds[0][threadIdx.x][k] = nA[k]; sm.lds[1][threadIdx.x][k] = nB[k]; }
    __syncthreads();
    PM_ENV_STAMP(4, blk);
    if (threadIdx.x < 6) {
        long long t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += sm.red[w][threadIdx.x];
        sp.partials[(size_t)blk * 8 + threadIdx.x] = t;
    }
    write_opp_lists(sp, sm.ol, blk, i, valid, onew);
    PM_ENV_STAMP(5, blk);
    copy_rows7<kEnvWTObs>(sp.obsA, sm.lds[0], i0, sp.n);
    copy_rows7<kEnvWTObs>(sp.obsB, sm.lds[1], i0, sp.n);
    PM_ENV_STAMP_DRAIN(6, blk);
}

// The plain step's env kernel: env blocks first, then the learner-forward blocks (measured:
// dispatching the forward blocks first lengthens the kernel by ~1 us; last, they finish inside the
// env blocks' time).
__global__ __launch_bounds__(kBlock) void k_env(const pm_selfplay sp) {
    const int blk = (int)blockIdx.x;
    const int nenv = (sp.n + kBlock - 1) / kBlock;
    if (blk >= nenv) {
        env_fwd_block(sp, blk - nenv);
        return;
    }
    __shared__ __attribute__((aligned(16))) EnvSmem sm;
    env_block<false>(sp, blk, sm, nullptr);
}

// The fused step's first kernel (pm_selfplay_actenv): blocks [0, ceil(B/8)) sample the update's batch
// and compute its stable rows (sample_fwd_block16); every other block acts for modelB and ticks its 256
// arenas (env_block<true>). Replaces k_act_sp(PM_ACT_B) + k_env of the overlapped step, bit for bit.
union ActEnvShared {
    ActEnvSmem ae;
    SampleFwd16Smem sf16;
};
__global__ __launch_bounds__(kBlock) void k_actenv(const pm_selfplay sp) {
    __shared__ __attribute__((aligned(16))) ActEnvShared sh;
    const int nsb = (sp.batch + kSampBlock - 1) / kSampBlock;  // sampler blocks, 8 samples each
    if ((int)blockIdx.x < nsb) {
        PM_BLK(0);
        sample_fwd_block16(sp, (int)blockIdx.x, sh.sf16);
        PM_BLK_END();
        return;
    }
    env_block<true>(sp, (int)blockIdx.x - nsb, sh.ae.e, sh.ae.lw);
}

// ------------------------------------------------------------------------------------ init
__global__ __launch_bounds__(kBlock) void k_sp_init(const pm_selfplay sp) {
    __shared__ __attribute__((aligned(16))) float lds[kBlock][7];
    const int i0 = blockIdx.x * kBlock;
    const int i = i0 + threadIdx.x;
    float oA[7] = {0}, oB[7] = {0};
    int net = 0;
    if (i < sp.n) {
        const uint32_t ns = (uint32_t)sp.st.serves[i];
        const U4 q = philox((uint32_t)i, TAG_OPP, ns, 0u, sp.seed_env);
        net = (sp.n_pool > 0 && u53(q.x, q.y) < sp.pool_ratio) ? 1 + below(q.z, (uint32_t)sp.n_pool) : 0;
        sp.opp[i] = net;
        Arena a;
        double vx, vy, spn;
        philox_serve(sp.env, (uint32_t)i, ns, sp.seed_env, vx, vy, spn);
        serve(a, vx, vy, spn);
        store_arena(sp.st, i, a);
        sp.st.serves[i] = (int32_t)ns + 1;
        sp.ep_reward[i] = 0.f;
        observe(a, oA, oB);
    }
    {
        __shared__ OppListSmem ol;
        write_opp_lists(sp, ol, blockIdx.x, i, i < sp.n, net);
    }
    store_rows7(sp.obsA, lds, oA, i0, sp.n);
    store_rows7(sp.obsB, lds, oB, i0, sp.n);
}

// ------------------------------------------------------------------------------------ U > 1 updates
// Updates 1..U-1 of a vector step: the PER sample over the replay as this step's push left it (one
// wave per sample), then the batch forward of every row (no pending push: k_env's forward blocks'
// job, on their own launch).
__global__ __launch_bounds__(256) void k_resample(const pm_selfplay sp) {
    __shared__ PerSampleSmem sm;
    sample_block(sp, (int)blockIdx.x, false, sm);
}
__global__ __launch_bounds__(kBlock) void k_batch_fwd(const pm_selfplay sp) { env_fwd_block(sp, (int)blockIdx.x, false); }

namespace {
int launch_act(const pm_selfplay* sp, int part, hipStream_t st) {
    const ActGrid g{sp->n, sp->n_pool + 1, sp->chunk_A, sp->chunk_P, part == PM_ACT_A ? 0 : 1};
    const int nsb = part == PM_ACT_A ? 0 : (sp->batch + PER_BS - 1) / PER_BS;
    int blocks = part == PM_ACT_B ? nsb + g.nb() : nsb + g.blocks();
    if (part != PM_ACT_B && sp->featB) blocks += (feat_ntiles(sp->n) + kFeatTilesAct - 1) / kFeatTilesAct;
    hipLaunchKernelGGL(k_act_sp, dim3(blocks), dim3(kActBlock), 0, st, *sp, part);
    PM_LAUNCHED("k_act_sp");
    return PM_OK;
}
}  // namespace

int pm::selfplay_launch_init(const pm_selfplay* sp, hipStream_t st) {
    hipLaunchKernelGGL(k_sp_init, dim3(pm_blocks(sp->n, kBlock)), dim3(kBlock), 0, st, *sp);
    PM_LAUNCHED("k_sp_init");
    return PM_OK;
}

extern "C" int pm_selfplay_act(const pm_selfplay* sp, void* stream) {
    return pm_selfplay_act_part(sp, PM_ACT_ALL, stream);
}

extern "C" int pm_selfplay_act_part(const pm_selfplay* sp, int32_t part, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    PM_REQUIRE(part == PM_ACT_ALL || part == PM_ACT_B || part == PM_ACT_A, PM_E_ARG,
               "pm_selfplay_act_part: part=%d", part);
    return launch_act(sp, part, pm_stream(stream));
}

extern "C" int pm_selfplay_env(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    const unsigned nfwd = pm_blocks(2 * sp->batch, 128);  // batch rows not in the push range (env_fwd_block)
    hipLaunchKernelGGL(k_env, dim3(pm_blocks(sp->n, kBlock) + nfwd), dim3(kBlock), 0, pm_stream(stream), *sp);
    PM_LAUNCHED("k_env");
    return PM_OK;
}

extern "C" int pm_selfplay_actenv(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    const unsigned nsb = pm_blocks(sp->batch, kSampBlock);  // sampler blocks (sample_fwd_block16)
    pm_launch(PM_TIMER_ACTENV, k_actenv, dim3(nsb + pm_blocks(sp->n, kBlock)), dim3(kBlock), pm_stream(stream), *sp);
    PM_LAUNCHED("k_actenv");
    return PM_OK;
}

extern "C" int pm_selfplay_rollout(const pm_selfplay* sp, void* stream) {
    int rc = pm_selfplay_act(sp, stream);
    return rc ? rc : pm_selfplay_env(sp, stream);
}

extern "C" int pm_selfplay_resample(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    hipStream_t st = pm_stream(stream);
    hipLaunchKernelGGL(k_resample, dim3((sp->batch + PER_BS - 1) / PER_BS), dim3(256), 0, st, *sp);
    PM_LAUNCHED("k_resample");
    hipLaunchKernelGGL(k_batch_fwd, dim3(pm_blocks(2 * sp->batch, 128)), dim3(kBlock), 0, st, *sp);
    PM_LAUNCHED("k_batch_fwd");
    return PM_OK;
}

#ifdef PM_DIAG
// This unit's copies of the stamp buffers (pm_dev.h): what k_act_sp / k_env / k_actenv wrote.
extern "C" int pm_diag_read_sp_rollout(uint64_t* out, int32_t n) {  // pm_diag_buf: slots 64, 65, 70 (k_act_sp), 72 (env block 0)
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_buf), sizeof(uint64_t) * (n < 256 ? n : 256));
    return e == hipSuccess ? 0 : (int)e;
}
extern "C" int pm_diag_clear_sp_rollout(void) {
    static const unsigned long long z[256] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(pm_diag_buf), z, sizeof(z));
}
extern "C" int pm_diag_read_blk(uint64_t* out) {  // k_act_sp's blocks / k_actenv's sampler blocks
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_blk), sizeof(uint64_t) * 8 * 4096);
}
extern "C" int pm_diag_read_env(uint64_t* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_env), sizeof(uint64_t) * 8 * 1024);
}
extern "C" int pm_diag_read_env_place(uint64_t* out) {  // the env blocks' CU | XCC << 16
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_env_place), sizeof(uint64_t) * 1024);
}
#endif
