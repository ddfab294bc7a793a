// K9 — self-play rollout, K vector steps per launch (BASELINE configs[1]).
//
// The rollout of scripts/train_iterative.py:239-242 for n arenas in lockstep: per vector step both
// players act — modelA greedy on its folded weights (:240; modelA keeps NoisyNet's frozen epsilon
// buffers), modelB NoisyNet with fresh noise per vector step shared by all arenas (reset_noise in
// select_action_B, :125) and epsilon-greedy (:126-130) — then PongEnv2P.step ticks every arena and
// finished ones are served again (the step-keyed Philox serve of pm_env_step's production autoreset).
// Stepped as launches, one vector step is three kernels (fold, act, env) that move the fp64 state and
// the observations through HBM; here every arena stays in registers for all K steps and only its final
// state leaves the CU.
//
// Two kernels per launch:
//   k_rollout_heads — one block per step folds modelB's heads with that step's noise (gen_noise +
//     fold_heads_from, exactly pm_qnet_fold FRESH) into the F_H/F_BH fragment order: 264 floats per
//     step in a caller workspace (PM_ROLL_HEADS);
//   then one of
//   k_rollout16 (pm_rollout, inference only) — a block of 8 waves owns one tile of 16 arenas: 4 096
//     arenas are 256 blocks, one per CU. The forwards run as 16 x 16 x 4 MFMAs split over the waves by
//     player and row tile, the head chains as 4 x 4 x 1 MFMAs on wave 0, which also keeps and ticks the
//     fp64 arenas (the comment above kR16Block);
//   k_rollout_push (pm_rollout_push, §8f3, the collecting rollout) — a block of 4 waves owns one tile of
//     32 arenas (65 536 arenas, 16 blocks per CU queued) and also writes every vector step's
//     transitions straight from registers into the replay ring, as memory.push((oB, aB, rB, nB, done))
//     does in the training loop (train_iterative.py:242-243, :56-63): one 64-byte row (s[7], r, s'[7],
//     bits(aB | done << 8)), its priority and its PER leaf, with ep_reward carried per arena (:238,
//     :245) and the episodes' win / reward counts (:247-249). 16-arena tiles lose here: 4 096 queued
//     blocks that each tick their arenas on one wave of eight ran 688 against 298 us per 15-step launch.
// In both, the block's last wave streams the next step's heads global -> LDS (global_load_lds, 1 KB,
// double-buffered) while it computes the current step, so the heads never cost a round trip on the
// step's critical path, and the step-keyed serve and player B's epsilon branch, pure functions of
// (arena, step, seed), are drawn a step ahead by waves that would otherwise idle during the tick.
//
// Bit-identical to `steps` repetitions of pm_qnet_fold(paramsB, FRESH, seed_net, c) ->
// pm_qnet_act({wA}, NULL, w_B, obsA, obsB, epsilon, seed_env, c) -> pm_env_step(autoreset, seed_env,
// c) with c = counter0 + s (tests/test_gpu_rollout.py).
#include <cmath>

#include "pm_host.h"
#include "pm_mfma.h"
#include "pm_per.h"

using namespace pm;

namespace {

// The heads fold, the heads fetches, the serve draw and the collecting launch's body (rollout_push_body, with
// the comment on its wave roles and register budget): shared as text with pm_rollout_pop.hip.
#include "pm_rollout_push.inc"

__global__ __launch_bounds__(kHeadsBlock) void k_rollout_heads(const float* __restrict__ paramsB, uint64_t seed_net,
                                                               uint64_t counter0, float* __restrict__ ws) {
    rollout_heads_body(paramsB, seed_net, counter0, ws, blockIdx.x);
}

// 65 536 arenas are 16 blocks per CU queued: capped at 168 registers the kernel fits 3 waves per SIMD,
// 19.9 against 21.0 us per vector step with the compiler's own budget (same-box A/B,
// profiles/r3_roll_ab.txt).
__global__ __launch_bounds__(kRollBlock) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_rollout_push(
    const pm_env_params p, const pm_env_state s, const float* __restrict__ wA, const float* __restrict__ wB,
    const float* __restrict__ ws, double eps, uint64_t seed_env, uint64_t counter0, int steps,
    float* __restrict__ obsA, float* __restrict__ obsB, long long* __restrict__ stats, int n, const RollPush rp) {
    rollout_push_body<false>(p, s, wA, wB, ws, eps, seed_env, counter0, steps, obsA, obsB, stats, n, rp, RollN{},
                             blockIdx.x);
}

// pm_rollout_push_n with nstep > 1: the same launch with wave 3's n-step window (nstep_push). The window's 9 KB
// of LDS leave two blocks per CU, so the kernel takes the compiler's own register budget instead of the cap.
__global__ __launch_bounds__(kRollBlock) void k_rollout_push_n(
    const pm_env_params p, const pm_env_state s, const float* __restrict__ wA, const float* __restrict__ wB,
    const float* __restrict__ ws, double eps, uint64_t seed_env, uint64_t counter0, int steps,
    float* __restrict__ obsA, float* __restrict__ obsB, long long* __restrict__ stats, int n, const RollPush rp,
    const RollN rn) {
    rollout_push_body<true>(p, s, wA, wB, ws, eps, seed_env, counter0, steps, obsA, obsB, stats, n, rp, rn,
                            blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------
// The inference launch, on 16-arena tiles: v_mfma_f32_16x16x4_f32 is, like the 32x32x2 form, a
// k-ordered fmaf chain bit for bit (tools/mfma_order_probe.hip: 0 of 102 400 outputs differ), so a
// QNet forward computed in 16-row / 16-column tiles over the SAME k sequences as tile_hidden /
// tile_heads gives the same bits. Half the tile width doubles the tiles: 4 096 arenas are 256 blocks,
// one per CU, instead of 128 blocks on half the chip, and each block's MFMA chain is half as long.
//
// Block = 8 waves, wave 4p + rt: player p, row tile rt (16 of the 64 units) of both layers.
//   layer 1 (K 8: bias + 7 inputs, 2 MFMAs) -> ReLU -> LDS in layer 2's k order (tile_hidden's pair
//   sequence (t, r) -> units 32t + rho(r) + {0, 4}) -> layer 2 (K 64, 16 MFMAs from the bias) -> ReLU
//   -> LDS in the head chains' order -> wave 0: both players' head chains (lanes 32p + 16h + col: half
//   h of column col, tile_heads' per-half fmaf chains and cross-half add), the actions, then the fp64
//   tick of the 16 arenas (kept in wave 0's registers, replicated over its four lane groups) and the
//   next observations into LDS. Three barriers per vector step (every wave computing all four layer-1
//   tiles into a slab of its own, to drop the first, ran 4.13 us per step against 2.69:
//   profiles/r4_roll16_ab.txt). Every LDS array a lane group reads as float4 runs keeps its 16 columns
//   side by side (conflict-free ds_read_b128; the first layout, [col][64], ran 3.67 us per step).
constexpr int kR16Block = 512;

#ifdef PM_DIAG
// k_rollout16's per-step phases (diagnostic build only): waves 0 (heads + tick) and 1 (a layer wave)
// of block 0 add the s_memtime cycles between phase points over every step of the launch.
static __device__ unsigned long long pm_diag_roll[2][8];
#define ROLL_T(k)                                                                 \
    do {                                                                          \
        if (diag) {                                                               \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();         \
            dacc[(k)] += now_ - dprev;                                            \
            dprev = now_;                                                         \
        }                                                                         \
    } while (0)
#else
#define ROLL_T(k) \
    do {          \
    } while (0)
#endif

// (l2_pos / l2_unit / head_pos, the layers' hand-over orders, f32x4v16, heads_to_opw and xor16_sum:
// pm_mfma.h, shared with k_actenv's sampler blocks.)
struct Roll16Shared {
    // the layer operands of the launch: every wave reads its own into registers once (2 + 16 + 4), so
    // no step re-reads them
    __attribute__((aligned(16))) float img2[2][4][4][64][4];  // [p][rt][s4][lane][e]: layer-2 A, instruction 4 s4 + e
    __attribute__((aligned(16))) float img1[2][4][64][2];     // [p][rt][lane][s]: layer-1 A
    __attribute__((aligned(16))) float b2v[2][4][4][4];       // [p][rt][g][r]: b2[16 rt + 4 g + r]
    __attribute__((aligned(16))) float hfA[264];              // modelA's heads (F_H / F_BH order)
    __attribute__((aligned(16))) float hfB[2][320];           // modelB's heads of the step, double-buffered
    // the two staging arrays are read as float4 runs whose 16 lanes per lane group sit side by side
    // (lane col at [..][col][4]): one ds_read_b128 pass per lane group, no bank conflict
    __attribute__((aligned(16))) float h1s[2][4][4][16][4];   // [p][g][s >> 2][col][s & 3]: layer-2 B of instruction s
    __attribute__((aligned(16))) float c2s[2][2][8][16][4];   // [p][h][q >> 2][col][q & 3]: ReLU(layer 2), chain order
    float ob[2][16][8];                                       // [p][col]: the observations of the step
    // the draws of step st (buffer st & 1), made by waves 1 and 2 during step st - 1's heads + tick (an
    // idle window of those waves): the step-keyed serve (used if the arena's episode ends) and player
    // B's epsilon branch (-1: the argmax stands, else the random action)
    ServeDraw sdraw[2][16];
    int epsa[2][16];
    // the head weights by output, opw[set][h][j][q] = weight of output j (V, A0, A1, A2) at chain
    // position q of half h; set 0 = modelA (once), 1 + b = modelB of step buffer b (rearranged from hfB
    // by wave 7 while it is idle)
    __attribute__((aligned(16))) float opw[3][2][4][32];
};

// The heads' cross-lane moves, on the gfx950 row / half swaps instead of ds_bpermute round trips on
// wave 0's chain: xor16_sum (pm_mfma.h) and halves_bcast: lanes 0-31's value in both halves (lo)
// and lanes 32-63's (hi), one v_permlane32_swap for both.
__device__ __forceinline__ void halves_bcast(int v, int& lo, int& hi) {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    lo = (int)r[0];
    hi = (int)r[1];
}

// Step ctr's per-arena draws into buffer b, split so that neither outlasts wave 0's heads + tick (a
// single drawing wave, three Philox blocks in a row behind a lane-group branch, was the last to reach
// barrier C). Wave 1: the serve's two Philox blocks at once, lane group 0 on the first tag and group
// 1 on the second, group 1's block handed to group 0 by a row swap, then the serve's fp64 stages;
// wave 2: player B's epsilon branch, philox64 keyed as K1's act draw. Pure functions of (arena,
// step, seed): drawn a step ahead, bit-identical.
__device__ __forceinline__ void roll16_serve(const pm_env_params& p, Roll16Shared& sm, int i, uint64_t ctr, int b,
                                             uint64_t seed, int g) {
    const U4 r = philox((uint32_t)i, g == 1 ? (TAG_SERVE_STEP | 0x100u) : TAG_SERVE_STEP, (uint32_t)ctr,
                        (uint32_t)(ctr >> 32), seed);
    const auto sx = __builtin_amdgcn_permlane16_swap(r.x, r.x, false, false);
    const auto sy = __builtin_amdgcn_permlane16_swap(r.y, r.y, false, false);
    const auto sz = __builtin_amdgcn_permlane16_swap(r.z, r.z, false, false);
    const auto sw = __builtin_amdgcn_permlane16_swap(r.w, r.w, false, false);
    // [1]: rows 1 and 3's block in rows 0 and 2
    const ServeDraw d = serve_from_blocks(p, r, U4{sx[1], sy[1], sz[1], sw[1]});
    if (g == 0) sm.sdraw[b][threadIdx.x & 15] = d;
}
__device__ __forceinline__ void roll16_eps(Roll16Shared& sm, int i, uint64_t ctr, int b, double eps, uint64_t seed,
                                           int g) {
    if (g == 0) {
        const U4 rr = philox64((uint32_t)i, TAG_ACT, ctr, seed);
        sm.epsa[b][threadIdx.x & 15] = u53(rr.x, rr.y) < eps ? (int)below(rr.z, 3u) : -1;
    }
}

__device__ __forceinline__ void rollout16_body(const pm_env_params& p, const pm_env_state& s, const float* __restrict__ wA,
                                               const float* __restrict__ wB, const float* __restrict__ ws, double eps,
                                               uint64_t seed_env, uint64_t counter0, int steps, float* __restrict__ obsA,
                                               float* __restrict__ obsB, long long* __restrict__ stats, int n) {
    __shared__ Roll16Shared sm;
    const int t = threadIdx.x, lane = t & 63, col = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int player = wv >> 2, rt = wv & 3;
    const int i = blockIdx.x * 16 + col;
    const bool valid = i < n;
    // ---- operand images from the plain effective weights (once per launch; global reads hit L2)
    for (int k = t; k < 2 * 4 * 4 * 64 * 4; k += kR16Block) {
        const int pp = k >> 12, r2 = (k >> 10) & 3, s4 = (k >> 8) & 3, ln = (k >> 2) & 63, e = k & 3;
        const float* w = pp ? wB : wA;
        (&sm.img2[0][0][0][0][0])[k] = w[W2 + (16 * r2 + (ln & 15)) * 64 + l2_unit(4 * (4 * s4 + e) + (ln >> 4))];
    }
    for (int k = t; k < 2 * 4 * 64 * 2; k += kR16Block) {
        const int pp = k >> 9, r2 = (k >> 7) & 3, ln = (k >> 1) & 63, sx = k & 1;
        const float* w = pp ? wB : wA;
        const int row = 16 * r2 + (ln & 15), kk = 4 * sx + (ln >> 4);  // input k' = 0 is the constant 1 (b1)
        (&sm.img1[0][0][0][0])[k] = kk == 0 ? w[B1 + row] : w[W1 + row * 7 + kk - 1];
    }
    if (t < 128) {
        const int pp = t >> 6, r2 = (t >> 4) & 3, gg = (t >> 2) & 3, r = t & 3;
        (&sm.b2v[0][0][0][0])[t] = (pp ? wB : wA)[B2 + 16 * r2 + 4 * gg + r];
    }
    if (t < 260) sm.hfA[t] = t < 256 ? wA[PLAIN + F_H + t] : wA[PLAIN + F_BH + t - 256];
    if (wv == 7) fetch_heads(ws, 0, sm.hfB[0], lane);
    if (wv == 1) roll16_serve(p, sm, i, counter0, 0, seed_env, g);
    if (wv == 2) roll16_eps(sm, i, counter0, 0, eps, seed_env, g);
    // ---- wave 0 keeps the 16 arenas (every lane group a copy) and ticks them
    Arena a{};
    int fin = 0, winB = 0, ptA = 0, ptB = 0;  // per arena: |count| <= steps < 2^31
    if (wv == 0) {
        a = load_arena(s, valid ? i : n - 1);
        float oA[7], oB[7];
        observe(a, oA, oB);
        if (g < 2)
#pragma unroll
            for (int k = 0; k < 7; ++k) sm.ob[g][col][k] = g ? oB[k] : oA[k];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wv == 7) heads_to_opw(sm.opw, 1, sm.hfB[0]);  // its own fetch of hfB[0] has landed (same wave)
    if (wv == 6) heads_to_opw(sm.opw, 0, wA + PLAIN + F_H);  // modelA's heads straight from global
    __syncthreads();
    // the wave's layer-1 and layer-2 A operands and layer-2 bias, constant over the launch
    const float4* im2 = reinterpret_cast<const float4*>(sm.img2[player][rt][0][lane]);
    float4 w2r[4];
    const float2 w1r = *reinterpret_cast<const float2*>(sm.img1[player][rt][lane]);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const float4 w = im2[s4 * 64];  // through a value: w2r[s4] = im2[..] compiles to a different kernel
        w2r[s4] = w;
    }
    const float4 b2r = *reinterpret_cast<const float4*>(sm.b2v[player][rt][g]);
#ifdef PM_DIAG
    const bool diag = blockIdx.x == 0 && wv < 2;
    unsigned long long dacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dprev = __builtin_amdgcn_s_memtime();
#endif
    for (int st = 0; st < steps; ++st) {
        const uint64_t ctr = counter0 + (uint64_t)st;
        if (wv == 7 && st + 1 < steps) fetch_heads_async(ws, st + 1, sm.hfB[(st + 1) & 1], lane);  // lands during the step
        // wave 0: lane 32 pp + 16 h + 4 cg + j's head A operands, the weights of output j of player pp's
        // half h. Read at the step's start (wave 7 wrote this step's set before the last barrier C), so
        // the reads retire under the layers instead of holding wave 0 at barrier B
        float hw4[32];
        if (wv == 0) {
            const float* src = sm.opw[(lane >> 5) ? 1 + (st & 1) : 0][(lane >> 4) & 1][lane & 3];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 w = *reinterpret_cast<const float4*>(src + 4 * k);
                hw4[4 * k] = w.x; hw4[4 * k + 1] = w.y; hw4[4 * k + 2] = w.z; hw4[4 * k + 3] = w.w;
            }
        }
        // layer 1, the wave's row tile (K 8: bias + 7 inputs, input k' = 4 s + g) -> ReLU -> LDS
        {
            const float* o = sm.ob[player][col];
            // both inputs read together (one LDS wait, not a masked read, a wait, a read, a wait)
            const float o0 = o[g == 0 ? 0 : g - 1];
            const float x0 = g == 0 ? 1.0f : o0, x1 = o[3 + g];
            const f32x4v16 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4v16 c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r.x, x0, zero, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1r.y, x1, c1, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // unit 16 rt + 4 g + r -> its slot in layer 2's k order
                const int q = l2_pos(16 * rt + 4 * g + r), sq = q >> 2;
                sm.h1s[player][q & 3][sq >> 2][col][sq & 3] = relu(c1[r]);
            }
        }
        ROLL_T(0);        // step start (barrier C) -> layer 1 issued
        __syncthreads();  // (A) the player's layer 1
        ROLL_T(1);
        float bs[16];
        {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 v = *reinterpret_cast<const float4*>(sm.h1s[player][g][k][col]);
                bs[4 * k] = v.x; bs[4 * k + 1] = v.y; bs[4 * k + 2] = v.z; bs[4 * k + 3] = v.w;
            }
        }
        f32x4v16 c2 = {b2r.x, b2r.y, b2r.z, b2r.w};

#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const float4 w = w2r[s4];
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, bs[4 * s4 + 0], c2, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, bs[4 * s4 + 1], c2, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, bs[4 * s4 + 2], c2, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, bs[4 * s4 + 3], c2, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * rt + 4 * g + r, q = head_pos(u);
            sm.c2s[player][(u >> 2) & 1][q >> 2][col][q & 3] = relu(c2[r]);
        }
        if (wv == 7) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next step's heads landed
        ROLL_T(2);        // layer 2 + staging
        __syncthreads();  // (B) both players' layer 2
        ROLL_T(3);
        if (wv == 0) {
            // heads on the matrix cores: one chain of 32 v_mfma_f32_4x4x1_16b_f32 (a k-ordered fmaf
            // chain bit for bit, tools/mfma4_probe.hip) covers every (player, half, column): block b =
            // lanes 4b..4b+3 = (pp, h, column group cg) multiplies the 4 outputs' weights (A: lane
            // 4b + j supplies output j) by 4 columns' ReLU(layer 2) (B: lane 4b + j supplies column
            // 4 cg + j), so lane 32 pp + 16 h + col ends with the four partial sums of tile_heads' half
            // chains for its column, in tile_heads' fmaf order
            const int hp = lane >> 5, hh = (lane >> 4) & 1;
            const float* hf = hp ? sm.hfB[st & 1] : sm.hfA;
            float xb[32];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 x = *reinterpret_cast<const float4*>(sm.c2s[hp][hh][k][col]);
                xb[4 * k] = x.x; xb[4 * k + 1] = x.y; xb[4 * k + 2] = x.z; xb[4 * k + 3] = x.w;
            }
            // player B's epsilon branch read before the chain, not behind the argmax, and the step's
            // serve draw (applied to the arenas whose episode ends) before the tick, not inside its branch
            const int ea = sm.epsa[st & 1][col];
            ServeDraw sd = sm.sdraw[st & 1][col];
            f32x4v16 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 32; ++q) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(hw4[q], xb[q], acc, 0, 0, 0);
            // every operand read issued ahead of the chain (one wait per read, in order)
            __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);  // DS reads
            __builtin_amdgcn_sched_group_barrier(0x008, 32, 0);  // the MFMAs
            // + the other half (both lanes get the same bits)
            float v = xor16_sum(acc[0]), a0 = xor16_sum(acc[1]), a1 = xor16_sum(acc[2]), a2 = xor16_sum(acc[3]);
            v += hf[256];
            a0 += hf[257];
            a1 += hf[258];
            a2 += hf[259];
            const float mean = ((a0 + a1) + a2) / 3.0f;  // A.mean(dim=1)
            const float qv[3] = {v + (a0 - mean), v + (a1 - mean), v + (a2 - mean)};
            int act = argmax3(qv);
            // random.random() < eps ? randint(0, 2) : argmax (train_iterative.py:126-130)
            if (hp) act = ea >= 0 ? ea : act;
            int aA, aB;
            halves_bcast(act, aA, aB);  // rows 0 and 1 (2 and 3) hold the same actions
            ROLL_T(4);  // heads + actions
            float rA, rB;
            const int d = tick(p, a, aA, aB, rA, rB);
            ptA += rA > 0.f ? 1 : 0;
            ptB += rB > 0.f ? 1 : 0;
            if (d) {  // env.reset() with K1's step-keyed production serve
                fin += 1;
                winB += rB > 0.f ? 1 : 0;
                serve_finish(sd);
                serve(a, sd.vx, sd.vy, sd.spin);
            }
            float oA[7], oB[7];
            observe(a, oA, oB);
            if (g < 2)
#pragma unroll
                for (int k = 0; k < 7; ++k) sm.ob[g][col][k] = g ? oB[k] : oA[k];
            ROLL_T(5);  // tick + next observations
        } else if (wv == 1 && st + 1 < steps) {  // the next step's draws
            roll16_serve(p, sm, i, ctr + 1, (st + 1) & 1, seed_env, g);
        } else if (wv == 2 && st + 1 < steps) {
            roll16_eps(sm, i, ctr + 1, (st + 1) & 1, eps, seed_env, g);
        } else if (wv == 7 && st + 1 < steps) {
            heads_to_opw(sm.opw, 1 + ((st + 1) & 1), sm.hfB[(st + 1) & 1]);  // the next step's heads (landed before barrier B)
        }
        __syncthreads();  // (C) the next observations
        ROLL_T(6);
    }
#ifdef PM_DIAG
    if (diag && lane == 0)
#pragma unroll
        for (int k = 0; k < 8; ++k) pm_diag_roll[wv][k] = k < 7 ? dacc[k] : (unsigned long long)steps;
#endif
    if (wv == 0 && g == 0 && valid) {
        store_arena(s, i, a);
        float oA[7], oB[7];
        observe(a, oA, oB);
        store_row7(obsA + (size_t)i * 7, oA);
        store_row7(obsB + (size_t)i * 7, oB);
    }
    if (!stats || wv != 0) return;
    const bool mine = g == 0 && valid;  // one lane per arena
    long long v[4] = {mine ? fin : 0, mine ? winB : 0, mine ? ptA : 0, mine ? ptB : 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    long long mv = v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) mv = lane == k ? v[k] : mv;
    if (lane < 4) atomicAdd(reinterpret_cast<unsigned long long*>(stats + lane), (unsigned long long)mv);
}

__global__ __launch_bounds__(kR16Block) void k_rollout16(const pm_env_params p, const pm_env_state s,
                                                         const float* __restrict__ wA, const float* __restrict__ wB,
                                                         const float* __restrict__ ws, double eps, uint64_t seed_env,
                                                         uint64_t counter0, int steps, float* __restrict__ obsA,
                                                         float* __restrict__ obsB, long long* __restrict__ stats,
                                                         int n) {
    rollout16_body(p, s, wA, wB, ws, eps, seed_env, counter0, steps, obsA, obsB, stats, n);
}

}  // namespace

static int rollout_launch(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                          const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0,
                          int32_t steps, float* heads_ws, float* obsA, float* obsB, const RollPush* rp, void* per_work,
                          int64_t* stats, int32_t n, void* stream, const RollN* rn = nullptr) {
    const char* name = rp ? "pm_rollout_push" : "pm_rollout";
    PM_REQUIRE(n >= 0 && steps >= 0, PM_E_SIZE, "%s: n=%d steps=%d", name, n, steps);
    if (n == 0 || steps == 0) return PM_OK;
    PM_REQUIRE(p && s && s->x && s->y && s->vx && s->vy && s->spin && s->top && s->bot && s->scoreA && s->scoreB &&
                   s->bounces && wA && wB && paramsB && heads_ws && obsA && obsB,
               PM_E_ARG, "%s: null buffer", name);
    PM_REQUIRE((((uintptr_t)wA) | ((uintptr_t)wB) | ((uintptr_t)heads_ws)) % 16 == 0, PM_E_ARG,
               "%s: wA, wB and heads_ws must be 16-byte aligned", name);
    PM_REQUIRE(p->speed_scale_every > 0, PM_E_ARG, "%s: speed_scale_every must be > 0", name);
    hipStream_t st = pm_stream(stream);
    hipLaunchKernelGGL(k_rollout_heads, dim3(steps), dim3(kHeadsBlock), 0, st, paramsB, seed_net, counter0, heads_ws);
    PM_LAUNCHED("k_rollout_heads");
    if (rp) {  // two launches only because k_rollout_push_n takes the window as one argument more
        if (rn)
            pm_launch(PM_TIMER_ROLLOUT, k_rollout_push_n, dim3(pm_blocks(n, 32)), dim3(kRollBlock), st, *p, *s, wA, wB,
                      (const float*)heads_ws, (double)epsilon, seed_env, counter0, (int)steps, obsA, obsB,
                      reinterpret_cast<long long*>(stats), n, *rp, *rn);
        else
            pm_launch(PM_TIMER_ROLLOUT, k_rollout_push, dim3(pm_blocks(n, 32)), dim3(kRollBlock), st, *p, *s, wA, wB,
                      (const float*)heads_ws, (double)epsilon, seed_env, counter0, (int)steps, obsA, obsB,
                      reinterpret_cast<long long*>(stats), n, *rp);
        PM_LAUNCHED(rn ? "k_rollout_push_n" : "k_rollout_push");
        if (per_work) return per_launch_nodes(per_work, rp->cap, st);
        return PM_OK;
    }
    pm_launch(PM_TIMER_ROLLOUT, k_rollout16, dim3(pm_blocks(n, 16)), dim3(kR16Block), st, *p, *s, wA, wB,
              (const float*)heads_ws, (double)epsilon, seed_env, counter0, (int)steps, obsA, obsB,
              reinterpret_cast<long long*>(stats), n);
    PM_LAUNCHED("k_rollout16");
    return PM_OK;
}

#ifdef PM_DIAG
extern "C" int pm_diag_read_roll(uint64_t* out) {  // [2][8]: waves 0 / 1 of block 0, cycles per phase, [7] steps
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_roll), sizeof(pm_diag_roll));
}
#endif

extern "C" int pm_rollout(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                          const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0,
                          int32_t steps, float* heads_ws, float* obsA, float* obsB, int64_t* stats, int32_t n,
                          void* stream) {
    return rollout_launch(p, s, wA, wB, paramsB, epsilon, seed_env, seed_net, counter0, steps, heads_ws, obsA, obsB,
                          nullptr, nullptr, stats, n, stream);
}

// pm_rollout_push (rn null) and pm_rollout_push_n with nstep > 1.
static int rollout_push(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                        const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0,
                        int32_t steps, float* heads_ws, float* obsA, float* obsB, const pm_roll_replay* rp,
                        int64_t* stats, int32_t n, void* stream, const RollN* rn) {
    PM_REQUIRE(rp && rp->trans && rp->prios && rp->ep_reward, PM_E_ARG, "pm_rollout_push: null replay buffer");
    PM_REQUIRE(rp->cap > 0 && rp->pos >= 0 && rp->pos < rp->cap, PM_E_SIZE, "pm_rollout_push: pos=%lld cap=%lld",
               (long long)rp->pos, (long long)rp->cap);
    PM_REQUIRE(n >= 0 && steps >= 0 && (int64_t)steps * n <= rp->cap, PM_E_SIZE,
               "pm_rollout_push: steps * n = %lld exceeds cap %lld (a slot would be written twice in one launch)",
               (long long)steps * n, (long long)rp->cap);
    PM_REQUIRE(((uintptr_t)rp->trans) % 16 == 0 && ((uintptr_t)rp->per_work) % 16 == 0, PM_E_ARG,
               "pm_rollout_push: trans and per_work must be 16-byte aligned");
    const RollPush d{rp->trans, rp->prios, rp->per_work ? per_tree(rp->per_work, rp->cap).leaf : nullptr,
                     rp->ep_reward, rp->pos, rp->cap, rp->prio, rp->alpha};
    return rollout_launch(p, s, wA, wB, paramsB, epsilon, seed_env, seed_net, counter0, steps, heads_ws, obsA, obsB,
                          &d, rp->per_work, stats, n, stream, rn);
}

extern "C" int pm_rollout_push(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                               const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net,
                               uint64_t counter0, int32_t steps, float* heads_ws, float* obsA, float* obsB,
                               const pm_roll_replay* rp, int64_t* stats, int32_t n, void* stream) {
    return rollout_push(p, s, wA, wB, paramsB, epsilon, seed_env, seed_net, counter0, steps, heads_ws, obsA, obsB, rp,
                        stats, n, stream, nullptr);
}

extern "C" int pm_rollout_push_n(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                                 const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net,
                                 uint64_t counter0, int32_t steps, float* heads_ws, float* obsA, float* obsB,
                                 const pm_roll_replay* rp, int64_t* stats, int32_t n, int32_t nstep, double gamma,
                                 void* stream) {
    PM_REQUIRE(nstep >= 1 && nstep <= PM_NSTEP_MAX, PM_E_SIZE, "pm_rollout_push_n: nstep=%d (1..%d)", nstep,
               PM_NSTEP_MAX);
    PM_REQUIRE(std::isfinite(gamma), PM_E_ARG, "pm_rollout_push_n: gamma is not finite");
    const RollN rn{nstep, (float)gamma};
    return rollout_push(p, s, wA, wB, paramsB, epsilon, seed_env, seed_net, counter0, steps, heads_ws, obsA, obsB, rp,
                        stats, n, stream, nstep > 1 ? &rn : nullptr);  // nstep 1: the one-step launch as it is
}
