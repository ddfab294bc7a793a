// What the rollout kernels share, as text: included inside the anonymous namespace of pm_rollout.hip (the solo
// launches) and of pm_rollout_pop.hip (the population's, on one member per block), with pm_host.h, pm_mfma.h
// and pm_per.h included and `using namespace pm` in effect. The heads fold and the collecting launch's body are
// forceinline functions behind thin kernels in both units; `step` / `tile` are the block's step and 32-arena tile
// (blockIdx.x in the solo launches). Shared as text rather than through a header, as pm_dqr_sample_body.inc:
// the functions and the body's LDS block keep internal linkage in each unit, and the solo kernels their device
// text (profiles/rollout_pop_kernel_text.txt).
constexpr int kRollBlock = 256;  // waves 2p + j: player p (0 = A, 1 = B), layer-2 tile j; one tile of 32 arenas
constexpr int kHeadsBlock = 256;
static_assert(PM_ROLL_HEADS == 264, "heads workspace stride: 256 fragment floats + 4 biases + 4 pad");

// k_rollout_heads' body: step `step` of the launch, block-wide (kHeadsBlock threads).
__device__ __forceinline__ void rollout_heads_body(const float* __restrict__ paramsB, uint64_t seed_net,
                                                   uint64_t counter0, float* __restrict__ ws, unsigned step) {
    __shared__ float noise[132];
    __shared__ float heads[260];
    gen_noise(seed_net, TAG_NOISE_ACT, counter0 + step, noise, threadIdx.x, blockDim.x);
    __syncthreads();
    fold_heads_from(paramsB + PM_QNET_HEAD_OFF, nullptr, noise, PM_FOLD_TRAIN_FRESH, heads, nullptr, threadIdx.x,
                    blockDim.x);
    __syncthreads();
    float* hf = ws + (size_t)step * PM_ROLL_HEADS;
    heads_to_frags(heads, hf);
    if (threadIdx.x < 4) hf[260 + threadIdx.x] = 0.f;
}

// Stream step t's heads (PM_ROLL_HEADS floats at ws + t * PM_ROLL_HEADS) into dst: one 16-byte and one
// 4-byte global_load_lds (the latter's tail lanes re-read the biases' pad). Wave-wide; completes at
// the issuing wave's next vmcnt(0).
__device__ __forceinline__ void fetch_heads(const float* __restrict__ ws, int t, float* dst, int lane) {
    const float* src = ws + (size_t)t * PM_ROLL_HEADS;
    __builtin_amdgcn_global_load_lds((const void*)(reinterpret_cast<const float4*>(src) + lane), (lds_void*)dst, 16,
                                     0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(src + 256 + (lane & 7)), (lds_void*)(dst + 256), 4, 0, 0);
}

// fetch_heads for the loop: the same two LDS-DMA loads issued from inline asm. With the builtin the
// compiler cannot tell the DMA's LDS target from the weight image the next ds_reads hit and puts a
// vmcnt(0) right behind the fetch (measured in the ISA: the prefetch then overlapped nothing, and a
// collecting launch's replay stores were waited there too). Issued here, the only wait is the
// explicit vmcnt(0) the fetching wave executes before the step's second barrier.
__device__ __forceinline__ void fetch_heads_async(const float* __restrict__ ws, int t, float* dst, int lane) {
    const float* src = ws + (size_t)t * PM_ROLL_HEADS;
    const uint32_t m0a = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dst);
    const float4* g4 = reinterpret_cast<const float4*>(src) + lane;
    const float* g1 = src + 256 + (lane & 7);
    asm volatile(
        "s_mov_b32 m0, %0\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %3, off" ::"s"(m0a),
        "s"(m0a + 1024u), "v"(g4), "v"(g1)
        : "memory", "m0");
}

// serve_draw (pm_dev.h) after its two Philox blocks, for the kernels that draw both blocks at once in
// two lane groups: the same expressions on the same bits, so the draw is bit-identical.
__device__ __forceinline__ ServeDraw serve_from_blocks(const pm_env_params& p, const U4& r0, const U4& r1) {
    ServeDraw d;
    d.speed = p.speed_lo + (p.speed_hi - p.speed_lo) * u53(r0.x, r0.y);
    const bool first = u53(r0.z, r0.w) < 0.5;
    const double lo = first ? p.ang0_lo : p.ang1_lo, hi = first ? p.ang0_hi : p.ang1_hi;
    const double ang = lo + (hi - lo) * u53(r1.x, r1.y);
    d.rad = ang * (3.141592653589793 / 180.0);
    d.spin = p.spin_lo + (p.spin_hi - p.spin_lo) * u53(r1.z, r1.w);
    double sn, cs;
    sincos_serve(d.rad, sn, cs);
    d.vx = d.speed * cs;
    d.vy = d.speed * sn;
    return d;
}

// ---------------------------------------------------------------------------------------------------
// The collecting launch, on 32-arena tiles. Wave 2 p + j computes layer-2 tile j of player p's forward
// (p = 0: A on modelA's image, p = 1: B on modelB's features + the step's heads; layer 1 in both), so
// a forward is 40 dependent MFMAs on two SIMDs instead of 72 on one. Wave j = 0 runs the head chains
// over its tile's rows and hands the four partial sums per lane to wave j = 1 through LDS (part[]),
// which continues them over its rows: the same fmaf sequence as tile_heads, so every Q value and
// action is bit-identical to pm_qnet_act. Only wave 3 keeps the fp64 arena: it ticks, pushes, and
// publishes both players' next observations in LDS (a third barrier per step), and waves 0-1, idle
// during the tick, draw the next step's serves and player B's epsilon branch into LDS. (Ticking every
// arena in all 8 half-waves and drawing every serve in all four waves, which saves that barrier, left
// the launch bound by the replicated VALU work at 65 536 arenas.) Wave 3 issues the step's three
// stores right after the tick; the vmcnt(0) it already waits on for the next step's heads retires
// them a full step later, so no store latency reaches the step's critical path.

// The replay target (pm_roll_replay, device side).
struct RollPush {
    float* trans;
    float* prios;
    float* leaf;       // nullable: the PER leaves (prio^alpha) of pm_per_work_bytes(cap) work
    float* ep_reward;  // [n], carried
    int64_t pos, cap;  // ring slot of step 0's arena 0; steps * n <= cap, so no slot is written twice
    float prio, alpha;
};

struct RollShared {
    float lw[kLwFloats];   // modelA's fragment image
    float lwB[kLwFloats];  // modelB's feature fragments (its heads come from hf)
    float hf[2][320];      // modelB's heads of the step (fragment order, 256 + biases), double-buffered
    __attribute__((aligned(16))) float part[2][2][64][4];  // [step & 1][player] head chains after c2[0]
    int act[2][2][32];        // [step & 1][player][column]
    float ob[2][32][8];       // [player][column]: the step's observations
    ServeDraw sdraw[2][32];   // [step & 1][column]
    int epsa[2][32];          // [step & 1][column]: -1 = argmax stands, else player B's random action
};

// Step ctr's draws into buffer b. Wave 0 draws the serve's two Philox blocks at once (lanes 0-31 the
// first tag, lanes 32-63 the second, for the same arenas) and hands the second to lanes 0-31 by
// v_permlane32_swap: one block's instruction stream instead of two in a row, the same bits. Wave 1
// draws player B's epsilon branch.
__device__ __forceinline__ void roll_draws(const pm_env_params& p, RollShared& sm, int i, uint64_t ctr, int b,
                                           double eps, uint64_t seed, int wv, int lane) {
    const int col = lane & 31;
    if (wv == 0) {
        const U4 r = philox((uint32_t)i, lane >= 32 ? (TAG_SERVE_STEP | 0x100u) : TAG_SERVE_STEP, (uint32_t)ctr,
                            (uint32_t)(ctr >> 32), seed);
        const auto sx = __builtin_amdgcn_permlane32_swap(r.x, r.x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(r.y, r.y, false, false);
        const auto sz = __builtin_amdgcn_permlane32_swap(r.z, r.z, false, false);
        const auto sw = __builtin_amdgcn_permlane32_swap(r.w, r.w, false, false);
        // [0]: lanes 0-31's block in both halves, [1]: lanes 32-63's
        const ServeDraw d = serve_from_blocks(p, U4{sx[0], sy[0], sz[0], sw[0]}, U4{sx[1], sy[1], sz[1], sw[1]});
        if (lane < 32) sm.sdraw[b][col] = d;
    } else if (wv == 1 && lane < 32) {
        const U4 rr = philox64((uint32_t)i, TAG_ACT, ctr, seed);
        sm.epsa[b][col] = u53(rr.x, rr.y) < eps ? (int)below(rr.z, 3u) : -1;
    }
}

// The n-step window (pm_rollout_push_n): the launch's horizon N = nstep (1..PM_NSTEP_MAX) and g = (float)gamma.
struct RollN {
    int nstep;
    float g;
};

// Wave 3's pending transitions, per arena column: the one opened at step t sits in entry t & 7 until it is
// written (at most N <= 8 are pending, opened at consecutive steps, so no entry is reused while it is live).
// Lanes 0-31 own s | R, the half of the row they store; lanes 32-63 own the action, which goes into theirs.
// A pending transition's age is the step minus its opening step, so neither k nor f = g^age is stored.
struct RollWindow {
    __attribute__((aligned(16))) float sr[PM_NSTEP_MAX][32][8];  // s[7], R
    int act[PM_NSTEP_MAX][32];
};

// One step of the n-step window of arena i, for wave 3's lanes with a valid arena (lanes < 32 and lanes >= 32 hold
// the same arena and make the same decisions). Step st's transition (s = oB, aB) is opened; every pending one,
// age j = st - its opening step, takes the step's reward as R = R + g^j * rB (g^j the float32 product chain
// disc(j), g^0 = 1); then a pending transition is written with its horizon k = j + 1 if the episode ended
// (done = 1, all of them), if it has reached k = N, or at the launch's last step (done = 0). s' is the
// observation after the tick, before the serve. The one opened at step t goes to slot (pos + t * n + i) mod cap.
__device__ __forceinline__ void nstep_push(const RollPush& rp, const RollN& rn, int st, bool last, int n, int i,
                                           int lane, int col, const float (&oB)[7], int aB, float rB, int d,
                                           const Arena& a, int& first, float leafv) {
    __shared__ RollWindow win;
    const bool hi = lane >= 32;
    const int N = rn.nstep;
    if (!hi) {
        float4* e = reinterpret_cast<float4*>(win.sr[st & 7][col]);
        e[0] = make_float4(oB[0], oB[1], oB[2], oB[3]);
        e[1] = make_float4(oB[4], oB[5], oB[6], 0.f);
    } else {
        win.act[st & 7][col] = aB;
    }
    float nA[7], nB[7];
    observe(a, nA, nB);
    float f = 1.0f;
#pragma unroll
    for (int j = 0; j < PM_NSTEP_MAX; ++j) {
        const int t = st - j;
        if (j < N && t >= first) {
            const int w = t & 7;
            const bool write = d || last || j == N - 1;
            float4 lo0 = make_float4(0.f, 0.f, 0.f, 0.f), lo1 = lo0;
            int act = 0;
            if (!hi) {
                const float4* e = reinterpret_cast<const float4*>(win.sr[w][col]);
                lo0 = e[0];
                lo1 = e[1];
                lo1.w = lo1.w + f * rB;
                if (!write) win.sr[w][col][7] = lo1.w;
            } else if (write) {
                act = win.act[w][col];
            }
            if (write) {
                int64_t slot = rp.pos + (int64_t)t * n + i;
                if (slot >= rp.cap) slot -= rp.cap;
                float4* row = reinterpret_cast<float4*>(rp.trans + slot * PM_TRANS_F) + (lane >> 5) * 2;
                st_f4<false>(row, hi ? make_float4(nB[0], nB[1], nB[2], nB[3]) : lo0);
                st_f4<false>(row + 1, hi ? make_float4(nB[4], nB[5], nB[6], __int_as_float(act | (d << 8) | (j << 16)))
                                         : lo1);
                if (!hi) rp.prios[slot] = rp.prio;
                else if (rp.leaf) rp.leaf[slot] = leafv;
            }
        }
        f = f * rn.g;
    }
    if (d || last) first = st + 1;
    else if (st - first + 1 == N) first += 1;
}

// The bodies of both rollout kernels stay forceinline functions behind thin kernels: written straight
// into the kernel (parameters by value, not by reference) the same source compiles to different code.
// kN: the n-step variant (rn is read only there). The <false> instantiation is the one-step launch as it was.
template <bool kN>
__device__ __forceinline__ void rollout_push_body(const pm_env_params& p, const pm_env_state& s,
                                                  const float* __restrict__ wA, const float* __restrict__ wB,
                                                  const float* __restrict__ ws, double eps, uint64_t seed_env,
                                                  uint64_t counter0, int steps, float* __restrict__ obsA,
                                                  float* __restrict__ obsB, long long* __restrict__ stats, int n,
                                                  const RollPush& rp, const RollN& rn, int tile) {
    __shared__ __attribute__((aligned(16))) RollShared sm;
    const int lane = threadIdx.x & 63, col = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: SGPRs, not VGPRs
    const int player = wv >> 1, half = wv & 1;
    const int i = tile * 32 + col;
    const bool valid = i < n;
    stage_frags_lds(wA, sm.lw, tile);  // block-wide: chunks spread over the waves
    stage_frags_lds(wB, sm.lwB, tile + kLwChunks / 2);
    if (wv == 3) fetch_heads(ws, 0, sm.hf[0], lane);
    Arena a{};
    int fin = 0, winB = 0, ptA = 0, ptB = 0, winE = 0, rsum = 0;  // per arena: |count| <= steps < 2^31
    float er = 0.f, leafv = 0.f;
    [[maybe_unused]] int first = 0;  // kN: the opening step of the arena's oldest pending transition
    if (wv == 3) {
        a = load_arena(s, valid ? i : n - 1);
        float oA[7], oB[7];
        observe(a, oA, oB);
        if (lane < 32)
#pragma unroll
            for (int k = 0; k < 7; ++k) { sm.ob[0][col][k] = oA[k]; sm.ob[1][col][k] = oB[k]; }
        er = rp.ep_reward[valid ? i : n - 1];
        // memory.push's priority as a PER leaf (wave-uniform: kept in an SGPR)
        leafv = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(prio_pow(rp.prio, rp.alpha))));
    }
    roll_draws(p, sm, i, counter0, 0, eps, seed_env, wv, lane);
    const float* lw = player ? sm.lwB : sm.lw;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // both images, step 0's heads, observations and draws in LDS
    for (int st = 0; st < steps; ++st) {
        const uint64_t ctr = counter0 + (uint64_t)st;
        if (wv == 3 && st + 1 < steps) fetch_heads_async(ws, st + 1, sm.hf[(st + 1) & 1], lane);  // lands during the MFMAs
        float xs[4];
        tile_inputs(sm.ob[player][col], lane >> 5, xs);
        f32x16 c2;
        hidden_half(lw, xs, lane, half, c2);
        const float* hf = player ? sm.hf[st & 1] : sm.lw + F_H;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (half == 0) {
            heads_half(hf, c2, lane, 0, acc);
            *reinterpret_cast<float4*>(&sm.part[st & 1][player][lane][0]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        __syncthreads();  // the chains over layer-2 tile 0
        if (half == 1) {
            const float4 pa = *reinterpret_cast<const float4*>(&sm.part[st & 1][player][lane][0]);
            acc[0] = pa.x; acc[1] = pa.y; acc[2] = pa.z; acc[3] = pa.w;
            heads_half(hf, c2, lane, 1, acc);
            float q[3];
            heads_finish(acc, hf, q);
            int act = argmax3(q);
            if (player) {  // random.random() < eps ? randint(0, 2) : argmax (train_iterative.py:126-130)
                const int ea = sm.epsa[st & 1][col];
                if (ea >= 0) act = ea;
            }
            if (lane < 32) sm.act[st & 1][player][col] = act;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // wave 3: the next step's heads (and its stores)
        __syncthreads();  // both players' actions
        if (wv == 3) {
            const int aA = sm.act[st & 1][0][col], aB = sm.act[st & 1][1][col];
            float oB[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) oB[k] = sm.ob[1][col][k];  // the step's observation of B (push's s)
            float rA, rB;
            const int d = tick(p, a, aA, aB, rA, rB);
            ptA += rA > 0.f ? 1 : 0;
            ptB += rB > 0.f ? 1 : 0;
            er += rB;  // ep_reward += rB (:245)
            if (d) {
                winE += er > 0.f ? 1 : 0;
                rsum += (int)er;
            }
            if constexpr (kN) {
                if (valid) nstep_push(rp, rn, st, st + 1 == steps, n, i, lane, col, oB, aB, rB, d, a, first, leafv);
            } else if (valid) {  // memory.push((oB, aB, rB, nB, done)): lanes < 32 s, lanes >= 32 s'
                float nA[7], nB[7];
                observe(a, nA, nB);  // the terminal observation, before the serve
                int64_t slot = rp.pos + (int64_t)st * n + i;
                if (slot >= rp.cap) slot -= rp.cap;
                float4* row = reinterpret_cast<float4*>(rp.trans + slot * PM_TRANS_F) + (lane >> 5) * 2;
                const bool hi = lane >= 32;
                st_f4<false>(row, hi ? make_float4(nB[0], nB[1], nB[2], nB[3]) : make_float4(oB[0], oB[1], oB[2], oB[3]));
                st_f4<false>(row + 1, hi ? make_float4(nB[4], nB[5], nB[6], __int_as_float(aB | (d << 8)))
                                         : make_float4(oB[4], oB[5], oB[6], rB));
                if (!hi) rp.prios[slot] = rp.prio;
                else if (rp.leaf) rp.leaf[slot] = leafv;
            }
            if (d) er = 0.f;
            if (d) {  // env.reset() with K1's step-keyed production serve
                fin += 1;
                winB += rB > 0.f ? 1 : 0;
                ServeDraw sd = sm.sdraw[st & 1][col];
                serve_finish(sd);  // the rare |angle| >= 135 degree redo
                serve(a, sd.vx, sd.vy, sd.spin);
            }
            float oA[7], nB2[7];
            observe(a, oA, nB2);
            if (lane < 32)
#pragma unroll
                for (int k = 0; k < 7; ++k) { sm.ob[0][col][k] = oA[k]; sm.ob[1][col][k] = nB2[k]; }
        } else if (st + 1 < steps) {
            roll_draws(p, sm, i, ctr + 1, (st + 1) & 1, eps, seed_env, wv, lane);  // the next step's draws
        }
        __syncthreads();  // (C) the next observations
    }
    if (wv == 3 && lane < 32 && valid) {  // wave 3 writes the arenas and their observations
        store_arena(s, i, a);
        float oA[7], oB[7];
        observe(a, oA, oB);
        store_row7(obsA + (size_t)i * 7, oA);
        store_row7(obsB + (size_t)i * 7, oB);
        rp.ep_reward[i] = er;
    }
    if (!stats) return;  // block-uniform
    const bool mine = wv == 3 && lane < 32 && valid;  // one lane per arena
    long long v[6] = {mine ? fin : 0, mine ? winB : 0, mine ? ptA : 0, mine ? ptB : 0, mine ? winE : 0,
                      mine ? rsum : 0};
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
    long long mv = v[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) mv = lane == k ? v[k] : mv;
    if (wv == 3 && lane < 6) atomicAdd(reinterpret_cast<unsigned long long*>(stats + lane), (unsigned long long)mv);
}
