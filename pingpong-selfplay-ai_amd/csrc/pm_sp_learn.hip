// The self-play learner's learner unit: the kernels that train on the sampled batch and keep the
// replay's sum tree, optimizer state and derived weights, and the entry points that launch only them.
//
//   k_learn (1024 threads)   block 0: Q_B(s), Q_B(s'), Q_T(s') on the matrix cores, double-DQN targets,
//                            IS-weighted MSE, priority scatter, head grads [+ Adam / target sync /
//                            epsilon decay / counters / next weights when unsharded]; block 1: the
//                            push rows' forward and the sum-tree refresh; further blocks (launches
//                            with the next step's act): side-A act blocks and modelB's feature blocks
//   k_adam                   the sharded step's apply, after the all-reduce of sp.grad
//   k_prepare, k_tree_repaired   derived weights / the status bit of a full sum-tree rebuild
//   k_learn_multi            updates 1..U-1 of a vector step in one single-workgroup launch
//   k_prio_max + k_commit    the end of a step of U > 1 updates
//
// k_adam and multi_update share the apply section's helpers with k_learn: their code changes when
// they are compiled without it (DESIGN.md "The self-play learner's units").
#include "pm_sp.h"

#ifdef PM_DIAG
// k_learn's side blocks: [0] begin, [1] after the act blocks' sleep, [2] end, [3] role | rows << 16
static __device__ unsigned long long pm_diag_side[4][1024];
#define PM_SIDE(k, sb, v)                                                        \
    do {                                                                         \
        if (threadIdx.x == 0 && (sb) < 1024) pm_diag_side[(k)][(sb)] = (v);      \
    } while (0)
// latest time over the blocks of one role reaching a point (thread 0's atomic max, no barrier)
#define PM_STAMP_MAX_NB(slot)                                                                              \
    do {                                                                                                   \
        if (threadIdx.x == 0) atomicMax(&pm_diag_buf[(slot)], (unsigned long long)__builtin_amdgcn_s_memrealtime()); \
    } while (0)
#else
#define PM_SIDE(k, sb, v) \
    do {                  \
    } while (0)
#define PM_STAMP_MAX_NB(slot) \
    do {                      \
    } while (0)
#endif

// Actions ahead (ABI 26): the fused U = 1 learner launch hands k_actenv modelB's greedy ACTIONS for the
// next step (sp.gB, one byte per arena) instead of its 64 features (sp.featB, 256 B). The features
// crossed the launch boundary only because the acting heads were not final when the feature blocks
// computed them; they are final inside the same launch, right after the learner's Adam. So the learner
// publishes the 260 folded acting head values as tagged 8-byte granules (sp.gheads; push_publish's
// idiom: value and epoch tag in one agent-scope store, the data is the flag), the feature blocks keep
// their tiles' layer-2 accumulators in registers (at most two tiles per wave), poll for the granules
// after their last tile, and run the same tile_heads + argmax3 on the same accumulators with the same
// head values k_actenv's env blocks would: the same bits. A poll that expires (bounded) stores the
// block's tiles to featB as before and PM_GB_NONE to their gB; an env block's wave that finds the
// sentinel in a tile takes that tile from featB. The epoch (gheads word PM_GHEADS_EPOCH) is read by
// every block at its start and bumped by the learner at its very end, so a tag is never reused by a
// later launch (checkpoint restores included); a feature block dispatched after the learner ended
// (never when the grid fits the device: launch_learn checks) would wait for a tag nobody publishes
// and fall back.
__device__ __forceinline__ uint32_t* gh_epoch(const pm_selfplay& sp) {
    return reinterpret_cast<uint32_t*>(sp.gheads + PM_GHEADS_EPOCH);
}
constexpr int kAheadPollMax = 20000;  // as kPushPollMax (~20 ms)
__device__ __forceinline__ void gh_publish(const pm_selfplay& sp, int k, uint32_t tag, float v) {
    __hip_atomic_store(sp.gheads + k, ((uint64_t)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_learn's feature block in a launch with actions ahead: tiles [t0, t1) of 32 arenas, at most two per
// wave (t1 - t0 <= 2 waves: launch_learn checks). feat_tiles' tile code (the same accumulators), then
// the hand-off described above. Block-wide, every barrier block-uniform.
struct FeatAheadSmem {
    float lw[kLwFloats];  // modelB's acting fragment image (the feature layers)
    // the next step's acting heads from the granules: by output (pm_mfma.h opw_slot: tile_heads_mfma's A
    // operands), then the four biases
    __attribute__((aligned(16))) float hf[kOpwFloats + 8];
    int ok;               // every granule arrived
};
__device__ __forceinline__ void feat_tiles_ahead(const pm_selfplay& sp, FeatAheadSmem& sm, int t0, int t1, bool force_timeout) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, nw = blockDim.x >> 6;
    stage_frags_lds(sp.w_B, sm.lw, t0);
    const uint32_t tag = __hip_atomic_load(gh_epoch(sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    const int tl[2] = {t0 + wave, t0 + wave + nw};
    const bool has[2] = {tl[0] < t1, tl[1] < t1};  // wave-uniform; t1 - t0 <= 2 nw
    float xs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (has[k]) tile_inputs(sp.obsB + (size_t)min(tl[k] * 32 + (lane & 31), sp.n - 1) * 7, lane >> 5, xs[k]);
    if (t == 0) sm.ok = 1;
    __syncthreads();
    f32x16 c2[2][2] = {};
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (has[k]) tile_hidden(sm.lw, xs[k], lane, c2[k]);
    PM_STAMP_MAX_NB(68);
    // the learner's granules: thread k < 256 takes the head value of fragment slot k (heads_to_frags'
    // map), threads 256..259 the biases
    if (t < 260) {
        const int c = t & 3, r = (t >> 2) & 15, tt = (t >> 6) & 1, h = t >> 7;
        const int src = t < 256 ? c * 64 + 32 * tt + rho(r) + 4 * h : t;
        uint64_t g = 0;
        bool got = false;
        for (int it = 0; !force_timeout && it < kAheadPollMax; ++it) {
            g = __hip_atomic_load(sp.gheads + src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)(g >> 32) == tag) { got = true; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (got) sm.hf[t < 256 ? opw_slot(t) : kOpwFloats + t - 256] = __uint_as_float((uint32_t)g);
        else sm.ok = 0;
    }
    __syncthreads();
    PM_STAMP_MAX_NB(69);
    const bool ok = sm.ok != 0;  // block-uniform
    // the heads on the matrix cores (tile_heads_mfma: the VALU sweeps' LDS reads, 1 KB per wave and step
    // over ~18 tiles x 32 steps per CU, bound this tail, which ends the launch); a wave with two tiles
    // runs both chains in one sweep of the operands
    int a[2] = {PM_GB_NONE, PM_GB_NONE};
    if (ok) {
        float q0[3], q1[3];
        if (has[1]) {  // wave-uniform; has[1] implies has[0]
            tile_heads_mfma2(sm.hf, sm.hf + kOpwFloats, c2[0], c2[1], lane, q0, q1);
            a[0] = argmax3(q0);
            a[1] = argmax3(q1);
        } else if (has[0]) {
            tile_heads_mfma(sm.hf, sm.hf + kOpwFloats, c2[0], lane, q0);
            a[0] = argmax3(q0);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!has[k]) continue;  // wave-uniform
        const int arena = tl[k] * 32 + (lane & 31);
        if (!ok) feat_store(sp.featB, tl[k], lane, c2[k]);
        if (lane < 32 && arena < sp.n) sp.gB[arena] = (int8_t)a[k];
    }
}

// ------------------------------------------------------------------------------------ apply
struct __attribute__((aligned(16))) ApplySmem {  // 520-float arrays padded to whole 1 KB (16-B lane) global_load_lds chunks
    float hp[pad256(PM_QNET_NHEAD)];   // modelB head parameters (after the optimizer step)
    float tmu[pad256(PM_QNET_NHEAD)];  // targetB head parameters (mu used)
    float m[pad256(PM_QNET_NHEAD)], v[pad256(PM_QNET_NHEAD)];  // Adam moments
    float g[PM_QNET_NHEAD + 2];                // shard-summed grads | finished episodes | updated flag
    float ak[2];                               // Adam step size lr / (1 - b1^t), sqrt(1 - b2^t)
    float nact[132], ntrain[132];
    float heads[3][260];                       // folded acting / next-update / target heads
    double eps_next;                           // fused learner: eps * decay^D, computed early
};

// torch.optim.Adam's bias corrections for update number ts, computed in fp64 as torch does (Python
// floats), once per block (two fp64 pow per thread cost ~3 us of VALU in a 1024-thread block).
__device__ __forceinline__ void adam_consts(const pm_selfplay& sp, int64_t ts, ApplySmem& sm) {
    const double bc1 = 1.0 - pow(sp.beta1, (double)ts);
    const double bc2 = 1.0 - pow(sp.beta2, (double)ts);
    sm.ak[0] = (float)(sp.lr / bc1);
    sm.ak[1] = (float)sqrt(bc2);
}
// The same two constants from two lanes of one wave (lane `which` = 0: step size, 1: sqrt(bc2)), so
// the two fp64 pow run side by side instead of back to back.
__device__ __forceinline__ void adam_const_lane(const pm_selfplay& sp, int64_t ts, ApplySmem& sm, int which) {
    const double bc = 1.0 - pow(which ? sp.beta2 : sp.beta1, (double)ts);
    sm.ak[which] = which ? (float)sqrt(bc) : (float)(sp.lr / bc);
}

// Block-wide: the optimizer's inputs global -> LDS directly (global_load_lds, no wait until the
// caller's barrier). g: from LDS already when fused.
__device__ __forceinline__ void load_apply_inputs(const pm_selfplay& sp, ApplySmem& sm, bool with_grad) {
    copy_lds_f32x4<PM_QNET_NHEAD>(sp.paramsB + PM_QNET_HEAD_OFF, sm.hp);
    copy_lds_f32x4<PM_QNET_NHEAD>(sp.paramsT + PM_QNET_HEAD_OFF, sm.tmu);
    copy_lds_f32x4<PM_QNET_NHEAD>(sp.adam_m, sm.m);
    copy_lds_f32x4<PM_QNET_NHEAD>(sp.adam_v, sm.v);
    if (with_grad)
        for (int k = threadIdx.x; k < PM_QNET_NHEAD + 2; k += blockDim.x) sm.g[k] = sp.grad[k];
}

// Everything that follows from the head parameters once they are final for this step, from LDS:
// acting weights for the next vector step (select_action_B -> reset_noise, :125; the noise lands
// in modelB's epsilon buffers), the next update's modelB heads with fresh noise (reset_noise, :142)
// and targetB heads (eval mode: mu, :100), both in MFMA fragment order in learn_heads, plus that
// update's noise. Block-wide; noise already in sm.nact / sm.ntrain.
// gh_on (actions ahead): the folded acting heads also go out as granules of tag gh_tag for this launch's
// feature blocks, each from the thread that folded it (no barrier in front of the hand-off), before any
// fragment write.
__device__ __forceinline__ void derive_weights(const pm_selfplay& sp, ApplySmem& sm, bool gh_on = false, uint32_t gh_tag = 0) {
    const int t = threadIdx.x;
    float* lh = sp.learn_heads;
    // the three folds are independent: one pass on three 260-thread groups, one barrier, then the
    // three fragment writes
    // (threads 256..1023: in the fused learner threads < 256 are still refreshing level-2 tree nodes)
    const int g = (t - 256) >> 8, u = (t - 256) & 255;
    if (t >= 256 && g == 0) {
        fold_heads_from(sm.hp, nullptr, sm.nact, PM_FOLD_TRAIN_FRESH, sm.heads[0], sp.paramsB + PM_QNET_EPS_OFF, u, 256);
        if (gh_on) {  // fold_heads_from(tid u, 256 threads) wrote heads[0][u], and heads[0][256 + u] for u < 4
            gh_publish(sp, u, gh_tag, sm.heads[0][u]);
            if (u < 4) gh_publish(sp, 256 + u, gh_tag, sm.heads[0][256 + u]);
            PM_STAMP_T(22, 256);
        }
    } else if (t >= 256 && g == 1) {
        fold_heads_from(sm.hp, nullptr, sm.ntrain, PM_FOLD_TRAIN_FRESH, sm.heads[1], lh + 528, u, 256);
    } else if (t >= 256 && g == 2) {
        fold_heads_from(sm.tmu, nullptr, nullptr, PM_FOLD_EVAL, sm.heads[2], nullptr, u, 256);
    }
    __syncthreads();
    write_head_frags(sm.heads[0], sp.w_B);
    heads_to_frags(sm.heads[1], lh);
    heads_to_frags(sm.heads[2], lh + 264);
}

// derive_weights for an update of k_learn_multi that is not the launch's last: only what the next
// update reads, from LDS to LDS — the next update's modelB heads (fresh noise) and targetB heads.
// The acting weights and every global copy follow from the last update alone.
__device__ __forceinline__ void derive_weights_lds(ApplySmem& sm) {
    const int t = threadIdx.x;
    const int g = (t - 256) >> 8, u = (t - 256) & 255;
    if (t >= 256 && g == 1) {
        fold_heads_from(sm.hp, nullptr, sm.ntrain, PM_FOLD_TRAIN_FRESH, sm.heads[1], nullptr, u, 256);
    } else if (t >= 256 && g == 2) {
        fold_heads_from(sm.tmu, nullptr, nullptr, PM_FOLD_EVAL, sm.heads[2], nullptr, u, 256);
    }
    __syncthreads();
}

// Both noise draws at once, half of the block each.
__device__ __forceinline__ void gen_both_noises(const pm_selfplay& sp, ApplySmem& sm, uint64_t act_ctr,
                                                uint64_t train_ctr) {
    const int t = threadIdx.x, half = blockDim.x / 2;
    if (t < half) gen_noise(sp.seed_net, TAG_NOISE_ACT, act_ctr, sm.nact, t, half);
    else gen_noise(sp.seed_net, TAG_NOISE_TRAIN, train_ctr, sm.ntrain, t - half, half);
}
// The same draws on threads [t0, t0 + 512) only (the fused learner's waves with slack in its load
// phase). Same values: every noise element depends only on (seed, tag, counter, index).
__device__ __forceinline__ void gen_both_noises_on(const pm_selfplay& sp, ApplySmem& sm, uint64_t act_ctr,
                                                   uint64_t train_ctr, int t0) {
    const int u = (int)threadIdx.x - t0;
    if (u < 0 || u >= 512) return;
    if (u < 256) gen_noise(sp.seed_net, TAG_NOISE_ACT, act_ctr, sm.nact, u, 256);
    else gen_noise(sp.seed_net, TAG_NOISE_TRAIN, train_ctr, sm.ntrain, u - 256, 256);
}

// optimizer.step() (:161) on the shard-summed grads, target sync (:166-168), epsilon decay (:261),
// replay / step counters, then derive_weights for the next step. All inputs in LDS (sm) and `cs`
// (the control block as the kernel found it); only stores go to global memory. Both noises are in
// sm.nact / sm.ntrain and sm.eps_next holds eps * decay^D already (drawn / computed by idle waves
// while the callers' loads were in flight). Two parts: apply_adam (per-thread, no barrier: the fused
// learner runs it beside the sum-tree's level-2 refresh) and apply_finish (behind a barrier).
// torch.optim.Adam (single-tensor path) on head parameter k with gradient g (summed over shards).
__device__ __forceinline__ void adam_one(const pm_selfplay& sp, ApplySmem& sm, int k, float gsum, bool store = true) {
    const float step_size = sm.ak[0], bc2s = sm.ak[1];  // adam_consts, published before a barrier
    const float g = gsum / (float)sp.world;
    float m = sm.m[k], v = sm.v[k], p = sm.hp[k];
    m = m + (float)(1.0 - sp.beta1) * (g - m);                  // exp_avg.lerp_(grad, 1-beta1)
    v = v * (float)sp.beta2 + (float)(1.0 - sp.beta2) * g * g;  // mul_(beta2).addcmul_(g, g, 1-beta2)
    const float denom = sqrtf(v) / bc2s + (float)sp.adam_eps;
    p = p - step_size * (m / denom);
    if (store) {  // k_learn_multi keeps all but its last update's state in LDS only
        sp.paramsB[PM_QNET_HEAD_OFF + k] = p;
        sp.adam_m[k] = m;
        sp.adam_v[k] = v;
    }
    sm.hp[k] = p;
    sm.m[k] = m;  // k_learn_multi runs the next update from LDS
    sm.v[k] = v;
}
// adam_one on two parameters, every load first: the two chains (a square root and two divisions each) run
// side by side instead of the second's loads waiting behind the first's LDS stores
__device__ __forceinline__ void adam_two(const pm_selfplay& sp, ApplySmem& sm, int k0, float g0s, int k1, float g1s) {
    const float step_size = sm.ak[0], bc2s = sm.ak[1];
    const float g0 = g0s / (float)sp.world, g1 = g1s / (float)sp.world;
    float m0 = sm.m[k0], v0 = sm.v[k0], p0 = sm.hp[k0];
    float m1 = sm.m[k1], v1 = sm.v[k1], p1 = sm.hp[k1];
    m0 = m0 + (float)(1.0 - sp.beta1) * (g0 - m0);
    m1 = m1 + (float)(1.0 - sp.beta1) * (g1 - m1);
    v0 = v0 * (float)sp.beta2 + (float)(1.0 - sp.beta2) * g0 * g0;
    v1 = v1 * (float)sp.beta2 + (float)(1.0 - sp.beta2) * g1 * g1;
    const float d0 = sqrtf(v0) / bc2s + (float)sp.adam_eps;
    const float d1 = sqrtf(v1) / bc2s + (float)sp.adam_eps;
    p0 = p0 - step_size * (m0 / d0);
    p1 = p1 - step_size * (m1 / d1);
    sm.hp[k0] = p0;
    sm.hp[k1] = p1;
    sp.paramsB[PM_QNET_HEAD_OFF + k0] = p0;
    sp.adam_m[k0] = m0;
    sp.adam_v[k0] = v0;
    sp.paramsB[PM_QNET_HEAD_OFF + k1] = p1;
    sp.adam_m[k1] = m1;
    sp.adam_v[k1] = v1;
    sm.m[k0] = m0;
    sm.v[k0] = v0;
    sm.m[k1] = m1;
    sm.v[k1] = v1;
}
__device__ __forceinline__ void apply_adam(const pm_selfplay& sp, ApplySmem& sm) {
    const int t = threadIdx.x, nt = blockDim.x;
    if (sm.g[kGradN + 1] > 0.5f)
        for (int k = t; k < PM_QNET_NHEAD; k += nt) adam_one(sp, sm, k, sm.g[k]);
}
// mode (PM_UPD_*): FIRST commits the epsilon decay of the step's finished episodes, LAST the replay
// and step counters (with U > 1 updates per step pm_selfplay_commit does that after the last one).
__device__ __forceinline__ void apply_finish(const pm_selfplay& sp, ApplySmem& sm, const pm_ctrl& cs, int mode,
                                             bool gh_on = false, uint32_t gh_tag = 0) {
    const int t = threadIdx.x, nt = blockDim.x;
    const bool train = sm.g[kGradN + 1] > 0.5f;
    const int64_t ts = cs.train_steps + (train ? 1 : 0);
    const uint64_t step = cs.step;
    PM_STAMP(20);
    if (train && ts % sp.target_update_interval == 0) {  // targetB.load_state_dict(modelB) (:166-168)
        for (int k = t; k < PM_QNET_NHEAD; k += nt) sm.tmu[k] = sm.hp[k];
        for (int k = t; k < PM_QNET_NP; k += nt) {
            const int h = k - PM_QNET_HEAD_OFF;
            sp.paramsT[k] = (h >= 0 && h < PM_QNET_NHEAD) ? sm.hp[h] : sp.paramsB[k];
        }
        __syncthreads();
    }
    derive_weights(sp, sm, gh_on, gh_tag);
    PM_STAMP(21);
    if (t == 0) {
        pm_ctrl* c = sp.ctrl;
        if (mode & PM_UPD_FIRST) {
            const double e = sm.eps_next;  // eps * decay^D, D = finished episodes (all shards) (:261)
            c->epsilon = e > sp.min_epsilon ? e : sp.min_epsilon;
        }
        if (train) { c->train_steps = ts; c->frame_idx = cs.frame_idx + 1; }
        if (mode & PM_UPD_LAST) {
            c->pos = (cs.pos + sp.n) % sp.cap;
            const int64_t s = cs.size + sp.n;
            c->size = s < sp.cap ? s : sp.cap;
            c->step = step + 1;
        }
    }
}

// ------------------------------------------------------------------------------------ learner
// ---- the push-range rows of an update's batch: the samples whose replay row this step's k_actenv
// wrote (its sampler blocks cannot read them), s rows then s' rows, one 32-row tile per wave, in
// plist order (pcnt: per-wave counts of the ballot that built plist; B <= 256: waves 0..3).
// emit(j, nxt, lane, c2, qb, qt, rb) runs for the lanes that hold a row.
template <typename Emit>
__device__ __forceinline__ void push_rows_fwd(const pm_selfplay& sp, const float* lw, const float* hf,
                                              const int64_t* sidx, const int* plist, const int* pcnt, int wv, int lane,
                                              Emit emit) {
    int pre[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w) pre[w + 1] = pre[w] + pcnt[w];
    const int np = pre[4];
    if (wv * 32 >= 2 * np) return;  // wave-uniform
    const int rr = min(wv * 32 + (lane & 31), 2 * np - 1);
    const bool nxt = rr >= np;
    const int k = nxt ? rr - np : rr;
    // selects, not pre[w]: a dynamically indexed array is a scratch store + load round trip
    const int w = k >= pre[3] ? 3 : k >= pre[2] ? 2 : k >= pre[1] ? 1 : 0;
    const int pw = k >= pre[3] ? pre[3] : k >= pre[2] ? pre[2] : k >= pre[1] ? pre[1] : 0;
    const int j = plist[w * 64 + k - pw];
    f32x16 c2[2];
    float qb[3], qt[3], rb[2];
    batch_row_fwd(sp, lw, hf, hf + 264, sidx[j], nxt, lane, c2, qb, qt, rb);
    if (wv * 32 + (lane & 31) < 2 * np) emit(j, nxt, lane, c2, qb, qt, rb);
}

// The push-row hand-off inside k_learn: block 1 computes the push rows beside the learner's load
// phase and publishes them in hfeat rows [B, 2B) (hfeat row layout), then the flag word at hfeat row
// 2B = ctrl.step + 1. Publication follows the cross-CU rules for write-through hand-offs: every
// payload store and the flag store sc1, every storing wave waits vmcnt(0), a workgroup barrier,
// then one lane stores the flag; the learner polls the flag with sc1 loads from one lane, joins a
// barrier, and reads the payload with sc1 loads only. Block 1 reads the control block unsynchronised,
// so in a FIRST update it ALWAYS publishes its token (at once, with no rows, when the update does not
// train) and a learner that commits the control block in this launch (fused apply) waits for that
// token before the commit even when it needed no rows: block 1 can then never see the next step's
// control block and publish the token the NEXT launch's learner polls for with rows built from this
// step's push range. Block 1 waits for nothing, so it always completes; the poll is
// bounded anyway (kPushPollMax, ~20 ms): a flag that never came sets ctrl.status bit 0, which the
// host reports as an error (pongmi.selfplay.SelfPlayLearner.check_status), and an update whose push
// rows never came is void: it trains nothing (no scatter, gradients, Adam or train-step count), as
// an update before the replay holds a batch.
constexpr int kPushPollMax = 20000;
__device__ __forceinline__ bool push_handoff(int mode, bool train) { return (mode & PM_UPD_FIRST) && train; }
__device__ __forceinline__ int* push_flag(const pm_selfplay& sp) {
    return reinterpret_cast<int*>(sp.hfeat + (size_t)2 * sp.batch * 80);
}
__device__ __forceinline__ int push_token(const pm_ctrl& cs) { return (int)((uint32_t)cs.step + 1u); }
// the tree-refresh epoch (tree_block): word 1 of the flag row
__device__ __forceinline__ uint32_t* tr_epoch(const pm_selfplay& sp) {
    return reinterpret_cast<uint32_t*>(sp.hfeat + (size_t)2 * sp.batch * 80) + 1;
}
// The push rows as tagged 8-byte granules {tag, float bits} (round 5; tr bit 3, PONGMI_PUSHG): sample
// j's hfeat floats 0..74 at granule j * 76 + f of hfeat rows [2B + 8, 4B + 8) (ABI 22). The data is
// the flag: block 1 stores each granule once (sc1), with no drain, and the learner's loads of them are
// the poll, which saves the payload drain, the flag store's trip and the flag poll's (~2 us; MI355X
// guide: handoff-1to1 vs handoff-flag). The tag is this launch's tree-refresh epoch + 1 (tr_epoch:
// bumped by block 1 at the end of every launch with the tree block, so never reused by a later
// launch, checkpoint restores included). The flag word is still stored, right after block 1 read the
// control block: a learner that needed no rows waits for it before its commit; one that
// saw a granule of this launch's tag knows block 1 read this step's control block.
constexpr int kPushGF = 76;  // granule stride per sample (floats 0..74 used)
constexpr int kPushGN = 75;
__device__ __forceinline__ uint64_t* push_granules(const pm_selfplay& sp) {
    return reinterpret_cast<uint64_t*>(sp.hfeat + (size_t)(2 * sp.batch + 8) * 80);
}
__device__ __forceinline__ void push_publish(uint64_t* g, uint32_t tag, float v) {
    __hip_atomic_store(g, ((uint64_t)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane polls for block 1's token of this update (bounded). false: it never came (status bit 0 set).
__device__ __forceinline__ bool push_wait(const pm_selfplay& sp, const pm_ctrl& cs) {
    const int* flag = push_flag(sp);
    const int tok = push_token(cs);
    for (int it = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != tok; ++it) {
        if (it == kPushPollMax) {
            sp.ctrl->status = cs.status | PM_CTRL_PUSH_TIMEOUT;
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return true;
}

struct PushFwdSmem {
    float lw[kLwFloats];
    float hf[pad256(2 * 264)];
    int64_t sidx[PM_MAX_BATCH];
    int plist[PM_MAX_BATCH];
    int pcnt[16];
    float part[8][64][8];  // push_rows_fwd2: the head chains after layer-2 tile 0, per tile pair of waves
};

// push_rows_fwd on block 1's 16 waves, two per 32-row tile (hidden_half / heads_half, as
// k_rollout_push): wave 2k + jt computes layer-2 tile jt of tile 8 it + k (24 MFMAs deep instead
// of 40); wave jt = 0 runs the head chains over its 32 units and hands them to wave jt = 1 through
// LDS, which continues them in tile_heads' order. Bit-identical rows to push_rows_fwd.
__device__ __forceinline__ void push_rows_fwd2(const pm_selfplay& sp, PushFwdSmem& sm, int wv, int lane, float* pay,
                                               uint32_t gtag) {
    uint64_t* pg = push_granules(sp);
    // hfeat float f of sample j: a payload-row word (drained + flag) or a tagged granule
    auto put = [&](int j, int f, float v) {
        if (gtag) push_publish(pg + (size_t)j * kPushGF + f, gtag, v);
        else st_out<true>(pay + (size_t)j * 80 + f, v);
    };
    int pre[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w) pre[w + 1] = pre[w] + sm.pcnt[w];
    const int np = pre[4];
    const int ntile = (2 * np + 31) >> 5;
    const int jt = wv & 1, h = lane >> 5;
    const float* hf0 = sm.hf;
    const float* hf1 = sm.hf + 264;
    for (int it = 0; it * 8 < ntile; ++it) {  // block-uniform
        const int tile = it * 8 + (wv >> 1);
        const bool act = tile < ntile;  // wave-uniform
        f32x16 c2 = {};
        float ab[4] = {0.f, 0.f, 0.f, 0.f}, at[4] = {0.f, 0.f, 0.f, 0.f};
        float rb0 = 0.f, rb1 = 0.f;
        bool nxt = false, mine = false;
        int j = 0;
        if (act) {
            const int r0 = tile * 32 + (lane & 31);
            const int rr = min(r0, 2 * np - 1);
            nxt = rr >= np;
            const int k = nxt ? rr - np : rr;
            const int w = k >= pre[3] ? 3 : k >= pre[2] ? 2 : k >= pre[1] ? 1 : 0;
            const int pw = k >= pre[3] ? pre[3] : k >= pre[2] ? pre[2] : k >= pre[1] ? pre[1] : 0;
            j = sm.plist[w * 64 + k - pw];
            mine = r0 < 2 * np;
            const float* tr = sp.trans + sm.sidx[j] * PM_TRANS_F;
            float xs[4];
            tile_inputs(tr + (nxt ? 8 : 0), h, xs);
            rb0 = tr[7];
            rb1 = tr[15];
            hidden_half(sm.lw, xs, lane, jt, c2);
            if (mine && !nxt) {
#pragma unroll
                for (int q = 0; q < 16; ++q) put(j, 32 * jt + rho(q) + 4 * h, relu(c2[q]));
            }
            if (jt == 0) {
                heads_half(hf0, c2, lane, 0, ab);
                heads_half(hf1, c2, lane, 0, at);
                *reinterpret_cast<float4*>(&sm.part[wv >> 1][lane][0]) = make_float4(ab[0], ab[1], ab[2], ab[3]);
                *reinterpret_cast<float4*>(&sm.part[wv >> 1][lane][4]) = make_float4(at[0], at[1], at[2], at[3]);
            }
        }
        __syncthreads();  // the chains over layer-2 tile 0
        if (act && jt == 1) {
            const float4 pb = *reinterpret_cast<const float4*>(&sm.part[wv >> 1][lane][0]);
            const float4 pt = *reinterpret_cast<const float4*>(&sm.part[wv >> 1][lane][4]);
            ab[0] = pb.x; ab[1] = pb.y; ab[2] = pb.z; ab[3] = pb.w;
            at[0] = pt.x; at[1] = pt.y; at[2] = pt.z; at[3] = pt.w;
            heads_half(hf0, c2, lane, 1, ab);
            heads_half(hf1, c2, lane, 1, at);
            float qb[3], qt[3];
            heads_finish(ab, hf0, qb);
            heads_finish(at, hf1, qt);
            if (mine && h == 0) {
                if (!nxt) {
                    put(j, 64, qb[0]); put(j, 65, qb[1]); put(j, 66, qb[2]);
                    put(j, 67, rb0);  // reward
                    put(j, 71, rb1);  // action | done << 8 (float bits)
                } else {
                    put(j, 68, qb[0]); put(j, 69, qb[1]); put(j, 70, qb[2]);
                    put(j, 72, qt[0]); put(j, 73, qt[1]); put(j, 74, qt[2]);
                }
            }
        }
        if ((it + 1) * 8 < ntile) __syncthreads();  // block-uniform: part is reused
    }
}
// Returns the control block as block 1 read it (the tree refresh uses the same copy: the learner
// waits for block 1's token or granules, which follow this read, before it commits the next step's).
__device__ __forceinline__ pm_ctrl push_fwd_block(const pm_selfplay& sp, int mode, PushFwdSmem& sm, bool push2, bool pushg) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, B = sp.batch;
    PM_STAMP_ANY(50);
    stage_frags_lds(sp.w_B, sm.lw, 0);
    copy_lds_f32x4<2 * 264>(sp.learn_heads, sm.hf);
    const int64_t id = t < B ? sp.idx[t] : 0;
    const uint32_t gtag = pushg ? __hip_atomic_load(tr_epoch(sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
    __builtin_amdgcn_sched_barrier(0);
    const pm_ctrl cs = *sp.ctrl;
    const int64_t s_after = cs.size + sp.n < sp.cap ? cs.size + sp.n : sp.cap;
    if (!push_handoff(mode, s_after >= B)) {  // block-uniform: no rows to compute
        if ((mode & PM_UPD_FIRST) && t == 0) st_out<true>(push_flag(sp), push_token(cs));
        return cs;
    }
    if (pushg && t == 0) st_out<true>(push_flag(sp), push_token(cs));  // block 1 read the control block
    const bool ip = t < B && push_of(sp, cs.pos, cs.size, cs.max_prio).covers(id);
    const unsigned long long m = __ballot(ip);
    if (ip) sm.plist[wv * 64 + __popcll(m & ((1ull << lane) - 1ull))] = t;
    if (lane == 0) sm.pcnt[wv] = __popcll(m);
    if (t < B) sm.sidx[t] = id;
    __syncthreads();
    PM_STAMP_ANY(51);
    float* pay = sp.hfeat + (size_t)B * 80;
    if (push2)
        push_rows_fwd2(sp, sm, wv, lane, pay, gtag);
    else
        push_rows_fwd(sp, sm.lw, sm.hf, sm.sidx, sm.plist, sm.pcnt, wv, lane,
                      [&](int j, bool nxt, int ln, const f32x16 (&c2)[2], const float (&qb)[3], const float (&qt)[3],
                          const float (&rb)[2]) { store_hfeat<true>(pay, j, nxt, ln, c2, qb, qt, rb); });
    PM_STAMP_ANY(52);
    if (pushg) return cs;  // block-uniform: the granules need no drain, the flag is out
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's payload stores are complete
    __syncthreads();
    PM_STAMP_ANY(53);
    if (t == 0) st_out<true>(push_flag(sp), push_token(cs));
    return cs;
}

// ---- the sum-tree refresh block (round 5): block 1, after the push rows, refreshes every tree node
// the update changes, so the learner's chain ends with its gradients, Adam and the head folds.
// The learner refreshed them itself in two dependent global round trips behind its own stores
// (scatter stores acknowledged -> the touched level-1 nodes' leaves loaded -> level-1 stores
// acknowledged -> the touched level-2 nodes' children loaded: ~8 us of its ~24 us). Block 1 knows
// which nodes those are from the sample indices and the control block alone, so it loads their
// inputs into LDS long before the update's priorities exist:
//   - entries: the B sampled indices, plus (LAST) the next push range's segment ends (its partial
//     level-1 / level-2 nodes); one level-1 slot per distinct sub-block and one level-2 slot per
//     distinct chunk (LDS hash sets), a chunk's 16 positions mapped to the level-1 slots inside it;
//   - LDS DMA: the 64 leaves of every level-1 slot, the 16 level-1 nodes of every level-2 slot;
//   - the learner publishes, as tagged 8-byte granules (hfeat's hand-off rows, MI355X_MICROARCH.md
//     handoff-1to1: one sc1 store each, no flag, no fence), each sample's new leaf prio ** alpha, the
//     next push's max priority and whether the update scattered; block 1 applies the scatter's
//     winners (the last duplicate of an index, as the learner's hash) to its LDS leaves, sums every
//     level-1 slot from LDS with the pending push substituted (per_quarter's order), then every
//     level-2 slot from LDS with the refreshed / pushed children substituted (per_chunk_sum's order),
//     and writes the wholly pushed nodes as the learner did (constants).
// Same functions, same orders: the tree stays bit-identical to a rebuild
// (test_sum_tree_incremental_equals_rebuild). The granule tag is an epoch word block 1 bumps at
// its end (both blocks read it at their start; the next launch's tag is new). A poll that never
// completes (bounded) sets ctrl.status bit 2 and leaves the tree alone. PONGMI_TR=0 (A/B) keeps the
// refresh in the learner.
constexpr int kTrSlots = PM_MAX_BATCH + 8;  // distinct level-1 / level-2 nodes: samples + <= 4 push edges (x8 rows)
constexpr int kTrHash = 1024;                // open-addressing sets keyed by node id
constexpr uint32_t kTrEmpty = 0xFFFFFFFFu;
constexpr int kTrPollMax = 20000;
struct TreeRefreshSmem {
    __attribute__((aligned(16))) float lf[kTrSlots][PER_SUB];   // leaves of every level-1 slot (LDS DMA)
    __attribute__((aligned(16))) double ls[kTrSlots][PER_FAN];  // level-1 nodes of every level-2 slot (LDS DMA)
    double subv[kTrSlots];                                     // refreshed level-1 nodes
    uint32_t subid[kTrSlots], chid[kTrSlots];
    int16_t cmap[kTrSlots][PER_FAN];  // level-2 slot x position -> level-1 slot inside it (-1: none)
    uint32_t skey[kTrHash];
    int sslot[kTrHash];
    uint32_t ckey[kTrHash];
    int cslot[kTrHash];
    uint32_t ikey[512];  // sampled index -> winning sample (the last duplicate, as the learner's hash)
    int iwin[512];
    uint32_t eidx[kTrSlots];  // entries: sampled indices, then the push edges
    int esub[kTrSlots];
    float leaf_new[PM_MAX_BATCH];
    float maxp_next;
    int scattered, ok, nsub, nch;
};
__device__ __forceinline__ uint64_t* tr_granules(const pm_selfplay& sp) {
    return reinterpret_cast<uint64_t*>(sp.hfeat + (size_t)(2 * sp.batch + 1) * 80);
}
__device__ __forceinline__ void tr_publish(const pm_selfplay& sp, int k, uint32_t v, uint32_t tag) {
    __hip_atomic_store(tr_granules(sp) + k, ((uint64_t)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int tr_hash(uint32_t k, int bits) { return (int)((k * 2654435761u) >> (32 - bits)); }
__device__ __forceinline__ int tr_insert(uint32_t* key, uint32_t k, int bits) {
    const int mask = (1 << bits) - 1;
    int h = tr_hash(k, bits);
    for (;;) {
        const uint32_t old = atomicCAS(&key[h], kTrEmpty, k);
        if (old == kTrEmpty || old == k) return h;
        h = (h + 1) & mask;
    }
}
__device__ __forceinline__ int tr_lookup(const uint32_t* key, uint32_t k, int bits) {  // -1: absent
    const int mask = (1 << bits) - 1;
    for (int h = tr_hash(k, bits);; h = (h + 1) & mask) {
        const uint32_t v = key[h];
        if (v == k) return h;
        if (v == kTrEmpty) return -1;
    }
}

__device__ __forceinline__ void tree_block(const pm_selfplay& sp, int mode, TreeRefreshSmem& sm, const pm_ctrl& cs,
                                           int poll_max) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, B = sp.batch;
    PM_STAMP_ANY(55);
    const PerTree tree = per_tree(sp.per_work, sp.cap);
    const uint32_t tag = __hip_atomic_load(tr_epoch(sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    const bool last = mode & PM_UPD_LAST;
    const int64_t s_after = cs.size + sp.n < sp.cap ? cs.size + sp.n : sp.cap;
    const int ns = s_after >= B ? B : 0;  // an update that cannot train scatters nothing
    const int64_t npos = (cs.pos + sp.n) % sp.cap;
    const int64_t end1 = npos + sp.n < sp.cap ? npos + sp.n : sp.cap;
    const int64_t end2 = npos + sp.n - sp.cap;  // > 0: the wrapped part [0, end2)
    const int nedge = last ? (end2 > 0 ? 4 : 2) : 0;
    const int ne = ns + nedge;
    for (int k = t; k < kTrHash; k += kLearn) { sm.skey[k] = kTrEmpty; sm.ckey[k] = kTrEmpty; }
    for (int k = t; k < 512; k += kLearn) { sm.ikey[k] = kTrEmpty; sm.iwin[k] = -1; }
    for (int k = t; k < kTrSlots * PER_FAN; k += kLearn) (&sm.cmap[0][0])[k] = -1;
    if (t == 0) { sm.nsub = 0; sm.nch = 0; sm.ok = 1; }
    if (t < ne) {
        const int64_t e = t < ns ? sp.idx[t] : (t - ns == 0 ? npos : t - ns == 1 ? end1 - 1 : t - ns == 2 ? 0 : end2 - 1);
        sm.eidx[t] = (uint32_t)e;
    }
    __syncthreads();
    if (t < ne) {
        tr_insert(sm.skey, sm.eidx[t] / PER_SUB, 10);
        if (t < ns) atomicMax(&sm.iwin[tr_insert(sm.ikey, sm.eidx[t], 9)], t);
    }
    __syncthreads();
    if (t < kTrHash && sm.skey[t] != kTrEmpty) {  // compact: one level-1 slot per distinct sub-block
        const int s = atomicAdd(&sm.nsub, 1);
        sm.sslot[t] = s;
        sm.subid[s] = sm.skey[t];
    }
    __syncthreads();
    const int nsub = sm.nsub;
    if (t < ne) sm.esub[t] = sm.sslot[tr_lookup(sm.skey, sm.eidx[t] / PER_SUB, 10)];
    if (t < nsub) tr_insert(sm.ckey, sm.subid[t] / PER_FAN, 10);
    __syncthreads();
    if (t < kTrHash && sm.ckey[t] != kTrEmpty) {
        const int c = atomicAdd(&sm.nch, 1);
        sm.cslot[t] = c;
        sm.chid[c] = sm.ckey[t];
    }
    __syncthreads();
    const int nch = sm.nch;
    if (t < nsub) sm.cmap[sm.cslot[tr_lookup(sm.ckey, sm.subid[t] / PER_FAN, 10)]][sm.subid[t] % PER_FAN] = (int16_t)t;
    // LDS DMA: wave instruction i moves 1 KB: level-1 slots 4i .. 4i + 3 (64 leaves each) / level-2
    // slots 8i .. 8i + 7 (16 nodes each); lanes past the count re-read the last slot
    for (int i = wv; 4 * i < nsub; i += kLearn / 64) {
        const int s = min(4 * i + (lane >> 4), nsub - 1);
        __builtin_amdgcn_global_load_lds((const void*)(tree.leaf + (size_t)sm.subid[s] * PER_SUB + 4 * (lane & 15)),
                                         (lds_void*)&sm.lf[4 * i][0], 16, 0, 0);
    }
    for (int i = wv; 8 * i < nch; i += kLearn / 64) {
        const int c = min(8 * i + (lane >> 3), nch - 1);
        __builtin_amdgcn_global_load_lds((const void*)(tree.sub + (size_t)sm.chid[c] * PER_FAN + 2 * (lane & 7)),
                                         (lds_void*)&sm.ls[8 * i][0], 16, 0, 0);
    }
    PM_STAMP_ANY(56);
    // the learner's granules: [0, B) each sample's new leaf, B the next push's max priority, B + 1 flags
    if (t < B + 2) {
        uint64_t g = 0;
        bool got = false;
        for (int it = 0; it < poll_max; ++it) {
            g = __hip_atomic_load(tr_granules(sp) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)(g >> 32) == tag) { got = true; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (!got) sm.ok = 0;
        const uint32_t v = (uint32_t)g;
        if (t < B) sm.leaf_new[t] = __uint_as_float(v);
        else if (t == B) sm.maxp_next = __uint_as_float(v);
        else sm.scattered = (int)(v & 1u);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS DMA landed
    __syncthreads();
    PM_STAMP_ANY(57);
    if (!sm.ok) {  // block-uniform: the learner's granules never came; the tree is left as it was
        if (t == 0) {
            atomicOr(&sp.ctrl->status, PM_CTRL_TREE_TIMEOUT);
            __hip_atomic_store(tr_epoch(sp), tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    if (sm.scattered && t < ns && sm.iwin[tr_lookup(sm.ikey, sm.eidx[t], 9)] == t)
        sm.lf[sm.esub[t]][sm.eidx[t] % PER_SUB] = sm.leaf_new[t];  // the scatter's winner (:74-76)
    const float pval = last ? prio_pow(push_prio(s_after, sm.maxp_next), (float)sp.alpha) : 0.f;
    const PushRange next = last ? PushRange{npos, sp.n, sp.cap, pval} : PushRange{0, 0, sp.cap, 0.f};
    // the next push in 32-bit bounds (cap < 2^31): entries [q1lo, q1hi) and [0, q2hi); wholly pushed
    // level-1 nodes [p1lo, p1hi) and [0, p2hi) — what per_leaf / per_sub_pushed decide, without
    // their 64-bit ring arithmetic per element
    const int cap32 = (int)sp.cap;
    const int q1lo = last ? (int)npos : 0, q1hi = last ? (int)end1 : 0, q2hi = last && end2 > 0 ? (int)end2 : 0;
    const int p1lo = (q1lo + PER_SUB - 1) / PER_SUB, p1hi = q1hi / PER_SUB, p2hi = q2hi / PER_SUB;
    PM_STAMP_ANY(60);
    __syncthreads();
    // level 1: 4 lanes per slot (one quarter each, per_quarter's order), combined as per_combine
    for (int base = 0; base < 4 * nsub; base += kLearn) {
        const int k = base + t, s = min(k >> 2, nsub - 1), q = k & 3;
        const int lo = (int)sm.subid[s] * PER_SUB + 16 * q;
        float v[16];  // the quarter's 16 leaves, read before any select (no load under a branch)
        const float4* l4 = reinterpret_cast<const float4*>(&sm.lf[s][16 * q]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 x = l4[j];
            v[4 * j] = x.x; v[4 * j + 1] = x.y; v[4 * j + 2] = x.z; v[4 * j + 3] = x.w;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(v[j]));
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = lo + i;
            const bool pushed = (e >= q1lo && e < q1hi) || e < q2hi;
            const double x = (double)(pushed ? pval : v[i]);
            acc += e < cap32 ? x : 0.0;  // past cap: no leaf
        }
        const double node = per_combine(quad_f64<0>(acc), quad_f64<1>(acc), quad_f64<2>(acc), quad_f64<3>(acc));
        if (q == 0 && k < 4 * nsub) {
            sm.subv[s] = node;
            tree.sub[sm.subid[s]] = node;
        }
    }
    PM_STAMP_ANY(61);
    const double csub = per_sub_pushed_sum(next);
    {   // the wholly pushed level-1 nodes of the next push: one constant
        const int n1 = p1hi > p1lo ? p1hi - p1lo : 0;
        for (int k = t; k < n1 + p2hi; k += kLearn) tree.sub[k < n1 ? p1lo + k : k - n1] = csub;
    }
    PM_STAMP_ANY(62);
    __syncthreads();
    PM_STAMP_ANY(58);
    // level 2: every chunk slot from LDS, its refreshed / pushed children substituted (per_chunk_sum)
    const int nsub_tree = (int)tree.nsub;
    static_assert(PER_FAN == 16, "one DPP row per level-2 node");
    // one 16-lane DPP row per chunk slot: lane k of the row reads child k (consecutive LDS words; a
    // thread per slot reading its 16 children strided 128 B apart was a 32-way bank conflict per
    // read), and the row's lane 0 folds the 16 terms in per_chunk_sum's order (row_shl:k)
    for (int base = wv * 4; base < nch; base += kLearn / 16) {  // wave-uniform
        const int slot = min(base + (lane >> 4), nch - 1), k = lane & 15;
        const int m = sm.cmap[slot][k];
        const double old = sm.ls[slot][k];
        const double fresh = sm.subv[m >= 0 ? m : 0];
        const int sb = (int)sm.chid[slot] * PER_FAN + k;
        const bool pushed = (sb >= p1lo && sb < p1hi) || sb < p2hi;
        const double v = m >= 0 ? fresh : (pushed ? csub : old);
        const double x = sb < nsub_tree ? v : 0.0;
        double acc = 0.0;
        acc += x;
        acc += dpp_f64<0x101>(x); acc += dpp_f64<0x102>(x); acc += dpp_f64<0x103>(x);
        acc += dpp_f64<0x104>(x); acc += dpp_f64<0x105>(x); acc += dpp_f64<0x106>(x);
        acc += dpp_f64<0x107>(x); acc += dpp_f64<0x108>(x); acc += dpp_f64<0x109>(x);
        acc += dpp_f64<0x10A>(x); acc += dpp_f64<0x10B>(x); acc += dpp_f64<0x10C>(x);
        acc += dpp_f64<0x10D>(x); acc += dpp_f64<0x10E>(x); acc += dpp_f64<0x10F>(x);
        if (k == 0 && base + (lane >> 4) < nch) tree.chunk[sm.chid[slot]] = acc;
    }
    PM_STAMP_ANY(63);
    if (last) {  // the next push's other level-2 nodes: inside a segment (every boundary chunk holds an
                 // edge entry, so it has a slot), all 16 children wholly pushed: one constant
        double cc = 0.0;
#pragma unroll
        for (int k = 0; k < PER_FAN; ++k) cc += csub;
        const int c1lo = q1lo / PER_CHUNK, c1hi = (q1hi - 1) / PER_CHUNK + 1;
        const int c2hi = q2hi > 0 ? (q2hi - 1) / PER_CHUNK + 1 : 0;
        const int n1 = c1hi > c1lo ? c1hi - c1lo : 0;
        for (int k = t; k < n1 + c2hi; k += kLearn) {
            const int ch = k < n1 ? c1lo + k : k - n1;
            if (tr_lookup(sm.ckey, (uint32_t)ch, 10) < 0) tree.chunk[ch] = cc;
        }
    }
    PM_STAMP_ANY(59);
    if (t == 0) __hip_atomic_store(tr_epoch(sp), tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct LearnSmem {
    union {
        float gpart[16][256];  // gradient phase: per-wave partial sums
    } u;
    __attribute__((aligned(16))) float Hs[PM_MAX_BATCH][64];  // ReLU(features(s)) of the batch (LDS DMA rows)
    // hfeat row floats 64..75 of each sample as three float4 planes (LDS DMA: lane t's 16 B at
    // base + 16 t): Q_B(s) 0..2 | r 3 | Q_B(s') 4..6 | action|done bits 7 | Q_T(s') 8..10
    __attribute__((aligned(16))) float qv4[3][PM_MAX_BATCH][4];
    float coef[PM_MAX_BATCH][4]; // dL/d(V, A0, A1, A2) per sample
    float eps_tr[pad256(260)];    // the update's noise (eps section layout)
    int64_t sidx[PM_MAX_BATCH];
    uint32_t hkey[512];          // open-addressing set of sampled indices (last-duplicate-wins)
    int hwin[512];
    float red[16][8];
    long long cnt[16][6];        // per-wave episode counters of the rollout (phase 0)
    long long ctot[6];           // their sums (phase 1)
    int plist[PM_MAX_BATCH];     // samples whose row is in this step's push range, per wave slot
    int pcnt[16];
    int void_upd;                // the push-row hand-off timed out: this update trains nothing
    float loss_out;              // the update's loss, committed to the control block at the kernel's end
    ApplySmem ap;
};

// train_step (:134-168) for the batch k_act_sp sampled, plus the episode counters of the rollout and
// the sum-tree refresh. Single workgroup of 1024 threads; global loads are issued up front.
union LearnShared {
    LearnSmem learn;
    ActSharedLearn act;
    PushFwdSmem pf;
    TreeRefreshSmem tr;
    FeatAheadSmem fa;
};
static_assert(sizeof(LearnShared) <= 160 * 1024, "k_learn LDS");

// Block 0 is the learner. Blocks 1.. (pm_selfplay_learn_act) run the opponents' greedy act for the
// NEXT vector step (train_iterative.py:240, side A) on the observations k_env just wrote: those
// actions depend on nothing the learner changes, and the learner occupies one CU, so they ride in
// this launch on otherwise idle CUs instead of lengthening the next k_act_sp. act_block is
// block-size agnostic: a 1024-thread block stages, compacts and tiles a 4x larger chunk.
// mode (PM_UPD_*): FIRST = the update that follows this step's k_env (its batch may hold rows of the
// push k_env just made, which this kernel computes; it sums the rollout's episode counters); LAST =
// the step's last update (refreshes the sum tree for the next push, commits the step). U = 1: both.
// Block 1 is push_fwd_block; the side-A act blocks (launches with side blocks) follow it.
// A side block's start delay: n x s_sleep 16 (1 024 clocks each; n = 8 ~ the former s_sleep 127)
__device__ __forceinline__ void side_nap(int n) {
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(16);
}

// PG: the push rows as tagged granules (tr bit 3; a separate instantiation: the flag consumer's
// branch beside the granule sweep made the compiler wait for every granule load in turn).
template <bool PG>
__global__ __launch_bounds__(kLearn) void k_learn(const pm_selfplay sp, int chunkA, int chunkP, int mode, int tr, int ftiles, int sleepf, int ahead) {
    __shared__ __attribute__((aligned(16))) LearnShared shm;
    // tr: bit 0 the tree-refresh block, bit 1 push_rows_fwd2, bit 2 the apply's noise in phase 2
    // ahead: bit 0 actions ahead (the feature blocks store gB, the learner publishes the acting heads),
    // bit 1 test hook: the feature blocks' poll for them expires at once
    const bool push2 = (tr & 2) != 0, late_noise = (tr & 4) != 0;
    const int tr_poll = (tr & 16) ? 0 : kTrPollMax;  // bit 4: test hook, the refresh block's poll times out at once
    constexpr bool pushg = PG;
    tr &= 1;
    if (blockIdx.x > 0) {
        if (blockIdx.x == 1) {
            const pm_ctrl cs = push_fwd_block(sp, mode, shm.pf, push2, pushg);
            if (tr) {
                __syncthreads();  // the push rows' LDS is reused
                tree_block(sp, mode, shm.tr, cs, tr_poll);
            }
            return;
        }
        const int sb = (int)blockIdx.x - 2;  // side block index
        PM_SIDE(0, sb, __builtin_amdgcn_s_memrealtime());
        const ActGrid g{sp.n, sp.n_pool + 1, chunkA, chunkP, 0};
        const int fb = sb - g.blocks();
        if (fb >= 0) {  // block-uniform: modelB's features for the next step (sp.featB)
            if (sleepf & 2) side_nap(sleepf >> 8);
            const int t0 = fb * ftiles;
            if (ahead & 1) feat_tiles_ahead(sp, shm.fa, t0, min(t0 + ftiles, feat_ntiles(sp.n)), (ahead & 2) != 0);
            else feat_tiles(shm.act.lw, sp.w_B, sp.obsB, sp.n, t0, min(t0 + ftiles, feat_ntiles(sp.n)), sp.featB);
            PM_STAMP_MAX(67);
            PM_SIDE(2, sb, __builtin_amdgcn_s_memrealtime());
            PM_SIDE(3, sb, 1ull | ((unsigned long long)(min(t0 + ftiles, feat_ntiles(sp.n)) - t0) << 16));
            return;
        }
        // the learner's load phase is latency-bound under the side blocks' staging bursts: the role
        // with slack starts after its loads are in flight (side_sleep: the feature blocks by default)
        if (sleepf & 1) side_nap(sleepf >> 8);
        PM_SIDE(1, sb, __builtin_amdgcn_s_memrealtime());
        const TileOut outA{sp.aA, nullptr, -1.0, 0, 0};
        act_block(shm.act, g, sp.w_opp, sp.n_pool > 0 ? sp.opp : nullptr, nullptr, sp.obsA, nullptr, outA, outA,
                  sb, sp.n_pool + 1 <= kListNets ? sp.opp_list : nullptr, sp.opp_cnt);
        PM_STAMP_MAX(66);
        PM_SIDE(2, sb, __builtin_amdgcn_s_memrealtime());
        PM_SIDE(3, sb, 0ull | ((unsigned long long)shm.act.count << 16));
        return;
    }
    LearnSmem& sm = shm.learn;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int B = sp.batch;
    pm_ctrl* c = sp.ctrl;
    PM_STAMP(0);
    const pm_ctrl cs = *c;  // loop counters as the step found them (only this kernel / k_adam commit)
    const PerTree tree = per_tree(sp.per_work, sp.cap);
    const bool first = mode & PM_UPD_FIRST, last = mode & PM_UPD_LAST;

    // ---- phase 0: every independent load, issued before any use. LDS-bound arrays go global ->
    // LDS directly (global_load_lds); register loads are issued unconditionally (gating them on the
    // control block, or storing each to LDS right away, costs one round trip per load).
    const int nbr = (sp.n + kBlock - 1) / kBlock;
    copy_lds_f32x4<260>(sp.learn_heads + 528, sm.eps_tr);
    if (sp.fuse_apply) load_apply_inputs(sp, sm.ap, false);
    long long part[6] = {0, 0, 0, 0, 0, 0};
    if (first && t < nbr) {
#pragma unroll
        for (int k = 0; k < 6; ++k) part[k] = sp.partials[(size_t)t * 8 + k];
    }
    const float wraw_l = t < B ? sp.isw[t] : 0.f;
    const int64_t id_l = t < B ? sp.idx[t] : 0;
    const float eps_v = t < 260 ? sp.learn_heads[528 + t] : 0.f;
    const uint32_t tr_tag = tr ? __hip_atomic_load(tr_epoch(sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
    const uint32_t gh_tag = (ahead & 1) ? __hip_atomic_load(gh_epoch(sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
    // the rows k_env's forward blocks computed (hfeat [B][80]): sample t's Q block (floats 64..75,
    // phase 2's operands) global -> LDS (qv4 planes) here; its 64 features go global -> LDS below.
    // (Round 4 loaded it to registers: the compiler kept the float4[3] in scratch, a store that
    // waited for the load's round trip at the top of the phase.)
    if (t < PM_MAX_BATCH) {  // wave-uniform: waves 0..3
        const float4* src = reinterpret_cast<const float4*>(sp.hfeat + (size_t)min(t, B - 1) * 80 + 64);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            __builtin_amdgcn_global_load_lds((const void*)(src + k), (lds_void*)&sm.qv4[k][wv * 64][0], 16, 0, 0);
    }
    for (int b = t + kLearn; first && b < nbr; b += kLearn)  // n > 256 * 1024 arenas only
#pragma unroll
        for (int k = 0; k < 6; ++k) part[k] += sp.partials[(size_t)b * 8 + k];
    const int64_t s_after = cs.size + sp.n < sp.cap ? cs.size + sp.n : sp.cap;
    bool train = s_after >= B;  // cleared (block-uniformly) if the push rows never arrive: a void update
    const bool train0 = train;  // as phase 0 found it (the apply's noise counter)
    bool act = train && t < B;
    if (t == 0) sm.void_upd = 0;
    // fused: the optimizer's scalar prologue on waves with slack in this load phase (they are not
    // on the dependent idx -> replay-row path of waves 0-3): the Adam bias corrections (two fp64
    // pow) on the last thread, both NoisyNet draws of the apply on the upper half of the block
    PM_STAMP(35);
    if (sp.fuse_apply && !late_noise) {
        if (t >= kLearn - 2) adam_const_lane(sp, cs.train_steps + 1, sm.ap, t - (kLearn - 2));
        gen_both_noises_on(sp, sm.ap, cs.step + 1, (uint64_t)(cs.train_steps + (train ? 1 : 0)) + 1, kLearn / 2);
    }
    PM_STAMP(34);
    if (train && t < 260) sp.paramsB[PM_QNET_EPS_OFF + t] = eps_v;  // reset_noise leaves it in modelB
    const float wraw = act ? wraw_l : 0.f;
    const int64_t id = act ? id_l : 0;
    for (int k = t; k < 512; k += kLearn) { sm.hkey[k] = kHashEmpty; sm.hwin[k] = -1; }
    if (act) sm.sidx[t] = id;
    {   // samples whose replay row k_env was writing: computed here (phase 1)
        const bool ip = first && act && push_of(sp, cs.pos, cs.size, cs.max_prio).covers(id);
        const unsigned long long m = __ballot(ip);
        if (ip) sm.plist[wv * 64 + __popcll(m & ((1ull << lane) - 1ull))] = t;
        if (lane == 0) sm.pcnt[wv] = __popcll(m);
    }
    PM_STAMP(16);  // (NOWAIT build: wave 0 had idx and the control block)
#if defined(PM_DIAG) && !defined(PM_DIAG_NOWAIT)
    PM_STAMP(30);
    asm volatile("" ::"v"(wraw_l), "v"((int)id_l));
    PM_STAMP(31);
    PM_STAMP(32);
    PM_STAMP(33);
#endif
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const long long s = wave_sum(part[k]);
        if (lane == 0) sm.cnt[wv][k] = s;
    }
    PM_STAMP(17);  // (NOWAIT: the partials)
    {
        const float m = wave_max(wraw);
        if (lane == 0) sm.red[wv][0] = m;
    }
    PM_STAMP(18);  // (NOWAIT: isw)
    PM_STAMP_T(19, 960);  // the last wave reaches the DMA issue
    // ReLU(features(s)) of the batch: each hfeat row's 64 floats global -> LDS (4 rows per wave
    // instruction), issued after every register load of this phase so nothing here waits on them; the
    // first reader is phase 3 (drained before phase 2's barrier, or before the push-row copy)
    if (train)
        for (int ci = wv; 4 * ci < B; ci += kLearn / 64) {
            const int row = min(4 * ci + (lane >> 4), B - 1);
            __builtin_amdgcn_global_load_lds((const void*)(sp.hfeat + (size_t)row * 80 + 4 * (lane & 15)),
                                             (lds_void*)&sm.Hs[4 * ci][0], 16, 0, 0);
        }
#if defined(PM_DIAG) && !defined(PM_DIAG_NOWAIT)
    // (after the feature rows' DMA is issued, as in the product build: the stamps include it landing;
    // PM_DIAG_NOWAIT drops this wait, so the timeline's later phases run as in the product build)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // this wave's loads (incl. LDS DMA) landed
    PM_STAMP_T(40, 0); PM_STAMP_T(41, 256); PM_STAMP_T(42, 512); PM_STAMP_T(43, 960);
#endif
    __syncthreads();
    PM_STAMP(1);

    // ---- phase 1: counters; the batch forward on the matrix cores (one 32-row tile per wave)
    long long ep_fin = 0;
    bool waited = false;  // block-uniform: the push-row token was seen
    if (t < 6) {
        long long s = 0;
        for (int w = 0; w < 16; ++w) s += sm.cnt[w][t];
        sm.ctot[t] = s;  // read after the next barrier
    }
    if (sp.fuse_apply && first && !late_noise && t == kLearn - 1) {  // the per-episode epsilon decay (:261) beside the forward
        long long s = 0;                     // (same sum, same order as thread 0's ctot[0])
        for (int w = 0; w < 16; ++w) s += sm.cnt[w][0];
        sm.ap.eps_next = cs.epsilon * pow(sp.epsilon_decay, (double)(float)s);
        PM_STAMP_T(37, kLearn - 1);
    }
    if (train) {  // rows in the push range (s rows then s' rows)
        int pre[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < 4; ++w) pre[w + 1] = pre[w] + sm.pcnt[w];  // B <= 256: waves 0..3
        const int np = pre[4];
        if (np > 0 && push_handoff(mode, train)) {  // block-uniform: block 1 computes them
            waited = true;
            if constexpr (PG) {  // the granules: up to 4 per thread in flight, re-polled until their tags match
                const uint64_t* pg = push_granules(sp);
                const int tot = np * kPushGN;
                uint64_t g[4];
                int jf[4];
                auto issue = [&](int k0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = k0 + u * kLearn;
                        g[u] = (uint64_t)tr_tag << 32;  // past the end: no load (reads as arrived)
                        jf[u] = 0;
                        if (k < tot) {
                            const int q = k / kPushGN, f = k - q * kPushGN;
                            const int w = q >= pre[3] ? 3 : q >= pre[2] ? 2 : q >= pre[1] ? 1 : 0;
                            const int pw = q >= pre[3] ? pre[3] : q >= pre[2] ? pre[2] : q >= pre[1] ? pre[1] : 0;
                            jf[u] = sm.plist[w * 64 + q - pw] * kPushGF + f;
                            g[u] = __hip_atomic_load(pg + jf[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                };
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the feature rows' DMA, before rows are overwritten
                issue(t);  // the first round trip rides under the barrier
                __syncthreads();
                PM_STAMP(54);
                for (int k0 = t; k0 < tot; k0 += 4 * kLearn) {
                    if (k0 != t) issue(k0);
                    for (int it = 0;; ++it) {
                        bool done = true;
#pragma unroll
                        for (int u = 0; u < 4; ++u) done &= (uint32_t)(g[u] >> 32) == tr_tag;
                        if (done) break;
                        if (it == kPushPollMax) {  // never came: this update trains nothing (status bit 0)
                            sm.void_upd = 1;
                            sp.ctrl->status = cs.status | PM_CTRL_PUSH_TIMEOUT;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if ((uint32_t)(g[u] >> 32) != tr_tag)
                                g[u] = __hip_atomic_load(pg + jf[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (k0 + u * kLearn >= tot) break;
                        const int j = jf[u] / kPushGF, f = jf[u] - j * kPushGF;
                        const float v = __uint_as_float((uint32_t)g[u]);
                        if (f < 64) sm.Hs[j][f] = v;
                        else sm.qv4[(f - 64) >> 2][j][f & 3] = v;
                    }
                }
                PM_STAMP_T(36, 0);
            } else {
            if (t == 0 && !push_wait(sp, cs)) sm.void_upd = 1;
            PM_STAMP_T(36, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the feature rows' DMA, before rows are overwritten
            __syncthreads();
            PM_STAMP(54);
            const float* pay = sp.hfeat + (size_t)B * 80;
            for (int k = t; k < np * 76; k += kLearn) {
                const int q = k / 76, f = k - q * 76;
                const int w = q >= pre[3] ? 3 : q >= pre[2] ? 2 : q >= pre[1] ? 1 : 0;
                const int j = sm.plist[w * 64 + q - pre[w]];
                const float v = __hip_atomic_load(pay + (size_t)j * 80 + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (f < 64) sm.Hs[j][f] = v;
                else sm.qv4[(f - 64) >> 2][j][f & 3] = v;
            }
            }
        }
    }
    float wmax = sm.red[0][0];
    for (int w = 1; w < 16; ++w) wmax = fmaxf(wmax, sm.red[w][0]);
    if (t < PM_MAX_BATCH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the qv4 DMA (waves 0..3)
    __syncthreads();
    PM_STAMP(2);
    if (sm.void_upd) train = act = false;  // block-uniform: the hand-off timed out
    ep_fin = sm.ctot[0];
    // the rollout bookkeeping (:245-249) is committed at the kernel's end (commit_counters): stored
    // here, wave 0's vmcnt(0) before phase 2's barrier waited for these stores' acknowledgements

    // ---- phase 2: double-DQN targets, loss, priorities, bias grads
    float lossp = 0.f, prio = 0.f;
    float cf[4] = {0.f, 0.f, 0.f, 0.f};
    int slot = 0;
    if (act) {
        const float4 v0 = *reinterpret_cast<const float4*>(sm.qv4[0][t]);
        const float4 v1 = *reinterpret_cast<const float4*>(sm.qv4[1][t]);
        const float4 v2 = *reinterpret_cast<const float4*>(sm.qv4[2][t]);
        const float rwd = v0.w;
        const int bits = __float_as_int(v1.w);
        const int a = bits & 0xff, dn = (bits >> 8) & 1;
        const float qs[3] = {v0.x, v0.y, v0.z};
        const float qn[3] = {v1.x, v1.y, v1.z};
        const float qt[3] = {v2.x, v2.y, v2.z};
        const float q = qs[a];                                            // modelB(s).gather(a)   (:152)
        const float nq = qt[argmax3(qn)];                                 // targetB(ns)[argmax modelB(ns)]
        const float tgt = rwd + (float)sp.gamma * nq * (dn ? 0.f : 1.f);  // r + gamma*nq*(~d)     (:156)
        const float diff = q - tgt;
        const float w = wraw / wmax;                                      // w /= w.max() (:72)
        lossp = w * (diff * diff);
        const float g = 2.f * w * diff / (float)B;  // d mean(w (q-t)^2) / dq
        cf[0] = g;
#pragma unroll
        for (int k = 0; k < 3; ++k) cf[1 + k] = g * ((k == a ? 1.f : 0.f) - 1.f / 3.f);
        *reinterpret_cast<float4*>(sm.coef[t]) = make_float4(cf[0], cf[1], cf[2], cf[3]);
        prio = fabsf(diff) + 1e-6f;  // |err| + 1e-6 (:76)
        // update_priorities runs sequentially (:74-76): the last duplicate of an index wins
        const uint32_t key = (uint32_t)id;
        slot = (int)((key * 2654435761u) >> 23);
        for (;;) {
            const uint32_t old = atomicCAS(&sm.hkey[slot], kHashEmpty, key);
            if (old == kHashEmpty || old == key) break;
            slot = (slot + 1) & 511;
        }
        atomicMax(&sm.hwin[slot], t);
    } else if (sp.fuse_apply && late_noise && t >= kLearn / 2) {
        // the apply's scalar prologue on waves this phase leaves idle (late_noise; else in phase 0):
        // Adam's bias corrections (two fp64 pow) and both NoisyNet draws, consumed from phase 4 on.
        // (the train-step counter: `train` as phase 1 settled it, as the phase-0 draw would have it
        // when no hand-off timed out)
        // (and the per-episode epsilon decay (:261), one fp64 pow per lane in one instruction stream:
        // lane 61 decay^D, lanes 62 / 63 the Adam corrections)
        if (t >= kLearn - 3) {
            const int which = t - (kLearn - 2);  // -1: the epsilon decay
            long long s = 0;                     // (same sum, same order as thread 0's ctot[0])
            for (int w = 0; w < 16; ++w) s += sm.cnt[w][0];
            const double base = which < 0 ? sp.epsilon_decay : which ? sp.beta2 : sp.beta1;
            const double ex = which < 0 ? (double)(float)s : (double)(cs.train_steps + 1);
            const double p = pow(base, ex);
            if (which < 0) {
                if (first) sm.ap.eps_next = cs.epsilon * p;
            } else {
                const double bc = 1.0 - p;
                sm.ap.ak[which] = which ? (float)sqrt(bc) : (float)(sp.lr / bc);
            }
        }
        gen_both_noises_on(sp, sm.ap, cs.step + 1, (uint64_t)(cs.train_steps + (train0 ? 1 : 0)) + 1, kLearn / 2);
    }
    {
        const float s = wave_sum(lossp), mp = wave_max(prio);
#pragma unroll
        for (int k = 0; k < 4; ++k) cf[k] = wave_sum(cf[k]);
        if (lane == 0) {
            sm.red[wv][1] = s; sm.red[wv][2] = mp;
#pragma unroll
            for (int k = 0; k < 4; ++k) sm.red[wv][3 + k] = cf[k];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the feature rows (phase 3 reads them)
    __syncthreads();
    PM_STAMP(3);

    // ---- phase 3: priority scatter; head gradients (16 waves x 16 samples, fixed-order combine)
    float mpx = 0.f;
    if (train) {
        mpx = sm.red[0][2];
        for (int w = 1; w < 16; ++w) mpx = fmaxf(mpx, sm.red[w][2]);
    }
    const float leaf_v = act ? prio_pow(prio, (float)sp.alpha) : 0.f;
    if (tr) {  // the tree-refresh block's inputs (tree_block): every sample's leaf, the next push's max
               // priority and whether this update scatters, as tagged granules
        if (t < B) tr_publish(sp, t, __float_as_uint(leaf_v), tr_tag);
        if (t == B) tr_publish(sp, B, __float_as_uint(train ? fmaxf(cs.max_prio, mpx) : cs.max_prio), tr_tag);
        if (t == B + 1) tr_publish(sp, B + 1, train ? 1u : 0u, tr_tag);
    }
    if (train) {
        if (act && sm.hwin[slot] == t) {
            sp.prios[id] = prio;
            tree.leaf[id] = leaf_v;
            if (prio != prio) atomicOr(&sp.ctrl->status, PM_CTRL_NAN_PRIO);
        }
        if (t == 0) {
            float l = 0.f;
            for (int w = 0; w < 16; ++w) l += sm.red[w][1];
            sm.loss_out = l / (float)B;  // committed at the kernel's end, with the counters
        }
        const int col = t & 63;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        const int j0 = wv * 16, j1 = min(j0 + 16, B);
        for (int j = j0; j < j1; ++j) {
            const float4 k4 = *reinterpret_cast<const float4*>(sm.coef[j]);
            const float h = sm.Hs[j][col];
            g[0] = fmaf(k4.x, h, g[0]);
            g[1] = fmaf(k4.y, h, g[1]);
            g[2] = fmaf(k4.z, h, g[2]);
            g[3] = fmaf(k4.w, h, g[3]);
        }
        // lw / hf are dead: the forward finished before the last barrier
#pragma unroll
        for (int r = 0; r < 4; ++r) sm.u.gpart[wv][r * 64 + col] = g[r];
    }
    const float max_prio_next = train ? fmaxf(cs.max_prio, mpx) : cs.max_prio;
    if (!tr) __threadfence_block();  // phase 4 re-reads the scattered leaves (this workgroup: no L2 writeback)
    __syncthreads();
    PM_STAMP(4);

    // ---- phase 4: gradients out; sum tree: sub-blocks of the scatter and of the next push range
    // not the last update: no pending push (empty range: refreshed nodes are plain sums of the leaves)
    const PushRange next = last ? push_of(sp, (cs.pos + sp.n) % sp.cap, s_after, max_prio_next)
                                : PushRange{0, 0, sp.cap, 0.f};
    if (train) {
        if (t < 256) {  // dL/dW_mu = sum_j coef_j h_j; dL/dW_sigma = dL/dW_mu * eps (the update's noise)
            float g = 0.f;
#pragma unroll
            for (int w = 0; w < 16; ++w) g += sm.u.gpart[w][t];
            const int row = t >> 6, col = t & 63;
            float* gs = sm.ap.g;
            const int a = row - 1;  // fc_V.weight_mu / _sigma, or fc_A.weight_mu / _sigma (row a)
            const int kmu = row == 0 ? col : 130 + a * 64 + col, ksg = row == 0 ? 65 + col : 325 + a * 64 + col;
            const float gsg = g * sm.eps_tr[row == 0 ? P_VWEP - PM_QNET_EPS_OFF + col
                                                     : P_AWEP - PM_QNET_EPS_OFF + a * 64 + col];
            gs[kmu] = g;
            gs[ksg] = gsg;
            if (sp.fuse_apply) {  // the optimizer step on the two parameters this thread owns
                adam_two(sp, sm.ap, kmu, g, ksg, gsg);
            }
        } else if (t < 260) {  // dL/db_mu = sum_j coef_j
            const int k = t - 256;
            float g = 0.f;
            for (int w = 0; w < 16; ++w) g += sm.red[w][3 + k];
            float* gs = sm.ap.g;
            // fc_V.bias_mu / _sigma, or fc_A.bias_mu / _sigma (k - 1)
            const int kmu = k == 0 ? 64 : 322 + k - 1, ksg = k == 0 ? 129 : 517 + k - 1;
            const float gsg = g * sm.eps_tr[k == 0 ? P_VBEP - PM_QNET_EPS_OFF : P_ABEP - PM_QNET_EPS_OFF + k - 1];
            gs[kmu] = g;
            gs[ksg] = gsg;
            if (sp.fuse_apply) {
                adam_two(sp, sm.ap, kmu, g, ksg, gsg);
            }
        }
        // actions ahead: thread t < 260 owns both parameters (mu, sigma) of the acting head value t,
        // final as of its two adam_one calls. It folds that value here (fold_heads_from's k = t
        // iteration: the expression derive_weights evaluates again for w_B, on the same operands) and
        // hands it to the feature blocks ~2 us before the block-wide fold behind the next barriers.
        if ((ahead & 1) && t < 260) {
            fold_heads_from(sm.ap.hp, nullptr, sm.ap.nact, PM_FOLD_TRAIN_FRESH, sm.ap.heads[0], nullptr, t, kLearn);
            gh_publish(sp, t, gh_tag, sm.ap.heads[0][t]);
            PM_STAMP(22);
        }
        PM_STAMP(8); PM_STAMP_T(9, 960);
        if (!tr) {  // level-1 nodes of the scatter: 4 lanes per sampled index (duplicates recompute the
                    // same node from the same leaves: identical values)
            const int j = min(t >> 2, B - 1);
            const int64_t sb = sm.sidx[j] / PER_SUB;
            const double v = per_sub_sum4(tree.leaf, sb, next);
            if ((t & 3) == 0) tree.sub[sb] = v;
        }
        PM_STAMP(10); PM_STAMP_T(11, 960);
    } else {
        for (int k = t; k < kGradN; k += kLearn) sm.ap.g[k] = 0.f;
    }
    if (t == 0) { sm.ap.g[kGradN] = (float)ep_fin; sm.ap.g[kGradN + 1] = train ? 1.f : 0.f; }
    if (!tr) {  // level-1 nodes of the next push: wholly pushed ones are one constant; the <= 4 partially
                // pushed ones at the segment ends are summed from the leaves by 4 lanes of wave 0 each
        const RingNodes rn = ring_nodes(next, PER_SUB);
        const double csub = per_sub_pushed_sum(next);
        for (int64_t k = t; k < rn.count(); k += kLearn) {
            const int64_t sb = rn.at(k);
            if (per_sub_pushed(sb, next)) tree.sub[sb] = csub;
        }
        PM_STAMP(12); PM_STAMP_T(13, 960);
        if (wv == 0) {
            const int g = lane >> 2;
            const bool ok = g < 4 && (g < 2 ? rn.na : rn.nb) > 0;
            const int64_t sb = !ok ? 0 : g == 0 ? rn.a0 : g == 1 ? rn.a0 + rn.na - 1 : g == 2 ? 0 : rn.nb - 1;
            const double v = per_sub_sum4(tree.leaf, sb, next);
            if (ok && (lane & 3) == 0 && !per_sub_pushed(sb, next)) tree.sub[sb] = v;
        }
    }
    PM_STAMP(14); PM_STAMP_T(15, 960);
    if (!tr) __threadfence_block();  // phase 5 re-reads the level-1 nodes (this workgroup: no L2 writeback)
    __syncthreads();
    PM_STAMP(5);
    for (int k = t; k < kGradN + 2; k += kLearn) sp.grad[k] = sm.ap.g[k];
    // ---- phase 5: level-2 nodes over the refreshed sub-blocks; beside them (fused) the target sync
    // and the three head folds of derive_weights, which run on threads 256.. (level 2's are < 256)
    if (!tr && act && sm.hwin[slot] == t) {
        const int64_t ch = id / PER_CHUNK;
        tree.chunk[ch] = per_chunk_sum(tree, ch);
    }
    if (!tr) {
        const RingNodes rn = ring_nodes(next, PER_CHUNK);
        for (int64_t k = t; k < rn.count(); k += kLearn) {
            const int64_t ch = rn.at(k);
            tree.chunk[ch] = per_chunk_sum(tree, ch);
        }
    }
    PM_STAMP(6);
    if (sp.fuse_apply && first && !waited) {  // block 1 read the control block before this launch commits it
        if (t == 0) push_wait(sp, cs);
        __syncthreads();
    }
    // unsharded: Adam ran with the gradients (phase 4), and with it the acting heads' hand-off; an update
    // that did not train (block-uniform) publishes them from the block-wide fold
    if (sp.fuse_apply) apply_finish(sp, sm.ap, cs, mode, (ahead & 1) && !train, gh_tag);
    if (t == 0) {  // the counters, last: no store of theirs sits in front of a phase's vmcnt(0) wait
        // the heads' epoch: this launch's tag is spent (every feature block read the epoch at its start)
        if (ahead & 1) __hip_atomic_store(gh_epoch(sp), gh_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (first) {  // rollout bookkeeping (:245-249)
            c->ep_step = ep_fin;
            c->episodes = cs.episodes + ep_fin;
            c->ep_A = cs.ep_A + sm.ctot[1]; c->win_A = cs.win_A + sm.ctot[2];
            c->ep_P = cs.ep_P + sm.ctot[3]; c->win_P = cs.win_P + sm.ctot[4];
            c->reward_B = cs.reward_B + (double)sm.ctot[5];
        }
        if (train) {
            c->last_loss = sm.loss_out;
            c->max_prio = max_prio_next;  // n > batch pushes of max_prio survive the scatter
        }
    }
    PM_STAMP(7);
}

// ------------------------------------------------------------------------------------ Adam + commit
// The scalar prologue (both noises, the bias-correction and epsilon-decay pows) runs while the
// loads are in flight: every thread reads the all-reduced updated flag and episode count itself.
__global__ __launch_bounds__(kLearn) void k_adam(const pm_selfplay sp, int mode) {
    __shared__ ApplySmem sm;
    const int t = threadIdx.x;
    const pm_ctrl cs = *sp.ctrl;
    load_apply_inputs(sp, sm, true);
    const float D = sp.grad[kGradN], upd = sp.grad[kGradN + 1];  // finished episodes | updated flag (all shards)
    const int64_t ts = cs.train_steps + (upd > 0.5f ? 1 : 0);
    gen_both_noises_on(sp, sm, cs.step + 1, (uint64_t)ts + 1, kLearn / 2);
    if (t >= kLearn - 2) adam_const_lane(sp, cs.train_steps + 1, sm, t - (kLearn - 2));
    if (t == kLearn / 2 - 1) sm.eps_next = cs.epsilon * pow(sp.epsilon_decay, (double)D);  // as apply_update's D
    __syncthreads();
    apply_adam(sp, sm);
    __syncthreads();
    apply_finish(sp, sm, cs, mode);
}

// pm_selfplay_prepare: features + acting weights of the current step + next update's heads
__global__ __launch_bounds__(kLearn) void k_prepare(const pm_selfplay sp) {
    __shared__ ApplySmem sm;
    write_feature_frags(sp.paramsB, sp.w_B);
    load_apply_inputs(sp, sm, false);
    gen_both_noises(sp, sm, sp.ctrl->step, (uint64_t)sp.ctrl->train_steps + 1);
    __syncthreads();
    derive_weights(sp, sm);
}

// pm_selfplay_commit, pass 1: max(prios[0, size)) (memory.push: prios.max(), :57) as float bits into
// ctrl->max_bits (priorities are > 0, so the int order of the bits is the float order).
constexpr int kMaxBlocks = 512;
__global__ __launch_bounds__(256) void k_prio_max(const pm_selfplay sp) {
    __shared__ float red[4];
    const pm_ctrl* c = sp.ctrl;
    const int64_t s = c->size + sp.n;
    const int64_t size = s < sp.cap ? s : sp.cap;
    const int64_t n4 = size / 4;
    const float4* p4 = reinterpret_cast<const float4*>(sp.prios);
    float m = 0.f;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n4; k += (int64_t)gridDim.x * 256) {
        const float4 v = p4[k];
        m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    if (blockIdx.x == 0 && threadIdx.x < size - 4 * n4) m = fmaxf(m, sp.prios[4 * n4 + threadIdx.x]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        atomicMax(&sp.ctrl->max_bits, __float_as_int(m));
    }
}

// pm_selfplay_commit, pass 2 (one workgroup): max_prio = that maximum; the sum tree's level-1 then
// level-2 nodes over the next push range with the push substituted (as k_learn's LAST update does);
// pos / size / step advance.
__global__ __launch_bounds__(kLearn) void k_commit(const pm_selfplay sp) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    pm_ctrl* c = sp.ctrl;
    const pm_ctrl cs = *c;
    const PerTree tree = per_tree(sp.per_work, sp.cap);
    const int64_t s = cs.size + sp.n;
    const int64_t s_after = s < sp.cap ? s : sp.cap;
    const float mp = __int_as_float(cs.max_bits);
    const PushRange next = push_of(sp, (cs.pos + sp.n) % sp.cap, s_after, mp);
    {
        const RingNodes rn = ring_nodes(next, PER_SUB);
        const double csub = per_sub_pushed_sum(next);
        for (int64_t k = t; k < rn.count(); k += kLearn) {
            const int64_t sb = rn.at(k);
            if (per_sub_pushed(sb, next)) tree.sub[sb] = csub;
        }
        if (wv == 0) {  // the <= 4 partially pushed nodes at the segment ends, 4 lanes each
            const int g = lane >> 2;
            const bool ok = g < 4 && (g < 2 ? rn.na : rn.nb) > 0;
            const int64_t sb = !ok ? 0 : g == 0 ? rn.a0 : g == 1 ? rn.a0 + rn.na - 1 : g == 2 ? 0 : rn.nb - 1;
            const double v = per_sub_sum4(tree.leaf, sb, next);
            if (ok && (lane & 3) == 0 && !per_sub_pushed(sb, next)) tree.sub[sb] = v;
        }
    }
    __threadfence_block();
    __syncthreads();
    {
        const RingNodes rn = ring_nodes(next, PER_CHUNK);
        for (int64_t k = t; k < rn.count(); k += kLearn) {
            const int64_t ch = rn.at(k);
            tree.chunk[ch] = per_chunk_sum(tree, ch);
        }
    }
    if (t == 0) {
        c->max_prio = mp;
        c->max_bits = 0;
        c->pos = (cs.pos + sp.n) % sp.cap;
        c->size = s_after;
        c->step = cs.step + 1;
    }
}

// ------------------------------------------------------------------------------------ U > 1 in one launch
// k_learn_multi: updates 1..U-1 of a vector step (after update 0's k_learn, before pm_selfplay_commit)
// as ONE single-workgroup launch, instead of k_resample + k_batch_fwd + k_learn per update (three
// launches, two of them on other CUs, ~30 us per update). Bit-identical to that sequence: the same
// PER descent (the chunk-level prefix in per_round_prefix's order, per_group_find for levels 1 and
// 0), the same head chains as tile_heads, and k_learn's phases 2-5 and fused apply in the same
// arithmetic order. What makes one workgroup enough:
//   - the features are frozen (train_iterative.py:97), so the batch forward needs only the heads:
//     ReLU(features(s)) of every replay row is stored at push time (sp.frow, written by k_actenv from
//     featB), features(s') of row i is frow[(i + n) % cap] (the same arena's next push) or, for this
//     step's own push, featB; a done row's s' never enters the target (nq * (1 - done)), so the
//     post-reset features stand in for the terminal ones there;
//   - the sum tree's top level (<= 1024 chunk sums) lives in LDS for all the updates; tree reads go
//     around L1 (nontemporal loads), so the workgroup's own scatters and refreshes are always seen;
//   - head parameters, Adam moments, the update's noisy heads and the next noise stay in LDS; the
//     global copies are written as the sequence of launches would leave them.
constexpr int kMultiChunks = PER_ROUND;  // level-2 nodes kept in LDS (capacity <= 1 M entries)

struct MultiSmem {
    float Hs[PM_MAX_BATCH][68];   // ReLU(features(s)) of the batch (k_learn's Hs); 16-byte rows
    float qv[PM_MAX_BATCH][12];   // Q_B(s) 0..2 | r 3 | Q_B(s') 4..6 | action|done bits 7 | Q_T(s') 8..10
    float coef[PM_MAX_BATCH][4];
    float gpart[16][256];
    float hf[2][264];             // the update's modelB heads (fresh noise) | targetB heads, fragment order
    float eps_tr[pad256(260)];    // the update's noise (eps section layout)
    double chunk[kMultiChunks];   // level-2 nodes
    double incl[kMultiChunks];    // their inclusive prefix (per_round_prefix)
    double wsum[16];
    int64_t sidx[PM_MAX_BATCH];
    uint32_t hkey[512];
    int hwin[512];
    float red[16][8];
    double total;
    double pa[PM_MAX_BATCH];      // the drawn leaf's value per sample (its IS weight's pow in a pass of its own)
    int64_t ts, frame;            // train_steps, frame_idx as the updates advance them
    float maxp, loss;
    ApplySmem ap;
    // the kernel's arguments, copied once: multi_update (not inlined) reads them through a reference,
    // which for the kernel-argument struct itself meant a private (scratch) copy read per use
    pm_selfplay sp;
};
static_assert(sizeof(MultiSmem) <= 160 * 1024, "k_learn_multi LDS");

template <typename T>
__device__ __forceinline__ T ld_nt(const T* p) { return __builtin_nontemporal_load(p); }
typedef float f32x4v __attribute__((ext_vector_type(4)));
// 16 consecutive floats [lo, lo + 16) around L1 (4 x 16-byte loads; scalar loads past cap read 0).
// 16-scalar-load sweeps of a 4-lane group per sample cost 15 us per level here (one request per lane
// and load), the 16-byte ones a tenth of that.
__device__ __forceinline__ void ld_nt16(const float* p, int64_t lo, int64_t cap, float (&v)[16]) {
    if (lo + 16 <= cap) {
        const f32x4v* p4 = reinterpret_cast<const f32x4v*>(p + lo);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4v x = __builtin_nontemporal_load(p4 + q);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = lo + i < cap ? ld_nt(p + lo + i) : 0.f;
    }
}

// per_quarter / per_sub_sum4 (no pending push) with loads around L1.
__device__ __forceinline__ double multi_quarter(const float* leaf, int64_t sb, int k, int64_t cap) {
    const int64_t lo = sb * PER_SUB + 16 * k;
    float v[16];
    ld_nt16(leaf, lo, cap, v);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += lo + i < cap ? (double)v[i] : 0.0;
    return acc;
}
__device__ __forceinline__ double multi_sub_sum4(const float* leaf, int64_t sb, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const double q = multi_quarter(leaf, sb, lane & 3, cap);
    return per_combine(quad_f64<0>(q), quad_f64<1>(q), quad_f64<2>(q), quad_f64<3>(q));
}
__device__ __forceinline__ double multi_chunk_sum(const PerTree& t, int64_t c) {
    typedef double f64x2v __attribute__((ext_vector_type(2)));
    double v[PER_FAN];
    if (c * PER_FAN + PER_FAN <= t.nsub) {  // sub is 256-byte aligned: 16-byte loads of the node's 16
        const f64x2v* p = reinterpret_cast<const f64x2v*>(t.sub + c * PER_FAN);
#pragma unroll
        for (int k = 0; k < PER_FAN / 2; ++k) {
            const f64x2v x = __builtin_nontemporal_load(p + k);
            v[2 * k] = x.x;
            v[2 * k + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER_FAN; ++k) v[k] = c * PER_FAN + k < t.nsub ? ld_nt(t.sub + c * PER_FAN + k) : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PER_FAN; ++k) acc += v[k];
    return acc;
}

// One lane half's share of tile_heads: the fmaf chains over this half's 32 units (32 tt + 8 q4 + 4 h
// + e, in tile_heads' (t, r) order with r = 4 q4 + e), x[16 tt + 4 q4 + e] = ReLU'd feature. The
// cross-half add and the rest follow in half_heads_finish (lanes t and t ^ 1 hold the two halves).
__device__ __forceinline__ void half_chains(const float* hf, int h, const float (&x)[32], float (&s)[4]) {
    float v = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const float4* hw = reinterpret_cast<const float4*>(hf + h * 128);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const float4 w = hw[k];  // (t, r) = (k >> 4, k & 15): unit 32 t + rho(r) + 4 h
        v = fmaf(w.x, x[k], v);
        a0 = fmaf(w.y, x[k], a0);
        a1 = fmaf(w.z, x[k], a1);
        a2 = fmaf(w.w, x[k], a2);
    }
    s[0] = v; s[1] = a0; s[2] = a1; s[3] = a2;
}
// The same chains for two rows with one sweep of the weights (the sweep's LDS reads bound this phase).
__device__ __forceinline__ void half_chains2(const float* hf, int h, const float (&xa)[32], const float (&xb)[32],
                                             float (&sa)[4], float (&sb)[4]) {
    float v = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, u = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    const float4* hw = reinterpret_cast<const float4*>(hf + h * 128);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const float4 w = hw[k];
        v = fmaf(w.x, xa[k], v);
        a0 = fmaf(w.y, xa[k], a0);
        a1 = fmaf(w.z, xa[k], a1);
        a2 = fmaf(w.w, xa[k], a2);
        u = fmaf(w.x, xb[k], u);
        b0 = fmaf(w.y, xb[k], b0);
        b1 = fmaf(w.z, xb[k], b1);
        b2 = fmaf(w.w, xb[k], b2);
    }
    sa[0] = v; sa[1] = a0; sa[2] = a1; sa[3] = a2;
    sb[0] = u; sb[1] = b0; sb[2] = b1; sb[3] = b2;
}
__device__ __forceinline__ void half_heads_finish(const float* hf, const float (&s)[4], float (&q)[3]) {
    float v = s[0] + __shfl_xor(s[0], 1), a0 = s[1] + __shfl_xor(s[1], 1);  // v_h0 + v_h1 in either lane
    float a1 = s[2] + __shfl_xor(s[2], 1), a2 = s[3] + __shfl_xor(s[3], 1);
    v += hf[256];
    a0 += hf[257];
    a1 += hf[258];
    a2 += hf[259];
    const float mean = ((a0 + a1) + a2) / 3.0f;
    q[0] = v + (a0 - mean);
    q[1] = v + (a1 - mean);
    q[2] = v + (a2 - mean);
}

// Half h's 32 ReLU'd features of a replay row from frow (8 float4: units 32 tt + 8 q4 + 4 h + 0..3) ...
__device__ __forceinline__ void load_frow_half(const float* frow, int64_t slot, int h, float (&x)[32]) {
    const float4* p = reinterpret_cast<const float4*>(frow + slot * 64) + h;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = p[2 * k];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
}
// ... or of one arena from featB (feat_tiles' layout: tile a / 32, piece 4 tt + q4, lane half h,
// component e; pre-ReLU there).
__device__ __forceinline__ void load_featB_half(const float* featB, int a, int h, float (&x)[32]) {
    const float4* p = reinterpret_cast<const float4*>(featB) + (size_t)(a >> 5) * 8 * 64 + 32 * h + (a & 31);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = p[k * 64];
        x[4 * k] = relu(v.x); x[4 * k + 1] = relu(v.y); x[4 * k + 2] = relu(v.z); x[4 * k + 3] = relu(v.w);
    }
}

// per_group_find<16> over lv[k] = lo + k < size ? (double)f[k] : 0 with the leaves kept as floats.
__device__ __forceinline__ int group_find16f(const float (&f)[16], int64_t lo, int64_t size, double x, double& before,
                                             double& val) {
    const int lane = threadIdx.x & 63, q = lane & 3, g0 = lane & ~3;
    auto lv = [&](int e) { return lo + e < size ? (double)f[e] : 0.0; };
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc += lv(e);
    const double s0 = quad_f64<0>(acc), s1 = quad_f64<1>(acc), s2 = quad_f64<2>(acc);
    const double ex = q == 0 ? 0.0 : (q == 1 ? s0 : (q == 2 ? s0 + s1 : (s0 + s1) + s2));
    int hit = -1, nz = -1;
    double hb = 0.0, hv = 0.0, nb = 0.0, nv = 0.0, run = ex;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const double v = lv(e);
        if (hit < 0 && run + v > x) { hit = e; hb = run; hv = v; }
        if (v > 0.0) { nz = e; nb = run; nv = v; }
        run += v;
    }
    const unsigned gh = (unsigned)(__ballot(hit >= 0) >> g0) & 15u;
    const unsigned gn = (unsigned)(__ballot(nz >= 0) >> g0) & 15u;
    int src, k;
    if (gh) {
        src = __ffs(gh) - 1;
        k = hit;
    } else {
        src = gn ? 31 - __clz(gn) : 0;
        k = nz < 0 ? 0 : nz;
        hb = nz < 0 ? ex : nb;
        hv = nz < 0 ? 0.0 : nv;
    }
    const int kk = quad_sel_i32(k, src);
    before = quad_sel_f64(hb, src);
    val = quad_sel_f64(hv, src);
    return src * 16 + kk;
}

// The update's noise in eps-section layout from the FRESH fold's draws (what fold_heads_from writes
// to its eps_out), threads [0, 260).
__device__ __forceinline__ void noise_to_eps(const float* noise, float* eps) {
    const int k = threadIdx.x;
    if (k >= 260) return;
    const int row = k < 256 ? k >> 6 : k - 256, col = k & 63;
    const bool w = k < 256;
    float ep;
    int eo;
    if (row == 0) {
        ep = w ? noise[64] * noise[col] : noise[64];
        eo = w ? E_VWEP + col : E_VBEP;
    } else {
        const int a = row - 1;
        ep = w ? noise[129 + a] * noise[65 + col] : noise[129 + a];
        eo = w ? E_AWEP + a * 64 + col : E_ABEP + a;
    }
    eps[eo] = ep;
}

// One update of k_learn_multi. A function of its own (not inlined): inside the kernel's loop the
// compiler hoisted every loop-invariant address and kernel-argument load out of it and spilled them
// (~700 B of scratch per lane at the 128-VGPR cap of a 1024-thread workgroup). `sp` is the kernel's
// LDS copy (MultiSmem::sp): a reference to the kernel-argument struct itself made the compiler
// materialise it in scratch and read every field from there (720 -> 204 B of scratch per lane,
// 32.6 -> 34.3 M env-steps/s at U = 64, r5ai).
#ifndef PM_MULTI_INLINE
#define PM_MULTI_INLINE __noinline__
#endif
__device__ PM_MULTI_INLINE void multi_update(const pm_selfplay& sp, MultiSmem& sm, int64_t size, int64_t nb, int64_t c_pos,
                                          uint64_t c_step, bool final) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, B = sp.batch;
    const PerTree tree = per_tree(sp.per_work, sp.cap);
    PM_STAMP(100);
    const int64_t ts = sm.ts, frame = sm.frame + 1;  // frame_idx += 1 before sampling (:136)
    for (int k = t; k < 512; k += kLearn) { sm.hkey[k] = kHashEmpty; sm.hwin[k] = -1; }
    PM_STAMP(119);
    // ---- PER sample (per_sample_block, no pending push): level 2 over the LDS chunk sums
    {
        double run[4] = {0.0, 0.0, 0.0, 0.0}, acc = 0.0, incl = 0.0;
        if (t < 256) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t ch = 4 * t + e;
                acc += ch < nb ? sm.chunk[ch] : 0.0;
                run[e] = acc;
            }
        }
        PM_STAMP(120);
        incl = wave_incl_scan(acc, lane);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0.0;
        if (lane == 63) sm.wsum[wv] = incl;
        PM_STAMP(121);
        __syncthreads();
        PM_STAMP(122);
        if (t < 256) {
            double wb = 0.0;
            for (int w = 0; w < wv; ++w) wb += sm.wsum[w];
            const double ex = wb + excl;
#pragma unroll
            for (int e = 0; e < 4; ++e) sm.incl[4 * t + e] = ex + run[e];
        }
        if (t == 0) sm.total = ((0.0 + sm.wsum[0]) + sm.wsum[1]) + sm.wsum[2] + sm.wsum[3];
        __syncthreads();
    }
    PM_STAMP(101);
    const double total = sm.total;
    {
        const int j = t >> 2, q = t & 3;
        const int n = (int)nb;
        double x = 0.0, before = 0.0;
        int64_t blk = 0;
        {
            const U4 r = philox64((uint32_t)j, TAG_PER, (uint64_t)frame, sp.seed_env);
            const double uu = j < B ? u53(r.x, r.y) : 0.0;
            x = uu * total;
            if (total > 0.0) {
                int lo = 0, hi = n;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sm.incl[mid] > x) hi = mid;
                    else lo = mid + 1;
                }
                if (lo < n) {
                    blk = lo;
                    before = lo ? sm.incl[lo - 1] : 0.0;
                } else {  // the last nonzero chunk: the first to reach the end value
                    int l2 = 0, h2 = n - 1;
                    while (l2 < h2) {
                        const int mid = (l2 + h2) >> 1;
                        if (sm.incl[mid] >= sm.incl[n - 1]) h2 = mid;
                        else l2 = mid + 1;
                    }
                    blk = l2;
                    before = l2 ? sm.incl[l2 - 1] : 0.0;
                }
            }
        }
        PM_STAMP(111);
        double sv[4];
        const int64_t s0 = blk * PER_FAN + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[e] = s0 + e < tree.nsub ? ld_nt(tree.sub + s0 + e) : 0.0;
        double b1, v1;
        const int64_t sb = blk * PER_FAN + per_group_find<4>(sv, x - before, b1, v1);
        PM_STAMP(112);
        float lf[16];
        const int64_t lo = sb * PER_SUB + 16 * q;
        ld_nt16(tree.leaf, lo, sp.cap, lf);
        double b0, pa;
        const int k = group_find16f(lf, lo, size, x - before - b1, b0, pa);
        PM_STAMP(113);
        // ---- the sample's three head evaluations on the same 4 lanes, each lane one sweep of one head
        // set's weights (those LDS reads bound this phase): lanes 0-1 (lane halves h) run Q_B(s) and
        // Q_B(s') on modelB's heads, lanes 2-3 Q_T(s') on targetB's. The row loads are issued as soon as
        // the descent has the index; lanes 0-1 keep the features of s for Hs, lane 1 loads the reward
        // and action|done bits, lane 0 forms the IS weight while the loads are in flight.
        const int64_t id = sb * PER_SUB + k;
        const int h = q & 1, set = q >> 1;
        float xs[32], xn[32];
        float rb[2] = {0.f, 0.f};
        {
            int64_t a = id - c_pos;
            if (a < 0) a += sp.cap;
            if (a < sp.n) {  // this step's push: s' = the observations featB holds
                load_featB_half(sp.featB, (int)a, h, xn);
            } else {
                int64_t nx = id + sp.n;
                if (nx >= sp.cap) nx -= sp.cap;
                load_frow_half(sp.frow, nx, h, xn);
            }
        }
        if (set == 0) {
            load_frow_half(sp.frow, id, h, xs);
            if (h) {
                const float* tr = sp.trans + id * PM_TRANS_F;
                rb[0] = tr[7];
                rb[1] = tr[15];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 32; ++e) xs[e] = xn[e];
        }
#ifdef PM_DIAG
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PM_STAMP(117);
#endif
        const float* hfs = sm.hf[set];
        float s1[4], s2[4], q1[3], q2[3];
        half_chains2(hfs, h, xs, xn, s1, s2);  // set 0: Q_B(s), Q_B(s'); set 1: Q_T(s') (twice)
        half_heads_finish(hfs, s1, q1);
        half_heads_finish(hfs, s2, q2);
        PM_STAMP(118);
        if (j < B) {
            if (set == 0) {
#pragma unroll
                for (int e = 0; e < 32; e += 4)  // units 32 tt + 8 q4 + 4 h + 0..3: one 16-byte store each
                    *reinterpret_cast<float4*>(&sm.Hs[j][32 * (e >> 4) + 8 * ((e >> 2) & 3) + 4 * h]) =
                        make_float4(xs[e], xs[e + 1], xs[e + 2], xs[e + 3]);
                if (h == 0) {
                    sm.qv[j][0] = q1[0]; sm.qv[j][1] = q1[1]; sm.qv[j][2] = q1[2];
                    sm.qv[j][4] = q2[0]; sm.qv[j][5] = q2[1]; sm.qv[j][6] = q2[2];
                    sm.sidx[j] = id;
                    sm.pa[j] = pa;
                    if (final) sp.idx[j] = id;
                } else {
                    sm.qv[j][3] = rb[0];
                    sm.qv[j][7] = rb[1];
                }
            } else if (h == 0) {
                sm.qv[j][8] = q1[0]; sm.qv[j][9] = q1[1]; sm.qv[j][10] = q1[2];
            }
        }
    }
    __syncthreads();
    PM_STAMP(102);
    // this update's noise is left in modelB's epsilon buffers by its phase 0 (reset_noise); the
    // target sync below copies it from there
    const bool act = t < B;
    // the IS weights (size * P(i))^-beta, one fp64 pow per lane on the batch's waves only (every
    // wave running it for its 16 samples cost ~3 us of VALU issue)
    const float wraw = act ? (float)pow((double)size * (sm.pa[t] / total), -beta_of(sp, frame)) : 0.f;
    {
        const float m = wave_max(wraw);
        if (lane == 0) sm.red[wv][0] = m;
    }
    __syncthreads();
    if (act && final) sp.isw[t] = wraw;
    const int64_t id = act ? sm.sidx[t] : 0;
    PM_STAMP(103);
    float wmax = sm.red[0][0];
    for (int w = 1; w < 16; ++w) wmax = fmaxf(wmax, sm.red[w][0]);
    // no barrier: the TD phase below writes sm.red[.][1..6], never the [.][0] just read
    PM_STAMP(104);
    // ---- k_learn phase 2: double-DQN targets, loss, priorities, bias grads
    float lossp = 0.f, prio = 0.f;
    float cf[4] = {0.f, 0.f, 0.f, 0.f};
    int slot = 0;
    if (act) {
        const float rwd = sm.qv[t][3];
        const int bits = __float_as_int(sm.qv[t][7]);
        const int a = bits & 0xff, dn = (bits >> 8) & 1;
        const float qs[3] = {sm.qv[t][0], sm.qv[t][1], sm.qv[t][2]};
        const float qn[3] = {sm.qv[t][4], sm.qv[t][5], sm.qv[t][6]};
        const float qt[3] = {sm.qv[t][8], sm.qv[t][9], sm.qv[t][10]};
        const float q = qs[a];
        const float nq = qt[argmax3(qn)];
        const float tgt = rwd + (float)sp.gamma * nq * (dn ? 0.f : 1.f);
        const float diff = q - tgt;
        const float w = wraw / wmax;
        lossp = w * (diff * diff);
        const float g = 2.f * w * diff / (float)B;
        cf[0] = g;
#pragma unroll
        for (int k = 0; k < 3; ++k) cf[1 + k] = g * ((k == a ? 1.f : 0.f) - 1.f / 3.f);
        *reinterpret_cast<float4*>(sm.coef[t]) = make_float4(cf[0], cf[1], cf[2], cf[3]);
        prio = fabsf(diff) + 1e-6f;
        const uint32_t key = (uint32_t)id;
        slot = (int)((key * 2654435761u) >> 23);
        for (;;) {
            const uint32_t old = atomicCAS(&sm.hkey[slot], kHashEmpty, key);
            if (old == kHashEmpty || old == key) break;
            slot = (slot + 1) & 511;
        }
        atomicMax(&sm.hwin[slot], t);
    } else if (t >= kLearn / 2) {  // the apply's scalar prologue on waves the TD phase leaves idle:
        if (t >= kLearn - 2) adam_const_lane(sp, ts + 1, sm.ap, t - (kLearn - 2));  // Adam's corrections
        gen_both_noises_on(sp, sm.ap, c_step + 1, (uint64_t)(ts + 1) + 1, kLearn / 2);  // both noises
    }
    {
        const float s = wave_sum(lossp), mp = wave_max(prio);
#pragma unroll
        for (int k = 0; k < 4; ++k) cf[k] = wave_sum(cf[k]);
        if (lane == 0) {
            sm.red[wv][1] = s; sm.red[wv][2] = mp;
#pragma unroll
            for (int k = 0; k < 4; ++k) sm.red[wv][3 + k] = cf[k];
        }
    }
    __syncthreads();
    PM_STAMP(105);
    // ---- phase 3: priority scatter; head gradient partials (16 waves x 16 samples)
    if (act && sm.hwin[slot] == t) {
        sp.prios[id] = prio;
        tree.leaf[id] = prio_pow(prio, (float)sp.alpha);
        if (prio != prio) atomicOr(&sp.ctrl->status, PM_CTRL_NAN_PRIO);
    }
    {
        float mpx = sm.red[0][2];
        for (int w = 1; w < 16; ++w) mpx = fmaxf(mpx, sm.red[w][2]);
        float l = 0.f;
        for (int w = 0; w < 16; ++w) l += sm.red[w][1];
        if (t == 0) {
            sm.loss = l / (float)B;
            sm.maxp = fmaxf(sm.maxp, mpx);
        }
        const int col = t & 63;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        const int j0 = wv * 16, j1 = min(j0 + 16, B);
        for (int j = j0; j < j1; ++j) {
            const float4 k4 = *reinterpret_cast<const float4*>(sm.coef[j]);
            const float h = sm.Hs[j][col];
            g[0] = fmaf(k4.x, h, g[0]);
            g[1] = fmaf(k4.y, h, g[1]);
            g[2] = fmaf(k4.z, h, g[2]);
            g[3] = fmaf(k4.w, h, g[3]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sm.gpart[wv][r * 64 + col] = g[r];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the scatter's stores are in L2 before the
    __syncthreads();                                   // refresh's L1-bypassing loads
    PM_STAMP(106);
    // ---- phase 4: gradients + Adam on the thread that forms each; level-1 nodes of the scatter
    if (t < 256) {
        float g = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) g += sm.gpart[w][t];
        const int row = t >> 6, col = t & 63;
        float* gs = sm.ap.g;
        const int a = row - 1;
        const int kmu = row == 0 ? col : 130 + a * 64 + col, ksg = row == 0 ? 65 + col : 325 + a * 64 + col;
        const float gsg = g * sm.eps_tr[row == 0 ? P_VWEP - PM_QNET_EPS_OFF + col
                                                 : P_AWEP - PM_QNET_EPS_OFF + a * 64 + col];
        gs[kmu] = g;
        gs[ksg] = gsg;
        adam_one(sp, sm.ap, kmu, g, final);
        adam_one(sp, sm.ap, ksg, gsg, final);
    } else if (t < 260) {
        const int k = t - 256;
        float g = 0.f;
        for (int w = 0; w < 16; ++w) g += sm.red[w][3 + k];
        float* gs = sm.ap.g;
        const int kmu = k == 0 ? 64 : 322 + k - 1, ksg = k == 0 ? 129 : 517 + k - 1;
        const float gsg = g * sm.eps_tr[k == 0 ? P_VBEP - PM_QNET_EPS_OFF : P_ABEP - PM_QNET_EPS_OFF + k - 1];
        gs[kmu] = g;
        gs[ksg] = gsg;
        adam_one(sp, sm.ap, kmu, g, final);
        adam_one(sp, sm.ap, ksg, gsg, final);
    }
    PM_STAMP(115);
    {
        const int j = min(t >> 2, B - 1);
        const int64_t sb = sm.sidx[j] / PER_SUB;
        const double v = multi_sub_sum4(tree.leaf, sb, sp.cap);
        PM_STAMP(116);
        if ((t & 3) == 0) tree.sub[sb] = v;
    }
    if (t == 0) { sm.ap.g[kGradN] = 0.f; sm.ap.g[kGradN + 1] = 1.f; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // level-1 stores land before level 2 reads them
    __syncthreads();
    PM_STAMP(107);
    if (final)
        for (int k = t; k < kGradN + 2; k += kLearn) sp.grad[k] = sm.ap.g[k];
    // ---- phase 5: level-2 nodes of the scatter (global and the LDS copy)
    if (act && sm.hwin[slot] == t) {
        const int64_t ch = id / PER_CHUNK;
        const double v = multi_chunk_sum(tree, ch);
        tree.chunk[ch] = v;
        sm.chunk[ch] = v;
    }
    // ---- apply_finish (mode 0): target sync, next weights; counters at the end of the launch
    if (t == 0) { sm.ts = ts + 1; sm.frame = frame; }
    if ((ts + 1) % sp.target_update_interval == 0) {  // targetB.load_state_dict(modelB) (:166-168)
        for (int k = t; k < PM_QNET_NHEAD; k += kLearn) sm.ap.tmu[k] = sm.ap.hp[k];
        for (int k = t; k < PM_QNET_NP; k += kLearn) {
            const int h = k - PM_QNET_HEAD_OFF, e = k - PM_QNET_EPS_OFF;
            sp.paramsT[k] = (h >= 0 && h < PM_QNET_NHEAD) ? sm.ap.hp[h]
                            : (e >= 0 ? sm.eps_tr[e] : sp.paramsB[k]);  // eps: this update's noise
        }
        __syncthreads();
    }
    PM_STAMP(108);
    if (final) {
        derive_weights(sp, sm.ap);  // w_B, learn_heads (global), modelB's eps buffers <- the acting noise
        __syncthreads();
    } else {
        derive_weights_lds(sm.ap);
    }
    PM_STAMP(109);
    heads_to_frags(sm.ap.heads[1], sm.hf[0]);
    heads_to_frags(sm.ap.heads[2], sm.hf[1]);
    noise_to_eps(sm.ap.ntrain, sm.eps_tr);
    // no vmcnt(0) here: the next update's global reads (level-1 nodes, leaves) see stores that were
    // drained at phases 3 / 4; its LDS state is complete at this barrier
    __syncthreads();
    PM_STAMP(124);
}

__global__ __launch_bounds__(kLearn, 1) void k_learn_multi(const pm_selfplay sp, int updates) {
    __shared__ __attribute__((aligned(16))) MultiSmem sm;
    const int t = threadIdx.x, B = sp.batch;
    const PerTree tree = per_tree(sp.per_work, sp.cap);
    pm_ctrl* c = sp.ctrl;
    const int64_t c_pos = c->pos, c_size = c->size;
    const uint64_t c_step = c->step;
    const int64_t s_all = c_size + sp.n;
    const int64_t size = s_all < sp.cap ? s_all : sp.cap;  // the replay as this step's push left it
    if (size < B) return;  // block-uniform: no update trains (each would only re-derive the same weights)
    const int64_t nb = (size + PER_CHUNK - 1) / PER_CHUNK;
    // ---- state into LDS
    for (int k = t; k < kMultiChunks; k += kLearn) sm.chunk[k] = k < tree.nchunk ? ld_nt(tree.chunk + k) : 0.0;
    for (int k = t; k < 2 * 264; k += kLearn) sm.hf[k / 264][k % 264] = sp.learn_heads[k];
    for (int k = t; k < 260; k += kLearn) sm.eps_tr[k] = sp.learn_heads[528 + k];
    load_apply_inputs(sp, sm.ap, false);
    if (t == 0) {  // loop-carried counters live in LDS (registers are the scarce resource here)
        sm.ts = c->train_steps;
        sm.frame = c->frame_idx;
        sm.maxp = c->max_prio;
        sm.loss = c->last_loss;
    }
    for (int k = t; k < (int)(sizeof(pm_selfplay) / 4); k += kLearn)
        reinterpret_cast<uint32_t*>(&sm.sp)[k] = reinterpret_cast<const uint32_t*>(&sp)[k];
    __syncthreads();

    for (int u = 1; u < updates; ++u) multi_update(sm.sp, sm, size, nb, c_pos, c_step, u == updates - 1);
    if (t == 0) {
        c->train_steps = sm.ts;
        c->frame_idx = sm.frame;
        c->last_loss = sm.loss;
        c->max_prio = sm.maxp;
    }
}

// prepare: derived weights + a full rebuild of the PER sum tree (with the coming push substituted).
// Call after init and after any host-side change of parameters, priorities or counters.
extern "C" int pm_selfplay_prepare(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    hipStream_t st = pm_stream(stream);
    hipLaunchKernelGGL(k_prepare, dim3(1), dim3(kLearn), 0, st, *sp);
    PM_LAUNCHED("k_prepare");
    return per_launch_build(sp->prios, sp->cap, (float)sp->alpha, sp->ctrl, sp->n, sp->per_work, st);
}

namespace {
__global__ void k_tree_repaired(pm_ctrl* c) {
    if (threadIdx.x == 0 && (c->status & PM_CTRL_TREE_TIMEOUT))
        c->status = (c->status & ~PM_CTRL_TREE_TIMEOUT) | PM_CTRL_TREE_REPAIRED;
}
}  // namespace

// After a tree-refresh timeout (ctrl.status bit 2: the sums disagree with the leaves the learner
// scattered): a full rebuild of the PER sum tree from prios + ctrl (the pending push substituted, as
// pm_selfplay_prepare), then status bit 2 -> bit 3. Nothing else is re-derived.
extern "C" int pm_selfplay_repair_tree(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    hipStream_t st = pm_stream(stream);
    if ((rc = per_launch_build(sp->prios, sp->cap, (float)sp->alpha, sp->ctrl, sp->n, sp->per_work, st))) return rc;
    hipLaunchKernelGGL(k_tree_repaired, dim3(1), dim3(64), 0, st, sp->ctrl);
    PM_LAUNCHED("k_tree_repaired");
    return PM_OK;
}

// The side-A act grid of k_learn's extra blocks (1024 threads: four act blocks' worth each).
// k_learn_multi's preconditions: features of every live replay row stored (frow_ready), the current
// observations' features in featB (the update-0 launch computes them), the fused apply, a sum tree
// whose top level fits LDS.
bool pm::selfplay_multi_ok(const pm_selfplay* sp) {
    return sp->frow && sp->frow_ready && sp->featB && sp->fuse_apply && sp->world == 1 &&
           (sp->cap + PER_CHUNK - 1) / PER_CHUNK <= kMultiChunks && ((uintptr_t)sp->frow & 15) == 0;
}

int pm::selfplay_launch_multi(const pm_selfplay* sp, int updates, hipStream_t st) {
    pm_launch(PM_TIMER_LEARN_MULTI, k_learn_multi, dim3(1), dim3(kLearn), st, *sp, updates);
    PM_LAUNCHED("k_learn_multi");
    return PM_OK;
}

namespace {
// k_learn's side blocks (launches with the next step's side-A act): one CU each (the launch's LDS), so
// they run in ONE round beside the learner only if they fit the CUs the learner and block 1 leave, and
// they end together only if their work is even. They are sized from the opponent draw's expected
// rows: each net's chunk (a multiple of 256 arenas, so the act reads the env kernel's lists) is
// expected to hold kSideRows rows (~15 full 32-row tiles for 16 waves), and the feature tiles are
// spread over the CUs left (>= 16 per block). At configs[2] (pool 8, ratio 0.33): 86 modelA blocks
// (768 arenas, ~515 rows), 48 pool blocks (11 776 arenas, ~486 rows), 114 feature blocks of 18 tiles:
// 250 blocks. (Round 4's grid, 4x the act kernel's chunks and 16 feature tiles, was 64 + 128 + 128
// side blocks in two rounds; measured r5m: modelA blocks of ~705 rows ended 22 us after the learner
// started, the second round's feature blocks 23.8 us, the learner ~19 us.)
struct LearnGrid {
    ActGrid g;
    int ftiles;
};
constexpr int kSideRows = 480;
// Which side blocks start with a ~3.4 us s_sleep, so the learner's load phase is not queued behind
// their staging bursts (PONGMI_SIDE_SLEEP: bit 0 act blocks, bit 1 feature blocks). Default 2 since
// the one-round grid: the feature blocks have the slack (r5o, same box, two interleaved passes:
// 2 -> 1.79 / 1.81 G env-steps/s, 0 -> 1.81 / 1.77, 1 (round 4) -> 1.76 / 1.75, 3 -> 1.75 / 1.75).
// PONGMI_SIDE_NAP: the delay in units of 1 024 clocks (default 8, ~3.4 us), bits 8.. of the argument.
// With actions ahead the feature blocks store nothing while the learner loads and wait for it at their
// end, so they start after a short nap only (kNapAhead; profiles/act_ahead_ab.txt).
constexpr int kNapAhead = 2;
int side_sleep(bool ahead) {
    const char* e = getenv("PONGMI_SIDE_SLEEP");
    const char* n = getenv("PONGMI_SIDE_NAP");
    const int roles = e && *e ? atoi(e) : 2, nap = n && *n ? atoi(n) : (ahead ? kNapAhead : 8);
    return (roles & 3) | (std::max(0, std::min(nap, 64)) << 8);
}
int device_cus() {
    static const int v = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return cus;
    }();
    return v;
}
int side_chunk(double p) {
    if (!(p > 0.0)) return kListMaxLearn;
    const double c = std::ceil(kSideRows / p / 256.0) * 256.0;
    return c >= kListMaxLearn ? kListMaxLearn : (c < 256.0 ? 256 : (int)c);
}
LearnGrid learn_grid(const pm_selfplay* sp) {
    const int ntiles = feat_ntiles(sp->n);
    const double pp = sp->n_pool > 0 ? sp->pool_ratio : 0.0;
    const ActGrid g{sp->n, sp->n_pool + 1, side_chunk(1.0 - pp), side_chunk(sp->n_pool > 0 ? pp / sp->n_pool : 0.0), 0};
    // the feature blocks take the CUs the act blocks leave; when (nearly) none are left (n well above
    // configs[2]'s 65 536: the act blocks alone fill the chip) they share the chip over the whole
    // device instead, so no block runs thousands of tiles in series
    const int left = device_cus() - 2 - g.blocks();
    const int slots = left >= 32 ? left : device_cus();
    int ft = (ntiles + slots - 1) / slots;
    ft = std::max(ft, kFeatTilesLearn);
    return LearnGrid{g, std::min(ft, std::max(ntiles, 1))};
}

// The sum-tree refresh in block 1 (tree_block) unless PONGMI_TR=0 (the learner's own refresh, A/B).
// Read per launch (a getenv per k_learn launch is host work beside the GPU's): the variants are
// bitwise equal (test_learner_variants_are_bitwise_identical switches them between launches).
int tree_refresh_block() {
    const int v = [] {
        const char* e = getenv("PONGMI_TR");
        const char* p = getenv("PONGMI_PUSH2");  // block 1's push rows on two waves per tile (default 1)
        const char* q = getenv("PONGMI_LATE_NOISE");  // the apply's noise / Adam constants in phase 2 (default 1)
        const char* g = getenv("PONGMI_PUSHG");  // push rows as tagged granules (default 1; needs TR and PUSH2)
        const int tr = e && *e ? (atoi(e) != 0) : 1, p2 = p && *p ? (atoi(p) != 0) : 1;
        const int pg = (g && *g ? (atoi(g) != 0) : 1) && tr && p2;
        const char* f = getenv("PONGMI_TR_FORCE_TIMEOUT");  // test hook: block 1's granule poll times out
        return tr | (p2 << 1) | ((q && *q ? (atoi(q) != 0) : 1) << 2) | (pg << 3) | ((f && *f && atoi(f) != 0) << 4);
    }();
    return v;
}

unsigned learn_blocks(const pm_selfplay* sp, bool with_act, const LearnGrid& lg) {
    unsigned blocks = 2u + (with_act ? (unsigned)lg.g.blocks() : 0u);  // learner, push-row block, side blocks
    if (with_act && sp->featB) blocks += (unsigned)((feat_ntiles(sp->n) + lg.ftiles - 1) / lg.ftiles);
    return blocks;
}

// Actions ahead (k_learn's `ahead` argument; pm_selfplay_act_ahead): the fused U = 1 learner launch with
// the side blocks, whose heads are final inside the launch (the sharded step's are only after k_adam, a
// step of U > 1 updates keeps training after it, and k_learn_multi needs the features themselves: frow).
// The feature blocks park their tiles' accumulators in registers, two tiles per wave at most, and wait for
// the learner, so all of them must be resident beside it: one block per CU (the launch's LDS).
// PONGMI_ACT_AHEAD=0: the featB path from the same library (A/B; read per launch, bit-identical).
// PONGMI_AHEAD_FORCE_TIMEOUT=1 (bit 1): test hook, the feature blocks' poll expires at once.
int act_ahead(const pm_selfplay* sp, int mode, bool with_act, const LearnGrid& lg) {
    if (!with_act || !sp->fuse_apply || mode != (PM_UPD_FIRST | PM_UPD_LAST) || !sp->featB || !sp->gB || !sp->gheads ||
        sp->frow || lg.ftiles > 2 * (kLearn / 64) || (int)learn_blocks(sp, with_act, lg) > device_cus())
        return 0;
    const char* e = getenv("PONGMI_ACT_AHEAD");
    if (e && *e && atoi(e) == 0) return 0;
    const char* f = getenv("PONGMI_AHEAD_FORCE_TIMEOUT");
    return 1 | ((f && *f && atoi(f) != 0) << 1);
}

}  // namespace

int pm::selfplay_launch_learn(const pm_selfplay* sp, bool with_act, hipStream_t st, int mode) {
    const LearnGrid lg = learn_grid(sp);
    const ActGrid& g = lg.g;
    const unsigned blocks = learn_blocks(sp, with_act, lg);
    const int tr = tree_refresh_block();
    const int ahead = act_ahead(sp, mode, with_act, lg);
    pm_launch(PM_TIMER_LEARN, (tr & 8) ? k_learn<true> : k_learn<false>, dim3(blocks), dim3(kLearn), st, *sp, g.chunk0,
              g.chunk1, mode, tr, lg.ftiles, side_sleep(ahead & 1), ahead);
    PM_LAUNCHED("k_learn");
    return PM_OK;
}

extern "C" int pm_selfplay_learn(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    return rc ? rc : selfplay_launch_learn(sp, false, pm_stream(stream));
}

extern "C" int pm_selfplay_learn_act(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    return rc ? rc : selfplay_launch_learn(sp, true, pm_stream(stream));
}

extern "C" int pm_selfplay_act_ahead(const pm_selfplay* sp, int32_t mode, int32_t with_act) {
    if (selfplay_check(sp)) return 0;
    return act_ahead(sp, (int)mode, with_act != 0, learn_grid(sp)) & 1;
}

extern "C" int pm_selfplay_apply(const pm_selfplay* sp, void* stream) {
    return pm_selfplay_apply_ex(sp, PM_UPD_FIRST | PM_UPD_LAST, stream);
}

extern "C" int pm_selfplay_apply_ex(const pm_selfplay* sp, int32_t mode, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    PM_REQUIRE(mode >= 0 && mode <= (PM_UPD_FIRST | PM_UPD_LAST), PM_E_ARG, "pm_selfplay_apply_ex: mode=%d", mode);
    if (sp->fuse_apply) return PM_OK;  // learn already applied (unsharded, fused)
    hipLaunchKernelGGL(k_adam, dim3(1), dim3(kLearn), 0, pm_stream(stream), *sp, (int)mode);
    PM_LAUNCHED("k_adam");
    return PM_OK;
}

extern "C" int pm_selfplay_learn_ex(const pm_selfplay* sp, int32_t mode, int32_t with_act, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    PM_REQUIRE(mode >= 0 && mode <= (PM_UPD_FIRST | PM_UPD_LAST), PM_E_ARG, "pm_selfplay_learn_ex: mode=%d", mode);
    return selfplay_launch_learn(sp, with_act != 0, pm_stream(stream), (int)mode);
}

extern "C" int pm_selfplay_commit(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    hipStream_t st = pm_stream(stream);
    const int64_t blocks = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (sp->cap + 4095) / 4096));
    hipLaunchKernelGGL(k_prio_max, dim3((unsigned)blocks), dim3(256), 0, st, *sp);
    PM_LAUNCHED("k_prio_max");
    hipLaunchKernelGGL(k_commit, dim3(1), dim3(kLearn), 0, st, *sp);
    PM_LAUNCHED("k_commit");
    return PM_OK;
}

#ifdef PM_DIAG
// This unit's copies of the stamp buffers (pm_dev.h): what k_learn / k_learn_multi / k_adam wrote.
extern "C" int pm_diag_read_side(uint64_t* out) {  // [4][1024]: k_learn side blocks (begin, after sleep, end, role | rows)
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_side), sizeof(uint64_t) * 4 * 1024);
}
extern "C" int pm_diag_read(uint64_t* out, int32_t n) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_buf), sizeof(uint64_t) * (n < 256 ? n : 256));
    return e == hipSuccess ? 0 : (int)e;
}
extern "C" int pm_diag_read_blk_learn(uint64_t* out) {  // act_block's PM_BLK stamps of k_learn's side-A blocks
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pm_diag_blk), sizeof(uint64_t) * 8 * 4096);
}
extern "C" int pm_diag_clear(void) {
    static const unsigned long long z[256] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(pm_diag_buf), z, sizeof(z));
}
#endif
