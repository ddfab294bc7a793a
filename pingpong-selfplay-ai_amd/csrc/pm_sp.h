// Internal header of the self-play learner's units: the constants and device helpers that both the
// rollout unit (pm_sp_rollout.hip: k_act_sp, k_env, k_actenv, k_sp_init, k_resample, k_batch_fwd) and
// the learner unit (pm_sp_learn.hip: k_learn, k_adam, k_prepare, k_prio_max, k_commit, k_learn_multi,
// k_tree_repaired) use, and the host functions that the units and the compositions in pm_selfplay.hip
// call across each other. A helper that only one unit uses lives in that unit. A kernel's code is a
// function of its unit (DESIGN.md "The self-play learner's units"): a change here recompiles both, so
// compare with tools/kernel_text.py before measuring.
#pragma once
#include <algorithm>
#include <cmath>

#include "pm_host.h"
#include "pm_mfma.h"
#include "pm_per.h"

using namespace pm;  // every includer is one of the three pm_s*.hip units

namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kRowBlock, "row staging assumes kRowBlock-thread blocks");
constexpr int kLearn = 1024;              // k_learn / k_adam / k_prepare block
constexpr int kGradN = PM_GRAD_EPISODES;  // grad[kGradN] = finished episodes, grad[kGradN + 1] = updated flag
static_assert(PM_GRAD_EPISODES == PM_QNET_NHEAD && PM_GRAD_UPDATED == kGradN + 1 && PM_GRAD_LEN >= kGradN + 2, "grad layout");
constexpr uint32_t kHashEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ double beta_of(const pm_selfplay& sp, int64_t frame) {  // :137
    const double b = sp.beta_start + (double)frame * (1.0 - sp.beta_start) / (double)sp.beta_frames;
    return b < 1.0 ? b : 1.0;
}

// The push k_env makes this step: [pos, pos + n) mod cap at max(prios) (1.0 into an empty buffer, :57).
__device__ __forceinline__ float push_prio(int64_t size, float max_prio) { return size == 0 ? 1.0f : max_prio; }
__device__ __forceinline__ PushRange push_of(const pm_selfplay& sp, int64_t pos, int64_t size, float max_prio) {
    return PushRange{pos, sp.n, sp.cap, prio_pow(push_prio(size, max_prio), (float)sp.alpha)};
}
}  // namespace

// pm_ctrl.status bits (pongmi.selfplay.SelfPlayLearner.check_status reports them)
constexpr int PM_CTRL_PUSH_TIMEOUT = 1;
constexpr int PM_CTRL_NAN_PRIO = 2;  // a NaN |TD error| was scattered (its PER leaf is 0: never sampled)
constexpr int PM_CTRL_TREE_TIMEOUT = 4;
constexpr int PM_CTRL_TREE_REPAIRED = 8;  // a stale tree was rebuilt by pm_selfplay_repair_tree

// Feature tiles per feature block: 8 (256-thread blocks, two tiles per wave) / 16 (k_learn's 1024).
constexpr int kFeatTilesAct = 8, kFeatTilesLearn = 16;
__host__ __device__ inline int feat_ntiles(int n) { return (n + 31) / 32; }

// The three QNet evaluations of train_step (:152-155) for one 32-row tile of the sampled batch on
// the matrix cores: row r < B is s of sample r, row r >= B is s' of sample r - B (the same replay
// row). This lane's row: trans row `id`, `nxt` selects s'. Returns the pre-ReLU features (MFMA
// accumulator layout) and Q_B / Q_T of the row (heads from learn_heads, staged in hf0 / hf1).
// Every output column depends only on its own row, so which tile or kernel computes a row never
// changes a bit of it. rb: the row's reward and action|done bits (trans slots 7 and 15), loaded with
// the operands (a load placed after the MFMAs costs its consumer one more round trip).
__device__ __forceinline__ void batch_row_fwd(const pm_selfplay& sp, const float* lw, const float* hf0, const float* hf1,
                                              int64_t id, bool nxt, int lane, f32x16 (&c2)[2], float (&qb)[3],
                                              float (&qt)[3], float (&rb)[2]) {
    float xs[4];
    const float* tr = sp.trans + id * PM_TRANS_F;
    tile_inputs(tr + (nxt ? 8 : 0), lane >> 5, xs);
    rb[0] = tr[7];
    rb[1] = tr[15];
    tile_hidden(lw, xs, lane, c2);
    tile_heads(hf0, c2, lane, qb);
    tile_heads(hf1, c2, lane, qt);
}

// Rows of the batch whose replay row is NOT in this step's push range are stable while the env tick
// runs: they are computed beside it (one tile per wave) into hfeat [B][80] (features of s | Q_B(s)
// 0..2, r at 3, Q_B(s') 4..6, action|done bits at 7, Q_T(s') 8..10 at 64..); k_learn computes the
// rest. Carrying r and the bits here spares k_learn a load that depends on idx.
template <bool WT = false>
__device__ __forceinline__ void store_hfeat(float* hfeat, int j, bool nxt, int lane, const f32x16 (&c2)[2],
                                            const float (&qb)[3], const float (&qt)[3], const float (&rb)[2]) {
    float* row = hfeat + (size_t)j * 80;
    const int h = lane >> 5;
    if (!nxt) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) st_out<WT>(&row[32 * t + rho(q) + 4 * h], relu(c2[t][q]));
    }
    if (h == 0) {
        if (!nxt) {
            st_out<WT>(&row[64], qb[0]); st_out<WT>(&row[65], qb[1]); st_out<WT>(&row[66], qb[2]);
            st_out<WT>(&row[67], rb[0]);  // reward
            st_out<WT>(&row[71], rb[1]);  // action | done << 8 (float bits)
        } else {
            st_out<WT>(&row[68], qb[0]); st_out<WT>(&row[69], qb[1]); st_out<WT>(&row[70], qb[2]);
            st_out<WT>(&row[72], qt[0]); st_out<WT>(&row[73], qt[1]); st_out<WT>(&row[74], qt[2]);
        }
    }
}

// Host functions called across the units (as dqn_check in pm_dqn_pop.h).
namespace pm {
int selfplay_check(const pm_selfplay* sp);                        // pm_selfplay.hip: every entry point's argument check
int selfplay_launch_init(const pm_selfplay* sp, hipStream_t st);  // pm_sp_rollout.hip: k_sp_init
// pm_sp_learn.hip: k_learn (with_act: with the next step's side-A act and feature blocks)
int selfplay_launch_learn(const pm_selfplay* sp, bool with_act, hipStream_t st, int mode = PM_UPD_FIRST | PM_UPD_LAST);
// pm_sp_learn.hip: k_learn_multi's preconditions, and its launch (updates 1..U-1 of a vector step)
bool selfplay_multi_ok(const pm_selfplay* sp);
int selfplay_launch_multi(const pm_selfplay* sp, int updates, hipStream_t st);
}  // namespace pm
