// The batched self-play learner: one vector step of scripts/train_iterative.py:239-245 for n arenas,
// nothing returns to the host. This file holds the argument check and the steps composed of the two
// units' launches; the kernels live in pm_sp_rollout.hip and pm_sp_learn.hip (pm_sp.h: what they share).
//
//   pm_selfplay_step_overlap   the fused step (the default):
//       k_actenv   sampler blocks draw the update's PER sample off the sum tree (which already accounts
//                  for the push about to be made) and compute its stable rows' forward; every other block
//                  acts for modelB, ticks its 256 arenas, pushes to the replay, keeps the episode books
//       k_learn    block 0 trains on the batch [+ Adam / target sync / epsilon decay / counters / next
//                  weights when unsharded], block 1 computes the push rows and refreshes the sum tree,
//                  the side blocks act for the opponents and modelB's features (or actions) of the
//                  NEXT step
//       (sharded: RCCL all-reduce of sp.grad, then k_adam)
//   pm_selfplay_step           the plain step: k_act_sp (both players' act + the PER sample), k_env
//                              (env tick + push + the batch's stable rows), k_learn without side blocks
//                              [, k_adam]
//   pm_selfplay_step_multi     U > 1 updates: k_actenv, k_learn (first update) [, k_adam], then
//                              k_learn_multi (updates 1..U-1 in one launch) or, without its
//                              preconditions, k_resample + k_batch_fwd + k_learn [+ k_adam] per update;
//                              k_prio_max + k_commit end the step
//
// Every loop counter lives in the device control block (pm_ctrl), so a whole vector step can be
// replayed from a captured graph.
#include "pm_sp.h"

int pm::selfplay_check(const pm_selfplay* sp) {
    PM_REQUIRE(sp && sp->ctrl && sp->trans && sp->prios && sp->per_work && sp->idx && sp->isw && sp->grad &&
                   sp->partials && sp->hfeat && sp->w_opp && sp->paramsB && sp->paramsT && sp->w_B && sp->adam_m &&
                   sp->adam_v && sp->opp && sp->ep_reward,
               PM_E_ARG, "pm_selfplay: null buffer");
    PM_REQUIRE(sp->n > 0 && sp->batch >= 1 && sp->batch <= PM_MAX_BATCH && sp->n > sp->batch && sp->cap >= sp->n &&
                   sp->cap < 0xFFFFFFFFll,
               PM_E_SIZE, "pm_selfplay: n=%d batch=%d cap=%lld", sp->n, sp->batch, (long long)sp->cap);
    PM_REQUIRE(sp->n_pool >= 0 && sp->n_pool <= 4096 && sp->world >= 1, PM_E_SIZE, "pm_selfplay: n_pool/world");
    PM_REQUIRE(sp->obsA && sp->obsB && sp->aA && sp->aB && sp->learn_heads && sp->opp_list && sp->opp_cnt, PM_E_ARG,
               "pm_selfplay: null buffer");
    PM_REQUIRE(!sp->fuse_apply || sp->world == 1, PM_E_ARG, "pm_selfplay: fuse_apply needs world == 1");
    PM_REQUIRE(sp->chunk_A > 0 && sp->chunk_A <= kListMax && sp->chunk_P > 0 && sp->chunk_P <= kListMax, PM_E_SIZE,
               "pm_selfplay: chunk_A/chunk_P must be in [1, %d]", kListMax);
    PM_REQUIRE(((((uintptr_t)sp->w_opp) | ((uintptr_t)sp->w_B) | ((uintptr_t)sp->prios) | ((uintptr_t)sp->per_work) |
                 ((uintptr_t)sp->paramsB) | ((uintptr_t)sp->paramsT) | ((uintptr_t)sp->adam_m) | ((uintptr_t)sp->adam_v) |
                 ((uintptr_t)sp->learn_heads)) &
                15) == 0,
               PM_E_ARG, "pm_selfplay: w_opp / w_B / prios / per_work / paramsB / paramsT / adam_m / adam_v / "
                         "learn_heads must be 16-byte aligned");
    PM_REQUIRE(sp->env.speed_scale_every > 0 && sp->target_update_interval > 0 && sp->beta_frames > 0, PM_E_ARG,
               "pm_selfplay: zero interval");
    return PM_OK;
}

extern "C" int pm_selfplay_init(const pm_selfplay* sp, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    if ((rc = selfplay_launch_init(sp, pm_stream(stream)))) return rc;
    return pm_selfplay_prepare(sp, stream);
}

extern "C" int pm_selfplay_step_multi(const pm_selfplay* sp, int32_t updates, void* stream) {
    int rc = selfplay_check(sp);
    if (rc) return rc;
    PM_REQUIRE(updates >= 1, PM_E_ARG, "pm_selfplay_step_multi: updates=%d", updates);
    PM_REQUIRE(sp->world == 1, PM_E_ARG, "pm_selfplay_step_multi: unsharded only (world=%d)", sp->world);
    if (updates == 1) return pm_selfplay_step_overlap(sp, stream);
    hipStream_t st = pm_stream(stream);
    if ((rc = pm_selfplay_actenv(sp, stream))) return rc;
    if ((rc = selfplay_launch_learn(sp, true, st, PM_UPD_FIRST))) return rc;
    if ((rc = pm_selfplay_apply_ex(sp, PM_UPD_FIRST, stream))) return rc;
    if (selfplay_multi_ok(sp)) {  // updates 1..U-1 in one single-workgroup launch
        if ((rc = selfplay_launch_multi(sp, (int)updates, st))) return rc;
        return pm_selfplay_commit(sp, stream);
    }
    for (int u = 1; u < updates; ++u) {
        if ((rc = pm_selfplay_resample(sp, stream))) return rc;
        if ((rc = selfplay_launch_learn(sp, false, st, 0))) return rc;
        if ((rc = pm_selfplay_apply_ex(sp, 0, stream))) return rc;
    }
    return pm_selfplay_commit(sp, stream);
}

extern "C" int pm_selfplay_step(const pm_selfplay* sp, void* stream) {
    int rc = pm_selfplay_rollout(sp, stream);
    if (!rc) rc = pm_selfplay_learn(sp, stream);
    return rc ? rc : pm_selfplay_apply(sp, stream);
}

extern "C" int pm_selfplay_step_overlap(const pm_selfplay* sp, void* stream) {
    int rc = pm_selfplay_actenv(sp, stream);
    if (!rc) rc = pm_selfplay_learn_act(sp, stream);
    return rc ? rc : pm_selfplay_apply(sp, stream);
}
