// The population learner's member record (pm_dqn_pop_*, include/pongmi.h) and what its three translation
// units share: pm_dqn_pop.hip owns the handle, the validation and the list of writable buffers; the kernels live
// beside the bodies they call, k_dqp_update in pm_dqn.hip and k_dqp_sample / k_dqp_scatter in pm_dqn_replay.hip.
// The table itself (its row read, its life cycle, the aliasing rule) is pm_pop.h's.
#pragma once
#include "pm_pop.h"

// One row of the device table: workgroup p of every population launch runs pop_member(tab, p). rp is all zeros
// in a population created without a replay.
struct pm_dqn_member {
    pm_dqn d;
    pm_dqn_opt o;
    pm_dqn_replay rp;
};

namespace pm {
// pm_dqn.hip: pm_dqn's argument check, then pm_dqn_opt's (a null record is the defaults and passes).
int dqn_check(const pm_dqn* d, const pm_dqn_opt* o);
// pm_dqn.hip: one learner launch, its kernel chosen there and nowhere else. with_opt false: the plain kernels;
// true: the _opt ones on *o (null = the defaults), or with a horizon buffer hz the _n ones (apply has none).
// gate: DQN_UPDATE_GATED's, the launch does nothing when gate[0] < 0 (the sampler's mark of a void update).
enum DqnStage { DQN_GRADS, DQN_APPLY, DQN_UPDATE, DQN_UPDATE_GATED };
int dqn_launch(DqnStage stage, const pm_dqn* d, bool with_opt, const pm_dqn_opt* o, const uint8_t* hz,
               const int64_t* gate, hipStream_t st);
// pm_dqn_replay.hip: what pm_dqn_replay_update checks behind pm_dqn's and pm_dqn_opt's own checks.
int dqn_replay_check(const pm_dqn* d, const pm_dqn_replay* rp, int32_t updates);
// One launch each, grid n. gated: the idx[0] < 0 gate of k_dqr_update_opt (the replay path).
// hzt: the members' horizon buffers (device [n], entries nullable), or null for the kernels without a horizon.
int dqp_launch_update(const pm_dqn_member* tab, const uint8_t* const* hzt, int n, int gated, hipStream_t st);
int dqp_launch_sample(const pm_dqn_member* tab, uint8_t* const* hzt, int n, int upd, hipStream_t st);
int dqp_launch_scatter(const pm_dqn_member* tab, int n, hipStream_t st);
}  // namespace pm
