// The population learner's member record (pm_dqn_pop_*, include/pongmi.h) and what its three translation
// units share: pm_dqn_pop.hip owns the handle, the validation and the device table; the kernels live beside
// the bodies they call, k_dqp_update in pm_dqn.hip and k_dqp_sample / k_dqp_scatter in pm_dqn_replay.hip.
#pragma once
#include <vector>

#include "pm_host.h"

// One row of the device table: workgroup p of every population launch runs tab[p]. rp is all zeros in a
// population created without a replay.
struct pm_dqn_member {
    pm_dqn d;
    pm_dqn_opt o;
    pm_dqn_replay rp;
};
static_assert(sizeof(pm_dqn_member) % 8 == 0 && alignof(pm_dqn_member) == 8, "copied as 64-bit words");

namespace pm {

#if defined(__HIPCC__)
// This workgroup's record. The table is written by the host only (pm_dqn_pop_create / _rebind) and never
// during a launch, so it is read through the constant address space: block-uniform scalar loads that the
// compiler may repeat at a use instead of holding 76 SGPRs live, exactly as it treats the solo kernels'
// by-value arguments. No lane issues a vector load for it.
__device__ __forceinline__ pm_dqn_member dqp_member(const pm_dqn_member* tab) {
    typedef const uint64_t __attribute__((address_space(4))) cword;
    constexpr int kWords = sizeof(pm_dqn_member) / 8;
    cword* src = (cword*)(tab + blockIdx.x);
    uint64_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = src[i];
    pm_dqn_member m;
    __builtin_memcpy(&m, w, sizeof(m));
    return m;
}
#endif

// The populations' aliasing rule (pm_dqn_pop.hip; shared with pm_rollout_pop.hip): a byte range [lo, hi) that a
// launch may write for `member`, named `kind` in the error.
struct PopRange {
    uintptr_t lo, hi;
    int member;
    const char* kind;
};
void pop_add(std::vector<PopRange>& v, int p, const char* kind, const void* ptr, size_t bytes);  // skips null / empty
// PM_E_ARG naming both members and buffers if a range of one member meets a range of another. Sorts v.
int pop_check_overlap(const char* who, std::vector<PopRange>& v);
// The last error behind "who: member p: ", with code rc.
int pop_member_fail(int rc, const char* who, int p);

// pm_dqn_replay.hip: what pm_dqn_replay_update checks behind pm_dqn's and pm_dqn_opt's own checks.
int dqn_replay_check(const pm_dqn* d, const pm_dqn_replay* rp, int32_t updates);
// One launch each, grid n. gated: the idx[0] < 0 gate of k_dqr_update_opt (the replay path).
int dqp_launch_update(const pm_dqn_member* tab, int n, int gated, hipStream_t st);
int dqp_launch_sample(const pm_dqn_member* tab, int n, int upd, hipStream_t st);
int dqp_launch_scatter(const pm_dqn_member* tab, int n, hipStream_t st);
}  // namespace pm
