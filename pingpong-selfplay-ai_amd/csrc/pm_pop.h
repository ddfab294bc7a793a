// What the population interfaces share (pm_dqn_pop_*, pm_rollout_pop_*; include/pongmi.h): a device table of
// per-member records that workgroup p reads row p of, the host life cycle of that table, and the rule that no
// writable buffer of one member meets one of another's. A population owns its record type, its member check, its
// list of writable buffers and its kernels; the host functions are defined in pm_pop.cpp.
#pragma once
#include <vector>

#include "pm_host.h"

namespace pm {

#if defined(__HIPCC__)
// Row p of a table. The table is written by the host only (pop_table_create / _rebind) and never during a launch,
// so it is read through the constant address space: block-uniform scalar loads that the compiler may repeat at a
// use instead of holding a record's SGPRs live (76 for a pm_dqn_member), exactly as it treats a solo kernel's
// by-value arguments. No lane issues a vector load for it.
template <class T>
__device__ __forceinline__ T pop_member(const T* tab, unsigned p) {
    static_assert(sizeof(T) % 8 == 0 && alignof(T) == 8, "copied as 64-bit words");
    typedef const uint64_t __attribute__((address_space(4))) cword;
    constexpr int kWords = sizeof(T) / 8;
    cword* src = (cword*)(tab + p);
    uint64_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = src[i];
    T m;
    __builtin_memcpy(&m, w, sizeof(m));
    return m;
}
#endif

// The table's life cycle, for a caller that has finished every check of its own (so a machine without a GPU
// reports the same codes). A failed HIP call is PM_E_LAUNCH, "who: <the call>: <HIP's text>".
// A new device copy of host[0, bytes) in *dev; synchronous. On failure nothing stays allocated (*dev is stale).
int pop_table_create(const char* who, const void* host, size_t bytes, void** dev);
// Overwrites dev with host[0, bytes). Launches already on the stream read the old table: they finish first.
int pop_table_rebind(const char* who, void* dev, const void* host, size_t bytes, hipStream_t st);
int pop_table_free(const char* who, void* dev);

// The aliasing rule: a byte range [lo, hi) that a launch may write for `member`, named `kind` in the error.
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

}  // namespace pm
