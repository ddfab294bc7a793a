// The populations' shared table layer (pm_pop.h), host code only: the device table's life cycle and the
// aliasing rule that pm_dqn_pop.hip and pm_rollout_pop.hip apply to their own lists of writable buffers.
#include <algorithm>
#include <cstdio>

#include "pm_pop.h"

namespace pm {

int pop_table_create(const char* who, const void* host, size_t bytes, void** dev) {
    hipError_t e = hipMalloc(dev, bytes);
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "%s: hipMalloc: %s", who, hipGetErrorString(e));
    e = hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);  // synchronous
    if (e == hipSuccess) return PM_OK;
    (void)hipFree(*dev);
    return pm_fail(PM_E_LAUNCH, "%s: hipMemcpy: %s", who, hipGetErrorString(e));
}

int pop_table_rebind(const char* who, void* dev, const void* host, size_t bytes, hipStream_t st) {
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "%s: hipStreamSynchronize: %s", who, hipGetErrorString(e));
    e = hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? PM_OK : pm_fail(PM_E_LAUNCH, "%s: hipMemcpy: %s", who, hipGetErrorString(e));
}

int pop_table_free(const char* who, void* dev) {
    const hipError_t e = hipFree(dev);
    return e == hipSuccess ? PM_OK : pm_fail(PM_E_LAUNCH, "%s: hipFree: %s", who, hipGetErrorString(e));
}

// A failed per-member check: its message behind the member's index.
int pop_member_fail(int rc, const char* who, int p) {
    char msg[400];
    snprintf(msg, sizeof(msg), "%s", pm_last_error());
    return pm_fail(rc, "%s: member %d: %s", who, p, msg);
}

void pop_add(std::vector<PopRange>& v, int p, const char* kind, const void* ptr, size_t bytes) {
    if (ptr && bytes) v.push_back(PopRange{(uintptr_t)ptr, (uintptr_t)ptr + bytes, p, kind});
}

// No writable byte range of one member may meet one of another's. Sorted by start, a range conflicts exactly
// when it starts below the furthest end seen so far among the OTHER members' ranges: the furthest end overall
// (top) and the furthest among members other than top's (other) are enough to know that.
int pop_check_overlap(const char* who, std::vector<PopRange>& v) {
    std::sort(v.begin(), v.end(), [](const PopRange& a, const PopRange& b) { return a.lo < b.lo; });
    const PopRange* top = nullptr;
    const PopRange* other = nullptr;
    for (const PopRange& r : v) {
        const PopRange* hit = nullptr;
        if (top && top->member != r.member && r.lo < top->hi) hit = top;
        else if (top && top->member == r.member && other && r.lo < other->hi) hit = other;
        if (hit) {
            const PopRange& a = hit->member < r.member ? *hit : r;
            const PopRange& b = hit->member < r.member ? r : *hit;
            return pm_fail(PM_E_ARG, "%s: member %d: its %s overlaps member %d's %s (writable buffers must be disjoint)", who,
                           b.member, b.kind, a.member, a.kind);
        }
        if (!top || r.hi > top->hi) {
            if (top && top->member != r.member && (!other || top->hi > other->hi)) other = top;
            top = &r;
        } else if (r.member != top->member && (!other || r.hi > other->hi)) {
            other = &r;
        }
    }
    return PM_OK;
}

}  // namespace pm
