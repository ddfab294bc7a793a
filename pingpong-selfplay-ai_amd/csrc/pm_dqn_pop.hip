// K12 — a population of stand-alone DQN learners (pm_dqn_pop_*, include/pongmi.h): n independent members,
// each a pm_dqn with its own pm_dqn_opt and, optionally, its own pm_dqn_replay, trained by one launch per
// phase with a grid of n workgroups. This unit is host code: the handle, the validation (all of it before
// the first HIP call, so a machine without a GPU reports the same codes), the aliasing rule and the device
// table. The kernels are k_dqp_update (pm_dqn.hip) and k_dqp_sample / k_dqp_scatter (pm_dqn_replay.hip):
// the solo kernels' bodies on tab[blockIdx.x].
//
// Why no ordering between workgroups is needed: a member reads and writes its own buffers only (the
// aliasing rule below makes that a checked fact), what two members may share is read-only during every
// launch, and the three phases of a replay update are separate launches on one stream, so member p's
// sampler has finished before member p's update starts, as in the solo path. The only atomic is the
// atomicOr on a member's own status word.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "pm_dqn_pop.h"

extern "C" int64_t pm_per_work_bytes(int64_t cap);

struct pm_dqn_pop {
    pm_dqn_member* tab;  // device, [n]
    int32_t n;
    int32_t has_replay;
};

namespace pm {

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

namespace {

using pm::PopRange;
constexpr auto add = pm::pop_add;

// Every buffer a launch may write for member p, with its size in bytes.
void writable(std::vector<PopRange>& v, int p, const pm_dqn& d, const pm_dqn_opt& o, const pm_dqn_replay* rp) {
    const size_t B = (size_t)d.batch;
    add(v, p, "params", d.params, sizeof(float) * PM_QNET_NP);
    add(v, p, "target", d.target, sizeof(float) * PM_QNET_NP);
    add(v, p, "adam_m", d.adam_m, sizeof(float) * PM_DQN_NPARAM);
    add(v, p, "adam_v", d.adam_v, sizeof(float) * PM_DQN_NPARAM);
    add(v, p, "grad", d.grad, sizeof(float) * (PM_DQN_NPARAM + 8));
    add(v, p, "stats", d.stats, sizeof(pm_dqn_stats));
    add(v, p, "td", d.td, sizeof(float) * B);
    add(v, p, "q", d.q, sizeof(float) * 3 * B);
    add(v, p, "norm", o.norm, sizeof(float));
    if (!rp) return;
    add(v, p, "s", d.s, sizeof(float) * 7 * B);
    add(v, p, "ns", d.ns, sizeof(float) * 7 * B);
    add(v, p, "act", d.act, sizeof(int32_t) * B);
    add(v, p, "rew", d.rew, sizeof(float) * B);
    add(v, p, "done", d.done, B);
    add(v, p, "isw", d.isw, sizeof(float) * B);
    add(v, p, "idx", rp->idx, sizeof(int64_t) * B);
    add(v, p, "prios", rp->prios, sizeof(float) * (size_t)rp->cap);
    add(v, p, "per_work", rp->per_work, (size_t)pm_per_work_bytes(rp->cap));
}

// Everything pm_dqn_pop_create and _rebind reject, and the table they upload. No HIP call.
int build_table(const char* who, const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, int32_t n,
                std::vector<pm_dqn_member>& tab) {
    PM_REQUIRE(n >= 1 && n <= PM_DQN_POP_MAX, PM_E_SIZE, "%s: n=%d (1..%d)", who, n, PM_DQN_POP_MAX);
    PM_REQUIRE(d, PM_E_ARG, "%s: null descriptor array", who);
    tab.assign((size_t)n, pm_dqn_member{});
    for (int p = 0; p < n; ++p) {
        if (int rc = pm::dqn_check(&d[p])) return pm::pop_member_fail(rc, who, p);
        if (opt)
            if (int rc = pm::dqn_check_opt(&opt[p])) return pm::pop_member_fail(rc, who, p);
        if (rp) {
            if (int rc = pm::dqn_replay_check(&d[p], &rp[p], 1)) return pm::pop_member_fail(rc, who, p);
            PM_REQUIRE(rp[p].cap > 0, PM_E_SIZE, "%s: member %d: cap=%lld", who, p, (long long)rp[p].cap);
        }
        tab[p].d = d[p];
        if (opt) tab[p].o = opt[p];
        if (rp) tab[p].rp = rp[p];
    }
    std::vector<PopRange> v;
    v.reserve((size_t)n * 18);
    for (int p = 0; p < n; ++p) writable(v, p, tab[p].d, tab[p].o, rp ? &tab[p].rp : nullptr);
    return pm::pop_check_overlap(who, v);
}

}  // namespace

extern "C" int pm_dqn_pop_create(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, int32_t n,
                                 pm_dqn_pop** out) {
    const char* who = "pm_dqn_pop_create";
    PM_REQUIRE(out, PM_E_ARG, "%s: null out", who);
    *out = nullptr;
    std::vector<pm_dqn_member> tab;
    if (int rc = build_table(who, d, opt, rp, n, tab)) return rc;
    pm_dqn_member* dev = nullptr;
    hipError_t e = hipMalloc((void**)&dev, sizeof(pm_dqn_member) * (size_t)n);
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "%s: hipMalloc: %s", who, hipGetErrorString(e));
    e = hipMemcpy(dev, tab.data(), sizeof(pm_dqn_member) * (size_t)n, hipMemcpyHostToDevice);  // synchronous
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return pm_fail(PM_E_LAUNCH, "%s: hipMemcpy: %s", who, hipGetErrorString(e));
    }
    *out = new pm_dqn_pop{dev, n, rp ? 1 : 0};
    return PM_OK;
}

extern "C" int pm_dqn_pop_rebind(pm_dqn_pop* pop, const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp,
                                 void* stream) {
    const char* who = "pm_dqn_pop_rebind";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    std::vector<pm_dqn_member> tab;
    if (int rc = build_table(who, d, opt, rp, pop->n, tab)) return rc;
    // launches already on the stream read the old table: they finish before it is overwritten
    hipError_t e = hipStreamSynchronize(pm_stream(stream));
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "%s: hipStreamSynchronize: %s", who, hipGetErrorString(e));
    e = hipMemcpy(pop->tab, tab.data(), sizeof(pm_dqn_member) * (size_t)pop->n, hipMemcpyHostToDevice);
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "%s: hipMemcpy: %s", who, hipGetErrorString(e));
    pop->has_replay = rp ? 1 : 0;
    return PM_OK;
}

extern "C" int pm_dqn_pop_update(const pm_dqn_pop* pop, void* stream) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_update: null handle");
    return pm::dqp_launch_update(pop->tab, pop->n, 0, pm_stream(stream));
}

extern "C" int pm_dqn_pop_replay_update(const pm_dqn_pop* pop, int32_t updates, void* stream) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_replay_update: null handle");
    PM_REQUIRE(pop->has_replay, PM_E_ARG, "pm_dqn_pop_replay_update: the population was created without replay descriptors");
    PM_REQUIRE(updates > 0, PM_E_SIZE, "pm_dqn_pop_replay_update: updates=%d", updates);
    hipStream_t st = pm_stream(stream);
    for (int k = 0; k < updates; ++k) {
        if (int rc = pm::dqp_launch_sample(pop->tab, pop->n, k, st)) return rc;
        if (int rc = pm::dqp_launch_update(pop->tab, pop->n, 1, st)) return rc;
        if (int rc = pm::dqp_launch_scatter(pop->tab, pop->n, st)) return rc;
    }
    return PM_OK;
}

extern "C" int pm_dqn_pop_info(const pm_dqn_pop* pop, int32_t* n, int32_t* has_replay) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_info: null handle");
    if (n) *n = pop->n;
    if (has_replay) *has_replay = pop->has_replay;
    return PM_OK;
}

extern "C" int pm_dqn_pop_destroy(pm_dqn_pop* pop) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_destroy: null handle");
    hipError_t e = hipFree(pop->tab);
    delete pop;
    if (e != hipSuccess) return pm_fail(PM_E_LAUNCH, "pm_dqn_pop_destroy: hipFree: %s", hipGetErrorString(e));
    return PM_OK;
}
