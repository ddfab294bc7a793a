// K12 — a population of stand-alone DQN learners (pm_dqn_pop_*, include/pongmi.h): n independent members,
// each a pm_dqn with its own pm_dqn_opt and, optionally, its own pm_dqn_replay, trained by one launch per
// phase with a grid of n workgroups. This unit is host code: the handle, the validation (all of it before
// the first HIP call, so a machine without a GPU reports the same codes) and the list of a member's writable
// buffers; the device table and the aliasing rule are the shared layer's (pm_pop.h). The kernels are
// k_dqp_update (pm_dqn.hip) and k_dqp_sample / k_dqp_scatter (pm_dqn_replay.hip): the solo kernels' bodies on
// tab[blockIdx.x].
//
// Why no ordering between workgroups is needed: a member reads and writes its own buffers only (the
// aliasing rule makes that a checked fact), what two members may share is read-only during every
// launch, and the three phases of a replay update are separate launches on one stream, so member p's
// sampler has finished before member p's update starts, as in the solo path. The only atomic is the
// atomicOr on a member's own status word.
#include "pm_dqn_pop.h"

struct pm_dqn_pop {
    pm_dqn_member* tab;  // device, [n]
    int32_t n;
    int32_t has_replay;
    std::vector<pm_dqn_member> host;  // the bound table, for pm_dqn_nstep_pop_set's aliasing check
    std::vector<uint8_t*> hz;         // the members' horizon buffers (pm_dqn_nstep_pop_set): empty, or n entries
    uint8_t** hz_dev;                 // device copy of hz once one was attached, else null
    int32_t use_n;                    // a member has a horizon buffer: the launches are the _n kernels
};

namespace {

using pm::PopRange;
constexpr auto add = pm::pop_add;

// Every buffer a launch may write for member p, with its size in bytes.
void writable(std::vector<PopRange>& v, int p, const pm_dqn& d, const pm_dqn_opt& o, const pm_dqn_replay* rp,
              const uint8_t* hz) {
    const size_t B = (size_t)d.batch;
    add(v, p, "horizon", hz, B);  // the replay gather writes it
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
                std::vector<pm_dqn_member>& tab, const std::vector<uint8_t*>& hz) {
    PM_REQUIRE(n >= 1 && n <= PM_DQN_POP_MAX, PM_E_SIZE, "%s: n=%d (1..%d)", who, n, PM_DQN_POP_MAX);
    PM_REQUIRE(d, PM_E_ARG, "%s: null descriptor array", who);
    tab.assign((size_t)n, pm_dqn_member{});
    for (int p = 0; p < n; ++p) {
        if (int rc = pm::dqn_check(&d[p], opt ? &opt[p] : nullptr)) return pm::pop_member_fail(rc, who, p);
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
    for (int p = 0; p < n; ++p)
        writable(v, p, tab[p].d, tab[p].o, rp ? &tab[p].rp : nullptr, hz.empty() ? nullptr : hz[(size_t)p]);
    return pm::pop_check_overlap(who, v);
}

}  // namespace

extern "C" int pm_dqn_pop_create(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, int32_t n,
                                 pm_dqn_pop** out) {
    const char* who = "pm_dqn_pop_create";
    PM_REQUIRE(out, PM_E_ARG, "%s: null out", who);
    *out = nullptr;
    std::vector<pm_dqn_member> tab;
    if (int rc = build_table(who, d, opt, rp, n, tab, {})) return rc;
    pm_dqn_member* dev;
    if (int rc = pm::pop_table_create(who, tab.data(), sizeof(pm_dqn_member) * (size_t)n, (void**)&dev)) return rc;
    *out = new pm_dqn_pop{dev, n, rp ? 1 : 0, std::move(tab), {}, nullptr, 0};
    return PM_OK;
}

extern "C" int pm_dqn_pop_rebind(pm_dqn_pop* pop, const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp,
                                 void* stream) {
    const char* who = "pm_dqn_pop_rebind";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    std::vector<pm_dqn_member> tab;
    if (int rc = build_table(who, d, opt, rp, pop->n, tab, pop->hz)) return rc;
    if (int rc = pm::pop_table_rebind(who, pop->tab, tab.data(), sizeof(pm_dqn_member) * (size_t)pop->n, pm_stream(stream)))
        return rc;
    pop->has_replay = rp ? 1 : 0;
    pop->host = std::move(tab);
    return PM_OK;
}

extern "C" int pm_dqn_nstep_pop_set(pm_dqn_pop* pop, const pm_dqn_nstep* ns, void* stream) {
    const char* who = "pm_dqn_nstep_pop_set";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    const size_t n = (size_t)pop->n;
    std::vector<uint8_t*> hz(n, nullptr);
    int32_t use_n = 0;
    for (size_t p = 0; ns && p < n; ++p) {
        hz[p] = ns[p].horizon;
        if (hz[p]) use_n = 1;
    }
    std::vector<PopRange> v;
    v.reserve(n * 19);
    for (size_t p = 0; p < n; ++p)
        writable(v, (int)p, pop->host[p].d, pop->host[p].o, pop->has_replay ? &pop->host[p].rp : nullptr, hz[p]);
    if (int rc = pm::pop_check_overlap(who, v)) return rc;
    if (pop->hz_dev) {  // launches on the stream read the old pointers: they finish first
        if (int rc = pm::pop_table_rebind(who, pop->hz_dev, hz.data(), sizeof(uint8_t*) * n, pm_stream(stream))) return rc;
    } else if (use_n) {
        if (int rc = pm::pop_table_create(who, hz.data(), sizeof(uint8_t*) * n, (void**)&pop->hz_dev)) {
            pop->hz_dev = nullptr;
            return rc;
        }
    }
    pop->hz = use_n ? std::move(hz) : std::vector<uint8_t*>{};
    pop->use_n = use_n;
    return PM_OK;
}

extern "C" int pm_dqn_pop_update(const pm_dqn_pop* pop, void* stream) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_update: null handle");
    return pm::dqp_launch_update(pop->tab, pop->use_n ? pop->hz_dev : nullptr, pop->n, 0, pm_stream(stream));
}

extern "C" int pm_dqn_pop_replay_update(const pm_dqn_pop* pop, int32_t updates, void* stream) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_dqn_pop_replay_update: null handle");
    PM_REQUIRE(pop->has_replay, PM_E_ARG, "pm_dqn_pop_replay_update: the population was created without replay descriptors");
    PM_REQUIRE(updates > 0, PM_E_SIZE, "pm_dqn_pop_replay_update: updates=%d", updates);
    hipStream_t st = pm_stream(stream);
    uint8_t* const* hzt = pop->use_n ? pop->hz_dev : nullptr;
    for (int k = 0; k < updates; ++k) {
        if (int rc = pm::dqp_launch_sample(pop->tab, hzt, pop->n, k, st)) return rc;
        if (int rc = pm::dqp_launch_update(pop->tab, hzt, pop->n, 1, st)) return rc;
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
    int rc = pm::pop_table_free("pm_dqn_pop_destroy", pop->tab);
    if (pop->hz_dev)
        if (const int rc2 = pm::pop_table_free("pm_dqn_pop_destroy", pop->hz_dev)) rc = rc2;
    delete pop;  // even when hipFree failed
    return rc;
}
