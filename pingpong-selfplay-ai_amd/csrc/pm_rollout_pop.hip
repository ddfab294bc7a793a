// K13 — the collecting rollout for a population (pm_rollout_pop_*, include/pongmi.h): n members of m arenas
// each, every member against its own opponent into its own prioritized replay, one launch per phase.
//
// A solo collecting rollout (pm_rollout_push) is three launches and, in Python, a fold and a 4-byte host read of
// max(prios); a population of n members pays that n times per collect step, and a member's few hundred arenas
// are a dozen blocks of a launch shaped for 65 536. Here the members' records sit in a device table (pm_pop.h,
// as pm_dqn_pop's) and four launches serve all of them:
//   k_rpp_prios  grid n: member p's pushed priority, max(prios[0:fill]) or 1.0f into an empty ring, written to
//                prio_dev. A maximum has no order to keep, so it is the value DeviceReplay.push_prio() reads back
//                on the host, taken where the priorities are (members without prio_dev push rp.prio);
//   k_rpp_heads  grid steps x n: k_rollout_heads' body on member p's paramsB, seed_net and heads_ws;
//   k_rpp_push   grid n * ceil(m / 32): block b runs k_rollout_push's body (pm_rollout_push.inc: the same wave
//                roles, MFMA order, draws a step ahead, heads prefetch and store placement) on tile b % tiles of
//                member b / tiles. The member's m arenas are presented to the body as a state of their own (the
//                state pointers moved to the member's slice), so every Philox draw is keyed by the member-local
//                arena index and the ring slot is (pos + st * m + j) mod cap, as in a solo launch over m arenas;
//   k_rpp_nodes  grid node blocks x n: k_per_nodes' computation per member (per_sub_sum4, 16-node chunk sums in
//                the same order); blocks past a member's level-1 nodes and members without per_work exit.
// The table holds each ring's pos and fill as they were when it was bound; a launch gets `advance`, the
// transitions every member has pushed since (all push steps * m per call), and derives pos and fill from it, so
// a loop of collects never rebinds and never synchronises.
//
// Why no ordering between blocks is needed: a block writes its own tile's arenas, observations and ep_reward,
// ring slots pos + st * m + j of its own member (distinct per (st, j): steps * m <= cap), and adds to its own
// member's stats; the aliasing rule below makes "its own member's" a checked fact. What members may share (wA,
// paramsB) is read-only in every launch.
#include <algorithm>
#include <cmath>

#include "pm_mfma.h"
#include "pm_per.h"
#include "pm_pop.h"

using namespace pm;

struct pm_rollout_pop {
    pm_roll_member* tab;  // device, [n]
    pm_env_params p;
    pm_env_state s;  // n * m arenas
    int32_t n, m, steps_max;
    int32_t any_prio;     // a member has prio_dev
    int64_t node_blocks;  // the most 64-node blocks any member's tree has (0: no member has per_work)
    void* rn;             // device RollN [n] once pm_rollout_nstep_pop_set has given a horizon above 1, else null
    int32_t use_n;        // a member's nstep is above 1: the push is k_rpp_push_n
};

namespace {

#include "pm_rollout_push.inc"

// The ring's fill and write slot `advance` transitions after the table was bound.
__device__ __forceinline__ int64_t rpp_fill(const pm_roll_member& mb, int64_t advance) {
    const int64_t f = mb.size + advance;
    return f < mb.rp.cap ? f : mb.rp.cap;
}
__device__ __forceinline__ int64_t rpp_pos(const pm_roll_member& mb, int64_t advance) {
    return (int64_t)((uint64_t)(mb.rp.pos + advance) % (uint64_t)mb.rp.cap);
}

// max(prios[0:fill]) as torch's max gives it (a NaN priority gives NaN), 1.0f into an empty ring. One block per
// member: 16 waves, four independent 16-byte loads per thread and round where prios is 16-byte aligned (a ring of
// 65 536 entries is four rounds; with one load in flight per thread the launch cost more than the rollout it serves).
constexpr int kPriosBlock = 1024;
__global__ __launch_bounds__(kPriosBlock) void k_rpp_prios(const pm_roll_member* tab, int64_t advance) {
    __shared__ float red[kPriosBlock / 64];
    __shared__ int bad[kPriosBlock / 64];
    const pm_roll_member mb = pop_member(tab, blockIdx.x);
    if (!mb.prio_dev) return;  // block-uniform
    const int64_t fill = rpp_fill(mb, advance);
    const float* __restrict__ prios = mb.rp.prios;
    float mx = -INFINITY;
    int nan = 0;
    const int64_t n4 = ((uintptr_t)prios % 16 == 0) ? fill / 4 : 0;
    const float4* p4 = reinterpret_cast<const float4*>(prios);
    for (int64_t e = threadIdx.x; e < n4; e += 4 * kPriosBlock) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = e + k * kPriosBlock;
            v[k] = p4[i < n4 ? i : e];  // past the end: the round's first element again
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mx = fmaxf(fmaxf(mx, v[k].x), fmaxf(v[k].y, fmaxf(v[k].z, v[k].w)));
            nan |= (v[k].x != v[k].x) | (v[k].y != v[k].y) | (v[k].z != v[k].z) | (v[k].w != v[k].w);
        }
    }
    for (int64_t e = n4 * 4 + threadIdx.x; e < fill; e += kPriosBlock) {
        const float v = prios[e];
        mx = fmaxf(mx, v);
        nan |= v != v;
    }
    mx = wave_max(mx);
    nan = wave_sum(nan);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = mx; bad[threadIdx.x >> 6] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = red[0];
        int anynan = bad[0];
        for (int k = 1; k < kPriosBlock / 64; ++k) { v = fmaxf(v, red[k]); anynan |= bad[k]; }
        mb.prio_dev[0] = fill == 0 ? 1.0f : (anynan ? __int_as_float(0x7fc00000) : v);
    }
}

__global__ __launch_bounds__(kHeadsBlock) void k_rpp_heads(const pm_roll_member* tab, uint64_t counter0) {
    const pm_roll_member mb = pop_member(tab, blockIdx.y);
    rollout_heads_body(mb.paramsB, mb.seed_net, counter0, mb.heads_ws, blockIdx.x);
}

// k_rollout_push's body on one member's tile, under the solo kernel's register cap (3 waves per SIMD; the table's
// pointers cost it 12 bytes of scratch, one 8-byte spill, where the solo kernel has none). With the compiler's own
// budget (208 registers, 2 waves per SIMD, no scratch) a collect step of 256 x 2048 arenas took 1335-1384 us
// against 1214-1254, and one of 1 x 256 48-52 us against 52-56 (profiles/rollout_pop_ab.txt): the population
// launch is for many members, so it keeps the cap.
__global__ __launch_bounds__(kRollBlock) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_rpp_push(
    const pm_env_params p, const pm_env_state s, const pm_roll_member* __restrict__ tab, int m, int tiles,
    uint64_t counter0, int steps, int64_t advance, float* __restrict__ obsA, float* __restrict__ obsB) {
    const unsigned mem = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - mem * (unsigned)tiles;
    const pm_roll_member mb = pop_member(tab, mem);
    const size_t off = (size_t)mem * (size_t)m;  // the member's first arena
    const pm_env_state sl{s.x + off,   s.y + off,   s.vx + off,     s.vy + off,     s.spin + off,    s.top + off,
                          s.bot + off, s.scoreA + off, s.scoreB + off, s.bounces + off, nullptr};
    const float prio = mb.prio_dev ? mb.prio_dev[0] : mb.rp.prio;  // k_rpp_prios' value (an earlier launch)
    const RollPush rp{mb.rp.trans,
                      mb.rp.prios,
                      mb.rp.per_work ? per_tree(mb.rp.per_work, mb.rp.cap).leaf : nullptr,
                      mb.rp.ep_reward,
                      rpp_pos(mb, advance),
                      mb.rp.cap,
                      prio,
                      mb.rp.alpha};
    rollout_push_body<false>(p, sl, mb.wA, mb.wB, mb.heads_ws, (double)mb.epsilon, mb.seed_env, counter0, steps,
                             obsA + off * 7, obsB + off * 7, reinterpret_cast<long long*>(mb.stats), m, rp, RollN{},
                             (int)tile);
}

// k_rpp_push with the n-step window (k_rollout_push_n's body), member p's horizon and discount in rnt[p]; a member
// with nstep 1 writes the one-step rows. Like the solo kernel it takes the compiler's own register budget. The
// member-slicing prologue is k_rpp_push's, repeated on purpose: behind one rpp_push_body<kN> both kernels compiled
// to different and longer text (2835 -> 2843 and 3955 -> 4012 instructions).
__global__ __launch_bounds__(kRollBlock) void k_rpp_push_n(
    const pm_env_params p, const pm_env_state s, const pm_roll_member* __restrict__ tab,
    const RollN* __restrict__ rnt, int m, int tiles, uint64_t counter0, int steps, int64_t advance,
    float* __restrict__ obsA, float* __restrict__ obsB) {
    const unsigned mem = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - mem * (unsigned)tiles;
    const pm_roll_member mb = pop_member(tab, mem);
    const RollN rn = rnt[mem];
    const size_t off = (size_t)mem * (size_t)m;  // the member's first arena
    const pm_env_state sl{s.x + off,   s.y + off,   s.vx + off,     s.vy + off,     s.spin + off,    s.top + off,
                          s.bot + off, s.scoreA + off, s.scoreB + off, s.bounces + off, nullptr};
    const float prio = mb.prio_dev ? mb.prio_dev[0] : mb.rp.prio;
    const RollPush rp{mb.rp.trans,
                      mb.rp.prios,
                      mb.rp.per_work ? per_tree(mb.rp.per_work, mb.rp.cap).leaf : nullptr,
                      mb.rp.ep_reward,
                      rpp_pos(mb, advance),
                      mb.rp.cap,
                      prio,
                      mb.rp.alpha};
    rollout_push_body<true>(p, sl, mb.wA, mb.wB, mb.heads_ws, (double)mb.epsilon, mb.seed_env, counter0, steps,
                            obsA + off * 7, obsB + off * 7, reinterpret_cast<long long*>(mb.stats), m, rp, rn,
                            (int)tile);
}

// k_per_nodes (pm_replay.hip) per member, on the member's tree. No pending push range: the leaves are written.
__global__ __launch_bounds__(256) void k_rpp_nodes(const pm_roll_member* tab) {
    __shared__ double subl[64];
    const pm_roll_member mb = pop_member(tab, blockIdx.y);
    if (!mb.rp.per_work) return;  // block-uniform, as the next
    const PerTree tr = per_tree(mb.rp.per_work, mb.rp.cap);
    if ((int64_t)blockIdx.x * 64 >= tr.nsub) return;
    per_nodes_block(tr, PushRange{0, 0, mb.rp.cap, 0.f}, subl);
}

// One member's record: everything pm_rollout_push rejects, for m arenas and launches of up to steps_max steps.
int check_member(const char* who, const pm_roll_member& mb, int32_t m, int32_t steps_max) {
    const pm_roll_replay& rp = mb.rp;
    PM_REQUIRE(mb.wA && mb.wB && mb.paramsB && mb.heads_ws, PM_E_ARG, "%s: null wA, wB, paramsB or heads_ws", who);
    PM_REQUIRE(rp.trans && rp.prios && rp.ep_reward, PM_E_ARG, "%s: null replay buffer", who);
    PM_REQUIRE((((uintptr_t)mb.wA) | ((uintptr_t)mb.wB) | ((uintptr_t)mb.heads_ws)) % 16 == 0, PM_E_ARG,
               "%s: wA, wB and heads_ws must be 16-byte aligned", who);
    PM_REQUIRE(((uintptr_t)rp.trans) % 16 == 0 && ((uintptr_t)rp.per_work) % 16 == 0, PM_E_ARG,
               "%s: trans and per_work must be 16-byte aligned", who);
    PM_REQUIRE(rp.cap > 0 && rp.pos >= 0 && rp.pos < rp.cap, PM_E_SIZE, "%s: pos=%lld cap=%lld", who,
               (long long)rp.pos, (long long)rp.cap);
    PM_REQUIRE(mb.size >= 0 && mb.size <= rp.cap, PM_E_SIZE, "%s: size=%lld cap=%lld", who, (long long)mb.size,
               (long long)rp.cap);
    PM_REQUIRE((int64_t)steps_max * m <= rp.cap, PM_E_SIZE,
               "%s: steps_max * m = %lld exceeds cap %lld (a slot would be written twice in one launch)", who,
               (long long)steps_max * m, (long long)rp.cap);
    PM_REQUIRE(std::isfinite(mb.epsilon), PM_E_ARG, "%s: epsilon is not finite", who);
    return PM_OK;
}

// Every buffer a launch may write for member p, with its size in bytes.
void writable(std::vector<PopRange>& v, int p, const pm_roll_member& mb, int32_t m, int32_t steps_max) {
    const size_t cap = (size_t)mb.rp.cap;
    pop_add(v, p, "trans", mb.rp.trans, sizeof(float) * PM_TRANS_F * cap);
    pop_add(v, p, "prios", mb.rp.prios, sizeof(float) * cap);
    pop_add(v, p, "per_work", mb.rp.per_work, (size_t)per_work_bytes(mb.rp.cap));
    pop_add(v, p, "ep_reward", mb.rp.ep_reward, sizeof(float) * (size_t)m);
    pop_add(v, p, "heads_ws", mb.heads_ws, sizeof(float) * PM_ROLL_HEADS * (size_t)steps_max);
    pop_add(v, p, "stats", mb.stats, sizeof(int64_t) * 6);
    pop_add(v, p, "prio_dev", mb.prio_dev, sizeof(float));
    pop_add(v, p, "wB", mb.wB, sizeof(float) * PM_QNET_NW);
}

// Everything pm_rollout_pop_create and _rebind reject, and what the handle derives from the table. No HIP call.
int check_table(const char* who, const pm_roll_member* mb, int32_t n, int32_t m, int32_t steps_max, int32_t* any_prio,
                int64_t* node_blocks) {
    PM_REQUIRE(mb, PM_E_ARG, "%s: null member array", who);
    *any_prio = 0;
    *node_blocks = 0;
    for (int p = 0; p < n; ++p) {
        if (int rc = check_member(who, mb[p], m, steps_max)) return pop_member_fail(rc, who, p);
        if (mb[p].prio_dev) *any_prio = 1;
        if (mb[p].rp.per_work) *node_blocks = std::max<int64_t>(*node_blocks, (per_tree(nullptr, mb[p].rp.cap).nsub + 63) / 64);
    }
    PM_REQUIRE(*node_blocks <= 0x7fffffff, PM_E_SIZE, "%s: a member's tree has %lld node blocks", who,
               (long long)*node_blocks);
    std::vector<PopRange> v;
    v.reserve((size_t)n * 8);
    for (int p = 0; p < n; ++p) writable(v, p, mb[p], m, steps_max);
    return pop_check_overlap(who, v);
}

}  // namespace

extern "C" size_t pm_roll_member_sizeof(void) { return sizeof(pm_roll_member); }

extern "C" int pm_rollout_pop_create(const pm_env_params* p, const pm_env_state* s, const pm_roll_member* members,
                                     int32_t n, int32_t m, int32_t steps_max, pm_rollout_pop** out) {
    const char* who = "pm_rollout_pop_create";
    PM_REQUIRE(out, PM_E_ARG, "%s: null out", who);
    *out = nullptr;
    PM_REQUIRE(n >= 1 && n <= PM_DQN_POP_MAX, PM_E_SIZE, "%s: n=%d (1..%d)", who, n, PM_DQN_POP_MAX);
    PM_REQUIRE(m >= 1 && (int64_t)n * m <= 0x7fffffff, PM_E_SIZE, "%s: m=%d, n * m = %lld (m >= 1, n * m < 2^31)", who, m,
               (long long)n * m);
    PM_REQUIRE(steps_max >= 1, PM_E_SIZE, "%s: steps_max=%d", who, steps_max);
    PM_REQUIRE(p && s && s->x && s->y && s->vx && s->vy && s->spin && s->top && s->bot && s->scoreA && s->scoreB &&
                   s->bounces,
               PM_E_ARG, "%s: null env parameters or state", who);
    PM_REQUIRE(p->speed_scale_every > 0, PM_E_ARG, "%s: speed_scale_every must be > 0", who);
    int32_t any_prio;
    int64_t node_blocks;
    if (int rc = check_table(who, members, n, m, steps_max, &any_prio, &node_blocks)) return rc;
    pm_roll_member* dev;
    if (int rc = pop_table_create(who, members, sizeof(pm_roll_member) * (size_t)n, (void**)&dev)) return rc;
    *out = new pm_rollout_pop{dev, *p, *s, n, m, steps_max, any_prio, node_blocks, nullptr, 0};
    return PM_OK;
}

extern "C" int pm_rollout_pop_rebind(pm_rollout_pop* pop, const pm_roll_member* members, void* stream) {
    const char* who = "pm_rollout_pop_rebind";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    int32_t any_prio;
    int64_t node_blocks;
    if (int rc = check_table(who, members, pop->n, pop->m, pop->steps_max, &any_prio, &node_blocks)) return rc;
    if (int rc = pop_table_rebind(who, pop->tab, members, sizeof(pm_roll_member) * (size_t)pop->n, pm_stream(stream)))
        return rc;
    pop->any_prio = any_prio;
    pop->node_blocks = node_blocks;
    return PM_OK;
}

extern "C" int pm_rollout_pop_push(const pm_rollout_pop* pop, uint64_t counter0, int32_t steps, int64_t advance,
                                   float* obsA, float* obsB, void* stream) {
    const char* who = "pm_rollout_pop_push";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    PM_REQUIRE(steps >= 0 && steps <= pop->steps_max, PM_E_SIZE, "%s: steps=%d (0..steps_max=%d)", who, steps,
               pop->steps_max);
    PM_REQUIRE(advance >= 0, PM_E_SIZE, "%s: advance=%lld", who, (long long)advance);
    if (steps == 0) return PM_OK;
    PM_REQUIRE(obsA && obsB, PM_E_ARG, "%s: null observation buffer", who);
    hipStream_t st = pm_stream(stream);
    const int n = pop->n, m = pop->m, tiles = (int)pm_blocks(m, 32);
    if (pop->any_prio) {
        hipLaunchKernelGGL(k_rpp_prios, dim3(n), dim3(kPriosBlock), 0, st, (const pm_roll_member*)pop->tab, advance);
        PM_LAUNCHED("k_rpp_prios");
    }
    hipLaunchKernelGGL(k_rpp_heads, dim3(steps, n), dim3(kHeadsBlock), 0, st, (const pm_roll_member*)pop->tab, counter0);
    PM_LAUNCHED("k_rpp_heads");
    if (pop->use_n)
        pm_launch(PM_TIMER_ROLLOUT, k_rpp_push_n, dim3((unsigned)n * (unsigned)tiles), dim3(kRollBlock), st, pop->p,
                  pop->s, (const pm_roll_member*)pop->tab, (const RollN*)pop->rn, m, tiles, counter0, (int)steps,
                  advance, obsA, obsB);
    else
        pm_launch(PM_TIMER_ROLLOUT, k_rpp_push, dim3((unsigned)n * (unsigned)tiles), dim3(kRollBlock), st, pop->p,
                  pop->s, (const pm_roll_member*)pop->tab, m, tiles, counter0, (int)steps, advance, obsA, obsB);
    PM_LAUNCHED(pop->use_n ? "k_rpp_push_n" : "k_rpp_push");
    if (pop->node_blocks) {
        hipLaunchKernelGGL(k_rpp_nodes, dim3((unsigned)pop->node_blocks, n), dim3(256), 0, st,
                           (const pm_roll_member*)pop->tab);
        PM_LAUNCHED("k_rpp_nodes");
    }
    return PM_OK;
}

extern "C" int pm_rollout_nstep_pop_set(pm_rollout_pop* pop, const int32_t* nstep, const double* gamma, void* stream) {
    const char* who = "pm_rollout_nstep_pop_set";
    PM_REQUIRE(pop, PM_E_ARG, "%s: null handle", who);
    PM_REQUIRE(!nstep == !gamma, PM_E_ARG, "%s: nstep and gamma are given together, or both null", who);
    std::vector<RollN> rn((size_t)pop->n, RollN{1, 0.f});
    int32_t use_n = 0;
    for (int p = 0; nstep && p < pop->n; ++p) {
        PM_REQUIRE(nstep[p] >= 1 && nstep[p] <= PM_NSTEP_MAX, PM_E_SIZE, "%s: member %d: nstep=%d (1..%d)", who, p,
                   nstep[p], PM_NSTEP_MAX);
        PM_REQUIRE(std::isfinite(gamma[p]), PM_E_ARG, "%s: member %d: gamma is not finite", who, p);
        rn[(size_t)p] = RollN{nstep[p], (float)gamma[p]};
        if (nstep[p] > 1) use_n = 1;
    }
    const size_t bytes = sizeof(RollN) * (size_t)pop->n;
    if (pop->rn) {  // launches on the stream read the old horizons: they finish first
        if (int rc = pop_table_rebind(who, pop->rn, rn.data(), bytes, pm_stream(stream))) return rc;
    } else if (use_n) {
        if (int rc = pop_table_create(who, rn.data(), bytes, &pop->rn)) {
            pop->rn = nullptr;
            return rc;
        }
    }
    pop->use_n = use_n;
    return PM_OK;
}

extern "C" int pm_rollout_pop_info(const pm_rollout_pop* pop, int32_t* n, int32_t* m, int32_t* steps_max) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_rollout_pop_info: null handle");
    if (n) *n = pop->n;
    if (m) *m = pop->m;
    if (steps_max) *steps_max = pop->steps_max;
    return PM_OK;
}

extern "C" int pm_rollout_pop_destroy(pm_rollout_pop* pop) {
    PM_REQUIRE(pop, PM_E_ARG, "pm_rollout_pop_destroy: null handle");
    int rc = pop_table_free("pm_rollout_pop_destroy", pop->tab);
    if (pop->rn)
        if (const int rc2 = pop_table_free("pm_rollout_pop_destroy", pop->rn)) rc = rc2;
    delete pop;  // even when hipFree failed
    return rc;
}
