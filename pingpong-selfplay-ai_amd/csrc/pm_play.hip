// K8 — the match megakernel: whole greedy episodes in one launch.
//
// The evaluators (scripts/train_iterative.py:171-196 eval_vs_model / eval_vs_pool), the round-robin
// tournament (tests/test_round_robin.py:290-330) and the arena (tests/arena.py:294-320) play
// episodes with frozen nets: reset with a given serve, both players greedy, tick until a score
// reaches max_score. Stepping that as act + env launches per tick moves the fp64 state through HBM
// and pays ~6 launches per tick for a few thousand arenas; here every arena lives in registers for
// its whole episode:
//
//   block = 4 waves = 4 tiles of 32 columns over a range of arenas that share one (net A, net B)
//   pair (the host groups arenas by pair and splits each group into block ranges); both nets'
//   fragment images (2 x 20 KB) are staged into LDS once; then each wave loops: observe -> QNet
//   forward of player A and of player B on the matrix cores (pm_mfma.h tile_hidden / tile_heads,
//   exact f32) -> argmax -> PongEnv2P.step (pm_dev.h tick, fp64). A column whose episode ends
//   takes the next arena of the block's range (lane refill), so the matrix cores keep working on
//   live episodes instead of finished ones; the wave leaves when its range is exhausted and its
//   columns are done, or at max_steps.
//
// Both 32-lane halves of a wave hold the same arena (the MFMA tile layout gives column lane & 31 to
// both halves), so the tick runs duplicated at no cost in a 64-wide wave. Net id -1 is
// HardcodedBallFollower (tests/test_round_robin.py:207-228): move toward the ball x beyond a 0.01
// float32 tolerance. Outputs per arena: final scores, episode length and the sign of rB - rA on the
// last tick (the evaluators' win test, train_iterative.py:180). No barrier after the staging one,
// so each wave leaves on its own; every wave exits by max_steps (arenas still running then, or
// never started, are counted in *status).
#include "pm_host.h"
#include "pm_play.h"

using namespace pm;

namespace {

// 2 x 20 KB weight images + the block's slot table: 68 KB, two blocks per CU
struct PlayShared {
    float lw[2][kLwFloats];
    double sv[kMaxSlots * 3];  // serves of the block's slots (vx, vy, spin)
    int ord[kMaxSlots];        // arena of each slot
    int next;                  // next unclaimed slot
};

// Column c of a wave (both lane halves) plays slots of its block's range one after another: slot
// c first, then the next unclaimed slot (LDS counter) whenever its episode ends. The slot table
// (arena + serve per slot) is staged in LDS with the weights, so a refill is an LDS read.
//
// REC = true is the recording instantiation (pm_play_rec): a column reads its arena's record row when
// it starts a slot and, after each tick, lanes < 32 of a recorded column store the tick (pm_play.h
// PlayRec). REC = false is pm_play's kernel, with no `rec` argument at all.
template <bool REC, typename... Rec>
__global__ __launch_bounds__(kPlayBlock) void k_play(const pm_env_params p, const float* __restrict__ w, int n_nets,
                                                     const int32_t* __restrict__ blk_nets,
                                                     const int32_t* __restrict__ blk_range,
                                                     const int32_t* __restrict__ order,
                                                     const double* __restrict__ serves, int n, int max_steps,
                                                     int32_t* __restrict__ scoreA, int32_t* __restrict__ scoreB,
                                                     int32_t* __restrict__ length, int8_t* __restrict__ last,
                                                     int32_t* __restrict__ status, const Rec... rec) {
    static_assert(sizeof...(Rec) == (REC ? 1 : 0), "one PlayRec when recording, none otherwise");
    __shared__ __attribute__((aligned(16))) PlayShared sm;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31;
    int netA = blk_nets[2 * b], netB = blk_nets[2 * b + 1];
    const int start = blk_range[2 * b], count = blk_range[2 * b + 1];
    const bool bad_net = netA < -1 || netA >= n_nets || netB < -1 || netB >= n_nets;
    const bool bad_range = count < 0 || count > kMaxSlots || start < 0;
    const int live = (bad_net || bad_range) ? 0 : count;  // block-uniform; a bad block plays nothing
    if (live > 0) {
        if (netA >= 0) stage_frags_lds(w + (size_t)netA * PM_QNET_NW, sm.lw[0], b);
        if (netB >= 0) stage_frags_lds(w + (size_t)netB * PM_QNET_NW, sm.lw[1], b + kLwChunks / 2);
        copy_lds_dwords(serves + (size_t)start * 3, sm.sv, live * 6);
        copy_lds_dwords(order + start, sm.ord, live);
    }
    if (threadIdx.x == 0) sm.next = kPlayArenas;
    __syncthreads();  // images and slot table in LDS (waits vmcnt(0)); `next` set

    const int s0 = wv * 32 + col;  // this column's first slot
    int slot = s0 < live ? s0 : -1;
    int arena = -1, bad = 0, len = 0;
    int row = -1;  // REC: the running episode's record row
    Arena a;
    serve(a, 0.0, 0.0, 0.0);
    bool done = true;
    for (int t = 0;; ++t) {
        // (re)fill: a column with no live episode takes its next slot (reset() with the host-drawn
        // serve, envs/my_pong_env_2p.py:83-114); columns that ended claim the next unclaimed one
        if (done && slot >= 0) {  // identical in both halves of a column
            arena = sm.ord[slot];
            serve(a, sm.sv[slot * 3 + 0], sm.sv[slot * 3 + 1], sm.sv[slot * 3 + 2]);
            len = 0;
            done = false;
            if (arena < 0 || arena >= n) { bad += 1; done = true; arena = -1; }
            if constexpr (REC) row = done ? -1 : rec_row_of(rec_arg(rec...), arena, bad);
            slot = -2;  // claim another when this episode ends
        }
        if (__ballot(done && slot == -2) != 0) {  // wave-uniform
            int k = live;
            if (done && slot == -2 && lane < 32) k = atomicAdd(&sm.next, 1);
            k = __shfl(k, col);
            if (done && slot == -2) slot = k < live ? k : -1;
            if (__ballot(done && slot >= 0) != 0) continue;  // start the claimed slots before stepping
        }
        if (__ballot(!done) == 0 || t >= max_steps) break;  // wave-uniform
        float oA[7], oB[7];
        observe(a, oA, oB);
        int aA, aB;
        if constexpr (REC) {
            const PlayRec& r = rec_arg(rec...);
            const bool here = !done && rec_here(r, row, len, lane);  // tick index len: before ++len
            float q[3];
            if (netA >= 0) {
                aA = greedy(sm.lw[0], oA, lane, q);
                if (here) rec_q(r, row, len, 0, q);
            } else {
                aA = follower(oA);
                if (here) rec_q_none(r, row, len, 0);
            }
            if (netB >= 0) {
                aB = greedy(sm.lw[1], oB, lane, q);
                if (here) rec_q(r, row, len, 1, q);
            } else {
                aB = follower(oB);
                if (here) rec_q_none(r, row, len, 1);
            }
        } else {
            aA = netA >= 0 ? greedy(sm.lw[0], oA, lane) : follower(oA);
            aB = netB >= 0 ? greedy(sm.lw[1], oB, lane) : follower(oB);
        }
        if (!done) {
            float rA, rB;
            const int d = tick(p, a, aA, aB, rA, rB);
            if constexpr (REC) {
                if (rec_here(rec_arg(rec...), row, len, lane)) rec_tick(rec_arg(rec...), row, len, a, aA, aB);
            }
            ++len;
            if (d) {
                if (lane < 32) {
                    scoreA[arena] = a.sA;
                    scoreB[arena] = a.sB;
                    length[arena] = len;
                    last[arena] = (int8_t)(rB > rA ? 1 : (rA > rB ? -1 : 0));
                }
                done = true;
            }
        }
    }
    if (lane < 32) {
        // cut by max_steps: the running episode, and this column's claimed slot if any
        const int lost = (!done && arena >= 0 ? 1 : 0) + bad + (slot >= 0 ? 1 : 0);
        if (lost) atomicAdd(status, lost);
        if ((bad_net || bad_range) && lane == 0 && wv == 0) atomicAdd(status, 1);
    }
}

// the checks and the launch behind pm_play (rec == nullptr) and pm_play_rec
int play_launch(const char* who, const pm_env_params* p, const float* w_nets, int32_t n_nets, const int32_t* blk_nets,
                const int32_t* blk_range, int32_t n_blocks, const int32_t* order, const double* serves, int32_t n,
                int32_t max_steps, int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
                const PlayRec* rec, void* stream) {
    PM_REQUIRE(n >= 0 && n_blocks >= 0 && n_nets >= 0 && max_steps >= 0, PM_E_SIZE,
               "%s: n=%d n_blocks=%d n_nets=%d max_steps=%d", who, n, n_blocks, n_nets, max_steps);
    if (rec) {
        PM_REQUIRE(rec->n_rec >= 0 && (rec->n_rec == 0 || rec->cap > 0), PM_E_SIZE, "%s: n_rec=%d rec_cap=%d", who,
                   rec->n_rec, rec->cap);
        PM_REQUIRE(rec->n_rec == 0 || (rec->row && rec->f64 && rec->q && rec->i32), PM_E_ARG,
                   "%s: null record buffer", who);
    }
    if (n_blocks == 0) return PM_OK;
    PM_REQUIRE(p && blk_nets && blk_range && order && serves && scoreA && scoreB && length && last && status,
               PM_E_ARG, "%s: null buffer", who);
    PM_REQUIRE(n_nets == 0 || (w_nets && (((uintptr_t)w_nets) & 15) == 0), PM_E_ARG,
               "%s: w_nets must be non-null and 16-byte aligned", who);
    PM_REQUIRE(p->speed_scale_every > 0, PM_E_ARG, "%s: speed_scale_every must be > 0", who);
    if (rec && rec->n_rec > 0)
        hipLaunchKernelGGL((k_play<true, PlayRec>), dim3(n_blocks), dim3(kPlayBlock), 0, pm_stream(stream), *p, w_nets,
                           n_nets, blk_nets, blk_range, order, serves, n, max_steps, scoreA, scoreB, length, last,
                           status, *rec);
    else
        hipLaunchKernelGGL(k_play<false>, dim3(n_blocks), dim3(kPlayBlock), 0, pm_stream(stream), *p, w_nets, n_nets,
                           blk_nets, blk_range, order, serves, n, max_steps, scoreA, scoreB, length, last, status);
    PM_LAUNCHED("k_play");
    return PM_OK;
}

}  // namespace

extern "C" int pm_play(const pm_env_params* p, const float* w_nets, int32_t n_nets, const int32_t* blk_nets,
                       const int32_t* blk_range, int32_t n_blocks, const int32_t* order, const double* serves,
                       int32_t n, int32_t max_steps, int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last,
                       int32_t* status, void* stream) {
    return play_launch("pm_play", p, w_nets, n_nets, blk_nets, blk_range, n_blocks, order, serves, n, max_steps,
                       scoreA, scoreB, length, last, status, nullptr, stream);
}

extern "C" int pm_play_rec(const pm_env_params* p, const float* w_nets, int32_t n_nets, const int32_t* blk_nets,
                           const int32_t* blk_range, int32_t n_blocks, const int32_t* order, const double* serves,
                           int32_t n, int32_t max_steps, int32_t* scoreA, int32_t* scoreB, int32_t* length,
                           int8_t* last, int32_t* status, const int32_t* rec_row, int32_t n_rec, int32_t rec_cap,
                           double* rec_f64, float* rec_q, int32_t* rec_i32, void* stream) {
    const PlayRec rec{rec_row, n_rec, rec_cap, rec_f64, rec_q, rec_i32};
    return play_launch("pm_play_rec", p, w_nets, n_nets, blk_nets, blk_range, n_blocks, order, serves, n, max_steps,
                       scoreA, scoreB, length, last, status, &rec, stream);
}
