// K8 for QNetRNN players: whole greedy episodes in one launch when at least one side is a QNetRNN
// (tests/test_round_robin.py:290-330, tests/arena.py:294-320, scripts/train_rnn_iterative.py's
// evaluators). The block layout is k_play's (pm_play.hip): 4 waves = 4 tiles of 32 columns over a
// range of slots that share one (player A, player B) pair, arenas in registers, slot table in LDS,
// a column whose episode ends taking the next unclaimed slot. Each side is block-uniform:
//
//   id >= 0   QNet `id`: 20 KB fragment image in LDS, greedy() per wave;
//   id == -1  HardcodedBallFollower;
//   id <= -2  QNetRNN `-2 - id`: one rnn_core step per tick over the block's 128 columns (wave w
//             column c = row 32 w + c), small tables in LDS (one set per side), the big weights
//             streamed through the 32 KB ring as in K5.
//
// (h, c) per column and side live in a caller-provided scratch [block][side][column][h 128 | c 128]
// (256 KB per block), read and written in place in rnn_core's float4 unit order. The host never
// zeroes it: the first tick of every episode runs with zero = true (init_hidden per episode).
//
// rnn_core has a barrier per ring stage, so every wave runs it the same number of times: the tick
// loop is block-uniform (__syncthreads_or of "any column live or still claiming"); a column with no
// live episode runs the step with valid = false (no stores, action ignored). The refill at the top
// of a tick is barrier-free. The block leaves when its range is exhausted and all columns are done,
// or at max_steps (episodes cut then, and slots never started, are counted in *status).
#include "pm_host.h"
#include "pm_play.h"
#include "pm_rnn.h"

using namespace pm;

namespace {

constexpr int kHcFloats = 256;  // per column and side: h 128 | c 128

// ring 32 KB + 2 table sets 10.1 KB + one QNet image 20 KB + slot table 28 KB: ~90 KB, one block per CU
struct PlayRnnShared {
    float ring[2 * kStageFloats];
    float hw[2][kHwFloats];
    float lw[kLwFloats];       // the QNet side's image (at most one side is a QNet)
    double sv[kMaxSlots * 3];  // serves of the block's slots (vx, vy, spin)
    int ord[kMaxSlots];        // arena of each slot
    int next;                  // next unclaimed slot
};
static_assert(kHwFloats % 4 == 0, "table sets stay 16-byte aligned");

enum : int { KIND_QNET = 0, KIND_FOLLOWER = 1, KIND_RNN = 2 };
__device__ __forceinline__ int kind_of(int id) { return id >= 0 ? KIND_QNET : (id == -1 ? KIND_FOLLOWER : KIND_RNN); }

// One side's greedy action for this lane's column. Block-wide when the side is a QNetRNN.
__device__ __forceinline__ int side_action(int kind, const float* __restrict__ w_rnn, PlayRnnShared& sm, int side,
                                           const float (&o)[7], bool zero, bool valid, float* hc, int lane) {
    if (kind == KIND_RNN) {  // block-uniform
        float xs[4];
        inputs_of(o, lane >> 5, xs);
        int a = 1;
        rnn_core(w_rnn, sm.ring, sm.hw[side], xs, zero, valid, hc, hc + 128, hc, hc + 128, 0,
                 [&](const float (&q)[3]) { a = argmax3(q); });
        return a;
    }
    return kind == KIND_QNET ? greedy(sm.lw, o, lane) : follower(o);
}

// side_action for the recording kernel: a lane with `here` set also stores the q values the argmax
// consumed as tick t of its record row, at once (they are not kept across the other side's step: the
// kernel has no register to spare).
__device__ __forceinline__ int side_action_rec(int kind, const float* __restrict__ w_rnn, PlayRnnShared& sm, int side,
                                               const float (&o)[7], bool zero, bool valid, float* hc, int lane,
                                               const PlayRec& rec, bool here, int row, int t) {
    if (kind == KIND_RNN) {  // block-uniform
        float xs[4];
        inputs_of(o, lane >> 5, xs);
        int a = 1;
        rnn_core(w_rnn, sm.ring, sm.hw[side], xs, zero, valid, hc, hc + 128, hc, hc + 128, 0,
                 [&](const float (&q)[3]) {
                     a = argmax3(q);
                     if (here) rec_q(rec, row, t, side, q);
                 });
        return a;
    }
    if (kind == KIND_QNET) {
        float q[3];
        const int a = greedy(sm.lw, o, lane, q);
        if (here) rec_q(rec, row, t, side, q);
        return a;
    }
    if (here) rec_q_none(rec, row, t, side);
    return follower(o);
}

// REC = true is the recording instantiation (pm_play_rnn_rec), as k_play's: the record row is read
// when a column starts a slot, and lanes < 32 of a recorded column store each tick (pm_play.h
// PlayRec). No barrier is added and the loop stays block-uniform. REC = false is pm_play_rnn's
// kernel, with no `rec` argument at all.
template <bool REC, typename... Rec>
__global__ __launch_bounds__(kPlayBlock, 1) void k_play_rnn(
    const pm_env_params p, const float* __restrict__ w_qnet, int n_qnet, const float* __restrict__ w_rnn, int n_rnn,
    const int32_t* __restrict__ blk_nets, const int32_t* __restrict__ blk_range, const int32_t* __restrict__ order,
    const double* __restrict__ serves, int n, int max_steps, float* hc_scratch, int32_t* __restrict__ scoreA,
    int32_t* __restrict__ scoreB, int32_t* __restrict__ length, int8_t* __restrict__ last, int32_t* __restrict__ status,
    const Rec... rec) {
    static_assert(sizeof...(Rec) == (REC ? 1 : 0), "one PlayRec when recording, none otherwise");
    __shared__ __attribute__((aligned(16))) PlayRnnShared sm;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 31;
    const int idA = blk_nets[2 * b], idB = blk_nets[2 * b + 1];
    const int start = blk_range[2 * b], count = blk_range[2 * b + 1];
    const int kA = kind_of(idA), kB = kind_of(idB);
    const int rA_ = -2 - idA, rB_ = -2 - idB;  // RNN net of each side (when its kind is KIND_RNN)
    const bool bad_net = (kA == KIND_QNET && idA >= n_qnet) || (kB == KIND_QNET && idB >= n_qnet) ||
                         (kA == KIND_RNN && (rA_ < 0 || rA_ >= n_rnn)) || (kB == KIND_RNN && (rB_ < 0 || rB_ >= n_rnn)) ||
                         (kA != KIND_RNN && kB != KIND_RNN);  // pairs without a QNetRNN belong to pm_play
    const bool bad_range = count < 0 || count > kMaxSlots || start < 0;
    const int live = (bad_net || bad_range) ? 0 : count;  // block-uniform; a bad block plays nothing
    const float* wA = w_rnn;
    const float* wB = w_rnn;
    if (live > 0) {
        if (kA == KIND_RNN) { wA = w_rnn + (size_t)rA_ * PM_RNN_NW; stage_tables(wA, sm.hw[0]); }
        if (kB == KIND_RNN) { wB = w_rnn + (size_t)rB_ * PM_RNN_NW; stage_tables(wB, sm.hw[1]); }
        if (kA == KIND_QNET) stage_frags_lds(w_qnet + (size_t)idA * PM_QNET_NW, sm.lw, b);
        if (kB == KIND_QNET) stage_frags_lds(w_qnet + (size_t)idB * PM_QNET_NW, sm.lw, b);
        copy_lds_dwords(serves + (size_t)start * 3, sm.sv, live * 6);
        copy_lds_dwords(order + start, sm.ord, live);
    }
    if (threadIdx.x == 0) sm.next = kPlayArenas;
    __syncthreads();  // tables, image and slot table in LDS (waits vmcnt(0)); `next` set

    // this column's (h, c) rows, one per side
    float* hcA = hc_scratch + (((size_t)b * 2 + 0) * kPlayArenas + wv * 32 + col) * kHcFloats;
    float* hcB = hc_scratch + (((size_t)b * 2 + 1) * kPlayArenas + wv * 32 + col) * kHcFloats;

    const int s0 = wv * 32 + col;  // this column's first slot
    int slot = s0 < live ? s0 : -1;
    int arena = -1, bad = 0, len = 0;
    int row = -1;  // REC: the running episode's record row
    Arena a;
    serve(a, 0.0, 0.0, 0.0);
    bool done = true, fresh = false;
    for (int t = 0;; ++t) {
        // refill (no barrier): a column whose episode ended claims the next unclaimed slot, and a
        // column holding a slot starts it (reset() with the host-drawn serve,
        // envs/my_pong_env_2p.py:83-114) with a zero hidden state. Identical in both lane halves.
        if (__ballot(done && slot == -2) != 0) {  // wave-uniform
            int k = live;
            if (done && slot == -2 && lane < 32) k = atomicAdd(&sm.next, 1);
            k = __shfl(k, col);
            if (done && slot == -2) slot = k < live ? k : -1;
        }
        if (done && slot >= 0) {
            arena = sm.ord[slot];
            serve(a, sm.sv[slot * 3 + 0], sm.sv[slot * 3 + 1], sm.sv[slot * 3 + 2]);
            len = 0;
            done = false;
            fresh = true;
            if (arena < 0 || arena >= n) { bad += 1; done = true; arena = -1; }
            if constexpr (REC) row = done ? -1 : rec_row_of(rec_arg(rec...), arena, bad);
            slot = -2;  // claim another when this episode ends
        }
        // block-uniform exit: nothing live and nobody left to claim a slot, or the tick budget
        if (!__syncthreads_or(!done || slot == -2) || t >= max_steps) break;
        float oA[7], oB[7];
        observe(a, oA, oB);
        int aA, aB;
        if constexpr (REC) {
            const PlayRec& r = rec_arg(rec...);
            const bool here = !done && rec_here(r, row, len, lane);  // tick index len: before ++len
            aA = side_action_rec(kA, wA, sm, 0, oA, fresh, !done, hcA, lane, r, here, row, len);
            aB = side_action_rec(kB, wB, sm, 1, oB, fresh, !done, hcB, lane, r, here, row, len);
        } else {
            aA = side_action(kA, wA, sm, 0, oA, fresh, !done, hcA, lane);
            aB = side_action(kB, wB, sm, 1, oB, fresh, !done, hcB, lane);
        }
        fresh = false;
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
        const int lost = (!done && arena >= 0 ? 1 : 0) + bad;  // cut by max_steps, or an invalid arena id
        if (lost) atomicAdd(status, lost);
    }
    if (threadIdx.x == 0) {
        const int unclaimed = live - min(sm.next, live);  // slots never started (max_steps)
        if (unclaimed > 0) atomicAdd(status, unclaimed);
        if (bad_net || bad_range) atomicAdd(status, 1);
    }
}

}  // namespace

extern "C" size_t pm_play_rnn_scratch_bytes(int32_t n_blocks) {
    return n_blocks > 0 ? (size_t)n_blocks * 2 * kPlayArenas * kHcFloats * sizeof(float) : 0;
}

namespace {

// the checks and the launch behind pm_play_rnn (rec == nullptr) and pm_play_rnn_rec
int play_rnn_launch(const char* who, const pm_env_params* p, const float* w_qnet, int32_t n_qnet, const float* w_rnn,
                    int32_t n_rnn, const int32_t* blk_nets, const int32_t* blk_range, int32_t n_blocks,
                    const int32_t* order, const double* serves, int32_t n, int32_t max_steps, float* hc_scratch,
                    int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
                    const PlayRec* rec, void* stream) {
    PM_REQUIRE(n >= 0 && n_blocks >= 0 && n_qnet >= 0 && n_rnn >= 0 && max_steps >= 0, PM_E_SIZE,
               "%s: n=%d n_blocks=%d n_qnet=%d n_rnn=%d max_steps=%d", who, n, n_blocks, n_qnet, n_rnn, max_steps);
    if (rec) {
        PM_REQUIRE(rec->n_rec >= 0 && (rec->n_rec == 0 || rec->cap > 0), PM_E_SIZE, "%s: n_rec=%d rec_cap=%d", who,
                   rec->n_rec, rec->cap);
        PM_REQUIRE(rec->n_rec == 0 || (rec->row && rec->f64 && rec->q && rec->i32), PM_E_ARG,
                   "%s: null record buffer", who);
    }
    if (n_blocks == 0) return PM_OK;
    PM_REQUIRE(p && blk_nets && blk_range && order && serves && hc_scratch && scoreA && scoreB && length && last && status,
               PM_E_ARG, "%s: null buffer", who);
    PM_REQUIRE(n_qnet == 0 || (w_qnet && (((uintptr_t)w_qnet) & 15) == 0), PM_E_ARG,
               "%s: w_qnet must be non-null and 16-byte aligned", who);
    PM_REQUIRE(n_rnn == 0 || (w_rnn && (((uintptr_t)w_rnn) & 15) == 0), PM_E_ARG,
               "%s: w_rnn must be non-null and 16-byte aligned", who);
    PM_REQUIRE((((uintptr_t)hc_scratch) & 15) == 0, PM_E_ARG, "%s: hc_scratch must be 16-byte aligned", who);
    PM_REQUIRE(p->speed_scale_every > 0, PM_E_ARG, "%s: speed_scale_every must be > 0", who);
    if (rec && rec->n_rec > 0)
        hipLaunchKernelGGL((k_play_rnn<true, PlayRec>), dim3(n_blocks), dim3(kPlayBlock), 0, pm_stream(stream), *p,
                           w_qnet, n_qnet, w_rnn, n_rnn, blk_nets, blk_range, order, serves, n, max_steps, hc_scratch,
                           scoreA, scoreB, length, last, status, *rec);
    else
        hipLaunchKernelGGL(k_play_rnn<false>, dim3(n_blocks), dim3(kPlayBlock), 0, pm_stream(stream), *p, w_qnet,
                           n_qnet, w_rnn, n_rnn, blk_nets, blk_range, order, serves, n, max_steps, hc_scratch, scoreA,
                           scoreB, length, last, status);
    PM_LAUNCHED("k_play_rnn");
    return PM_OK;
}

}  // namespace

extern "C" int pm_play_rnn(const pm_env_params* p, const float* w_qnet, int32_t n_qnet, const float* w_rnn,
                           int32_t n_rnn, const int32_t* blk_nets, const int32_t* blk_range, int32_t n_blocks,
                           const int32_t* order, const double* serves, int32_t n, int32_t max_steps, float* hc_scratch,
                           int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
                           void* stream) {
    return play_rnn_launch("pm_play_rnn", p, w_qnet, n_qnet, w_rnn, n_rnn, blk_nets, blk_range, n_blocks, order, serves,
                           n, max_steps, hc_scratch, scoreA, scoreB, length, last, status, nullptr, stream);
}

extern "C" int pm_play_rnn_rec(const pm_env_params* p, const float* w_qnet, int32_t n_qnet, const float* w_rnn,
                               int32_t n_rnn, const int32_t* blk_nets, const int32_t* blk_range, int32_t n_blocks,
                               const int32_t* order, const double* serves, int32_t n, int32_t max_steps,
                               float* hc_scratch, int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last,
                               int32_t* status, const int32_t* rec_row, int32_t n_rec, int32_t rec_cap, double* rec_f64,
                               float* rec_q, int32_t* rec_i32, void* stream) {
    const PlayRec rec{rec_row, n_rec, rec_cap, rec_f64, rec_q, rec_i32};
    return play_rnn_launch("pm_play_rnn_rec", p, w_qnet, n_qnet, w_rnn, n_rnn, blk_nets, blk_range, n_blocks, order,
                           serves, n, max_steps, hc_scratch, scoreA, scoreB, length, last, status, &rec, stream);
}
