// Device helpers shared by the match megakernels (K8: pm_play.hip, pm_playrnn.hip): block shape,
// slot-table staging, and the non-recurrent players on register-resident observations.
#pragma once
#include "pm_mfma.h"

namespace pm {

constexpr int kPlayBlock = 256;
constexpr int kPlayArenas = kPlayBlock / 2;  // columns per block: 4 tiles of 32
constexpr int kMaxSlots = 1024;              // slots per block range (staged in LDS)

// n dwords global -> LDS with global_load_lds (4 B per lane, no registers); published by the
// caller's __syncthreads(). The tail of the last wave instruction re-reads the last dword.
__device__ __forceinline__ void copy_lds_dwords(const void* __restrict__ src, void* dst, int n) {
    if (n <= 0) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const uint32_t* s = static_cast<const uint32_t*>(src);
    uint32_t* d = static_cast<uint32_t*>(dst);
    for (int c = wv; c * 64 < n; c += nw) {
        const int k = min(c * 64 + lane, n - 1);
        __builtin_amdgcn_global_load_lds((const void*)(s + k), (lds_void*)(d + c * 64), 4, 0, 0);
    }
}

// layer-1 B operands from register-resident observations (tile_inputs with a register array)
__device__ __forceinline__ void inputs_of(const float (&o)[7], int h, float (&xs)[4]) {
    xs[0] = h ? o[0] : 1.0f;
    xs[1] = h ? o[2] : o[1];
    xs[2] = h ? o[4] : o[3];
    xs[3] = h ? o[6] : o[5];
}

__device__ __forceinline__ int follower(const float (&o)[7]) {  // obs: ball_x [0], own paddle x [4]
    const float tol = 0.01f;
    return o[0] < o[4] - tol ? 0 : (o[0] > o[4] + tol ? 2 : 1);
}

// the greedy action and the q values its argmax consumed (the same in both lane halves)
__device__ __forceinline__ int greedy(const float* lw, const float (&o)[7], int lane, float (&q)[3]) {
    float xs[4];
    inputs_of(o, lane >> 5, xs);
    f32x16 c2[2];
    tile_hidden(lw, xs, lane, c2);
    tile_heads(lw + F_H, c2, lane, q);
    return argmax3(q);
}

// The plain kernels' greedy: the same body, not a call of the one above. Written as a wrapper it
// compiled k_play<false> to a different schedule than before recording existed.
__device__ __forceinline__ int greedy(const float* lw, const float (&o)[7], int lane) {
    float xs[4];
    inputs_of(o, lane >> 5, xs);
    f32x16 c2[2];
    tile_hidden(lw, xs, lane, c2);
    float q[3];
    tile_heads(lw + F_H, c2, lane, q);
    return argmax3(q);
}

// ---------------------------------------------------------------- tick records (the REC kernels)
// Recorded arenas get a row of rec_cap ticks in three caller buffers; rec_row[arena] is the row, -1
// for the arenas that are not recorded. Tick t of row r (t = the episode's tick index, from 0):
//   f64[r][t][7]    x, y, vx, vy, spin, top paddle x, bottom paddle x after the tick
//   q[r][t][2][3]   the q values side A's / side B's argmax consumed (quiet NaN: ball follower)
//   i32[r][t][5]    aA, aB, scoreA, scoreB, bounce count after the tick
// Ticks at or beyond cap are not stored. All stores come from lanes < 32 (one per column).
struct PlayRec {
    const int32_t* row;  // [n]
    int32_t n_rec, cap;
    double* f64;
    float* q;
    int32_t* i32;
};

// The kernels take the PlayRec as a trailing parameter pack: one PlayRec when REC, none otherwise, so
// the REC = false kernels keep the kernel-argument segment (and with it the code) they had before
// recording existed. rec_arg(rec...) is the PlayRec inside an `if constexpr (REC)`.
__device__ __forceinline__ const PlayRec& rec_arg(const PlayRec& rec) { return rec; }

// the record row of a column's new episode (arena already validated): one load per episode start.
// A row outside [-1, n_rec) records nothing and adds to `bad` (counted into *status at the end).
__device__ __forceinline__ int rec_row_of(const PlayRec& rec, int arena, int& bad) {
    const int r = rec.row[arena];
    if (r < -1 || r >= rec.n_rec) { bad += 1; return -1; }
    return r;
}

__device__ __forceinline__ bool rec_here(const PlayRec& rec, int row, int t, int lane) {
    return row >= 0 && t < rec.cap && lane < 32;
}

__device__ __forceinline__ void rec_q(const PlayRec& rec, int row, int t, int side, const float (&q)[3]) {
    float* d = rec.q + ((size_t)row * rec.cap + t) * 6 + side * 3;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
}

__device__ __forceinline__ void rec_q_none(const PlayRec& rec, int row, int t, int side) {
    const float nan = __builtin_nanf("");
    const float q[3] = {nan, nan, nan};
    rec_q(rec, row, t, side, q);
}

__device__ __forceinline__ void rec_tick(const PlayRec& rec, int row, int t, const Arena& a, int aA, int aB) {
    const size_t k = (size_t)row * rec.cap + t;
    double* f = rec.f64 + k * 7;
    f[0] = a.x; f[1] = a.y; f[2] = a.vx; f[3] = a.vy; f[4] = a.spin; f[5] = a.top; f[6] = a.bot;
    int32_t* i = rec.i32 + k * 5;
    i[0] = aA; i[1] = aB; i[2] = a.sA; i[3] = a.sB; i[4] = a.bounces;
}

}  // namespace pm
