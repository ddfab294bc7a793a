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

__device__ __forceinline__ int greedy(const float* lw, const float (&o)[7], int lane) {
    float xs[4];
    inputs_of(o, lane >> 5, xs);
    f32x16 c2[2];
    tile_hidden(lw, xs, lane, c2);
    float q[3];
    tile_heads(lw + F_H, c2, lane, q);
    return argmax3(q);
}

}  // namespace pm
