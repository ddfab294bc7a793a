// K10 — the stand-alone double-DQN learner: train_step (scripts/train_iterative.py:141-168) on a batch
// the caller supplies, heads only (the reference: features frozen, :97) or over all 5 192 parameters.
//
//   k_dqn_grads  one workgroup of 1024 threads (16 waves), nothing to wait for but its own barriers:
//     phase 0  noise (reset_noise, :142: Philox(seed_net, TAG_NOISE_TRAIN, stats.steps + 1), read on the
//              device), both nets' fragment images and folded heads into LDS.
//     phase 1  the three forwards on 32-row tiles (v_mfma_f32_32x32x2_f32, pm_mfma.h's tile_hidden, so
//              Q_B(s) is bit for bit what pm_qnet_q gives): waves 0..7 Q_T(s') then Q_B(s) of tile w,
//              keeping the hidden activations in registers; waves 8..15 Q_B(s') of tile w - 8. Where
//              targetB's feature layers equal modelB's bit for bit (checked in phase 0), Q_T(s') is the
//              target heads on Q_B(s')'s hidden layers instead: the same bits, 16 tile forwards not 24.
//     phase 2  per row: a* (first maximum), t, td, dL/dq; the loss and the head bias gradients as DPP
//              wave sums (pm_dev.h wave_sum) of waves 0..3 added in wave order. h1 / h2 go to LDS as
//              [row][unit] (two 64 KB arrays over the fragment images, which are dead by now).
//     phase 3  head dW = h2^T G on v_mfma_f32_16x16x4_f32 (waves 8..11, one 16-unit tile each, K = the
//              batch rows in order), while waves 0..7 form dh2 in registers and, with train_features,
//              dh1 = (dh2 W2) * relu'(h1) on 32x32x2 with dh2 as the A operand straight from registers.
//     phase 4  dW2 = dh2^T h1: 16 tiles of 16x16, one per wave, K = the batch rows in order; db2 as 16
//              partial column sums of 16 rows each, added in order.
//     phase 5  dW1 | db1 = dh1^T [s | 1]: 4 tiles of 16 units (waves 0..3), K = the batch rows in order, the
//              [s | 1] rows staged in LDS over h1 (loaded under phase 4).
//   Every sum has one fixed order and there is no atomic: the gradient is a pure function of the inputs.
//   Rows >= batch are never read; their operands are zeros.
//   k_dqn_apply  grad / count, torch.optim.Adam over [4672, 5192) or all of [0, 5192), target sync, counters.
//   k_dqn_update both bodies in one launch (pm_dqn_update), a barrier between them.
//   k_*_opt      the same bodies with a pm_dqn_opt (pm_dqn_*_opt): phase 2 may form the Huber (smooth-L1) loss
//     term and dL/dq instead of the squared ones, and the apply body may clip on the total norm of grad /
//     count over the trained slots: per thread the squares in fp64 in slot order, a DPP wave sum, the 16
//     wave sums through LDS under the barrier the body already has, added in wave order by every thread (no
//     further barrier, no global round trip, no atomic). The bodies are templates; the plain kernels are
//     their <false> instantiations and keep their device text (tools/kernel_text.py against the parent).
//   k_dqp_update the population learner's launch (pm_dqn_pop_update, and pm_dqn_pop_replay_update's middle
//     one): a grid of n workgroups, workgroup p running k_dqr_update_opt's code on the p-th record of a device
//     table. A member touches its own buffers only, so no workgroup waits for or orders itself against another.
#include <cmath>

#include "pm_dev.h"
#include "pm_dqn_pop.h"
#include "pm_host.h"
#include "pm_mfma.h"

static_assert(PM_DQN_NPARAM == PM_QNET_EPS_OFF, "the trainable part of a parameter block");

namespace pm {
namespace {

constexpr int kDqn = 1024;
constexpr int kRows = PM_MAX_BATCH;

// [row][unit] activations in LDS, 16-byte chunks XOR-swizzled by row: the accumulator layout's float4
// stores (32 lanes = 32 rows, same chunk) spread over 16 chunks, and a row's 16 / 32 consecutive units
// (the MFMA operand reads) still cover distinct banks.
__device__ __forceinline__ int swz(int b, int u) { return b * 64 + ((((u >> 2) ^ (b & 15)) << 2) | (u & 3)); }

struct DqnSmem {
    union {
        struct {
            float lwB[kLwFloats], lwT[kLwFloats];  // phases 0-1: fragment images (feature part)
        } f;
        struct {
            float r0[kRows * 64];  // h1
            float r1[kRows * 64];  // h2, then dh2, then dh1
        } a;
    } u;
    float w2[4096];  // modelB's features.2.weight, plain (train_features)
    union {
        float G[kRows][4];  // dL/d(V, A0, A1, A2) per row
        float red[16][64];  // db2's partial column sums (G is dead by then)
    } g;
    float qt[kRows][3];  // Q_T(s')
    float qa[kRows];     // Q_B(s)[a]
    int na[kRows];       // argmax Q_B(s')
    float hfB[264], hfT[264];  // head fragments (F_H order | bh)
    float heads[2][260];
    float eps[260];            // modelB's epsilon buffers as this update uses them
    float noise[132];
    float wred[4][8];          // per wave: dbh[4], loss, q sum
};
static_assert(sizeof(DqnSmem) <= 160 * 1024, "one workgroup's LDS");

typedef float f32x4m __attribute__((ext_vector_type(4)));

// One tile's accumulator-layout values (lane = row tile * 32 + (lane & 31), units 32 jt + rho(r) + 4 h) into
// a [row][unit] array; rows >= batch get zeros.
__device__ __forceinline__ void store_acc_rows(float* r, int row, bool valid, int h, const f32x16 (&c)[2], bool do_relu) {
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v = make_float4(c[jt][4 * g], c[jt][4 * g + 1], c[jt][4 * g + 2], c[jt][4 * g + 3]);
            if (do_relu) v = make_float4(relu(v.x), relu(v.y), relu(v.z), relu(v.w));
            if (!valid) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(r + swz(row, 32 * jt + 8 * g + 4 * h)) = v;
        }
}

// Block-wide (kDqn threads). Returns with every store issued; the caller's barrier publishes them.
// kOpt: o.loss selects the row loss of phase 2; without it o is not read.
// kN: row t's target discounts by disc(k), k = ((hz[t] - 1) & 7) + 1 its horizon (pm_dqn_nstep; a null hz is k = 1
// for every row); without it hz is not read.
template <bool kOpt, bool kN = false>
__device__ __forceinline__ void dqn_grads_body(const pm_dqn& d, const pm_dqn_opt& o, DqnSmem& sm,
                                               const uint8_t* hz = nullptr) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int B = d.batch, ntiles = (B + 31) >> 5, nrows = ntiles * 32;
    const bool tf = d.train_features != 0;
    const int64_t steps = d.stats->steps;

    // ---- phase 0
    if (d.noise == PM_FOLD_TRAIN_FRESH) gen_noise(d.seed_net, TAG_NOISE_TRAIN, (uint64_t)(steps + 1), sm.noise, t, kDqn);
    write_feature_frag_image(d.params, sm.u.f.lwB);
    write_feature_frag_image(d.target, sm.u.f.lwT);
    if (tf)
        for (int k = t; k < 4096; k += kDqn) sm.w2[k] = d.params[W2 + k];
    // targetB's feature layers bit-equal to modelB's (always, while they are frozen; after a sync otherwise):
    // Q_T(s') then takes the hidden layers Q_B(s') computed, the same bits for a third less matrix work
    int differ = 0;
    for (int k = t; k < PM_QNET_HEAD_OFF; k += kDqn) differ |= __float_as_uint(d.params[k]) != __float_as_uint(d.target[k]);
    const bool shared_feat = !__syncthreads_or(differ);
    if (t < 256) {
        fold_heads_from(d.params + PM_QNET_HEAD_OFF, d.params + PM_QNET_EPS_OFF, sm.noise, d.noise, sm.heads[0], sm.eps, t, 256);
    } else if (t < 512) {
        fold_heads_from(d.target + PM_QNET_HEAD_OFF, nullptr, nullptr, PM_FOLD_EVAL, sm.heads[1], nullptr, t - 256, 256);
    } else if (d.noise != PM_FOLD_TRAIN_FRESH && t - 512 < 260) {
        sm.eps[t - 512] = d.params[PM_QNET_EPS_OFF + t - 512];
    }
    __syncthreads();
    heads_to_frags(sm.heads[0], sm.hfB);
    heads_to_frags(sm.heads[1], sm.hfT);
    if (d.noise == PM_FOLD_TRAIN_FRESH && t < 260) d.params[PM_QNET_EPS_OFF + t] = sm.eps[t];  // reset_noise()'s buffers
    __syncthreads();

    // ---- phase 1
    const int tile = wave & 7;
    const bool work = tile < ntiles;  // wave-uniform
    const int row = tile * 32 + col;
    const bool valid = row < B;
    const int rr = min(row, B - 1);
    f32x16 c1[2], c2[2];  // waves 0..7: ReLU(layer 1) and layer 2 (pre-ReLU) of Q_B(s), then the backward's values
    if (work) {
        float xs[4], q[3];
        if (wave >= 8) {
            f32x16 cn[2];
            tile_inputs(d.ns + (size_t)rr * 7, h, xs);
            tile_hidden(sm.u.f.lwB, xs, lane, cn);
            tile_heads(sm.hfB, cn, lane, q);
            if (h == 0 && valid) sm.na[row] = argmax3(q);
            if (shared_feat) {
                tile_heads(sm.hfT, cn, lane, q);
                if (h == 0 && valid) {
                    sm.qt[row][0] = q[0]; sm.qt[row][1] = q[1]; sm.qt[row][2] = q[2];
                }
            }
        } else {
            if (!shared_feat) {
                f32x16 cn[2];
                tile_inputs(d.ns + (size_t)rr * 7, h, xs);
                tile_hidden(sm.u.f.lwT, xs, lane, cn);
                tile_heads(sm.hfT, cn, lane, q);
                if (h == 0 && valid) {
                    sm.qt[row][0] = q[0]; sm.qt[row][1] = q[1]; sm.qt[row][2] = q[2];
                }
            }
            tile_inputs(d.s + (size_t)rr * 7, h, xs);
            tile_hidden_h1(sm.u.f.lwB, xs, lane, c1, c2);
            tile_heads(sm.hfB, c2, lane, q);
            if (h == 0 && valid) {
                const int a = d.act[row];
                sm.qa[row] = a == 0 ? q[0] : (a == 1 ? q[1] : q[2]);
                if (d.q) {
                    d.q[(size_t)row * 3 + 0] = q[0]; d.q[(size_t)row * 3 + 1] = q[1]; d.q[(size_t)row * 3 + 2] = q[2];
                }
            }
        }
    }
    __syncthreads();  // every forward is done: the fragment images are dead, r0 / r1 take their place

    // ---- phase 2
    if (work && wave < 8) {
        store_acc_rows(sm.u.a.r1, row, valid, h, c2, true);
        if (tf) store_acc_rows(sm.u.a.r0, row, valid, h, c1, false);
    }
    if (t < kRows) {  // waves 0..3, every lane: row t
        float gv = 0.f, gm = 0.f, lterm = 0.f, qv = 0.f;
        int a = -1;
        if (t < B) {
            a = d.act[t];
            qv = sm.qa[t];
            const int na = sm.na[t];
            const float nq = na == 0 ? sm.qt[t][0] : (na == 1 ? sm.qt[t][1] : sm.qt[t][2]);
            float disc = (float)d.gamma;
            if (kN && hz) {  // disc(k) = disc(k - 1) * g, float32 products in that order
                const float g = disc;
                const int k1 = (hz[t] - 1) & 7;
                for (int e = 0; e < k1; ++e) disc = disc * g;
            }
            const float tg = d.rew[t] + (disc * nq) * (d.done[t] ? 0.f : 1.f);  // r + gamma * nq * (~d)
            const float diff = qv - tg, w = d.isw ? d.isw[t] : 1.f;
            d.td[t] = fabsf(diff);
            lterm = w * (diff * diff);
            gv = (w * (1.0f / (float)B)) * (2.0f * diff);  // mean, then iw *, then pow(2)'s 2 * diff
            if (kOpt && o.loss == PM_DQN_LOSS_HUBER) {  // (iw * smooth_l1_loss(q, t, 'none', beta)).mean()
                const float beta = (float)o.huber_beta, ad = fabsf(diff);
                lterm = w * (ad < beta ? 0.5f * diff * diff / beta : ad - 0.5f * beta);
                gv = (w * (1.0f / (float)B)) * (ad < beta ? diff / beta : (diff > 0.f ? 1.0f : -1.0f));
            }
            gm = gv / 3.0f;                                // A.mean(dim=1)'s backward
        }
        const float g0 = gv, g1 = (a == 0 ? gv : 0.f) - gm, g2 = (a == 1 ? gv : 0.f) - gm, g3 = (a == 2 ? gv : 0.f) - gm;
        *reinterpret_cast<float4*>(sm.g.G[t]) = make_float4(g0, g1, g2, g3);
        const float s0 = wave_sum(g0), s1 = wave_sum(g1), s2 = wave_sum(g2), s3 = wave_sum(g3);
        const float sl = wave_sum(lterm), sq = wave_sum(qv);
        if (lane == 0) {
            sm.wred[wave][0] = s0; sm.wred[wave][1] = s1; sm.wred[wave][2] = s2; sm.wred[wave][3] = s3;
            sm.wred[wave][4] = sl; sm.wred[wave][5] = sq;
        }
    }
    __syncthreads();

    // ---- phase 3
    float* const grad = d.grad;
    if (t < 8) grad[PM_DQN_NPARAM + t] = t == 0 ? 1.0f : 0.0f;
    if (t < 6) {
        const float v = ((sm.wred[0][t] + sm.wred[1][t]) + sm.wred[2][t]) + sm.wred[3][t];
        float* gh = grad + PM_QNET_HEAD_OFF;
        if (t == 0) {
            gh[H_VBMU] = v;
            gh[H_VBSG] = v * sm.eps[E_VBEP];
        } else if (t < 4) {
            gh[H_ABMU + t - 1] = v;
            gh[H_ABSG + t - 1] = v * sm.eps[E_ABEP + t - 1];
        } else if (t == 4) {
            d.stats->loss = v / (float)B;
        } else {
            d.stats->q_mean = v / (float)B;
        }
    }
    if (wave >= 8 && wave < 12) {  // head dW: out[j][c] = sum_b h2[b][j] G[b][c], 16 units per wave
        const int jb = (wave - 8) * 16, c = lane & 15, kq = lane >> 4;
        f32x4m acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nrows; kb += 4) {
            const int b = kb + kq;
            const float av = sm.u.a.r1[swz(b, jb + c)];
            const float bv = c < 4 ? sm.g.G[b][c] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
        if (c < 4) {
            float* gh = grad + PM_QNET_HEAD_OFF;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jb + kq * 4 + r;
                const float v = acc[r];
                if (c == 0) {
                    gh[H_VWMU + j] = v;
                    gh[H_VWSG + j] = v * sm.eps[E_VWEP + j];
                } else {
                    gh[H_AWMU + (c - 1) * 64 + j] = v;
                    gh[H_AWSG + (c - 1) * 64 + j] = v * sm.eps[E_AWEP + (c - 1) * 64 + j];
                }
            }
        }
    }
    f32x16 d1[2] = {};  // dh1 of this wave's tile: rows rho(r) + 4 h of the tile, unit 32 it + col
    if (tf && work && wave < 8) {
        // dh2 = (G Wh) * relu'(c2), in c2's registers
        const float4 gq = *reinterpret_cast<const float4*>(sm.g.G[row]);
        const float4* hw = reinterpret_cast<const float4*>(sm.hfB + h * 128);
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float4 w = hw[jt * 16 + r];
                const float v = fmaf(w.w, gq.w, fmaf(w.z, gq.z, fmaf(w.y, gq.y, w.x * gq.x)));
                c2[jt][r] = c2[jt][r] > 0.f ? v : 0.f;  // relu'(0) = 0
            }
        // dh1[b][i] = sum_j dh2[b][j] W2[j][i]: A = dh2 (row b on the lane, k = the register's two units),
        // B = W2's rows, j in the accumulator's register order
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* wr = sm.w2 + (32 * jt + rho(r) + 4 * h) * 64 + col;
                d1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(c2[jt][r], wr[0], d1[0], 0, 0, 0);
                d1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(c2[jt][r], wr[32], d1[1], 0, 0, 0);
            }
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float h1v = sm.u.a.r0[swz(tile * 32 + rho(r) + 4 * h, 32 * it + col)];
                d1[it][r] = h1v > 0.f ? d1[it][r] : 0.f;
            }
    }
    if (!tf) return;  // block-uniform: heads only
    __syncthreads();  // head dW has read h2 and G

    // ---- phase 4
    if (work && wave < 8) store_acc_rows(sm.u.a.r1, row, valid, h, c2, false);  // dh2
    __syncthreads();
    // [s | 1] rows for phase 5, two per thread: loaded here, under dW2, stored over h1 once dW2 has read it
    float sx[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int k = t + e * kDqn, b = k >> 3, c = k & 7;
        sx[e] = b < B ? (c < 7 ? d.s[(size_t)b * 7 + c] : 1.0f) : 0.f;
    }
    {
        const int jb = (wave >> 2) * 16, ib = (wave & 3) * 16, c = lane & 15, kq = lane >> 4;
        f32x4m acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nrows; kb += 4) {
            const int b = kb + kq;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.u.a.r1[swz(b, jb + c)], sm.u.a.r0[swz(b, ib + c)], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) grad[W2 + (jb + kq * 4 + r) * 64 + ib + c] = acc[r];
        // db2: partial column sums of 16 rows each
        const int j = t & 63, p = t >> 6;
        float s = 0.f;
        for (int b = p * 16; b < min(p * 16 + 16, nrows); ++b) s += sm.u.a.r1[swz(b, j)];
        sm.g.red[p][j] = s;
    }
    __syncthreads();  // dW2 has read dh2

    // ---- phase 5
    if (t < 64) {
        float s = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) s += sm.g.red[p][t];
        grad[B2 + t] = s;
    }
    sm.u.a.r0[t] = sx[0];  // [row][8]
    sm.u.a.r0[t + kDqn] = sx[1];
    if (work && wave < 8) {  // dh1 rows of this tile: lane = unit, register = row
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int r = 0; r < 16; ++r) sm.u.a.r1[swz(tile * 32 + rho(r) + 4 * h, 32 * it + col)] = d1[it][r];
    }
    __syncthreads();
    if (wave < 4) {  // out[i][k] = sum_b dh1[b][i] [s | 1][b][k]: columns 0..6 dW1, column 7 db1
        const int ib = wave * 16, c = lane & 15, kq = lane >> 4;
        f32x4m acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < nrows; kb += 4) {
            const int b = kb + kq;
            const float bv = c < 8 ? sm.u.a.r0[b * 8 + c] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sm.u.a.r1[swz(b, ib + c)], bv, acc, 0, 0, 0);
        }
        if (c < 8) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ib + kq * 4 + r;
                if (c < 7) grad[W1 + i * 7 + c] = acc[r];
                else grad[B1 + i] = acc[r];
            }
        }
    }
}

// grad / count -> torch.optim.Adam (single-tensor path, as k_adam's adam_one) -> target sync -> counters.
// Every load is issued before the first store (the buffers may alias as far as the compiler knows, and a
// load behind a store would wait for it: five round trips instead of one over the whole net). Block-wide.
// kOpt: clip_grad_norm_ on grad / count over the trained slots (o.max_norm > 0) and the norm out (o.norm);
// nsq: the 16 waves' sums of squares, published by the barrier that publishes ak.
template <bool kOpt>
__device__ __forceinline__ void dqn_apply_body(const pm_dqn& d, const pm_dqn_opt& o, float (&ak)[2], double* nsq) {
    const int t = threadIdx.x;
    const float count = d.grad[PM_DQN_NPARAM];
    if (!(count > 0.5f)) return;  // nobody contributed (block-uniform)
    const int64_t steps = d.stats->steps + 1, at = d.stats->adam_t + 1;
    if (t < 2) {  // torch's bias corrections, in fp64 as Python floats
        const double bc = 1.0 - pow(t ? d.beta2 : d.beta1, (double)at);
        ak[t] = t ? (float)sqrt(bc) : (float)(d.lr / bc);
    }
    constexpr int kPer = (PM_QNET_NP + kDqn - 1) / kDqn;  // 6
    const int k0 = (d.train_features ? 0 : PM_QNET_HEAD_OFF) + t;
    float g[kPer], m[kPer], v[kPer], p[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int k = k0 + i * kDqn;
        if (k < PM_DQN_NPARAM) { g[i] = d.grad[k]; m[i] = d.adam_m[k]; v[i] = d.adam_v[k]; p[i] = d.params[k]; }
    }
    if (kOpt) {  // full waves: the return above is block-uniform
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (k0 + i * kDqn < PM_DQN_NPARAM) {
                const double gk = (double)(g[i] / count);
                ss += gk * gk;
            }
        ss = wave_sum(ss);
        if ((t & 63) == 0) nsq[t >> 6] = ss;
    }
    __syncthreads();  // ak; also orders every thread's read of stats before thread 0's write below
    const float step_size = ak[0], bc2s = ak[1];
    float coef = 1.0f;
    if (kOpt) {  // every thread adds the same 16 sums in the same order: one coefficient, no second barrier
        double ss = 0.0;
#pragma unroll
        for (int w = 0; w < kDqn / 64; ++w) ss += nsq[w];
        const float norm = (float)sqrt(ss);
        if (o.max_norm > 0.0) {
            const float cc = (float)(o.max_norm / ((double)norm + 1e-6));  // clip_coef
            coef = cc < 1.0f ? cc : 1.0f;                                  // clamp(clip_coef, max=1)
        }
        if (t == 0 && o.norm) *o.norm = norm;
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int k = k0 + i * kDqn;
        if (k < PM_DQN_NPARAM) {
            float gk = g[i] / count;
            if (kOpt) gk = gk * coef;
            float mk = m[i], vk = v[i];
            mk = mk + (float)(1.0 - d.beta1) * (gk - mk);                  // exp_avg.lerp_(grad, 1 - beta1)
            vk = vk * (float)d.beta2 + (float)(1.0 - d.beta2) * gk * gk;  // mul_(beta2).addcmul_(g, g, 1 - beta2)
            const float denom = sqrtf(vk) / bc2s + (float)d.adam_eps;
            d.params[k] = p[i] - step_size * (mk / denom);
            d.adam_m[k] = mk;
            d.adam_v[k] = vk;
        }
    }
    if (steps % d.target_update_interval == 0) {  // targetB.load_state_dict(modelB.state_dict()) (:166-168)
        __syncthreads();
        float c[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (t + i * kDqn < PM_QNET_NP) c[i] = d.params[t + i * kDqn];
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (t + i * kDqn < PM_QNET_NP) d.target[t + i * kDqn] = c[i];
    }
    if (t == 0) {
        d.stats->steps = steps;
        d.stats->adam_t = at;
    }
}

__global__ __launch_bounds__(kDqn, 1) void k_dqn_grads(const pm_dqn d) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    dqn_grads_body<false>(d, pm_dqn_opt{}, sm);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqn_apply(const pm_dqn d) {
    __shared__ float ak[2];
    dqn_apply_body<false>(d, pm_dqn_opt{}, ak, nullptr);
}

// pm_dqn_update: both in one launch, the gradient handed over through grad (the same loads and the same
// arithmetic as the two launches: bit-identical). The eight update kernels below spell their LDS blocks and their two
// body calls out one by one on purpose: behind one shared dqn_update_body<kOpt, kN> every one of them compiled to
// different text (17 to 27 lines, the same counts and resources), so the wrappers stay as they are.
__global__ __launch_bounds__(kDqn, 1) void k_dqn_update(const pm_dqn d) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    dqn_grads_body<false>(d, pm_dqn_opt{}, sm);
    __syncthreads();
    dqn_apply_body<false>(d, pm_dqn_opt{}, ak, nullptr);
}

// pm_dqn_replay_update's middle launch: k_dqn_update on the batch k_dqr_sample gathered, or nothing when
// that update is void (the sampler wrote -1 slots).
__global__ __launch_bounds__(kDqn, 1) void k_dqr_update(const pm_dqn d, const int64_t* gate) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    if (gate[0] < 0) return;  // block-uniform
    dqn_grads_body<false>(d, pm_dqn_opt{}, sm);
    __syncthreads();
    dqn_apply_body<false>(d, pm_dqn_opt{}, ak, nullptr);
}

// The four with a pm_dqn_opt (pm_dqn_*_opt): the same bodies, the loss chosen in phase 2 and the clip in apply.
__global__ __launch_bounds__(kDqn, 1) void k_dqn_grads_opt(const pm_dqn d, const pm_dqn_opt o) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    dqn_grads_body<true>(d, o, sm);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqn_apply_opt(const pm_dqn d, const pm_dqn_opt o) {
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    dqn_apply_body<true>(d, o, ak, nsq);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqn_update_opt(const pm_dqn d, const pm_dqn_opt o) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    dqn_grads_body<true>(d, o, sm);
    __syncthreads();
    dqn_apply_body<true>(d, o, ak, nsq);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqr_update_opt(const pm_dqn d, const pm_dqn_opt o, const int64_t* gate) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    if (gate[0] < 0) return;  // block-uniform: a void update takes no step and leaves *o.norm as it is
    dqn_grads_body<true>(d, o, sm);
    __syncthreads();
    dqn_apply_body<true>(d, o, ak, nsq);
}

// The three with a pm_dqn_nstep's horizon buffer (pm_dqn_*_n with a non-null horizon): the _opt kernels with kN.
__global__ __launch_bounds__(kDqn, 1) void k_dqn_grads_n(const pm_dqn d, const pm_dqn_opt o, const uint8_t* hz) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    dqn_grads_body<true, true>(d, o, sm, hz);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqn_update_n(const pm_dqn d, const pm_dqn_opt o, const uint8_t* hz) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    dqn_grads_body<true, true>(d, o, sm, hz);
    __syncthreads();
    dqn_apply_body<true>(d, o, ak, nsq);
}

__global__ __launch_bounds__(kDqn, 1) void k_dqr_update_n(const pm_dqn d, const pm_dqn_opt o, const uint8_t* hz,
                                                         const int64_t* gate) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    if (gate[0] < 0) return;  // block-uniform, as k_dqr_update_opt
    dqn_grads_body<true, true>(d, o, sm, hz);
    __syncthreads();
    dqn_apply_body<true>(d, o, ak, nsq);
}

// One population member per workgroup: the record is block-uniform and comes in by scalar loads (pop_member, pm_pop.h).
__global__ __launch_bounds__(kDqn, 1) void k_dqp_update(const pm_dqn_member* tab, int gated) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    const pm_dqn_member m = pop_member(tab, blockIdx.x);
    if (gated && m.rp.idx[0] < 0) return;  // block-uniform: this member's update is void; the others' are not
    dqn_grads_body<true>(m.d, m.o, sm);
    __syncthreads();
    dqn_apply_body<true>(m.d, m.o, ak, nsq);
}

// k_dqp_update with the members' horizon buffers (pm_dqn_nstep_pop_set): hzt[p] is member p's, or null.
__global__ __launch_bounds__(kDqn, 1) void k_dqp_update_n(const pm_dqn_member* tab, const uint8_t* const* hzt, int gated) {
    __shared__ __attribute__((aligned(16))) DqnSmem sm;
    __shared__ float ak[2];
    __shared__ double nsq[kDqn / 64];
    const pm_dqn_member m = pop_member(tab, blockIdx.x);
    if (gated && m.rp.idx[0] < 0) return;  // block-uniform
    dqn_grads_body<true, true>(m.d, m.o, sm, hzt[blockIdx.x]);
    __syncthreads();
    dqn_apply_body<true>(m.d, m.o, ak, nsq);
}

int check(const pm_dqn* d) {
    PM_REQUIRE(d, PM_E_ARG, "pm_dqn: null descriptor");
    PM_REQUIRE(d->params && d->target && d->adam_m && d->adam_v && d->grad && d->stats, PM_E_ARG, "pm_dqn: null buffer");
    PM_REQUIRE(d->s && d->ns && d->act && d->rew && d->done && d->td, PM_E_ARG, "pm_dqn: null batch buffer");
    PM_REQUIRE(d->batch >= 1 && d->batch <= PM_MAX_BATCH, PM_E_SIZE, "pm_dqn: batch %d (1..%d)", d->batch, PM_MAX_BATCH);
    PM_REQUIRE(d->noise == PM_FOLD_TRAIN || d->noise == PM_FOLD_TRAIN_FRESH, PM_E_ARG,
               "pm_dqn: noise %d (PM_FOLD_TRAIN or PM_FOLD_TRAIN_FRESH)", d->noise);
    PM_REQUIRE(d->target_update_interval >= 1, PM_E_ARG, "pm_dqn: target_update_interval");
    return PM_OK;
}

// A null opt is the defaults; huber_beta is only ever read with PM_DQN_LOSS_HUBER.
int check_opt(const pm_dqn_opt* o) {
    if (!o) return PM_OK;
    PM_REQUIRE(o->loss == PM_DQN_LOSS_SQUARED || o->loss == PM_DQN_LOSS_HUBER, PM_E_ARG,
               "pm_dqn_opt: loss %d (PM_DQN_LOSS_SQUARED or PM_DQN_LOSS_HUBER)", o->loss);
    PM_REQUIRE(o->loss != PM_DQN_LOSS_HUBER || (std::isfinite(o->huber_beta) && o->huber_beta > 0.0), PM_E_ARG,
               "pm_dqn_opt: huber_beta %g (> 0, finite)", o->huber_beta);
    PM_REQUIRE(std::isfinite(o->max_norm) && o->max_norm >= 0.0, PM_E_ARG, "pm_dqn_opt: max_norm %g (0: no clip; > 0, finite)",
               o->max_norm);
    return PM_OK;
}

pm_dqn_opt opt_or_default(const pm_dqn_opt* o) {
    pm_dqn_opt z{};  // PM_DQN_LOSS_SQUARED, max_norm 0, norm null
    return o ? *o : z;
}

}  // namespace

int dqn_check(const pm_dqn* d, const pm_dqn_opt* o) {
    if (int rc = check(d)) return rc;
    return check_opt(o);
}

// The one place where a stand-alone learner's kernel is chosen: the plain ones without an options record, the _opt
// ones with one (a null record is the defaults), the _n ones with one and a horizon buffer. The apply stage reads no
// horizon and has no _n form.
int dqn_launch(DqnStage stage, const pm_dqn* d, bool with_opt, const pm_dqn_opt* o, const uint8_t* hz,
               const int64_t* gate, hipStream_t st) {
    const pm_dqn_opt op = opt_or_default(o);
    const char* name;
    const auto launch = [&](auto kernel, const char* kernel_name, auto... more) {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(kDqn), 0, st, *d, more...);
        name = kernel_name;
    };
#define K(kernel) kernel, #kernel
    switch (3 * stage + (!with_opt ? 0 : hz && stage != DQN_APPLY ? 2 : 1)) {
        case 3 * DQN_GRADS + 0: launch(K(k_dqn_grads)); break;
        case 3 * DQN_GRADS + 1: launch(K(k_dqn_grads_opt), op); break;
        case 3 * DQN_GRADS + 2: launch(K(k_dqn_grads_n), op, hz); break;
        case 3 * DQN_APPLY + 0: launch(K(k_dqn_apply)); break;
        case 3 * DQN_APPLY + 1: launch(K(k_dqn_apply_opt), op); break;
        case 3 * DQN_UPDATE + 0: launch(K(k_dqn_update)); break;
        case 3 * DQN_UPDATE + 1: launch(K(k_dqn_update_opt), op); break;
        case 3 * DQN_UPDATE + 2: launch(K(k_dqn_update_n), op, hz); break;
        case 3 * DQN_UPDATE_GATED + 0: launch(K(k_dqr_update), gate); break;
        case 3 * DQN_UPDATE_GATED + 1: launch(K(k_dqr_update_opt), op, gate); break;
        case 3 * DQN_UPDATE_GATED + 2: launch(K(k_dqr_update_n), op, hz, gate); break;
        default: return pm_fail(PM_E_ARG, "dqn_launch: stage %d", (int)stage);
    }
#undef K
    PM_LAUNCHED(name);
    return PM_OK;
}

// The population's update picks by the same rule: the _n kernel with a table of horizon buffers.
int dqp_launch_update(const pm_dqn_member* tab, const uint8_t* const* hzt, int n, int gated, hipStream_t st) {
    if (hzt)
        hipLaunchKernelGGL(k_dqp_update_n, dim3(n), dim3(kDqn), 0, st, tab, hzt, gated);
    else
        hipLaunchKernelGGL(k_dqp_update, dim3(n), dim3(kDqn), 0, st, tab, gated);
    PM_LAUNCHED(hzt ? "k_dqp_update_n" : "k_dqp_update");
    return PM_OK;
}
}  // namespace pm

using namespace pm;

// Every pm_dqn_* entry below: the checks, then the launch. with_opt false: the plain kernels; a null pm_dqn_nstep, or
// one with a null horizon, is the _opt entry as it is (the same kernel).
static int dqn_entry(DqnStage stage, const pm_dqn* d, bool with_opt, const pm_dqn_opt* o, const pm_dqn_nstep* ns,
                     void* stream) {
    if (int rc = dqn_check(d, o)) return rc;
    return dqn_launch(stage, d, with_opt, o, ns ? ns->horizon : nullptr, nullptr, pm_stream(stream));
}

extern "C" size_t pm_dqn_opt_sizeof(void) { return sizeof(pm_dqn_opt); }
extern "C" size_t pm_dqn_nstep_sizeof(void) { return sizeof(pm_dqn_nstep); }

extern "C" int pm_dqn_grads(const pm_dqn* d, void* stream) { return dqn_entry(DQN_GRADS, d, false, nullptr, nullptr, stream); }
extern "C" int pm_dqn_apply(const pm_dqn* d, void* stream) { return dqn_entry(DQN_APPLY, d, false, nullptr, nullptr, stream); }
extern "C" int pm_dqn_update(const pm_dqn* d, void* stream) { return dqn_entry(DQN_UPDATE, d, false, nullptr, nullptr, stream); }

extern "C" int pm_dqn_grads_opt(const pm_dqn* d, const pm_dqn_opt* o, void* stream) {
    return dqn_entry(DQN_GRADS, d, true, o, nullptr, stream);
}
extern "C" int pm_dqn_apply_opt(const pm_dqn* d, const pm_dqn_opt* o, void* stream) {
    return dqn_entry(DQN_APPLY, d, true, o, nullptr, stream);
}
extern "C" int pm_dqn_update_opt(const pm_dqn* d, const pm_dqn_opt* o, void* stream) {
    return dqn_entry(DQN_UPDATE, d, true, o, nullptr, stream);
}

extern "C" int pm_dqn_grads_n(const pm_dqn* d, const pm_dqn_opt* o, const pm_dqn_nstep* ns, void* stream) {
    return dqn_entry(DQN_GRADS, d, true, o, ns, stream);
}
extern "C" int pm_dqn_update_n(const pm_dqn* d, const pm_dqn_opt* o, const pm_dqn_nstep* ns, void* stream) {
    return dqn_entry(DQN_UPDATE, d, true, o, ns, stream);
}
