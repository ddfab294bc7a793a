// The league: a population's fitness from greedy matches and the PBT source selection, all on the stream.
//
// pm_play (pm_play.hip) plays the matches; this unit is what stands around it so that no step of
// "who is winning, and who copies whom" touches the host:
//
//   k_lg_serves   serves[s] = the production serve (pm_dev.h philox_serve, TAG_SERVE) of index serve_idx[s]
//                 with serve count `round`: what k_play stages, in slot order, drawn where it is consumed.
//   k_lg_pairs    one workgroup per pair: its arenas' results summed into 8 int64.
//   k_lg_players  one wave per player: its pairs' sums with the sides resolved, and the win rate.
//   k_pbt_select  one workgroup: rank by fitness (ties by index, NaN last), a Philox draw per member, and for the
//                 bottom members a source among the top ones.
//
// Every sum is an integer sum, there is no atomic, and no workgroup waits for another: the results are pure
// functions of the inputs.
#include "pm_dev.h"
#include "pm_host.h"

using namespace pm;

namespace {

constexpr int kServeBlock = 256;
constexpr int kPairBlock = 256;
constexpr int kSelectBlock = PM_DQN_POP_MAX;  // one thread per member

__global__ __launch_bounds__(kServeBlock) void k_lg_serves(const pm_env_params p, const int32_t* __restrict__ serve_idx,
                                                            uint64_t seed, uint32_t round, double* __restrict__ serves,
                                                            int m) {
    const int s = blockIdx.x * kServeBlock + threadIdx.x;
    if (s >= m) return;
    double vx, vy, spin;
    philox_serve(p, (uint32_t)serve_idx[s], round, seed, vx, vy, spin);
    serves[(size_t)s * 3 + 0] = vx;
    serves[(size_t)s * 3 + 1] = vy;
    serves[(size_t)s * 3 + 2] = spin;
}

// pair_stats[k] = games, wins_A, wins_B, draws, points_A, points_B, ticks, unfinished over the pair's arenas
__global__ __launch_bounds__(kPairBlock) void k_lg_pairs(const int32_t* __restrict__ scoreA,
                                                          const int32_t* __restrict__ scoreB,
                                                          const int32_t* __restrict__ length,
                                                          const int32_t* __restrict__ pair_first,
                                                          int64_t* __restrict__ pair_stats) {
    __shared__ long long part[kPairBlock / 64][PM_LEAGUE_STATS];
    const int k = blockIdx.x;
    const int lo = pair_first[k], hi = pair_first[k + 1];
    long long v[PM_LEAGUE_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lo + (int)threadIdx.x; i < hi; i += kPairBlock) {
        const int len = length[i];
        if (len < 0) {
            v[7] += 1;
            continue;
        }
        const int a = scoreA[i], b = scoreB[i];
        v[0] += 1;
        v[1] += a > b ? 1 : 0;
        v[2] += b > a ? 1 : 0;
        v[3] += a == b ? 1 : 0;
        v[4] += a;
        v[5] += b;
        v[6] += len;
    }
    // every lane is back here (the loop has no early exit), so the full-wave DPP sums apply
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < PM_LEAGUE_STATS; ++j) {
        const long long s = wave_sum(v[j]);
        if (lane == 0) part[wv][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < PM_LEAGUE_STATS) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < kPairBlock / 64; ++w) s += part[w][threadIdx.x];
        pair_stats[(size_t)k * PM_LEAGUE_STATS + threadIdx.x] = s;
    }
}

// player_stats[q] = games, wins, losses, draws, points_for, points_against, ticks, unfinished; one wave per player
__global__ __launch_bounds__(64) void k_lg_players(const int64_t* __restrict__ pair_stats, int n_pairs,
                                                    const int32_t* __restrict__ player_off,
                                                    const int32_t* __restrict__ player_pairs,
                                                    int64_t* __restrict__ player_stats, float* __restrict__ fitness) {
    const int q = blockIdx.x;
    const int lo = player_off[q], hi = player_off[q + 1];
    long long v[PM_LEAGUE_STATS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = lo + (int)threadIdx.x; e < hi; e += 64) {
        const int entry = player_pairs[e];
        const int pair = entry >> 1, side = entry & 1;
        if (pair < 0 || pair >= n_pairs) continue;  // not a pair of this league: counts nowhere
        const int64_t* ps = pair_stats + (size_t)pair * PM_LEAGUE_STATS;
        v[0] += ps[0];
        v[1] += ps[1 + side];
        v[2] += ps[2 - side];
        v[3] += ps[3];
        v[4] += ps[4 + side];
        v[5] += ps[5 - side];
        v[6] += ps[6];
        v[7] += ps[7];
    }
    long long s[PM_LEAGUE_STATS];
#pragma unroll
    for (int j = 0; j < PM_LEAGUE_STATS; ++j) s[j] = wave_sum(v[j]);
    if (threadIdx.x < PM_LEAGUE_STATS) {
        long long mine = s[0];
#pragma unroll
        for (int j = 1; j < PM_LEAGUE_STATS; ++j) mine = (int)threadIdx.x == j ? s[j] : mine;
        player_stats[(size_t)q * PM_LEAGUE_STATS + threadIdx.x] = mine;
    }
    if (threadIdx.x == 0) fitness[q] = s[0] == 0 ? 0.0f : (float)s[1] / (float)s[0];
}

// Truncation selection. Thread p is member p (threads at or past n only keep the barriers).
__global__ __launch_bounds__(kSelectBlock) void k_pbt_select(const float* __restrict__ fitness, int n, int n_bottom,
                                                              int n_top, uint64_t seed, uint64_t round,
                                                              int32_t* __restrict__ rank, int64_t* __restrict__ src_of,
                                                              uint32_t* __restrict__ draw) {
    __shared__ float f[kSelectBlock];
    __shared__ int who[kSelectBlock];  // the member of each rank
    const int p = threadIdx.x;
    float mine = 0.f;
    if (p < n) {
        mine = fitness[p];
        mine = mine != mine ? -INFINITY : mine;
        f[p] = mine;
    }
    __syncthreads();
    int r = 0;
    if (p < n) {
        for (int a = 0; a < n; ++a) {
            const float fa = f[a];  // one address per wave: an LDS broadcast
            r += (fa > mine || (fa == mine && a < p)) ? 1 : 0;
        }
        who[r] = p;  // a permutation: the order is total
        rank[p] = r;
    }
    __syncthreads();
    if (p < n) {
        const U4 d = philox64((uint32_t)p, TAG_PBT, round, seed);
        draw[p] = d.y;
        src_of[p] = r >= n - n_bottom ? (int64_t)who[below(d.x, (uint32_t)n_top)] : (int64_t)p;
    }
}

}  // namespace

extern "C" int pm_league_serves(const pm_env_params* p, const int32_t* serve_idx, uint64_t seed, uint32_t round,
                                double* serves, int32_t m, void* stream) {
    PM_REQUIRE(m >= 0, PM_E_SIZE, "pm_league_serves: m=%d", m);
    if (m == 0) return PM_OK;
    PM_REQUIRE(p && serve_idx && serves, PM_E_ARG, "pm_league_serves: null buffer");
    PM_REQUIRE(p->speed_scale_every > 0, PM_E_ARG, "pm_league_serves: speed_scale_every must be > 0");
    hipLaunchKernelGGL(k_lg_serves, dim3(pm_blocks(m, kServeBlock)), dim3(kServeBlock), 0, pm_stream(stream), *p,
                       serve_idx, seed, round, serves, m);
    PM_LAUNCHED("k_lg_serves");
    return PM_OK;
}

extern "C" int pm_league_reduce(const int32_t* scoreA, const int32_t* scoreB, const int32_t* length,
                                const int32_t* pair_first, int32_t n_pairs, const int32_t* player_off,
                                const int32_t* player_pairs, int32_t n_players, int64_t* pair_stats,
                                int64_t* player_stats, float* fitness, void* stream) {
    PM_REQUIRE(n_pairs >= 0 && n_players >= 0, PM_E_SIZE, "pm_league_reduce: n_pairs=%d n_players=%d", n_pairs,
               n_players);
    PM_REQUIRE(n_pairs == 0 || (scoreA && scoreB && length && pair_first && pair_stats), PM_E_ARG,
               "pm_league_reduce: null buffer with n_pairs=%d", n_pairs);
    PM_REQUIRE(n_players == 0 || (player_off && player_stats && fitness && (n_pairs == 0 || player_pairs)), PM_E_ARG,
               "pm_league_reduce: null buffer with n_players=%d", n_players);
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_lg_pairs, dim3(n_pairs), dim3(kPairBlock), 0, pm_stream(stream), scoreA, scoreB, length,
                           pair_first, pair_stats);
        PM_LAUNCHED("k_lg_pairs");
    }
    if (n_players > 0) {
        hipLaunchKernelGGL(k_lg_players, dim3(n_players), dim3(64), 0, pm_stream(stream), pair_stats, n_pairs,
                           player_off, player_pairs, player_stats, fitness);
        PM_LAUNCHED("k_lg_players");
    }
    return PM_OK;
}

extern "C" int pm_pbt_select(const float* fitness, int32_t n, int32_t n_bottom, int32_t n_top, uint64_t seed,
                             uint64_t round, int32_t* rank, int64_t* src_of, uint32_t* draw, void* stream) {
    PM_REQUIRE(n >= 1 && n <= PM_DQN_POP_MAX && n_bottom >= 0 && n_top >= 1 && (int64_t)n_bottom + n_top <= n, PM_E_SIZE,
               "pm_pbt_select: n=%d (1..%d) n_bottom=%d n_top=%d (n_bottom >= 0, n_top >= 1, their sum <= n)", n,
               PM_DQN_POP_MAX, n_bottom, n_top);
    PM_REQUIRE(fitness && rank && src_of && draw, PM_E_ARG, "pm_pbt_select: null buffer");
    hipLaunchKernelGGL(k_pbt_select, dim3(1), dim3(kSelectBlock), 0, pm_stream(stream), fitness, n, n_bottom, n_top,
                       seed, round, rank, src_of, draw);
    PM_LAUNCHED("k_pbt_select");
    return PM_OK;
}
