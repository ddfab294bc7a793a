// Matchmaking on the league's results: who a member trains against next, and a rating of every player, both from
// pair_stats as pm_league_reduce left them, on the stream, with no host read.
//
//   k_lg_match  one workgroup per member p: wave 0 weighs every entry of p's pair list by how p did against the
//               opponent it names (prioritised fictitious self-play), draws one entry by Philox, and after a barrier
//               all 256 threads copy the opponent's folded net into row p of the table the collector plays from.
//   k_lg_rate   one workgroup: Bradley-Terry strengths by Jacobi steps of the MM update, the strengths double-buffered
//               in LDS.
//
// The exactness contract (pongmi/matchmaking.py restates both kernels in numpy; this unit builds with
// -ffp-contract=off and uses + - * / and conversions only):
//
//   k_lg_match  entry e = 2 * pair + side of p's list names the opponent o = pair_players[pair][1 - side]; it is
//     eligible iff 0 <= pair < n_pairs, 0 <= o < n_players, o != p and 0 <= net_of[o] < n_nets. With g = games and
//     s = 2 * wins of p's side + draws of the pair: x = g == 0 ? 0.5f : (float)s / (float)(2 * g);
//     HARD: f = 1.0f, then `power` times f = f * (1.0f - x); EVEN: f = (4.0f * x) * (1.0f - x);
//     q = (uint32_t)(f * 65535.0f) + 1 for an eligible entry, 0 otherwise. The prefix sums are int32 sums (a list of
//     at most PM_LEAGUE_MATCH_MAX entries: the kernel looks at no entry past that), so their order does not matter.
//     total = the sum of q; t = (r.x * total) >> 32 with r = Philox(seed), counter (p, purpose MATCH, round); the
//     pick is the first entry in list order whose inclusive prefix exceeds t.
//
//   k_lg_rate   an entry of q's list counts iff 0 <= pair < n_pairs, 0 <= o < n_players, o != q and g > 0.
//     S_q = the int64 sum of s over them, W_q = 0.5f * (float)S_q + 0.5f * prior. One wave per player. In every
//     step lane l starts from acc = 0.0f and adds, for the entries at list positions l, l + 64, l + 128, ... in
//     that order, acc = acc + (float)g / (r_q + r_o) (an entry that does not count adds nothing). The 64 lane sums
//     combine as pm_dev.h's wave_sum does: a[i] + a[i ^ 1], then + the value 2 lanes away, 4 away, 8 away (a
//     pairwise tree over adjacent blocks of 2, 4, 8, 16 lanes), then (row 0 + row 1) + (row 2 + row 3). Then
//     D_q = prior / (r_q + 1.0f) + that sum and r'_q = W_q / D_q; every r' of a step is computed from the r of the
//     step before (Jacobi). r starts at 1.0f.
//
// No input VALUE makes either kernel read or write outside its buffers: an entry is range-checked before it is used
// as an index, and so are the opponent and its net. player_off is structure, as for k_lg_players: it must describe
// player_pairs.
#include "pm_dev.h"
#include "pm_host.h"

using namespace pm;

namespace {

constexpr int kMatchBlock = 256;
constexpr int kRowVecs = PM_QNET_NW / 4;  // 2 486 16-byte vectors
constexpr int kRateBlock = 1024;
constexpr int kRateWaves = kRateBlock / 64;
static_assert(PM_QNET_NW % 4 == 0, "a weight row is whole 16-byte vectors");
static_assert((long long)PM_LEAGUE_MATCH_MAX * 65536 <= 2147483647LL, "a member's weights sum within int32");

// The weight of list entry `entry` of member p (0 = not eligible) and the opponent it names.
__device__ __forceinline__ int match_weight(int entry, int p, const int64_t* __restrict__ pair_stats,
                                            const int32_t* __restrict__ pair_players, int n_pairs, int n_players,
                                            const int32_t* __restrict__ net_of, int n_nets, int mode, int power,
                                            int& opp) {
    opp = -1;
    const int pair = entry >> 1, side = entry & 1;
    if (pair < 0 || pair >= n_pairs) return 0;
    const int o = pair_players[(size_t)pair * 2 + (1 - side)];
    if (o < 0 || o >= n_players || o == p) return 0;
    const int net = net_of[o];
    if (net < 0 || net >= n_nets) return 0;
    const int64_t* ps = pair_stats + (size_t)pair * PM_LEAGUE_STATS;
    const long long g = ps[0], s = 2 * ps[1 + side] + ps[3];
    const float x = g == 0 ? 0.5f : (float)s / (float)(2 * g);
    float f;
    if (mode == PM_MATCH_HARD) {
        f = 1.0f;
        for (int k = 0; k < power; ++k) f = f * (1.0f - x);
    } else {
        f = (4.0f * x) * (1.0f - x);
    }
    opp = o;
    return (int)((uint32_t)(f * 65535.0f) + 1u);
}

__global__ __launch_bounds__(kMatchBlock) void k_lg_match(
    const int64_t* __restrict__ pair_stats, const int32_t* __restrict__ pair_players, int n_pairs,
    const int32_t* __restrict__ player_off, const int32_t* __restrict__ player_pairs, int n_players,
    const int32_t* __restrict__ net_of, const float* __restrict__ w, int n_nets, int mode, int power, uint64_t seed,
    uint64_t round, float* __restrict__ wA_out, int32_t* __restrict__ opp, int32_t* __restrict__ total) {
    __shared__ int src_net;
    const int p = blockIdx.x;
    if (threadIdx.x < 64) {  // wave 0, whole: the DPP scan below needs every lane
        const int lane = threadIdx.x;
        const int lo = player_off[p];
        const int len = min(max(player_off[p + 1] - lo, 0), PM_LEAGUE_MATCH_MAX);
        int sum = 0;
        for (int base = 0; base < len; base += 64) {
            int o = -1;
            const int q = base + lane < len ? match_weight(player_pairs[lo + base + lane], p, pair_stats, pair_players,
                                                           n_pairs, n_players, net_of, n_nets, mode, power, o)
                                            : 0;
            sum += lane_i32(wave_incl_scan_i32(q), 63);
        }
        int pick = -1;
        if (sum > 0) {
            const U4 d = philox64((uint32_t)p, TAG_MATCH, round, seed);
            const int t = below(d.x, (uint32_t)sum);
            int carry = 0;
            for (int base = 0; base < len; base += 64) {
                int o = -1;
                const int q = base + lane < len ? match_weight(player_pairs[lo + base + lane], p, pair_stats,
                                                               pair_players, n_pairs, n_players, net_of, n_nets, mode,
                                                               power, o)
                                                : 0;
                const int incl = carry + wave_incl_scan_i32(q);
                const unsigned long long hit = __ballot(q > 0 && incl > t);
                if (hit) {  // wave-uniform
                    pick = __shfl(o, __ffsll((long long)hit) - 1);
                    break;
                }
                carry = lane_i32(incl, 63);
            }
        }
        if (lane == 0) {
            opp[p] = pick;
            total[p] = sum;
            src_net = pick >= 0 ? net_of[pick] : -1;  // an eligible entry's opponent: its net is in [0, n_nets)
        }
    }
    __syncthreads();
    const int net = src_net;
    if (net < 0) return;  // nobody to draw: the row stays as it is
    const float4* __restrict__ src = reinterpret_cast<const float4*>(w + (size_t)net * PM_QNET_NW);
    float4* __restrict__ dst = reinterpret_cast<float4*>(wA_out + (size_t)p * PM_QNET_NW);
    for (int i = threadIdx.x; i < kRowVecs; i += kMatchBlock) dst[i] = src[i];
}

__global__ __launch_bounds__(kRateBlock) void k_lg_rate(const int64_t* __restrict__ pair_stats,
                                                         const int32_t* __restrict__ pair_players, int n_pairs,
                                                         const int32_t* __restrict__ player_off,
                                                         const int32_t* __restrict__ player_pairs, int n_players,
                                                         int iterations, float prior, float* __restrict__ rating) {
    __shared__ float r[2][PM_LEAGUE_RATE_MAX];
    __shared__ float W[PM_LEAGUE_RATE_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q = threadIdx.x; q < n_players; q += kRateBlock) r[0][q] = 1.0f;
    for (int q = wv; q < n_players; q += kRateWaves) {  // wave-uniform
        const int lo = player_off[q], hi = player_off[q + 1];
        long long S = 0;
        for (int e = lo + lane; e < hi; e += 64) {
            const int entry = player_pairs[e];
            const int pair = entry >> 1, side = entry & 1;
            if (pair < 0 || pair >= n_pairs) continue;
            const int o = pair_players[(size_t)pair * 2 + (1 - side)];
            if (o < 0 || o >= n_players || o == q) continue;
            const int64_t* ps = pair_stats + (size_t)pair * PM_LEAGUE_STATS;
            if (ps[0] <= 0) continue;
            S += 2 * ps[1 + side] + ps[3];
        }
        S = wave_sum(S);
        if (lane == 0) W[q] = 0.5f * (float)S + 0.5f * prior;
    }
    __syncthreads();
    int cur = 0;
    for (int it = 0; it < iterations; ++it) {
        for (int q = wv; q < n_players; q += kRateWaves) {
            const int lo = player_off[q], hi = player_off[q + 1];
            const float rq = r[cur][q];  // one address per wave: an LDS broadcast
            float acc = 0.0f;
#pragma unroll 4
            for (int e = lo + lane; e < hi; e += 64) {
                const int entry = player_pairs[e];
                const int pair = entry >> 1, side = entry & 1;
                if (pair < 0 || pair >= n_pairs) continue;
                const int o = pair_players[(size_t)pair * 2 + (1 - side)];
                if (o < 0 || o >= n_players || o == q) continue;
                const long long g = pair_stats[(size_t)pair * PM_LEAGUE_STATS];
                if (g <= 0) continue;
                acc = acc + (float)g / (rq + r[cur][o]);
            }
            const float sum = wave_sum(acc);
            if (lane == 0) r[cur ^ 1][q] = W[q] / (prior / (rq + 1.0f) + sum);
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int q = threadIdx.x; q < n_players; q += kRateBlock) rating[q] = r[cur][q];
}

bool aligned(const void* ptr, size_t a) { return ((uintptr_t)ptr & (a - 1)) == 0; }

}  // namespace

extern "C" int pm_league_match(const int64_t* pair_stats, const int32_t* pair_players, int32_t n_pairs,
                               const int32_t* player_off, const int32_t* player_pairs, int32_t n_players,
                               const int32_t* net_of, const float* w, int32_t n_nets, int32_t n, int32_t mode,
                               int32_t power, uint64_t seed, uint64_t round, float* wA_out, int32_t* opp,
                               int32_t* total, void* stream) {
    PM_REQUIRE(n >= 1 && n <= PM_DQN_POP_MAX && n_players >= n && n_pairs >= 0 && n_nets >= 1, PM_E_SIZE,
               "pm_league_match: n=%d (1..%d) n_players=%d (>= n) n_pairs=%d (>= 0) n_nets=%d (>= 1)", n,
               PM_DQN_POP_MAX, n_players, n_pairs, n_nets);
    PM_REQUIRE(mode == PM_MATCH_HARD || mode == PM_MATCH_EVEN, PM_E_SIZE, "pm_league_match: mode=%d (PM_MATCH_HARD, "
               "PM_MATCH_EVEN)", mode);
    PM_REQUIRE(power >= 0 && power <= PM_MATCH_POWER_MAX, PM_E_SIZE, "pm_league_match: power=%d (0..%d)", power,
               PM_MATCH_POWER_MAX);
    PM_REQUIRE(player_off && net_of && w && wA_out && opp && total, PM_E_ARG, "pm_league_match: null buffer");
    PM_REQUIRE(n_pairs == 0 || (pair_stats && pair_players && player_pairs), PM_E_ARG,
               "pm_league_match: null buffer with n_pairs=%d", n_pairs);
    PM_REQUIRE(aligned(w, 16) && aligned(wA_out, 16), PM_E_ARG, "pm_league_match: w and wA_out must be 16-byte aligned");
    PM_REQUIRE(aligned(pair_stats, 8) && aligned(pair_players, 4) && aligned(player_off, 4) && aligned(player_pairs, 4) &&
                   aligned(net_of, 4) && aligned(opp, 4) && aligned(total, 4),
               PM_E_ARG, "pm_league_match: a misaligned buffer");
    const uintptr_t w0 = (uintptr_t)w, w1 = w0 + (size_t)n_nets * PM_QNET_NW * sizeof(float);
    const uintptr_t o0 = (uintptr_t)wA_out, o1 = o0 + (size_t)n * PM_QNET_NW * sizeof(float);
    PM_REQUIRE(o1 <= w0 || w1 <= o0, PM_E_ARG, "pm_league_match: wA_out overlaps w");
    hipLaunchKernelGGL(k_lg_match, dim3(n), dim3(kMatchBlock), 0, pm_stream(stream), pair_stats, pair_players, n_pairs,
                       player_off, player_pairs, n_players, net_of, w, n_nets, mode, power, seed, round, wA_out, opp,
                       total);
    PM_LAUNCHED("k_lg_match");
    return PM_OK;
}

extern "C" int pm_league_rate(const int64_t* pair_stats, const int32_t* pair_players, int32_t n_pairs,
                              const int32_t* player_off, const int32_t* player_pairs, int32_t n_players,
                              int32_t iterations, float prior, float* rating, void* stream) {
    PM_REQUIRE(n_players >= 0 && n_players <= PM_LEAGUE_RATE_MAX && n_pairs >= 0 && iterations >= 0 &&
                   iterations <= PM_LEAGUE_RATE_ITER_MAX,
               PM_E_SIZE, "pm_league_rate: n_players=%d (0..%d) n_pairs=%d (>= 0) iterations=%d (0..%d)", n_players,
               PM_LEAGUE_RATE_MAX, n_pairs, iterations, PM_LEAGUE_RATE_ITER_MAX);
    PM_REQUIRE(prior > 0.0f && prior <= 3.0e38f, PM_E_ARG, "pm_league_rate: prior=%g (positive and finite)",
               (double)prior);
    if (n_players == 0) return PM_OK;
    PM_REQUIRE(player_off && rating, PM_E_ARG, "pm_league_rate: null buffer");
    PM_REQUIRE(n_pairs == 0 || (pair_stats && pair_players && player_pairs), PM_E_ARG,
               "pm_league_rate: null buffer with n_pairs=%d", n_pairs);
    PM_REQUIRE(aligned(pair_stats, 8) && aligned(pair_players, 4) && aligned(player_off, 4) && aligned(player_pairs, 4) &&
                   aligned(rating, 4),
               PM_E_ARG, "pm_league_rate: a misaligned buffer");
    hipLaunchKernelGGL(k_lg_rate, dim3(1), dim3(kRateBlock), 0, pm_stream(stream), pair_stats, pair_players, n_pairs,
                       player_off, player_pairs, n_players, iterations, prior, rating);
    PM_LAUNCHED("k_lg_rate");
    return PM_OK;
}
