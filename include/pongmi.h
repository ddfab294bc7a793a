/*
 * pongmi.h — C-ABI of libpongmi.so, the MI355X (gfx950) hot path of pingpong-selfplay-ai:
 * batched PongEnv2P rollout (SoA fp64 arenas), fused two-player QNet acting, device replay +
 * prioritized sampling, and the double-DQN head update.
 *
 * The reference (MaxChen228/pingpong-selfplay-ai) is pure Python and has no FFI; every entry point
 * below replaces a Python function on its hot path, cited as reference file:line. The Python
 * mirror of the reference API (pingpong-selfplay-ai_amd/{envs,models,scripts}) binds these with
 * ctypes.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer owned by the caller (e.g. a torch tensor's
 *    data_ptr()); the library never allocates or frees caller memory. Parameter structs
 *    (pm_env_params, pm_env_state, pm_selfplay) are HOST structs passed by pointer and copied
 *    into the launch; the pointers inside them are device pointers.
 *  - Every call is asynchronous on `stream` (a hipStream_t; NULL = the null stream) and never
 *    synchronizes the host, so a caller may capture calls into a hipGraph.
 *  - Return 0 on success, a negative PM_E* code on an argument error, or a positive hipError_t
 *    if a launch failed. pm_last_error() returns a thread-local message for the last failure.
 *  - Randomness is Philox4x32-10, keyed by a 64-bit seed, countered by (index, purpose, step):
 *    results depend only on (seed, counters), never on launch geometry.
 */
#ifndef PONGMI_H
#define PONGMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_ABI_VERSION 27

#define PM_OK 0
#define PM_E_ARG (-1)     /* null / inconsistent argument */
#define PM_E_SIZE (-2)    /* size outside the supported range */
#define PM_E_LAUNCH (-3)  /* launch failed (see pm_last_error) */
#define PM_E_COMM (-4)    /* RCCL binding / communicator failure (see pm_last_error) */

/* ---------------------------------------------------------------- environment (K1) */

/* PongEnv2P constructor parameters (envs/my_pong_env_2p.py:19-81). The last six doubles are
 * derived constants the HOST computes with the reference's own Python expressions so the device
 * reproduces them bit for bit:
 *   half_width   = paddle_width/2                     (:152,190)
 *   speed_scale  = 1.0 + speed_increment              (:230)
 *   inertia      = (2/5) * ball_mass * radius**2      (envs/physics.py:9)
 *   jt_coef      = 2*ball_mass/7.0                    (envs/physics.py:10)
 *   inv_mass     = 1.0/ball_mass, inv_inertia = 1.0/inertia (correctly rounded reciprocals: the
 *                  device divides by ball_mass and inertia as q = a*inv; q + fma(-q, b, a)*inv,
 *                  which is the correctly rounded a/b, the quotient physics.py:20-21 computes)  */
typedef struct pm_env_params {
    double paddle_width, paddle_speed, magnus_factor, restitution, friction, ball_mass, radius;
    double speed_lo, speed_hi, spin_lo, spin_hi;
    double ang0_lo, ang0_hi, ang1_lo, ang1_hi;
    double half_width, speed_scale, inertia, jt_coef, inv_mass, inv_inertia;
    int32_t max_score, speed_scale_every, enable_spin, _pad;
} pm_env_params;

/* Struct-of-arrays arena state, [n] each (PongEnv2P attributes ball_x, ball_y, ball_vx, ball_vy,
 * spin, top_paddle_x, bottom_paddle_x, scoreA, scoreB, bounce_count). `serves` counts the resets
 * an arena has consumed: it indexes the injected serve table / the Philox serve stream. */
typedef struct pm_env_state {
    double *x, *y, *vx, *vy, *spin, *top, *bot;
    int32_t *scoreA, *scoreB, *bounces, *serves;
} pm_env_state;

/* PongEnv2P.reset (envs/my_pong_env_2p.py:83-114) for every arena with mask[i] != 0 (mask NULL =
 * all). Serve (vx, vy, spin) comes from `inject` when non-NULL — layout [n][inject_cap][3],
 * entry serves[i] mod inject_cap (parity mode: the host draws it with CPython's `random` exactly
 * as the reference does) — else from Philox(seed) with counter (i, serves[i]) (production mode:
 * speed~U(speed_lo,speed_hi), angle~U(ang0) or U(ang1) by a fair coin, spin~U(spin_lo,spin_hi)).
 * serves[i] is incremented. Writes obsA/obsB [n][7] (may be NULL). `status` (nullable, device
 * int32) is reserved for error bits. */
int pm_env_reset(const pm_env_params* p, const pm_env_state* s, const uint8_t* mask, const double* inject,
                 int32_t inject_cap, uint64_t seed, float* obsA, float* obsB, int32_t* status, int32_t n,
                 void* stream);

/* PongEnv2P.step (envs/my_pong_env_2p.py:116-225, physics.py:3-23, _maybe_scale_speed :227-232,
 * _get_obs :235-263) for n arenas: aA/aB [n] in {0,1,2}; writes obsA/obsB [n][7], rA/rB [n]
 * (values -1/0/+1), done [n]. With autoreset != 0, done arenas are then reset as pm_env_reset
 * (inject / seed as above); obsA/obsB then hold the post-reset observation, and term_obsA /
 * term_obsB (nullable, both or neither) the observation returned by the terminal step (the `nB`
 * the reference stores in replay, scripts/train_iterative.py:242-243):
 *   autoreset 1: every term row is written (the step's pre-reset observation of every arena);
 *   autoreset 2: only the rows of arenas with done[i] != 0 are written, the others keep their
 *                contents (next state for replay = done ? term_obs : obs; SURVEY.md §8d's 203 B
 *                per env-step). With autoreset 0 the term rows, if given, equal obs.
 * Serves of done arenas (ABI 15): with `inject` as pm_env_reset (serves[i] indexes the table and is
 * incremented); in production (inject NULL) from Philox(seed) keyed by (i, counter) — `counter` is
 * the caller's env-step count (PongEnv2PBatch passes its own) — so the draw needs nothing from
 * memory and overlaps the state loads; serves[i] is then neither read nor written. */
int pm_env_step(const pm_env_params* p, const pm_env_state* s, const int8_t* aA, const int8_t* aB, float* obsA,
                float* obsB, float* rA, float* rB, uint8_t* done, float* term_obsA, float* term_obsB,
                int32_t autoreset, const double* inject, int32_t inject_cap, uint64_t seed, uint64_t counter,
                int32_t* status, int32_t n, void* stream);

/* collide_sphere_with_moving_plane (envs/physics.py:3-23) over n rows: in [n][8] =
 * (vn, vt, u, omega, e, mu, m, R) fp64, with I = (2/5)*m*R**2 supplied per row in inertia[n]
 * (CPython's value); out [n][3] = (vn', vt', omega'). A test/diagnostic entry point. */
int pm_collide(const double* in, const double* inertia, double* out, int32_t n, void* stream);

/* The scalar drop-ins' fast path (ABI 23): one launch per call, no copy, no stream synchronisation.
 * `out` is device-visible memory, normally a host-mapped buffer (pm_host_mapped_alloc) the host
 * polls: the kernel writes its results, then `seq` into the 32-bit word after them with a
 * system-scope release.
 *   pm_env_step1  PongEnv2P.step (envs/my_pong_env_2p.py:116-225) of arena 0 of `s` with actions
 *                 (aA, aB), no autoreset: out = obsA[7] obsB[7] rA rB done (f32), seq at word 17.
 *                 Same tick as pm_env_step at n = 1, bit for bit.
 *   pm_env_reset1 PongEnv2P.reset (:83-114) of arena 0 with the host-drawn serve (vx, vy, spin);
 *                 serves[0] incremented: out = obsA[7] obsB[7] 0 0 0, seq at word 17.
 *   pm_collide1   collide_sphere_with_moving_plane (envs/physics.py:3-23) of one row (vn, vt, u,
 *                 omega, e, mu, m, R) with I = inertia: out = (vn', vt', omega') fp64, seq at word 6. */
int pm_env_step1(const pm_env_params* p, const pm_env_state* s, int32_t aA, int32_t aB, float* out, uint32_t seq,
                 void* stream);
int pm_env_reset1(const pm_env_state* s, double vx, double vy, double spin, float* out, uint32_t seq, void* stream);
int pm_collide1(const double* row, double inertia, double* out, uint32_t seq, void* stream);
/* Pinned host memory the device reads and writes directly (hipHostMalloc, mapped + coherent):
 * returns the host pointer (NULL on failure), *dev the device address of the same bytes. */
void* pm_host_mapped_alloc(int64_t bytes, void** dev);
int pm_host_mapped_free(void* host);

/* ---------------------------------------------------------------- QNet (K2) */

/* Packed QNet parameter block (models/qnet.py:52-69), PM_QNET_NP floats, in this order:
 *   features.0.weight [64,7] | features.0.bias [64] | features.2.weight [64,64] | features.2.bias [64]
 *   fc_V.{weight_mu [1,64], bias_mu [1], weight_sigma [1,64], bias_sigma [1]}
 *   fc_A.{weight_mu [3,64], bias_mu [3], weight_sigma [3,64], bias_sigma [3]}      (the 520 "heads",
 *        in the order train_iterative.py:101-104 hands them to Adam)
 *   fc_V.{weight_epsilon [1,64], bias_epsilon [1]} | fc_A.{weight_epsilon [3,64], bias_epsilon [3]}
 * Effective (folded) weights, PM_QNET_NW floats: the plain part W1 [64,7] | b1 [64] | W2 [64,64] |
 *   b2 [64] | Wh [4,64] (row 0 = V, rows 1..3 = A) | bh [4] (4932 floats, padded to 4936), then the
 *   same weights re-ordered into MFMA operand fragments (5008 floats) for the matrix-core forward.
 *   Produce it with pm_qnet_fold; treat the fragment part as opaque. */
#define PM_QNET_NP 5452
#define PM_QNET_NHEAD 520
#define PM_QNET_HEAD_OFF 4672
#define PM_QNET_EPS_OFF 5192
#define PM_QNET_NW 9944
/* The learner's packed exchange buffer sp->grad (float32, PM_GRAD_LEN), the one thing a sharded
 * update all-reduces (SUM): the 520 head gradients of this shard's batch, then the episodes this
 * shard finished in the vector step (update 0 only) and the "an update ran" flag (1 per shard, so
 * the sum counts the ranks that trained). Every rank then applies Adam to grads / world and decays
 * epsilon by the summed episode count. */
#define PM_GRAD_EPISODES 520
#define PM_GRAD_UPDATED 521
#define PM_GRAD_LEN 528

#define PM_FOLD_EVAL 0        /* NoisyLinear eval mode: W = mu                          (qnet.py:47-49) */
#define PM_FOLD_TRAIN 1       /* train mode with the block's epsilon buffers: mu+sigma*eps (qnet.py:44-46) */
#define PM_FOLD_TRAIN_FRESH 2 /* reset_noise() then train mode (qnet.py:33-41): fresh factorised
                                 Gaussian noise from Philox(seed, counter); written back into the
                                 block's epsilon slots when params_out != NULL                   */

/* Fold `count` parameter blocks [count][PM_QNET_NP] into effective weights [count][PM_QNET_NW].
 * counter_dev (nullable, device uint64) is added to `counter` so a captured graph advances it. */
int pm_qnet_fold(const float* params, float* params_out, int32_t mode, uint64_t seed, uint64_t counter,
                 const uint64_t* counter_dev, float* w_eff, int32_t count, void* stream);

/* QNet.forward (models/qnet.py:71-75) on effective weights: x [n][7] -> q [n][3]. */
int pm_qnet_q(const float* w_eff, const float* x, float* q, int32_t n, void* stream);

/* Both players' action selection for n arenas (fused, matrix cores):
 *   A: argmax_a Q_opp(obsA) with opponent weights w_opp[opp_id[i]] (opp_id NULL = net 0)
 *      (scripts/train_iterative.py:240; tests/arena.py:294-320)
 *   B: random.random() < epsilon ? randint(0,2) : argmax_a Q_B(obsB)          (train_iterative.py:124-130)
 * argmax keeps the first maximal index (torch). epsilon is *eps_dev when eps_dev != NULL.
 * qA/qB [n][3] nullable. Philox counter for the epsilon draws: (i, counter + *counter_dev).
 * Rows are grouped by opponent net: net 0 is gathered per chunk0 arenas, nets >= 1 per chunk1
 * arenas (0 = defaults 256 / 4096; at most 4096); choose each so a chunk holds >= ~64 of its rows. */
int pm_qnet_act(const float* w_opp, const int32_t* opp_id, int32_t n_opp, const float* w_B, const float* obsA,
                const float* obsB, float epsilon, const double* eps_dev, uint64_t seed, uint64_t counter,
                const uint64_t* counter_dev, int8_t* aA, int8_t* aB, float* qA, float* qB, int32_t n,
                int32_t chunk0, int32_t chunk1, void* stream);

/* K8 — whole greedy matches in one launch (the match megakernel, csrc/pm_play.hip). Replaces the
 * per-episode loops of scripts/train_iterative.py:171-196 (eval_vs_model / eval_vs_pool),
 * tests/test_round_robin.py:290-330 and tests/arena.py:294-320 for QNet and ball-follower players.
 * Every arena resets with its serve (vx, vy, spin) and plays until a score reaches max_score, both
 * players greedy (argmax, first max) on effective weights w_nets[net] (PM_QNET_NW floats each,
 * 16-B aligned; net -1 = HardcodedBallFollower). Work is given as slots: order[s] = arena of slot
 * s, serves[s] = its serve ([m][3] f64, slot order). Block b plays slots
 * [blk_range[2b], blk_range[2b] + blk_range[2b+1]) (at most 1024 slots) with nets
 * (blk_nets[2b], blk_nets[2b+1]) for (A, B), 128 at a time, a finished slot's column taking the
 * next one. max_steps bounds the ticks of each wave over all its slots. Outputs per arena: final
 * scores, length and last[i] = sign(rB - rA) of the final tick; arenas not finished keep the
 * caller's length (initialise it to -1). *status (device, zeroed by the caller) counts invalid net /
 * arena ids, invalid ranges and episodes cut by max_steps. All pointers except p are device
 * pointers. */
int pm_play(const pm_env_params* p, const float* w_nets, int32_t n_nets, const int32_t* blk_nets,
            const int32_t* blk_range, int32_t n_blocks, const int32_t* order, const double* serves, int32_t n,
            int32_t max_steps, int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
            void* stream);

/* K8 for QNetRNN players (csrc/pm_playrnn.hip): pm_play's whole-episode launch for pairs in which at
 * least one side is a QNetRNN (tests/test_round_robin.py:290-330, tests/arena.py:294-320 and the
 * evaluators of scripts/train_rnn_iterative.py). Slots, ranges, serves, outputs and *status are
 * pm_play's. Player ids in blk_nets: >= 0 QNet w_qnet[id] (PM_QNET_NW floats each), -1
 * HardcodedBallFollower, <= -2 QNetRNN w_rnn[-2 - id] (PM_RNN_NW floats each, pm_rnn_fold); both
 * weight arrays 16-B aligned. A block whose pair has no QNetRNN side, or an id out of range, plays
 * nothing and adds to *status. Every episode starts from a zero (h, c) (init_hidden); the states
 * live in hc_scratch (device, 16-B aligned, pm_play_rnn_scratch_bytes(n_blocks) bytes, contents
 * irrelevant on entry). max_steps bounds the ticks of each block over all its slots. */
int pm_play_rnn(const pm_env_params* p, const float* w_qnet, int32_t n_qnet, const float* w_rnn, int32_t n_rnn,
                const int32_t* blk_nets, const int32_t* blk_range, int32_t n_blocks, const int32_t* order,
                const double* serves, int32_t n, int32_t max_steps, float* hc_scratch,
                int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status, void* stream);
size_t pm_play_rnn_scratch_bytes(int32_t n_blocks);

/* K8 with tick records: pm_play / pm_play_rnn (same arguments, same results) that also store every
 * tick of chosen arenas, so a match can be watched or checked tick by tick after the launch.
 * rec_row[i] (device, [n]) is arena i's record row in [0, n_rec), or -1 for an arena that is not
 * recorded (an entry outside [-1, n_rec) records nothing and adds to *status; two arenas must not
 * share a row). Row r holds rec_cap ticks; tick t (0 = the first step after the serve) of row r is
 *   rec_f64[r][t][7]    x, y, vx, vy, spin, top paddle x, bottom paddle x after the tick
 *                       (pm_env_state's field order),
 *   rec_q[r][t][2][3]   the q values player A's and player B's argmax consumed on this tick
 *                       (quiet NaNs for a HardcodedBallFollower side),
 *   rec_i32[r][t][5]    action A, action B, scoreA, scoreB and the bounce count after the tick.
 * Ticks at or beyond rec_cap are not stored (length[] still reports the full length), and entries
 * past an episode's length keep the caller's contents. The buffers are device memory of n_rec *
 * rec_cap ticks each. n_rec < 0, or rec_cap <= 0 with n_rec > 0, is PM_E_SIZE; a null record buffer
 * with n_rec > 0 is PM_E_ARG; n_rec == 0 launches the plain kernel. */
int pm_play_rec(const pm_env_params* p, const float* w_nets, int32_t n_nets, const int32_t* blk_nets,
                const int32_t* blk_range, int32_t n_blocks, const int32_t* order, const double* serves, int32_t n,
                int32_t max_steps, int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
                const int32_t* rec_row, int32_t n_rec, int32_t rec_cap, double* rec_f64, float* rec_q,
                int32_t* rec_i32, void* stream);
int pm_play_rnn_rec(const pm_env_params* p, const float* w_qnet, int32_t n_qnet, const float* w_rnn, int32_t n_rnn,
                    const int32_t* blk_nets, const int32_t* blk_range, int32_t n_blocks, const int32_t* order,
                    const double* serves, int32_t n, int32_t max_steps, float* hc_scratch,
                    int32_t* scoreA, int32_t* scoreB, int32_t* length, int8_t* last, int32_t* status,
                    const int32_t* rec_row, int32_t n_rec, int32_t rec_cap, double* rec_f64, float* rec_q,
                    int32_t* rec_i32, void* stream);

/* The league (csrc/pm_league.hip; additive to ABI 27: pm_sizeof unchanged, no struct): what stands around
 * pm_play so that a population's fitness by greedy matches (the reference's eval_vs_model / eval_vs_pool,
 * scripts/train_iterative.py:171-196, and its round-robin, tests/test_round_robin.py:290-330) and the
 * truncation selection of population-based training are computed on the stream, with no host read. Every array
 * is a caller-owned device pointer; every call only enqueues; arguments are checked on the host before the first
 * HIP call. Integer sums only, no atomic, no workgroup waits for another.
 *
 *   pm_league_serves  serves[s] = the production serve of pm_env_reset (Philox(seed), counter (serve_idx[s],
 *     round): speed, angle interval, angle, spin) for slots s in [0, m): bit for bit what pm_env_reset draws for
 *     arena serve_idx[s] whose serve count is `round`. serves is [m][3] (vx, vy, spin) in slot order, as pm_play
 *     takes it. m == 0 is a no-op. PM_E_SIZE: m < 0; PM_E_ARG: a null pointer, p->speed_scale_every <= 0.
 *
 *   pm_league_reduce  two launches, grid n_pairs then grid n_players. Pair k owns arenas [pair_first[k],
 *     pair_first[k + 1]) of pm_play's per-arena outputs (pair_first holds n_pairs + 1 entries);
 *     pair_stats[k][PM_LEAGUE_STATS] = games, wins_A, wins_B, draws, points_A, points_B, ticks, unfinished: an
 *     arena with length < 0 counts in `unfinished` only; otherwise A wins when scoreA > scoreB, B when scoreB >
 *     scoreA, else it is a draw, and ticks sums length. Player q's pairs are player_pairs[player_off[q] :
 *     player_off[q + 1]] (player_off holds n_players + 1 entries), each entry 2 * pair + side (0 = the pair's A,
 *     1 = its B; an entry naming no pair of [0, n_pairs) counts nowhere); player_stats[q][PM_LEAGUE_STATS] =
 *     games, wins, losses, draws, points_for, points_against, ticks, unfinished summed over them;
 *     fitness[q] = (float)wins / (float)games, 0.0f when games == 0. PM_E_SIZE: a negative count; PM_E_ARG: a
 *     null pointer whose count is positive (player_pairs may be null while n_pairs == 0).
 *
 *   pm_pbt_select  one workgroup. f[p] = fitness[p], a NaN taken as -inf; member a is better than b iff f[a] >
 *     f[b] || (f[a] == f[b] && a < b); rank[p] = the number of members better than p (a permutation of 0..n-1).
 *     With r = Philox(seed), counter (p, purpose PBT, round): draw[p] = r.y for every p (for the caller's explore
 *     step); a member with rank[p] >= n - n_bottom gets src_of[p] = the member of rank (r.x * n_top) >> 32, every
 *     other member src_of[p] = p. PM_E_SIZE: n outside 1..PM_DQN_POP_MAX, n_bottom < 0, n_top < 1, n_bottom +
 *     n_top > n; PM_E_ARG: a null pointer. */
#define PM_LEAGUE_STATS 8
int pm_league_serves(const pm_env_params* p, const int32_t* serve_idx, uint64_t seed, uint32_t round,
                     double* serves, int32_t m, void* stream);
int pm_league_reduce(const int32_t* scoreA, const int32_t* scoreB, const int32_t* length,
                     const int32_t* pair_first, int32_t n_pairs,
                     const int32_t* player_off, const int32_t* player_pairs, int32_t n_players,
                     int64_t* pair_stats, int64_t* player_stats, float* fitness, void* stream);
int pm_pbt_select(const float* fitness, int32_t n, int32_t n_bottom, int32_t n_top, uint64_t seed, uint64_t round,
                  int32_t* rank, int64_t* src_of, uint32_t* draw, void* stream);

/* Matchmaking (csrc/pm_match.hip; additive to ABI 27 as the league is): after pm_league_reduce, every member's next
 * training opponent drawn from its results and that opponent's net copied into the collector's table, and a
 * Bradley-Terry rating of every player, each in one launch with no host read. pair_stats, player_off and
 * player_pairs are pm_league_reduce's; pair_players is [n_pairs][2] = (player A, player B); net_of[q] is player q's
 * row in the folded weight table w [n_nets][PM_QNET_NW], negative for a player without a net (the follower). Members
 * are players 0..n-1. Arguments are checked on the host before the first HIP call. An entry of a pair list, the
 * opponent it names and that opponent's net are range-checked before they index anything: no value in these
 * arrays makes a kernel touch memory outside them (player_off is structure and must describe player_pairs).
 *
 *   pm_league_match  grid n, block 256. Entry e = 2 * pair + side of member p's list names the opponent o =
 *     pair_players[pair][1 - side]; it is eligible iff 0 <= pair < n_pairs, 0 <= o < n_players, o != p and 0 <=
 *     net_of[o] < n_nets. With g = the pair's games and s = 2 * (wins of p's side) + draws, in float32 with + - * /
 *     only: x = g == 0 ? 0.5f : (float)s / (float)(2 * g); PM_MATCH_HARD: f = 1.0f multiplied `power` times by
 *     (1.0f - x), one after the other (power 0 = uniform); PM_MATCH_EVEN: f = (4.0f * x) * (1.0f - x); the entry's
 *     weight is q = (uint32_t)(f * 65535.0f) + 1, and 0 if it is not eligible. total[p] = the int32 sum of q;
 *     t = (r.x * total) >> 32 with r = Philox(seed), counter (p, purpose MATCH = 11, round); opp[p] = the opponent of
 *     the first entry in list order whose inclusive prefix sum exceeds t, and row net_of[opp[p]] of w is copied into
 *     row p of wA_out [n][PM_QNET_NW]. total[p] == 0: opp[p] = -1 and row p of wA_out is not written. A list holds
 *     at most PM_LEAGUE_MATCH_MAX entries (the sum then fits int32); the entry point cannot see the lists, so the
 *     caller checks that (pongmi.matchmaking.Matchmaker does), and the kernel looks at no entry past that many.
 *     PM_E_SIZE: n outside 1..PM_DQN_POP_MAX, n_players < n, n_pairs < 0, n_nets < 1, an unknown mode, power
 *     outside 0..PM_MATCH_POWER_MAX. PM_E_ARG: a null buffer (pair_stats, pair_players and player_pairs may be null
 *     while n_pairs == 0), w or wA_out not 16-byte aligned, another buffer not aligned to its element, wA_out
 *     [n rows] overlapping w [n_nets rows]. There is no no-op size.
 *
 *   pm_league_rate  one workgroup of 1024. An entry of player q's list counts iff 0 <= pair < n_pairs, 0 <= o <
 *     n_players, o != q and g > 0. W_q = 0.5f * (float)S_q + 0.5f * prior with S_q the int64 sum of s over them;
 *     r = 1.0f to begin with; each of `iterations` Jacobi steps sets r'_q = W_q / D_q, D_q = prior / (r_q + 1.0f) +
 *     sum over the entries of (float)g / (r_q + r_o): the prior is `prior` games against a virtual player of strength
 *     1, half of them won, which keeps an unbeaten player finite and fixes the scale (nothing is normalised).
 *     rating[q] = r_q after the last step. The order of the float32 additions is fixed: lane l of the player's wave
 *     adds the entries at list positions l, l + 64, ... in that order onto 0.0f, the 64 lane sums combine pairwise
 *     over adjacent blocks of 2, 4, 8 and 16 lanes and then as (row 0 + row 1) + (row 2 + row 3), and the prior's
 *     term is added to that from the left (csrc/pm_match.hip's header; pongmi.matchmaking.rate_host restates it bit
 *     for bit). n_players == 0 is a no-op. PM_E_SIZE: n_players outside 0..PM_LEAGUE_RATE_MAX (the strengths live in
 *     LDS twice, beside W), n_pairs < 0, iterations outside 0..PM_LEAGUE_RATE_ITER_MAX. PM_E_ARG: prior not
 *     positive and finite, a null buffer (as above), a buffer not aligned to its element. */
#define PM_MATCH_HARD 0
#define PM_MATCH_EVEN 1
#define PM_MATCH_POWER_MAX 8
#define PM_LEAGUE_MATCH_MAX 32767
#define PM_LEAGUE_RATE_MAX 4096
#define PM_LEAGUE_RATE_ITER_MAX 4096
int pm_league_match(const int64_t* pair_stats, const int32_t* pair_players, int32_t n_pairs,
                    const int32_t* player_off, const int32_t* player_pairs, int32_t n_players,
                    const int32_t* net_of, const float* w, int32_t n_nets, int32_t n, int32_t mode, int32_t power,
                    uint64_t seed, uint64_t round, float* wA_out, int32_t* opp, int32_t* total, void* stream);
int pm_league_rate(const int64_t* pair_stats, const int32_t* pair_players, int32_t n_pairs,
                   const int32_t* player_off, const int32_t* player_pairs, int32_t n_players,
                   int32_t iterations, float prior, float* rating, void* stream);

/* K9 — inference-only self-play rollout, `steps` vector steps in one launch (BASELINE configs[1];
 * csrc/pm_rollout.hip). Replaces the act/step loop of scripts/train_iterative.py:239-242 with the
 * learner switched off: per vector step c = counter0 + s, modelB's heads are refolded with fresh
 * noise (reset_noise, :125; Philox(seed_net, c) as pm_qnet_fold PM_FOLD_TRAIN_FRESH), player A acts
 * greedily on wA, player B epsilon-greedily on wB's features + the fresh heads (Philox(seed_env, c)
 * as pm_qnet_act), and every arena ticks with autoreset (the step-keyed serve of pm_env_step,
 * Philox(seed_env, c)). Bit-identical to that fold -> act -> env_step sequence. wA / wB: effective
 * weights (PM_QNET_NW, 16-B aligned; wB any fold of paramsB: only its feature layers are read);
 * paramsB: modelB's parameter block (PM_QNET_NP; its eps section is not written); heads_ws: device
 * workspace of steps * PM_ROLL_HEADS floats, 16-B aligned. On return the state holds the arenas after
 * the last step and obsA / obsB [n][7] their observations. stats (nullable, device, accumulated):
 * [0] episodes finished, [1] of them won by B, [2] points won by A, [3] points won by B. The serve
 * counters (s->serves) are neither read nor written. */
#define PM_ROLL_HEADS 264
int pm_rollout(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB, const float* paramsB,
               float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0, int32_t steps, float* heads_ws,
               float* obsA, float* obsB, int64_t* stats, int32_t n, void* stream);

/* §8f3 — the collecting rollout (ABI 18): pm_rollout's launch that also pushes every vector step's
 * transitions into a replay ring from registers, as the training loop's memory.push((oB, aB, rB, nB,
 * done)) (scripts/train_iterative.py:242-243, PrioritizedReplay.push :56-63) with the learner switched
 * off (no train_step between pushes, epsilon held for the launch). Step s's arena i lands in slot
 * (pos + s * n + i) mod cap: row (s = obsB before the step, r = rB, s' = the step's terminal obsB,
 * bits(aB | done << 8)), prios[slot] = prio, and, with per_work, the PER leaf powf(prio, alpha) —
 * after the launch the sum tree's nodes are rebuilt over the whole ring (per_work then is the
 * pm_per_work_bytes(cap) tree of pm_per_sample). ep_reward [n] is carried (ep_reward += rB, zeroed
 * on done). steps * n <= cap (no slot is written twice in one launch). stats (nullable, device,
 * accumulated) holds 6 entries: pm_rollout's four, then [4] episodes with ep_reward > 0 (the loop's
 * win, :247-248), [5] the sum of ep_reward over finished episodes. Bit-identical to `steps`
 * repetitions of pm_rollout's stepped composition with pm_env_step's terminal observations pushed
 * in arena order (tests/test_gpu_rollout.py). */
typedef struct pm_roll_replay {
    float *trans;      /* [cap][PM_TRANS_F], 16-byte aligned */
    float *prios;      /* [cap] */
    void *per_work;    /* nullable: PER sum tree (pm_per_work_bytes(cap), 16-byte aligned) */
    float *ep_reward;  /* [n] */
    int64_t pos, cap;  /* 0 <= pos < cap */
    float prio, alpha; /* the pushed priority (max(prios), or 1.0 into an empty buffer) and PER alpha */
} pm_roll_replay;
int pm_rollout_push(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                    const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0,
                    int32_t steps, float* heads_ws, float* obsA, float* obsB, const pm_roll_replay* rp, int64_t* stats,
                    int32_t n, void* stream);

/* The collecting rollout for a population (csrc/pm_rollout_pop.hip; additive to ABI 27 as pm_dqn_pop was:
 * pm_sizeof unchanged, a size function of its own, an opaque handle). n members of m arenas each play in one
 * launch per phase: member p owns arenas [p * m, (p + 1) * m) of ONE pm_env_state of n * m arenas (one
 * pm_env_params for all), plays its own opponent wA against its own modelB (wB / paramsB) and pushes into its
 * own prioritized replay. Member p's arenas, observations, ep_reward, ring rows, prios, PER leaves, tree nodes
 * and stats afterwards hold bit for bit what pm_rollout_push leaves for an m-arena state equal to the member's
 * slice with the member's wA, wB, paramsB, epsilon, seed_env, seed_net, the call's counter0 and the member's
 * current pos and pushed priority: every Philox draw is keyed by the member-local arena index 0..m-1.
 *   pm_roll_member  member p's record (a HOST array of n, free to reuse once create / rebind returns).
 *     rp.ep_reward is the member's own [m]; rp.pos / size are the ring's write slot and fill WHEN THE TABLE WAS
 *     BOUND; rp.prio is the pushed priority unless prio_dev is set (below). stats (nullable): the member's own
 *     6 x int64, accumulated (pm_rollout_push's six entries).
 *   pm_rollout_pop_create / _rebind  validate everything on the host before the first HIP call (so a machine
 *     without a GPU reports the same codes, the message naming the member), then upload the table with a
 *     synchronous copy; rebind (same n, m, steps_max) first waits for `stream`, since launches queued there
 *     read the old table. These are the interface's ONLY host synchronisations.
 *   pm_rollout_pop_push  only enqueues launches: `steps` vector steps (0 <= steps <= steps_max; 0 is a no-op)
 *     from Philox counter counter0. `advance` (>= 0) is the number of transitions each member has pushed since
 *     the table was bound (every member pushes steps * m per call, so it is one number): the launch writes from
 *     pos = (rp.pos + advance) mod cap into a ring of fill min(cap, size + advance), so a loop of collects never
 *     rebinds. In stream order: for members with prio_dev, prio_dev[0] = max(prios[0:fill]) (1.0f when the fill
 *     is 0: PrioritizedReplay.push's max(prios), taken on the device with no host read) and that value is the
 *     priority pushed; the heads of every (step, member); the rollout (one block per member and 32-arena tile);
 *     the tree nodes of every member with per_work. obsA / obsB are [n * m][7].
 *   pm_rollout_pop_info  n, m and steps_max (any pointer may be null). _destroy frees table and handle; the
 *     caller has let the launches finish.
 * PM_E_SIZE: n outside 1..PM_DQN_POP_MAX, m < 1, n * m past int32, steps_max < 1, steps outside 0..steps_max,
 * advance < 0; per member cap <= 0, pos outside [0, cap), size outside [0, cap], steps_max * m > cap (a slot
 * would be written twice in one launch). PM_E_ARG: a null handle, out, members, p, s or state / observation
 * array; speed_scale_every <= 0; per member a null wA, wB, paramsB, heads_ws, trans, prios or ep_reward; wA, wB,
 * heads_ws, trans or per_work not 16-byte aligned; epsilon not finite.
 * Aliasing (PM_E_ARG): trans, prios, per_work, ep_reward, heads_ws, stats, prio_dev and wB of one member must not
 * overlap, as byte ranges of their known sizes, any of those of another member. wA and paramsB are only read
 * and may be shared. */
typedef struct pm_roll_member {
    const float *wA;       /* the opponent's effective weights, PM_QNET_NW, 16-byte aligned */
    float *wB;             /* the member's feature image: any fold of paramsB, PM_QNET_NW, 16-byte aligned */
    const float *paramsB;  /* PM_QNET_NP, read in place */
    float *heads_ws;       /* steps_max * PM_ROLL_HEADS floats, 16-byte aligned */
    pm_roll_replay rp;
    int64_t size;          /* the ring's fill when the table was bound, 0..cap */
    float *prio_dev;       /* nullable, device [1]: see pm_rollout_pop_push */
    int64_t *stats;        /* nullable, device [6], accumulated */
    float epsilon;
    int32_t _pad;
    uint64_t seed_env, seed_net;
} pm_roll_member;
size_t pm_roll_member_sizeof(void);
typedef struct pm_rollout_pop pm_rollout_pop;
int pm_rollout_pop_create(const pm_env_params* p, const pm_env_state* s, const pm_roll_member* members, int32_t n,
                          int32_t m, int32_t steps_max, pm_rollout_pop** out);
int pm_rollout_pop_rebind(pm_rollout_pop* pop, const pm_roll_member* members, void* stream);
int pm_rollout_pop_push(const pm_rollout_pop* pop, uint64_t counter0, int32_t steps, int64_t advance, float* obsA,
                        float* obsB, void* stream);
int pm_rollout_pop_info(const pm_rollout_pop* pop, int32_t* n, int32_t* m, int32_t* steps_max);
int pm_rollout_pop_destroy(pm_rollout_pop* pop);

/* ---------------------------------------------------------------- QNetRNN (K5) */

/* Packed QNetRNN parameter block (models/qnet_rnn.py:58-101), PM_RNN_NP floats: the state_dict
 * tensors in modelB.parameters() order (features_extractor.{0,2}.{weight,bias}, lstm.{weight_ih_l0,
 * weight_hh_l0, bias_ih_l0, bias_hh_l0}, fc_shared_head.0 / fc_V / fc_A {weight_mu, bias_mu,
 * weight_sigma, bias_sigma}: 174 984 floats), then the NoisyLinear epsilon buffers (shared head,
 * V, A; weight then bias). Effective weights, PM_RNN_NW floats: an opaque MFMA fragment image. */
#define PM_RNN_NP 192012
#define PM_RNN_NPARAM 174984
#define PM_RNN_NW 157456

/* Fold `count` QNetRNN blocks [count][PM_RNN_NP] into effective weights [count][PM_RNN_NW]; modes
 * as pm_qnet_fold (NoisyLinear eval: mu; train: mu + sigma*eps; train_fresh: reset_noise() first,
 * Philox(seed, counter + *counter_dev) per net, written back into params_out when non-NULL). */
int pm_rnn_fold(const float* params, float* params_out, int32_t mode, uint64_t seed, uint64_t counter,
                const uint64_t* counter_dev, float* w_eff, int32_t count, void* stream);

/* One QNetRNN.forward step (models/qnet_rnn.py:107-144, T = 1) for n rows: x [n][7], (h, c)
 * [n][128] each read and overwritten with (h_n, c_n); reset[i] != 0 (nullable) starts row i from
 * init_hidden (zeros, :146-152); q [n][3]. */
int pm_rnn_q(const float* w_eff, const float* x, float* h, float* c, const uint8_t* reset, float* q, int32_t n,
             void* stream);

/* Both players' QNetRNN action selection (train_rnn_iterative.py:371-389, :571-581) for n arenas,
 * fused on the matrix cores: A greedy with w_opp[opp_id[i]] (opp_id NULL = net 0) on obsA and
 * (hA, cA); B on obsB and (hB, cB): random.random() < epsilon ? randint(0,2) : argmax, the forward
 * advancing (hB, cB) either way. reset (nullable) zeroes both players' state first (episode
 * start). Side A is grouped per net: with opp_list / opp_cnt (nullable; per-256-arena-block lists
 * as pm_selfplay's, consistent with opp_id) every net's arenas are packed into full 128-row groups,
 * otherwise chunks of chunk0 (net 0) / chunk1 (others) arenas are compacted (0 = 256 / 2048). */
int pm_rnn_act(const float* w_opp, const int32_t* opp_id, int32_t n_opp, const float* w_B, const float* obsA,
               const float* obsB, float* hA, float* cA, float* hB, float* cB, const uint8_t* reset, float epsilon,
               const double* eps_dev, uint64_t seed, uint64_t counter, const uint64_t* counter_dev, int8_t* aA,
               int8_t* aB, float* qA, float* qB, int32_t n, int32_t chunk0, int32_t chunk1, const int32_t* opp_list,
               const int32_t* opp_cnt, void* stream);

/* ---------------------------------------------------------------- DRQN update (K6) */

/* train_step_rnn (scripts/train_rnn_iterative.py:400-531) on a sampled batch of `batch` sequences
 * of length T: zero initial state; q = Q_B(obs)[last step][act[:, T-1]]; double-DQN target
 * y = rew[:, T-1] + gamma * Q_T(next)[argmax Q_B(next)] * (1 - done[:, T-1]) with modelB in train
 * mode (NoisyLinear mu + sigma * its epsilon buffers) and targetB in eval mode (mu);
 * loss = smooth_l1(q, y) (mean); gradients of all PM_RNN_NPARAM parameters by BPTT;
 * clip_grad_norm_(max_norm); Adam; targetB <- modelB every target_update_interval steps. */
typedef struct pm_drqn_stats {
    int64_t steps;  /* updates taken (train_steps_count: target sync every target_update_interval) */
    int64_t adam_t; /* the optimizer's step count (bias correction); a new optimizer restarts it at 0 */
    float loss;     /* smooth_l1 loss of the last update */
    float norm;     /* pre-clip total gradient norm of the last update (of the rank mean) */
    float q_mean;   /* mean q of the last batch */
    int32_t status; /* latched error bits: 2 = a hand-off inside pm_drqn_grads timed out on this replica;
                     * 4 = (before round 6) pm_drqn_apply's norm arrival timed out; no longer set;
                     * 8 = an update was voided (a timeout on any rank: no Adam step, no target sync) */
} pm_drqn_stats;

typedef struct pm_drqn {
    float *params;          /* [PM_RNN_NP] modelB, updated in place */
    float *target;          /* [PM_RNN_NP] targetB */
    float *adam_m, *adam_v; /* [PM_RNN_NPARAM] */
    float *grad;            /* [PM_RNN_NPARAM + 4] gradients in packed parameter order, then at
                             * [PM_RNN_NPARAM] the number of ranks that contributed (1 per enabled
                             * replica) and at [PM_RNN_NPARAM + 1] the number of ranks whose update
                             * timed out — all summed by the all-reduce; apply divides by the first
                             * and does nothing when the second is non-zero */
    void *work;             /* pm_drqn_work_bytes(batch, T) bytes, 16-byte aligned, ZERO-FILLED before the
                             * first pm_drqn_* call that uses it (pm_drqn_init does it): the in-launch
                             * hand-offs match granule tags against an epoch kept in the workspace, and
                             * a stale granule whose tag happened to match (hipMalloc / reused memory)
                             * would be read before its producer wrote it */
    pm_drqn_stats *stats;
    const float *obs, *next; /* [batch][T][7] */
    const int32_t *act;      /* [batch][T] */
    const float *rew;        /* [batch][T] */
    const uint8_t *done;     /* [batch][T] */
    const int32_t *enable;   /* nullable device flag: 0 = this replica skips the update (grads -> 0) */
    int32_t batch;           /* multiple of 32, <= 256 */
    int32_t T;               /* 1 .. 64 */
    int64_t target_update_interval;
    double gamma, lr, beta1, beta2, adam_eps, max_norm;
    int32_t poll_limit;     /* polls per in-launch hand-off before it times out: 0 = default (2^20);
                             * < 0 = none (every hand-off times out: a test hook for the void path) */
    int32_t reserved;
} pm_drqn;

/* Bytes of workspace for (batch, T), or -1 for exactly the sizes every other pm_drqn_* entry point
 * rejects: batch not a multiple of 32 in [32, 256], or T outside [1, 64]. Size the allocation from it
 * and treat -1 as an error before allocating anything. */
int64_t pm_drqn_work_bytes(int32_t batch, int32_t T);
/* Zero-fill d->work (pm_drqn_work_bytes(d->batch, d->T) bytes) on the stream (ABI 20): call once after
 * allocating the workspace, before the first pm_drqn_grads / pm_drqn_update on it. */
int pm_drqn_init(const pm_drqn *d, void *stream);
/* Forward + BPTT: grad <- d loss / d params of this replica's batch, grad[PM_RNN_NPARAM] <- 1
 * (all zero when *enable == 0). The NoisyLinear sigma slots are left for pm_drqn_apply, which
 * forms them as mu gradient x epsilon (linear, identical epsilon on every rank). */
int pm_drqn_grads(const pm_drqn *d, void *stream);
/* grad / grad[PM_RNN_NPARAM] -> clip_grad_norm_ -> Adam step -> target sync; stats updated.
 * Nothing happens when grad[PM_RNN_NPARAM] == 0. */
int pm_drqn_apply(const pm_drqn *d, void *stream);
/* pm_drqn_grads then pm_drqn_apply, the clip norm's shares summed by the weight-gradient tiles as they
 * store. pm_drqn_apply after an all-reduce forms the same shares of the summed gradient in the same
 * order (round 6), so with one rank the two paths give bit-identical parameters, clip active or not. */
int pm_drqn_update(const pm_drqn *d, void *stream);

/* ---------------------------------------------------------------- stand-alone double-DQN learner (K10) */

/* train_step (scripts/train_iterative.py:141-168) on a batch the caller supplies (ABI 27; csrc/pm_dqn.hip):
 * q = Q_B(s)[a]; a* = argmax Q_B(s') (first maximum); t = r + gamma * Q_T(s')[a*] * (1 - done), targetB
 * in eval mode (mu only); L = mean(isw * (q - t)^2); torch.optim.Adam; targetB <- modelB when the step
 * count, after its increment, is a multiple of target_update_interval. With train_features = 0 only the
 * 520 head parameters train (the reference freezes modelB.features, :97) and params, adam_m / adam_v and
 * grad keep their bits in [0, PM_QNET_HEAD_OFF). With train_features = 1 the backward runs on through
 * both ReLU layers (relu'(0) = 0) and Adam covers all PM_DQN_NPARAM slots, in the parameter block's
 * order. The gradient is a pure function of the inputs: every sum has one fixed order, there is no
 * atomic, and nothing in the launch waits for another workgroup. Rows at or past `batch` are not read.
 * Both blocks, grad and the moments are 16-byte aligned. */
#define PM_DQN_NPARAM 5192
typedef struct pm_dqn_stats {
    int64_t steps;  /* updates taken (train_steps: the target sync and the noise counter) */
    int64_t adam_t; /* the optimizer's step count (bias correction) */
    float loss;     /* loss of the last batch (this replica's) */
    float q_mean;   /* mean q of the last batch */
    int32_t status; /* 0 from pm_dqn_grads / apply / update (nothing in them can time out). Latched by
                       pm_dqn_replay_update, cleared by the caller:
                       bit 0: an update was void because the replay's sum tree has no mass (all priorities
                              zero or NaN);
                       bit 1: a NaN |q - t| was stored as a priority (its leaf is 0), as pm_ctrl.status bit 1;
                       bit 2: an update was void because a drawn slot lay outside [0, size) (the tree handed
                              over was not current) */
    int32_t _pad;
} pm_dqn_stats;

typedef struct pm_dqn {
    float *params, *target;       /* [PM_QNET_NP] modelB / targetB blocks (pongmi.qnet layout) */
    float *adam_m, *adam_v;       /* [PM_DQN_NPARAM]; heads-only mode touches [4672, 5192) only */
    float *grad;                  /* [PM_DQN_NPARAM + 8]: gradients, then [PM_DQN_NPARAM] = 1 per contributing
                                     rank (summed by the all-reduce) and 7 zeros */
    pm_dqn_stats *stats;          /* device */
    const float *s, *ns;          /* [batch][7] */
    const int32_t *act;           /* [batch] in {0, 1, 2} */
    const float *rew;             /* [batch] */
    const uint8_t *done;          /* [batch] */
    const float *isw;             /* nullable [batch] importance weights: null = all ones */
    float *td;                    /* [batch] |q - t| (update_priorities' errors, :163) */
    float *q;                     /* nullable [batch][3]: Q_B(s) as used by the loss */
    int32_t batch;                /* 1..PM_MAX_BATCH */
    int32_t train_features;       /* 0: heads only (the reference); 1: all PM_DQN_NPARAM parameters */
    int32_t noise;                /* PM_FOLD_TRAIN: the block's epsilon buffers as they are;
                                     PM_FOLD_TRAIN_FRESH: reset_noise() first (:142): Philox(seed_net,
                                     TAG_NOISE_TRAIN, stats->steps + 1) as the fused learner draws it, the
                                     counter read on the device, the noise written into params' epsilon
                                     buffers */
    int32_t _pad;
    int64_t target_update_interval;
    double gamma, lr, beta1, beta2, adam_eps;
    uint64_t seed_net;
} pm_dqn;

/* The three forwards, loss, td and grad (grad[PM_DQN_NPARAM] <- 1); stats->loss / q_mean written. */
int pm_dqn_grads(const pm_dqn* d, void* stream);
/* grad / grad[PM_DQN_NPARAM] -> Adam -> target sync -> stats->steps / adam_t + 1. Nothing happens when
 * grad[PM_DQN_NPARAM] == 0. */
int pm_dqn_apply(const pm_dqn* d, void* stream);
/* pm_dqn_grads then pm_dqn_apply on one replica, as one launch (the same arithmetic: bit-identical). */
int pm_dqn_update(const pm_dqn* d, void* stream);

/* Loss and clip options of the stand-alone learner (additive to ABI 27, as pm_dqn_replay: a size function
 * of its own, pm_sizeof unchanged). The _opt entry points run the same update as the plain ones with two
 * things a caller may choose, both torch's:
 *   loss      PM_DQN_LOSS_HUBER: with diff = q - t, ad = |diff|, w = isw or 1, beta = (float)huber_beta the
 *             row's loss term is w * (ad < beta ? 0.5f * diff * diff / beta : ad - 0.5f * beta) and
 *             dL/dq = (w / batch) * (ad < beta ? diff / beta : sign(diff)):
 *             (isw * F.smooth_l1_loss(q, t, reduction='none', beta=beta)).mean(). For beta = 1 the
 *             quadratic zone is HALF the squared loss: gradient diff, not PM_DQN_LOSS_SQUARED's 2 diff.
 *             td stays |q - t| (priorities do not depend on the loss); stats, q and everything behind
 *             dL/dq are formed as before. A row with diff == 0 contributes no gradient.
 *   max_norm  > 0: torch.nn.utils.clip_grad_norm_(trained parameters, max_norm) in the apply step, after
 *             gk = grad / count and before Adam, so replicas that all-reduce clip on the norm of the
 *             averaged gradient and every rank derives the same coefficient. norm = sqrt(sum gk^2) over
 *             the trained slots only ([PM_QNET_HEAD_OFF, PM_DQN_NPARAM) in heads-only mode, the sigma
 *             gradients included; [0, PM_DQN_NPARAM) with train_features), coef = min(1, (float)(max_norm /
 *             ((double)norm + 1e-6))), Adam consumes gk * coef. grad keeps the UNCLIPPED gradient, in its
 *             usual layout. The sum of squares has one fixed order and no atomic: per thread in fp64 in
 *             slot order, a wave sum, the 16 wave sums added in wave order. A clip that does not bite
 *             (coef == 1.0f) leaves every bit as without one.
 *   norm      nullable device float: the total norm before the clip of the last apply, written whenever it
 *             is non-null, clip or no clip; untouched where the apply step does nothing (count 0, or a
 *             void update of pm_dqn_replay_update_opt).
 * A null opt means the defaults: squared loss, no clip, no norm out; the results then equal the plain
 * entry points' bit for bit. PM_E_ARG, before any launch: an unknown loss; huber_beta <= 0 or not finite
 * with PM_DQN_LOSS_HUBER; max_norm < 0 or not finite; and whatever the plain entry point rejects. */
#define PM_DQN_LOSS_SQUARED 0   /* mean(isw * (q - t)^2): the reference, train_iterative.py:158 */
#define PM_DQN_LOSS_HUBER   1   /* mean(isw * smooth_l1(q - t, beta)) */
typedef struct pm_dqn_opt {
    int32_t loss;        /* PM_DQN_LOSS_* */
    int32_t _pad;
    double  huber_beta;  /* > 0, finite; read only with PM_DQN_LOSS_HUBER */
    double  max_norm;    /* 0: no clip; > 0, finite: clip_grad_norm_(trained parameters, max_norm) */
    float  *norm;        /* nullable, device [1]: total norm before the clip of the last apply */
} pm_dqn_opt;
size_t pm_dqn_opt_sizeof(void);
int pm_dqn_grads_opt(const pm_dqn* d, const pm_dqn_opt* opt, void* stream);  /* reads loss / huber_beta */
int pm_dqn_apply_opt(const pm_dqn* d, const pm_dqn_opt* opt, void* stream);  /* reads max_norm / norm */
int pm_dqn_update_opt(const pm_dqn* d, const pm_dqn_opt* opt, void* stream);

/* The same update drawn from a device replay (csrc/pm_dqn_replay.hip), `updates` times in one call, on the
 * stream, with no host synchronisation or copy. Per update: frame = d->stats->steps + 1 (read on the
 * device: frame_idx += 1 before sampling, :136), beta = min(1, beta_start + frame (1 - beta_start) /
 * beta_frames); d->batch slots drawn from the sum tree in per_work (pm_per_sample's draw over the fill
 * `size`; uniform j of update k is u[k * batch + j], or with u null u53(Philox(j, TAG_PER, frame, seed)),
 * the fused learner's convention); the weights (size P(i))^-beta divided in float32 by their maximum; the
 * sampled rows of trans copied into d's OWN batch buffers s, ns, act, rew, done and isw (written here
 * although pm_dqn declares them const; isw must not be null) and the slots into idx; pm_dqn_update's
 * update, bit for bit; prios[idx[j]] = td[j] + 1e-6f (the last duplicate in batch order wins), their
 * leaves, and the level-1 and level-2 tree nodes over them recomputed, so that per_work again equals a
 * pm_per_build of prios bit for bit and the next update, or the next call, draws from it as it is.
 * An update whose tree has no mass, or that draws a slot outside [0, size), is void: nothing is gathered,
 * there is no Adam step, no steps increment and no scatter, every idx[j] is -1 and stats->status latches
 * bit 0 or bit 2; a NaN td latches bit 1 (pm_dqn_stats). PM_E_ARG: a null descriptor or buffer (d->isw
 * included), trans or per_work not 16-byte aligned, and whatever pm_dqn_update rejects; PM_E_SIZE: size <=
 * 0, size > cap, updates <= 0, beta_frames <= 0. */
typedef struct pm_dqn_replay {
    float *trans;          /* [cap][PM_TRANS_F] ring (DeviceReplay.trans), 16-byte aligned */
    float *prios;          /* [cap] */
    void *per_work;        /* pm_per_work_bytes(cap): the sum tree over cap, current on entry, 16-byte aligned */
    int64_t *idx;          /* [d->batch] out: the last update's sampled slots */
    const double *u;       /* nullable [updates][d->batch]: the draws' uniforms (tests); null = Philox */
    int64_t cap, size;     /* 0 < size <= cap: entries [0, size) are filled */
    double alpha, beta_start;
    int64_t beta_frames;   /* > 0 */
    uint64_t seed;
} pm_dqn_replay;
size_t pm_dqn_replay_sizeof(void);
int pm_dqn_replay_update(const pm_dqn* d, const pm_dqn_replay* rp, int32_t updates, void* stream);
/* pm_dqn_replay_update with pm_dqn_update_opt as its update; a void update skips loss, clip and norm alike. */
int pm_dqn_replay_update_opt(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, int32_t updates,
                             void* stream);

/* A population of stand-alone learners (additive to ABI 27 as pm_dqn_opt was: pm_sizeof unchanged; the handle
 * is opaque, as pm_comm). n independent members, member p being (d[p], opt[p], rp[p]): its own modelB / targetB
 * blocks, Adam state, counters, hyper-parameters, loss and clip options, batch buffers and, with rp, its own
 * prioritized replay. Every launch has a grid of n workgroups and workgroup p runs member p from a device table
 * of the members' descriptors; n may exceed the number of compute units (the workgroups then queue). No
 * workgroup waits for another and there is no atomic but the one on a member's own status word.
 *   pm_dqn_pop_create  d, opt and rp are HOST arrays of n entries, free to reuse once it returns. opt may be
 *     null and a zeroed entry means the defaults; rp may be null: the population then has no replay path.
 *     Everything is validated on the host before the first HIP call (so a machine without a GPU reports the
 *     same codes), then the table is allocated and uploaded with a synchronous copy.
 *   pm_dqn_pop_rebind  replaces the table for the same n (a changed row count `batch`, replay fill `size`,
 *     uniforms pointer `u`, hyper-parameter, ...) after the same validation. It waits for `stream` before it
 *     overwrites the table, since launches already queued there read the old one.
 *   That wait and create's upload are the interface's ONLY host synchronisations: pm_dqn_pop_update and
 *   pm_dqn_pop_replay_update only enqueue launches.
 *   pm_dqn_pop_update  one launch. Member p's buffers afterwards hold bit for bit what
 *     pm_dqn_update_opt(&d[p], &opt[p]) leaves (with default options: what pm_dqn_update(&d[p]) leaves).
 *   pm_dqn_pop_replay_update  `updates` x three launches (draw + gather, update, scatter + tree refresh).
 *     Member p's result is bit for bit that of pm_dqn_replay_update_opt(&d[p], &opt[p], &rp[p], updates):
 *     prios, all three levels of per_work, idx, isw and the batch buffers included; uniform j of update k is
 *     rp[p].u[k * d[p].batch + j], or Philox where u is null. A member whose update is void keeps its own
 *     semantics (nothing gathered, no step, idx -1, its status bits latched, its norm untouched) and does not
 *     disturb the others. PM_E_ARG: a null handle or a population without rp; PM_E_SIZE: updates <= 0.
 *   pm_dqn_pop_info    n and whether the bound table has replay descriptors (either pointer may be null).
 *   pm_dqn_pop_destroy frees the table and the handle; the caller has let the launches finish.
 * Validation (create and rebind), the message naming the offending member index: PM_E_SIZE: n outside
 * 1..PM_DQN_POP_MAX; PM_E_ARG: a null d or out; per member whatever pm_dqn_update_opt rejects and, with rp,
 * whatever pm_dqn_replay_update_opt rejects (a null isw included).
 * Aliasing: a buffer that a launch writes for one member must not overlap, as a byte range of its known size,
 * any such buffer of another member (PM_E_ARG). Always writable: params, target, adam_m, adam_v, grad, stats,
 * td, a non-null q, a non-null opt.norm. With rp also: s, ns, act, rew, done, isw, idx, prios, per_work.
 * Buffers that are only read may be shared: without rp the batch buffers (n members sweeping hyper-parameters
 * on one batch), with rp the ring trans (one ring of experience, n learners, each with priorities of its own). */
#define PM_DQN_POP_MAX 1024
typedef struct pm_dqn_pop pm_dqn_pop;
int pm_dqn_pop_create(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, int32_t n, pm_dqn_pop** out);
int pm_dqn_pop_rebind(pm_dqn_pop* pop, const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_replay* rp, void* stream);
int pm_dqn_pop_update(const pm_dqn_pop* pop, void* stream);
int pm_dqn_pop_replay_update(const pm_dqn_pop* pop, int32_t updates, void* stream);
int pm_dqn_pop_info(const pm_dqn_pop* pop, int32_t* n, int32_t* has_replay);
int pm_dqn_pop_destroy(pm_dqn_pop* pop);

/* memory.push (:56-63) of n caller transitions, 0 < n <= cap, all device buffers: transition i goes to slot
 * (pos + i) mod cap as a PM_TRANS_F row, prios = prio (the caller's max(prios), 1 while empty), leaf =
 * prio^alpha, then the tree nodes overlapping the ring range are recomputed: per_work equals a pm_per_build
 * of prios bit for bit when it did before. act must hold 0..2 (the low 8 bits are stored). PM_E_ARG: a null
 * buffer, trans or per_work not 16-byte aligned; PM_E_SIZE: cap <= 0, n <= 0, n > cap, pos outside [0, cap). */
int pm_replay_push(float* trans, float* prios, void* per_work, int64_t cap, int64_t pos, float alpha, float prio,
                   const float* s, const int32_t* act, const float* rew, const float* ns, const uint8_t* done,
                   int32_t n, void* stream);

/* ---------------------------------------------------------------- n-step returns (additive to ABI 27) */

/* Multi-step targets for the stand-alone stack: pm_sizeof and every struct above are unchanged; new entry
 * points beside the old ones, which compute what they computed.
 * Row format. A replay row's horizon k (1..PM_NSTEP_MAX) is stored as k - 1 in bits 16..18 of the row's last
 * word, beside a | done << 8; the other bits stay as they are and readers mask with 7, so every bit pattern is a
 * valid horizon and every row written by pm_rollout_push / pm_replay_push decodes as one step. A ring may mix
 * horizons.
 * Discount. With g = (float)gamma: disc(1) = g, disc(k) = disc(k - 1) * g (float32 products in that order, no
 * fma). A row of horizon k has the target t = R + (disc(k) * nq) * (done ? 0 : 1): pm_dqn_update's for k = 1.
 * N-step reward. A pending transition keeps float32 (R, f), (0, 1) when it is opened; each tick with B's reward
 * r does R = R + f * r (a multiply, then an add), f = f * g, k += 1.
 *
 *   pm_dqn_nstep  horizon: device [d->batch] bytes, row j's horizon read as ((h - 1) & 7) + 1. pm_dqn_grads_n /
 *     pm_dqn_update_n are pm_dqn_grads_opt / pm_dqn_update_opt (opt nullable as there) with row j's target
 *     discounted by disc(horizon[j]); rows with done = 1 ignore it. A null pm_dqn_nstep or a null horizon IS the
 *     _opt entry: the same launch, bit for bit. The apply step has no horizon (pm_dqn_apply_opt).
 *   pm_dqn_replay_update_n  pm_dqn_replay_update_opt whose gather also decodes each sampled row's horizon into
 *     horizon[j], next to act and done, and whose update reads it there. PM_E_ARG: a null nstep or horizon.
 *   pm_dqn_nstep_pop_set  attaches horizon buffers to a population: nstep is a HOST array of n entries (a null
 *     array, or all-null horizons, detaches them), member p's update then being pm_dqn_update_n's and its replay
 *     update pm_dqn_replay_update_n's; members with a null horizon keep the one-step target. As
 *     pm_dqn_pop_rebind it validates on the host first and then waits for `stream`; the horizon buffers ([batch]
 *     bytes) join the aliasing rule, here and in every later rebind (PM_E_ARG, naming both members).
 *   pm_rollout_push_n  pm_rollout_push with a window of nstep ticks and g = (float)gamma. At step st arena i
 *     opens a pending transition (s = obsB before the step, aB); then every pending transition of the arena,
 *     the new one included, takes the tick's rB as above. If the tick ended the episode all of them are written
 *     with s' = the terminal observation, done = 1 and their own k and R, and the window is empty; otherwise the
 *     one that has reached k = nstep is written with s' = the observation after the tick and done = 0. After the
 *     launch's last step every transition still pending is written the same way with its shorter k and done = 0:
 *     nothing is carried between launches, and a shorter horizon is still a correct target because the row
 *     says which it has. The transition opened at step st goes to slot (pos + st * n + i) mod cap, so ring
 *     accounting, steps * n <= cap, the pushed priority, the PER leaves and the tree rebuild are
 *     pm_rollout_push's, every slot of the range is written once before the nodes are rebuilt, and the
 *     trajectory (actions, env state, observations), ep_reward and the six stats do not depend on nstep.
 *     nstep = 1 is pm_rollout_push: the same launch, bit for bit.
 *   pm_rollout_nstep_pop_set  member p of pm_rollout_pop_push collects as pm_rollout_push_n(nstep[p],
 *     gamma[p]): HOST arrays of n (both null: every member one step again). Validates on the host, then waits
 *     for `stream` where horizons were set before.
 *   pm_replay_push_n  pm_replay_push with row i's horizon (horizon[i] - 1) & 7 in bits 16..18; a null horizon is
 *     pm_replay_push.
 * Reported on the host before any HIP call: PM_E_SIZE: nstep outside 1..PM_NSTEP_MAX; PM_E_ARG: gamma not
 * finite (the population call naming the member); and whatever the entry without _n rejects. */
#define PM_NSTEP_MAX 8
typedef struct pm_dqn_nstep {
    uint8_t *horizon;  /* device [batch], 1..PM_NSTEP_MAX; read as ((h - 1) & 7) + 1 */
} pm_dqn_nstep;
size_t pm_dqn_nstep_sizeof(void);
int pm_dqn_grads_n(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_nstep* nstep, void* stream);
int pm_dqn_update_n(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_nstep* nstep, void* stream);
int pm_dqn_replay_update_n(const pm_dqn* d, const pm_dqn_opt* opt, const pm_dqn_nstep* nstep, const pm_dqn_replay* rp,
                           int32_t updates, void* stream);
int pm_dqn_nstep_pop_set(pm_dqn_pop* pop, const pm_dqn_nstep* nstep, void* stream);
int pm_rollout_push_n(const pm_env_params* p, const pm_env_state* s, const float* wA, const float* wB,
                      const float* paramsB, float epsilon, uint64_t seed_env, uint64_t seed_net, uint64_t counter0,
                      int32_t steps, float* heads_ws, float* obsA, float* obsB, const pm_roll_replay* rp, int64_t* stats,
                      int32_t n, int32_t nstep, double gamma, void* stream);
int pm_rollout_nstep_pop_set(pm_rollout_pop* pop, const int32_t* nstep, const double* gamma, void* stream);
int pm_replay_push_n(float* trans, float* prios, void* per_work, int64_t cap, int64_t pos, float alpha, float prio,
                     const float* s, const int32_t* act, const float* rew, const float* ns, const uint8_t* done,
                     const uint8_t* horizon, int32_t n, void* stream);

/* ---------------------------------------------------------------- QNetRNN self-play (K7) */

/* scripts/train_rnn_iterative.py's hot loop (:731-798) for n arenas: both players act with their
 * QNetRNN and (h, c) carried per arena (A greedy: modelA or a pool net, both eval mode; B
 * epsilon-greedy with fresh noise per vector step), env.step, SequenceReplayBuffer.push_step
 * (:107-116: whole episodes of length >= T are kept, the latest seq_cap of them), episode
 * bookkeeping and the next opponent / serve for finished arenas, then 64 sequences sampled
 * (:118-173) into a pm_drqn batch and train_step_rnn once the buffer holds > min_episodes. */
typedef struct pm_rnn_ctrl {
    uint64_t step;       /* vector steps taken */
    int64_t episodes;    /* finished episodes (global_episode_count) */
    int64_t seq_count;   /* episodes ever stored (length >= T) */
    int64_t seq_size;    /* episodes held: the newest min(seq_count, seq_cap), less any evicted by age */
    double epsilon;
    int64_t win_A, ep_A, win_P, ep_P;
    double reward_B;     /* summed rewards of finished episodes */
    int32_t status;      /* bit 0: a sampled step had been overwritten in its arena's ring (never, by
                            construction: kept for the check); bit 1: episodes left the buffer by age
                            before seq_cap newer ones did (their steps would leave the ring: depth is
                            too small for the episode lengths seen); bit 2: a finished trajectory
                            longer than depth / 2 steps was not stored */
    int32_t train;       /* 1 when this step's DRQN update was enabled */
} pm_rnn_ctrl;

typedef struct pm_rnn_selfplay {
    pm_env_params env;
    pm_env_state st;
    int32_t *opp;          /* [n] 0 = modelA, k >= 1 = pool net k */
    float *ep_reward;      /* [n] */
    int32_t *ep_len;       /* [n] steps into the current trajectory (the episode steps push_step
                              collected since the last done; a max_steps cut does not end it) */
    int32_t *ep_steps;     /* [n] steps into the current env episode (the max_steps cut)           */
    uint8_t *reset;        /* [n] 1: zero both players' (h, c) before the next act (episode start) */
    const float *w_opp;    /* [1 + n_pool][PM_RNN_NW] modelA, pool nets (eval-mode folds) */
    float *paramsB;        /* [PM_RNN_NP] modelB (the pm_drqn params); fresh noise written back */
    float *w_B;            /* [PM_RNN_NW] */
    float *hA, *cA, *hB, *cB;  /* [n][128] */
    float *obsA, *obsB;    /* [n][7] */
    int8_t *aA, *aB;       /* [n] */
    float *trans;          /* [depth][n][PM_TRANS_F] per-arena transition rings (s, r, s', a | done << 8) */
    int64_t *seq_eps;      /* [seq_cap][2]: arena | length << 32, first step */
    int64_t *seq_mark;     /* [depth] seq_count after step s's append, at s % depth (age eviction) */
    int64_t *fin;          /* [ceil(n / 256) * 256][2] scratch: stored episodes staged per env block */
    int64_t *partials;     /* [ceil(n / 256)][8] */
    int32_t *opp_list;     /* [n] per-256-arena-block opponent lists (written by the env kernel) */
    int32_t *opp_cnt;      /* [ceil(n / 256)][1 + n_pool] (offset << 16 | count) */
    int32_t *enable;       /* [1] set by the sampler: seq_size > min_episodes */
    pm_rnn_ctrl *ctrl;
    int32_t n, n_pool, depth, T, chunk_A, chunk_P;
    int32_t max_steps;     /* max_episode_steps (:751, config default 1000; 0 = no cut): an episode still
                              running after max_steps steps ends (counters, epsilon decay, new opponent,
                              env.reset, zero (h, c)) but its trajectory does not: push_step's
                              current_episode_trajectory keeps collecting until a done (:107-116) */
    int32_t _pad;
    int64_t seq_cap, min_episodes;
    double min_epsilon, epsilon_decay, pool_ratio;
    uint64_t seed_env, seed_net;
    const float *hA_in, *cA_in; /* nullable [n][128]: where the opponents' act reads (h, c) from (it writes
                                   hA / cA); null = in place. The overlapped step (ABI 10) alternates two
                                   buffers so a speculative act of the next step can be redone */
    float *qA, *qB;        /* nullable [n][3]: the Q values each player's act chose from (ABI 19; parity
                              tests read them beside the actions of the same launch) */
} pm_rnn_selfplay;

/* Ring safety: a stored trajectory is at most depth / 2 steps long (longer ones are dropped, status bit
 * 2), and an episode leaves the buffer once depth / 2 steps have passed since it finished (status bit
 * 1 if that happens before seq_cap newer episodes push it out), so every step a sample can reach is
 * still in its arena's ring. Size depth >= 2 x (the steps seq_cap episodes span + the longest
 * trajectory expected) and neither bit is ever set. */
/* Serve every arena, draw its first opponent, zero (h, c). */
int pm_rnn_selfplay_init(const pm_rnn_selfplay *sp, void *stream);
/* modelB's fold with fresh noise + both players' act (K5). */
int pm_rnn_selfplay_act(const pm_rnn_selfplay *sp, void *stream);
/* env tick + sequence store + counters; then, when d != NULL, sample d's batch and set *enable. */
int pm_rnn_selfplay_env(const pm_rnn_selfplay *sp, const pm_drqn *d, void *stream);
/* pm_rnn_selfplay_act then pm_rnn_selfplay_env. */
int pm_rnn_selfplay_rollout(const pm_rnn_selfplay *sp, const pm_drqn *d, void *stream);
/* rollout then pm_drqn_update(d) (d->enable should be sp->enable). */
int pm_rnn_selfplay_step(const pm_rnn_selfplay *sp, const pm_drqn *d, void *stream);
/* Replay ratio: the reference runs train_step_rnn once per env step (:776-777). Update u >= 1 of a
 * vector step samples its own batch (Philox counter (step, u); u = 0 is the env call's draw):
 * pm_rnn_selfplay_sample then pm_drqn_update. pm_rnn_selfplay_step_multi = rollout + update + (U - 1)
 * x [sample(u) + update]; U = 1 is pm_rnn_selfplay_step. */
int pm_rnn_selfplay_sample(const pm_rnn_selfplay *sp, const pm_drqn *d, int32_t u, void *stream);
int pm_rnn_selfplay_step_multi(const pm_rnn_selfplay *sp, const pm_drqn *d, int32_t updates, void *stream);
/* Overlapped act (ABI 10), as the DQN step's: part PM_ACT_ALL = pm_rnn_selfplay_act, PM_ACT_B = modelB's
 * fold + act only (select_action_for_model for B, :757-762), PM_ACT_A = the opponents' act only
 * (:753-755: modelA / pool nets, eval mode). pm_rnn_selfplay_step_overlap = act_part(B) + env + (fork to
 * side_stream: the NEXT step's act_part(A), on part of the chip) + `updates` DRQN updates + join. The
 * opponents' act depends on nothing the update writes, so the results are bit-identical to
 * pm_rnn_selfplay_step_multi. Contract: sp->aA holds the opponents' actions for the current
 * observations (act_part(A) once, then each overlapped step leaves them for the next). */
int pm_rnn_selfplay_act_part(const pm_rnn_selfplay *sp, int32_t part, void *stream);
int pm_rnn_selfplay_step_overlap(const pm_rnn_selfplay *sp, const pm_drqn *d, int32_t updates, void *side_stream,
                                 void *stream);
/* step_overlap without its act_part(B) (callers that time modelB's act on its own). */
int pm_rnn_selfplay_finish_overlap(const pm_rnn_selfplay *sp, const pm_drqn *d, int32_t updates, void *side_stream,
                                   void *stream);

/* ---------------------------------------------------------------- replay + PER (K4) */

/* Transition record, PM_TRANS_F floats per row (64 B): s [7] | r | s' [7] | bits(a | done << 8).
 * (memory.push((oB, aB, rB, nB, done)), scripts/train_iterative.py:243) Bits 16..18 of the last word hold an
 * n-step row's horizon - 1 ("n-step returns" above); they are zero in one-step rows. */
#define PM_TRANS_F 16

/* PrioritizedReplay.sample (scripts/train_iterative.py:64-73): `bs` indices drawn from
 * prios[0:size]^alpha (proportional, with replacement) using the uniforms u[bs] (NULL -> Philox)
 * exactly as np.random.choice does (cdf, searchsorted right); writes idx [bs] and the IS weight
 * w [bs] = (size*P(i))^-beta / max. Scratch: `work` of pm_per_work_bytes(cap) bytes. */
int64_t pm_per_work_bytes(int64_t cap);
int pm_per_sample(const float* prios, int64_t size, float alpha, float beta, const double* u, uint64_t seed,
                  uint64_t counter, int64_t* idx, float* w, int32_t bs, void* work, void* stream);

/* update_priorities (train_iterative.py:74-76): prios[idx[j]] = |err[j]| + 1e-6, sequential order
 * (the last duplicate index wins). */
int pm_per_update(float* prios, const int64_t* idx, const float* err, int32_t bs, void* stream);
/* Full rebuild of a PER sum tree over prios[0, cap) (leaves prio^alpha, then both node levels) into
 * `work` (pm_per_work_bytes(cap)): the tree pm_rollout_push maintains, after the host changed
 * priorities by other means (ABI 18). */
int pm_per_build(const float* prios, int64_t cap, float alpha, void* work, void* stream);

/* ---------------------------------------------------------------- self-play learner (K1+K2+K3+K4) */

/* Device control block (one per shard): the loop counters of scripts/train_iterative.py:106-118,
 * kept on the device so a vector step never syncs the host. */
typedef struct pm_ctrl {
    uint64_t step;           /* vector steps done                                       */
    int64_t pos, size;       /* replay ring position / fill (memory.pos, len(buffer))     */
    int64_t train_steps;     /* train_step() calls that updated (Adam t, target sync)     */
    int64_t frame_idx;       /* beta annealing counter (:136-137)                        */
    int64_t episodes;        /* global_episode_count (:107,234)                          */
    double epsilon;          /* exploration rate of B (:106,261)                         */
    float max_prio;          /* PER max priority for the next push (:57)                 */
    float last_loss;         /* loss of the last update                                  */
    int64_t ep_step;         /* episodes finished during the current vector step          */
    int64_t win_A, ep_A, win_P, ep_P; /* wins / episodes of B vs modelA and vs pool (:247-248) */
    double reward_B;         /* sum of rB over finished episodes                          */
    int32_t status;          /* bit 0: the push-row hand-off inside k_learn timed out; the learner
                                computes those rows itself from then on (results unchanged);
                                bit 1: an update scattered a NaN priority (a diverged loss: its PER
                                leaf is 0, never sampled; the reference's np.random.choice raises);
                                bit 2: k_learn's tree-refresh block never received the learner's
                                priorities (bounded poll): the sum tree was left stale, until
                                pm_selfplay_repair_tree rebuilds it (bit 2 -> bit 3);
                                bit 3: a stale tree was repaired (informational: state consistent) */
    int32_t max_bits;        /* pm_selfplay_commit scratch: float bits of max(prios); 0 between steps */
} pm_ctrl;

/* One shard of the batched self-play learner: every buffer is a device pointer, [n] = per arena. */
typedef struct pm_selfplay {
    pm_env_params env;
    pm_env_state st;
    int32_t *opp;            /* [n] opponent of the running episode: 0 = modelA, 1..n_pool = pool  */
    float *ep_reward;        /* [n] ep_reward of B (:238,245)                                     */
    float *w_opp;            /* [1+n_pool][PM_QNET_NW] opponent effective weights                */
    float *paramsB;          /* [PM_QNET_NP] modelB parameter block (trained heads)              */
    float *paramsT;          /* [PM_QNET_NP] targetB parameter block (eval mode: mu only)         */
    float *w_B;              /* [PM_QNET_NW] modelB acting weights for the current step           */
    float *adam_m, *adam_v;  /* [PM_QNET_NHEAD] Adam state                                        */
    float *trans;            /* [cap][PM_TRANS_F] replay ring                                     */
    float *prios;            /* [cap] priorities                                                  */
    void *per_work;          /* pm_per_work_bytes(cap): PER sum tree (16-byte aligned, as prios)  */
    int64_t *idx;            /* [batch] sampled indices                                           */
    float *isw;              /* [batch] IS weights                                                */
    float *grad;             /* [PM_QNET_NHEAD + 8] grads + packed counters (all-reduced when sharded) */
    int64_t *partials;       /* [ceil(n/256)][8] per-block episode counters of the rollout          */
    float *obsA, *obsB;      /* [n][7] observations of the current step (written by the env kernel) */
    int8_t *aA, *aB;         /* [n] actions of the current step (written by the act kernel)        */
    float *hfeat;            /* [4 * batch + 8][80], zero-filled before the first step: batch forward
                                scratch: rows [0, batch) features of s, Q values at 64.. (stable rows);
                                rows [batch, 2 batch) the push rows k_learn's block 1 hands to the
                                learner; row 2 batch word 0 its flag, word 1 the tree-refresh epoch;
                                rows 2 batch + 1 .. the learner -> tree-refresh granules (ABI 21);
                                rows [2 batch + 8, 4 batch + 8) the push rows as tagged 8-byte
                                granules, [batch][76] (ABI 22) */
    float *learn_heads;      /* [3][264] next update's modelB heads (fresh noise) and targetB heads in
                                MFMA fragment order, and that noise (epsilon-buffer layout)        */
    pm_ctrl *ctrl;
    int32_t *opp_list;       /* [n] per 256-arena block: its arenas grouped by opponent net (ascending)  */
    int32_t *opp_cnt;        /* [ceil(n/256)][n_pool+1] (offset << 16 | count) of each net in the block;
                                written by the env kernel (and init) for the next act, n_pool < 64   */
    int32_t n, n_pool, batch, world;
    int32_t chunk_A, chunk_P;  /* act grouping: arenas per chunk for modelA / pool nets (multiples of
                                  256 use opp_list; others compact opp in the act kernel)        */
    int32_t fuse_apply;        /* world == 1: learn also applies (pm_selfplay_apply is then a no-op) */
    int32_t _pad0;
    int64_t cap;
    double gamma, alpha, lr, beta1, beta2, adam_eps;  /* train_iterative.py:33-37, torch.optim.Adam defaults */
    double min_epsilon, epsilon_decay, pool_ratio, beta_start;
    int64_t beta_frames, target_update_interval;
    uint64_t seed_env;       /* rank-specific: serves, opponents, epsilon draws */
    uint64_t seed_net;       /* rank-independent: NoisyNet noise, so replicas stay identical */
    float *featB;            /* nullable [ceil(n/32)][8][64][4]: modelB's hidden features of the current
                                observations (ABI 11), computed ahead by the side-A act work (the learner
                                launch's extra blocks, pm_selfplay_act_part A / ALL); pm_selfplay_actenv
                                then evaluates only the heads. NULL: actenv computes the features */
    float *frow;             /* nullable [cap][64] (ABI 16): ReLU(modelB's hidden features) of every replay
                                row's s, written at push time by pm_selfplay_actenv from featB (the features
                                are frozen: train_iterative.py:97). Needs featB. */
    int32_t frow_ready;      /* nonzero: every replay row with a nonzero priority was pushed through actenv
                                since modelB's feature layers last changed, so frow is current; then
                                pm_selfplay_step_multi runs updates 1..U-1 as ONE single-workgroup launch
                                (k_learn_multi) instead of 3 launches per update */
    int32_t gB_ready;        /* host-set, as frow_ready (ABI 26): nonzero = gB holds, tile by tile, modelB's greedy
                                action for the observations now in obsB or the sentinel, i.e. the last launch
                                that wrote them was a pm_selfplay_learn_act for which pm_selfplay_act_ahead
                                answers 1. Zero after anything else that changes the observations, the
                                opponents or modelB (pm_selfplay_act_part A / ALL, prepare, init): featB is
                                then current for every tile and pm_selfplay_actenv reads it */
    int8_t *gB;              /* nullable [n] (ABI 26): modelB's greedy action (0..2) for the observations now in
                                obsB, stored by the feature blocks of pm_selfplay_learn_act once the learner
                                has published the next step's acting heads (gheads); pm_selfplay_actenv then
                                reads one byte per arena instead of 256 B of featB and runs no head pass.
                                PM_GB_NONE in all 32 arenas of a feature tile: that tile's hand-off timed out,
                                its features are in featB as before (the results are the same bits).
                                Fill with PM_GB_NONE before the first step. Not sp->aB: aB stays "the action
                                taken last step". Needs featB, gheads, fuse_apply, no frow */
    uint64_t *gheads;        /* nullable [PM_GHEADS_LEN], zero-filled before the first step (ABI 26): the
                                learner -> feature blocks hand-off inside pm_selfplay_learn_act. Granule k < 260
                                = (epoch tag << 32 | float bits) of folded acting head value k of the next
                                step (Wh [4][64] | bh [4]); word PM_GHEADS_EPOCH = the epoch, bumped by the
                                learner at the end of every launch that publishes */
} pm_selfplay;
#define PM_GB_NONE 3
#define PM_GHEADS_EPOCH 260
#define PM_GHEADS_LEN 264

/* Limits: 1 <= batch <= PM_MAX_BATCH (one learner workgroup), batch < n <= cap (every vector step
 * pushes n > batch transitions, which keeps the tracked max priority exact), n_pool <= 4096. */
#define PM_MAX_BATCH 256

/* One vector step of scripts/train_iterative.py:239-245 for all n arenas, as device work only:
 *   rollout: act (both players, :240-241; matrix-core kernel, which also draws this step's PER
 *            sample, :64-73, into sp->idx / sp->isw once the replay will hold >= batch) then env
 *            step (:242) + replay push (:243) + episode bookkeeping (:245-249, next opponent
 *            :235-236, env.reset :238);
 *   learn:   once the replay holds >= batch transitions: double-DQN loss/grads + priority update
 *            (train_step, :132-164) on the sampled batch, leaving grads and the finished-episode
 *            count in sp->grad; keeps the PER sum tree in sp->per_work current (incl. the next push);
 *   apply:   grads /= world, Adam on the 520 head parameters (:159-161), target sync every
 *            target_update_interval updates (:166-168), epsilon decay per finished episode
 *            (:261), replay/step counters, next step's acting noise (:125).
 * A sharded learner all-reduces sp->grad [PM_QNET_NHEAD + 8] (sum) between learn and apply.
 * pm_selfplay_step = rollout + learn + apply (unsharded). pm_selfplay_init serves every arena,
 * draws first opponents and folds the acting weights of step ctrl->step. */
int pm_selfplay_init(const pm_selfplay* sp, void* stream);
/* Re-derive everything the device keeps that follows from host-visible state: the weights that
 * follow from paramsB/paramsT (acting weights of step ctrl->step, the next update's noisy / target
 * heads) and a full rebuild of the PER sum tree from prios + ctrl. Call after the host changed
 * parameters, priorities or replay counters (checkpoint load, reset_B, promotion). Called by
 * pm_selfplay_init. */
int pm_selfplay_prepare(const pm_selfplay* sp, void* stream);
/* After ctrl.status bit 2 (a tree-refresh timeout): full rebuild of the PER sum tree from prios + ctrl,
 * then status bit 2 -> bit 3 (ABI 23). Test hook: PONGMI_TR_FORCE_TIMEOUT=1 makes the refresh block's
 * poll time out at once. */
int pm_selfplay_repair_tree(const pm_selfplay* sp, void* stream);
int pm_selfplay_rollout(const pm_selfplay* sp, void* stream); /* = pm_selfplay_act + pm_selfplay_env */
int pm_selfplay_act(const pm_selfplay* sp, void* stream);     /* actions -> sp->aA/aB; PER sample    */
int pm_selfplay_env(const pm_selfplay* sp, void* stream);     /* tick + push + bookkeeping + serves   */
int pm_selfplay_learn(const pm_selfplay* sp, void* stream);
int pm_selfplay_apply(const pm_selfplay* sp, void* stream);
int pm_selfplay_step(const pm_selfplay* sp, void* stream);

/* Overlapped stepping. The opponents' greedy actions (side A: modelA / pool nets, :240) depend only
 * on the observations and opponent ids k_env writes, not on anything the learner updates, and the
 * learner is a single workgroup, so the next vector step's side-A act rides in the learner's launch
 * on otherwise idle CUs.
 *   pm_selfplay_act_part: part PM_ACT_ALL = pm_selfplay_act; PM_ACT_B = PER sample + modelB's
 *     epsilon-greedy act (select_action_B, :124-130) only; PM_ACT_A = side A only.
 *   pm_selfplay_learn_act: pm_selfplay_learn, plus side-A actions for the observations the last
 *     pm_selfplay_env wrote (the next vector step's), into sp->aA.
 *   pm_selfplay_actenv: act_part(B) + env fused into one launch (k_actenv): every 256-arena block
 *     computes modelB's greedy actions for its arenas on the matrix cores and ticks them; the
 *     ceil(batch / 8) PER sampler blocks (8 samples each) also compute the batch rows k_env's forward
 *     blocks would, one 16-column tile per block (its samples' s and s' rows). Bit-identical to
 *     act_part(B) + env.
 *   pm_selfplay_step_overlap = actenv + learn_act + apply (unsharded).
 * Contract: before act_part(B) / actenv / step_overlap, sp->aA must hold side-A actions for the current
 * observations (pm_selfplay_act_part(A), or learn_act after the last env). Results are
 * bit-identical to pm_selfplay_step. */
#define PM_ACT_ALL 0
#define PM_ACT_B 1
#define PM_ACT_A 2
int pm_selfplay_act_part(const pm_selfplay* sp, int32_t part, void* stream);
int pm_selfplay_learn_act(const pm_selfplay* sp, void* stream);
int pm_selfplay_actenv(const pm_selfplay* sp, void* stream);
int pm_selfplay_step_overlap(const pm_selfplay* sp, void* stream);
/* Actions ahead (ABI 26). 1 if pm_selfplay_learn_ex(sp, mode, with_act) would leave modelB's greedy actions
 * for the next step in sp->gB instead of its features in sp->featB (pm_selfplay_learn_act = mode
 * PM_UPD_FIRST | PM_UPD_LAST with the act; pm_selfplay_step_overlap ends with it): the fused U = 1 step
 * (fuse_apply, both mode bits, with_act) with featB, gB and gheads set, frow NULL, and a learner grid
 * whose feature blocks are all resident beside the learner with at most two 32-arena tiles per wave
 * (up to configs[2]'s 65 536 arenas and somewhat above on a 256-CU device); 0 otherwise, and always
 * with PONGMI_ACT_AHEAD=0 in the environment (read per call: the A/B switch). The caller sets
 * sp->gB_ready to this answer for the next pm_selfplay_actenv, and to 0 once anything else rewrote the
 * observations or the networks. Test hook: PONGMI_AHEAD_FORCE_TIMEOUT=1 makes the feature blocks' poll
 * for the heads expire at once (every tile then takes the featB path). */
int pm_selfplay_act_ahead(const pm_selfplay* sp, int32_t mode, int32_t with_act);

/* Replay ratio: U >= 1 double-DQN updates per vector step. The reference trains once per env step
 * (train_iterative.py:243-244), i.e. once per pushed transition; U = n keeps that ratio for n arenas.
 *   update 0 (mode PM_UPD_FIRST) trains on the batch k_act_sp drew with this step's push pending, as
 *     the U = 1 step does, and carries the step's episode counters and epsilon decay (:245-261);
 *   updates 1..U-1 draw their batch with pm_selfplay_resample (PER sample + batch forward over the
 *     replay as this step's push left it; frame_idx, hence beta and the Philox draw, advance per
 *     update, :136-137) and run pm_selfplay_learn_ex / _apply_ex in mode 0;
 *   pm_selfplay_commit closes the step: max_prio = max(prios) over the replay (memory.push stores
 *     prios.max(), :57 — U * batch >= n scatters can lower the array maximum below the running
 *     maximum the U = 1 step tracks), the sum tree's nodes over the next push range, pos/size/step.
 * PM_UPD_FIRST | PM_UPD_LAST is the U = 1 update (pm_selfplay_learn / pm_selfplay_apply).
 * pm_selfplay_step_multi = actenv + learn_ex(FIRST, side-A act) + (U - 1) x [resample +
 * learn_ex(0)] + commit, unsharded, under step_overlap's contract (sp->aA holds side-A actions for
 * the current observations); U = 1 is pm_selfplay_step_overlap. Sharded callers run the same sequence
 * with an all-reduce of sp->grad and pm_selfplay_apply_ex after every learn_ex. */
#define PM_UPD_FIRST 1
#define PM_UPD_LAST 2
int pm_selfplay_learn_ex(const pm_selfplay* sp, int32_t mode, int32_t with_act, void* stream);
int pm_selfplay_apply_ex(const pm_selfplay* sp, int32_t mode, void* stream);
int pm_selfplay_resample(const pm_selfplay* sp, void* stream);
int pm_selfplay_commit(const pm_selfplay* sp, void* stream);
int pm_selfplay_step_multi(const pm_selfplay* sp, int32_t updates, void* stream);

/* ---------------------------------------------------------------- sharded steps (configs[3]) */

/* The learner's exchange step as a library-owned RCCL communicator. The reference is
 * single-process (scripts/train_iterative.py:80); the build shards arenas over one process per GPU
 * and sums the learner's gradient buffer once per update. Through torch.distributed that all-reduce
 * runs on the process group's own stream (an event hand-off each way) behind a Python call; the
 * *_step_sharded calls below issue a whole sharded vector step from C, with ncclAllReduce enqueued on
 * the caller's stream between the kernels (results identical to the Python sequence).
 *   rccl_path: the RCCL shared library to bind (dlopen at run time; pass the one the process already
 *     loaded, e.g. torch's bundled librccl.so, so a single RCCL instance serves both).
 *   pm_comm_unique_id: rank 0 creates the 128-byte id; the caller broadcasts it to every rank.
 *   pm_comm_init: collective over nranks processes (ncclCommInitRank on the current device).
 *   pm_comm_allreduce_f32: in-place SUM all-reduce of n floats on `stream`.
 *   pm_comm_info: the communicator's own view of the group, from RCCL itself (ncclCommCount,
 *     ncclCommUserRank, ncclCommCuDevice): a caller proves a sharded run really spans N ranks. */
#define PM_COMM_ID_BYTES 128
typedef struct pm_comm pm_comm;
int pm_comm_unique_id(const char* rccl_path, uint8_t* id);
int pm_comm_init(const char* rccl_path, const uint8_t* id, int32_t nranks, int32_t rank, pm_comm** out);
int pm_comm_allreduce_f32(pm_comm* comm, float* buf, int64_t n, void* stream);
int pm_comm_destroy(pm_comm* comm);
int pm_comm_info(const pm_comm* comm, int32_t* nranks, int32_t* rank, int32_t* device);
/* One sharded DQN vector step with `updates` updates (sp->world == comm ranks, fuse_apply 0):
 * actenv; per update u: [resample (u > 0)] + learn_ex (u = 0 with the next step's side-A act) +
 * all-reduce of sp->grad + apply_ex; commit when updates > 1. Same contract as step_overlap
 * (sp->aA holds the side-A actions for the current observations). */
int pm_selfplay_step_sharded(const pm_selfplay* sp, pm_comm* comm, int32_t updates, void* stream);
/* One sharded QNetRNN vector step: rollout; per update u: [sample(u) (u > 0)] + pm_drqn_grads +
 * all-reduce of d->grad (gradients + contributing-rank count) + pm_drqn_apply. */
int pm_rnn_selfplay_step_sharded(const pm_rnn_selfplay* sp, const pm_drqn* d, pm_comm* comm, int32_t updates,
                                 void* stream);
/* pm_rnn_selfplay_step_overlap (ABI 10) with every update's gradient all-reduced in stream order. */
int pm_rnn_selfplay_step_sharded_overlap(const pm_rnn_selfplay* sp, const pm_drqn* d, pm_comm* comm, int32_t updates,
                                         void* side_stream, void* stream);

/* ---------------------------------------------------------------- launch timing (benchmarks, diagnostics)
 * pm_timer_arm(kernel) queues one launch of that kernel, on the calling process's current device,
 * to be timed: the next untimed launch carries begin/end events in its own dispatch
 * (hipExtLaunchKernel), so no marker packet enters the stream and the kernel and its neighbours run
 * exactly as unarmed (a hipEventRecord marker between two launches costs several us of GPU time on
 * ROCm). Up to 64 launches per kernel may be armed or unread at once. pm_timer_read waits for the
 * oldest timed launch and returns its duration in ms (PM_E_ARG if none is left). Never arm while
 * capturing a hipGraph. */
#define PM_TIMER_ACTENV 0   /* k_actenv: modelB's act (heads) + env tick + replay push + PER sample */
#define PM_TIMER_LEARN 1    /* k_learn: the double-DQN update + side-A act + modelB's feature layers */
#define PM_TIMER_RNN_ACT 2  /* k_rnn_act */
#define PM_TIMER_ENV_STEP 3 /* k_env_step (K1, pm_env_step) */
#define PM_TIMER_ROLLOUT 4  /* k_rollout (K9, pm_rollout) */
#define PM_TIMER_DRQN 5     /* k_dq_recur (K6: the DRQN update's persistent recurrence, pm_drqn_grads) */
#define PM_TIMER_LEARN_MULTI 6 /* k_learn_multi: updates 1..U-1 of a vector step (pm_selfplay_step_multi, ABI 23) */
#define PM_TIMER_N 7
int pm_timer_arm(int32_t kernel);
int pm_timer_read(int32_t kernel, float* ms);

/* ---------------------------------------------------------------- misc */
const char* pm_last_error(void);
int pm_abi_version(void);
int32_t pm_sizeof(int32_t which); /* 0: pm_env_params 1: pm_env_state 2: pm_ctrl 3: pm_selfplay 4: pm_drqn
                                     5: pm_drqn_stats 6: pm_rnn_ctrl 7: pm_rnn_selfplay
                                     8: pm_roll_replay 9: pm_dqn 10: pm_dqn_stats */

#ifdef __cplusplus
}
#endif
#endif /* PONGMI_H */
