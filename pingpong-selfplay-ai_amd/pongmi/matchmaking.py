"""Self-play for a population: every member's next training opponent drawn from the league's results, and a
Bradley-Terry rating of every player, on the device (pm_league_match, pm_league_rate: csrc/pm_match.hip).

The reference's learner B plays a frozen opponent A taken from a pool of earlier nets and replaced as B improves
(scripts/train_iterative.py). For a population the pool is the league: after League.evaluate, pair_stats says how
every member did against every player it met, and League.w holds every player's folded net. A Matchmaker turns that
into the next opponents without reading anything back:

    league = League(env_kw, players, pairs)                       # members first
    mm = Matchmaker(league, mode="hard", power=2, initial=net)    # owns mm.wA [n, PM_QNET_NW]
    trainer = PopulationTrainer(env, mm.wA, population, replays, ...)   # the collector plays mm.wA's rows in place
    ...
    fitness = league.evaluate(population.params, g)
    opp, total = mm.assign(g)                                     # one launch: weigh, draw, copy the nets
    rating = mm.rate()                                            # one launch: a fitness League.select accepts

Member p draws among the entries of its pair list whose opponent is another player with a net. With x the share of
the points p took against that opponent (a win 1, a draw 1/2; 0.5 when they have not played), "hard" weighs an entry
by (1 - x) ** power: the opponents p loses to (prioritised fictitious self-play; power 0 is uniform); "even" by
4 x (1 - x): the opponents p is level with. Every weight is at least 1 / 65536 of the largest, so nobody is never
drawn. match_host and rate_host restate the kernels in numpy, bit for bit.
"""
import numpy as np
import torch

from . import _lib
from ._lib import (PM_LEAGUE_MATCH_MAX, PM_LEAGUE_RATE_MAX, PM_MATCH_EVEN, PM_MATCH_HARD, PM_MATCH_POWER_MAX,
                   PM_QNET_NW, check, ptr, stream_ptr)
from .league import PBTTrainer, explore

TAG_MATCH = 11  # pm_dev.h's purpose tag of the opponent draw
MODES = {"hard": PM_MATCH_HARD, "even": PM_MATCH_EVEN}
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _mode(mode, power, who):
    if mode not in MODES and mode not in MODES.values():
        raise ValueError(f"{who}: mode {mode!r} ('hard' or 'even')")
    if isinstance(power, bool) or not isinstance(power, (int, np.integer)) or not 0 <= power <= PM_MATCH_POWER_MAX:
        raise ValueError(f"{who}: power {power!r} (an integer 0..{PM_MATCH_POWER_MAX})")
    return MODES.get(mode, mode), int(power)


def league_tables(league):
    """(pair_players int32 [n_pairs, 2], net_of int32 [n_players]) of a League's host plan: who plays each pair, and
    every player's row in league.w (-1 for the follower)."""
    pair_players = np.array([[a, b] for a, b, _ in league.pairs], np.int32).reshape(-1, 2)
    net_of = np.array([k[1] if k[0] == "member" else -1 if k[0] == "follower" else league.n + k[1]
                       for k in league.kinds], np.int32)
    return pair_players, net_of


class Matchmaker:
    """Matchmaker(league, mode="hard", power=2, seed=0, initial=None).

    league   a League whose first n players are the members 0..n-1 (members_first), n >= 1.
    mode, power   "hard": (1 - x) ** power, power 0..8; "even": 4 x (1 - x) (power is not used).
    seed     the Philox key of the draws; the counter is (member, round).
    initial  a [PM_QNET_NW] net for every row of wA, or n of them ([n, PM_QNET_NW] or a list): what the members play
             until the first assign(). None leaves the rows zero.
    A league that is not members_first, a bad mode or power, a member whose pair list is longer than
    PM_LEAGUE_MATCH_MAX = 32 767 entries, or an `initial` of the wrong size raise ValueError before anything is
    allocated.

    wA is a contiguous float32 [n, PM_QNET_NW] tensor on the league's device; assign() rewrites its rows in place, so
    a PopulationRollout (or PopulationTrainer) given `wA` plays the assigned opponents with no further call.
    pair_players and net_of are derived from the league's host plan and uploaded once."""

    def __init__(self, league, *, mode="hard", power=2, seed=0, initial=None):
        n = league.n
        if not league.members_first or n < 1:
            raise ValueError("Matchmaker: the league's first n players must be the members 0..n-1 (n >= 1)")
        self.mode, self.power = _mode(mode, power, "Matchmaker")
        longest = int(np.diff(league.player_off[:n + 1].astype(np.int64)).max())
        if longest > PM_LEAGUE_MATCH_MAX:
            raise ValueError(f"Matchmaker: a member's pair list holds {longest} entries (at most {PM_LEAGUE_MATCH_MAX})")
        if initial is not None:
            if isinstance(initial, (list, tuple)):
                if len(initial) != n or not all(isinstance(t, torch.Tensor) and t.numel() == PM_QNET_NW
                                                for t in initial):
                    raise ValueError(f"Matchmaker: initial as a list holds n = {n} [{PM_QNET_NW}] tensors")
                initial = torch.stack([t.reshape(-1) for t in initial])
            if not isinstance(initial, torch.Tensor) or initial.dtype != torch.float32 or \
                    initial.numel() not in (PM_QNET_NW, n * PM_QNET_NW):
                raise ValueError(f"Matchmaker: initial must hold {PM_QNET_NW} or n x {PM_QNET_NW} float32 values")
        self.pair_players, self.net_of = league_tables(league)
        # ---- nothing above allocates
        self.league, self.n, self.seed = league, n, int(seed) & _MASK64
        dev = league.device
        both = torch.from_numpy(np.concatenate([self.pair_players.reshape(-1), self.net_of])).to(dev)  # one copy
        self.d_pair_players, self.d_net_of = both[:2 * league.n_pairs], both[2 * league.n_pairs:]
        self.wA = torch.zeros((n, PM_QNET_NW), dtype=torch.float32, device=dev)
        if initial is not None:
            self.wA.copy_(initial.to(dev).reshape(-1, PM_QNET_NW).expand(n, PM_QNET_NW))

    def assign(self, round, stream=None):
        """Draw every member's opponent from league.pair_stats as the last evaluate left it and copy that player's
        row of league.w into wA (pm_league_match). Returns the device tensors (opp int32 [n]: the opponent's player
        index, -1 for a member with nobody to draw, whose row stays; total int32 [n]: the member's weights summed).
        Enqueues one launch and reads nothing."""
        L = self.league
        i32 = dict(dtype=torch.int32, device=L.device)
        opp, total = torch.empty(self.n, **i32), torch.empty(self.n, **i32)
        check(_lib.load().pm_league_match(ptr(L.pair_stats), ptr(self.d_pair_players), L.n_pairs, ptr(L.d_player_off),
                                          ptr(L.d_player_pairs), L.n_players, ptr(self.d_net_of), ptr(L.w), L.w.shape[0],
                                          self.n, self.mode, self.power, self.seed, int(round) & _MASK64, ptr(self.wA),
                                          ptr(opp), ptr(total), stream_ptr(stream)), "pm_league_match")
        return opp, total

    def rate(self, iterations=32, prior=1.0, stream=None):
        """Bradley-Terry strengths of every player from league.pair_stats (pm_league_rate): `iterations` Jacobi steps
        from r = 1, with `prior` games against a virtual player of strength 1, half of them won. Returns a float32
        [n_players] device tensor, members first: League.select takes it as `fitness`. Enqueues one launch."""
        L = self.league
        if L.n_players > PM_LEAGUE_RATE_MAX:
            raise ValueError(f"Matchmaker.rate: {L.n_players} players (at most {PM_LEAGUE_RATE_MAX})")
        rating = torch.empty(L.n_players, dtype=torch.float32, device=L.device)
        check(_lib.load().pm_league_rate(ptr(L.pair_stats), ptr(self.d_pair_players), L.n_pairs, ptr(L.d_player_off),
                                         ptr(L.d_player_pairs), L.n_players, int(iterations), float(prior), ptr(rating),
                                         stream_ptr(stream)), "pm_league_rate")
        return rating


def _entries(pair_stats, pair_players, player_off, player_pairs, n_players, q):
    """Player q's list resolved as the kernels do: (valid: the pair exists and its opponent is another player, o: the
    opponent (0 where not valid), g: games, s: 2 * wins of q's side + draws), one value per entry."""
    ps = np.asarray(pair_stats).astype(np.int64, copy=False).reshape(-1, 8)  # no copy of an int64 table
    pp = np.asarray(pair_players).reshape(-1, 2)
    ent = np.asarray(player_pairs)[int(player_off[q]):int(player_off[q + 1])].astype(np.int64)
    pair, side = ent >> 1, ent & 1
    valid = (pair >= 0) & (pair < len(pp))
    if not len(pp):
        zero = np.zeros(len(ent), np.int64)
        return valid, zero, zero, zero
    pc = np.where(valid, pair, 0)
    o = pp[pc, 1 - side]
    valid &= (o >= 0) & (o < n_players) & (o != q)
    g = ps[pc, 0]
    s = 2 * ps[pc, 1 + side] + ps[pc, 3]
    return valid, np.where(valid, o, 0), g, s


def match_weights_host(pair_stats, pair_players, player_off, player_pairs, n_players, net_of, n_nets, p, mode, power):
    """(q int64, o int64) per entry of member p's list: pm_league_match's integer weights (0 = not eligible) and the
    opponents the entries name."""
    mode, power = _mode(mode, power, "match_host")
    f32 = np.float32
    ok, o, g, s = _entries(pair_stats, pair_players, player_off, player_pairs, n_players, p)
    net = np.asarray(net_of, np.int64)[o]
    ok = ok & (net >= 0) & (net < n_nets)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(g == 0, f32(0.5), s.astype(f32) / (2 * g).astype(f32)).astype(f32)
    if mode == PM_MATCH_HARD:
        f = np.ones(len(x), f32)
        for _ in range(power):
            f = f * (f32(1.0) - x)
    else:
        f = (f32(4.0) * x) * (f32(1.0) - x)
    with np.errstate(invalid="ignore"):
        q = np.where(ok, f * f32(65535.0), f32(0.0)).astype(np.uint32).astype(np.int64) + 1
    return np.where(ok, q, 0), o


def match_host(pair_stats, pair_players, player_off, player_pairs, n_players, net_of, n_nets, n, mode, power, seed,
               round):
    """The numpy model of pm_league_match on the oracle's Philox restatement: (opp int32 [n], total int32 [n]). Row p
    of wA_out becomes row net_of[opp[p]] of w where opp[p] >= 0."""
    from oracle import oracle as orc
    opp, total = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    r = orc.philox64(np.arange(n), TAG_MATCH, np.full(n, int(round) & _MASK64, np.uint64), int(seed) & _MASK64)[0]
    for p in range(n):
        if player_off[p + 1] - player_off[p] > PM_LEAGUE_MATCH_MAX:
            raise ValueError(f"match_host: member {p}'s list is longer than {PM_LEAGUE_MATCH_MAX} entries")
        q, o = match_weights_host(pair_stats, pair_players, player_off, player_pairs, n_players, net_of, n_nets, p,
                                  mode, power)
        cum = np.cumsum(q)
        total[p] = cum[-1] if len(cum) else 0
        if total[p] > 0:
            t = int(orc.below(r[p], int(total[p])))
            opp[p] = o[int(np.searchsorted(cum, t, side="right"))]  # the first inclusive prefix above t
    return opp, total


def _wave_sum(a):
    """pm_dev.h's wave_sum of 64 lane values along the last axis, in its order of additions."""
    for _ in range(4):  # adjacent blocks of 2, 4, 8, 16 lanes
        a = a[..., 0::2] + a[..., 1::2]
    return (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])


def rate_host(pair_stats, pair_players, player_off, player_pairs, n_players, iterations, prior, dtype=np.float32):
    """The numpy model of pm_league_rate: float32 [n_players], bit for bit the kernel's (its additions in the kernel's
    order). dtype=np.float64 runs the same iteration in double, for judging the float32 error."""
    ft = np.dtype(dtype).type
    n_players, prior = int(n_players), ft(np.float32(prior))
    lens = np.diff(np.asarray(player_off, np.int64)[:n_players + 1])
    C = int(-(-lens.max(initial=0) // 64))
    G = np.zeros((n_players, C * 64), ft)   # games as a float where the entry counts, else 0
    O = np.zeros((n_players, C * 64), np.int64)
    M = np.zeros((n_players, C * 64), bool)
    S = np.zeros(n_players, np.int64)
    for q in range(n_players):
        ok, o, g, s = _entries(pair_stats, pair_players, player_off, player_pairs, n_players, q)
        ok = ok & (g > 0)
        k = len(ok)
        M[q, :k], O[q, :k], G[q, :k] = ok, o, np.where(ok, g, 0).astype(ft)
        S[q] = s[ok].sum()
    W = ft(0.5) * S.astype(ft) + ft(0.5) * prior
    r = np.ones(n_players, ft)
    G, O, M = (a.reshape(n_players, C, 64) for a in (G, O, M))
    for _ in range(int(iterations)):
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(M, G / (r[:, None, None] + r[O]), ft(0.0)).astype(ft)
        acc = np.zeros((n_players, 64), ft)
        for c in range(C):  # lane l: list positions l, l + 64, ... in order
            acc = acc + term[:, c, :]
        r = (W / (prior / (r + ft(1.0)) + _wave_sum(acc))).astype(ft)
    return r


class SelfPlayPBTTrainer(PBTTrainer):
    """PBTTrainer with self-play: per generation

        trainer.run(iterations); fitness = league.evaluate(population.params, g, seed)
        [rating = matchmaker.rate(rate_iterations, prior)]        # fitness="rating": the members' ratings select
        matchmaker.assign(g)                                      # next generation's opponents, into matchmaker.wA
        src_of, rank, draw = league.select(...); population.exploit(src_of); explore(population, src_of, draw, factors)

    assign runs before exploit, so a member meets the nets as they were evaluated, not the copies that replace
    them. trainer's collector must play matchmaker.wA in place (build it with wA=matchmaker.wA). No host read is
    added to PBTTrainer's: run() returns the fitness that selected in every generation as a host array
    [generations, players], read once at the end."""

    def __init__(self, trainer, league, matchmaker, *, bottom=0.25, top=0.25, factors=None, seed=0, fitness="wins",
                 rate_iterations=32, prior=1.0):
        if fitness not in ("wins", "rating"):
            raise ValueError(f"SelfPlayPBTTrainer: fitness {fitness!r} ('wins' or 'rating')")
        if matchmaker.league is not league:
            raise ValueError("SelfPlayPBTTrainer: the matchmaker belongs to another league")
        super().__init__(trainer, league, bottom=bottom, top=top, factors=factors, seed=seed)
        rows = trainer.rollout.wA
        if len(rows) != league.n or any(rows[p].data_ptr() != matchmaker.wA[p].data_ptr() for p in range(league.n)):
            raise ValueError("SelfPlayPBTTrainer: the trainer's collector does not play matchmaker.wA in place "
                             "(pass wA=matchmaker.wA to PopulationTrainer)")
        self.matchmaker, self.fitness = matchmaker, fitness
        self.rate_iterations, self.prior = int(rate_iterations), float(prior)
        self.opponents = []  # per generation: assign()'s opp, a device tensor

    def run(self, generations, iterations):
        fits = []
        for _ in range(int(generations)):
            self.trainer.run(iterations)
            g = self.generation
            fitness = self.league.evaluate(self.population.params, g, self.seed)
            if self.fitness == "rating":
                fitness = self.matchmaker.rate(self.rate_iterations, self.prior)
            else:
                fitness = fitness.clone()  # the league overwrites its tensor in the next generation
            fits.append(fitness)
            opp, _ = self.matchmaker.assign(g)
            self.opponents.append(opp)
            src_of, _, draw = self.league.select(fitness, g, bottom=self.bottom, top=self.top, seed=self.seed)
            self.population.exploit(src_of)
            explore(self.population, src_of, draw, self.factors)
            self.generation += 1
        if not fits:
            return np.zeros((0, self.league.n_players), np.float32)
        return torch.stack(fits).cpu().numpy()
