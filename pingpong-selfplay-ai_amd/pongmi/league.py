"""A population's fitness from greedy matches, and the PBT step it drives, with no host read (pm_league_*,
pm_pbt_select: csrc/pm_league.hip).

The fitness the reference uses everywhere is a match result: eval_vs_model / eval_vs_pool
(scripts/train_iterative.py:171-196) and the round-robin (tests/test_round_robin.py:290-330). pongmi.play.play runs
such matches in the match megakernel, but draws nothing, plans its blocks and aggregates on the host on every
call. A League fixes everything static once (players, pairs, the block schedule, the players' pair lists, the weight
table) and then

    fitness = league.evaluate(population.params, round)            # fold, serves, fills, pm_play, reduce: enqueued
    src_of, rank, draw = league.select(fitness, round)             # pm_pbt_select: enqueued
    population.exploit(src_of)                                     # device gathers
    explore(population, src_of, draw)                              # the one small read: 12 n bytes

The serves are the production serve stream of pm_env_reset (Philox(seed), counter (index, round)), drawn on the
device in slot order; oracle.philox_serve restates them. With crn=True (common random numbers) the index is the
episode's index within its pair, so every pair faces the same serves in a round, and (i, j) and (j, i) the same
serves with the sides swapped; with crn=False it is the arena index.

Players are named by their index in `players`; arenas are the pairs' episodes back to back, pair k owning arenas
[pair_first[k], pair_first[k + 1]).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import PM_DQN_POP_MAX, PM_LEAGUE_STATS, PM_QNET_NP, PM_QNET_NW, check, ptr, stream_ptr
from .env import env_params
from .play import COLUMNS, FOLLOWER, MAX_SLOTS, plan_blocks

PAIR_STATS = ("games", "wins_A", "wins_B", "draws", "points_A", "points_B", "ticks", "unfinished")
PLAYER_STATS = ("games", "wins", "losses", "draws", "points_for", "points_against", "ticks", "unfinished")
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _is_member(x):
    return isinstance(x, tuple) and len(x) == 2 and x[0] == "member"


class League:
    """League(env_kw, players, pairs): who plays whom, fixed once.

    players  a list; an entry is ("member", p) or a plain index p >= 0 (member p of the population whose stacked
             parameters evaluate() takes), FOLLOWER (the HardcodedBallFollower), or a fixed net: a float32
             [PM_QNET_NW] tensor of effective weights, or anything pongmi.evaluate.folded_weights takes (a QNet
             module, a (state_dict, fold mode) pair), folded once here.
    pairs    [(player_A, player_B, episodes)] by player index. A player may meet itself only if it is the
             follower or a fixed net.
    n        the number of members (default: one more than the largest member index named).
    per_block, max_steps  as pongmi.play.play's; per_block None = the largest pair when every pair has fewer than
             128 episodes (one block per pair), else play's rule.
    Bad values raise ValueError before anything is allocated.

    The host plan stays on the object as numpy arrays (net_A / net_B per arena, blk_nets, blk_range, order,
    serve_idx, pair_first, player_off, player_pairs); the device copies are uploaded once, in one transfer."""

    def __init__(self, env_kw, players, pairs, *, n=None, device="cuda", per_block=None, crn=True, max_steps=1_000_000):
        players, pairs = list(players), [tuple(pr) for pr in pairs]
        kinds = []  # per player: ("member", p) | ("follower",) | ("fixed", j)
        fixed = []
        for q, pl in enumerate(players):
            if _is_member(pl) or (_is_int(pl) and pl >= 0):
                p = pl[1] if _is_member(pl) else pl
                if not _is_int(p) or p < 0:
                    raise ValueError(f"League: player {q}: member index {p!r}")
                kinds.append(("member", int(p)))
            elif _is_int(pl):
                if pl != FOLLOWER:
                    raise ValueError(f"League: player {q}: {pl} is neither a member index nor FOLLOWER")
                kinds.append(("follower",))
            else:
                if isinstance(pl, torch.Tensor) and (pl.dtype != torch.float32 or pl.numel() != PM_QNET_NW):
                    raise ValueError(f"League: player {q}: a fixed net given as a tensor holds {PM_QNET_NW} float32 "
                                     "effective weights")
                kinds.append(("fixed", len(fixed)))
                fixed.append(pl)
        named = [k[1] for k in kinds if k[0] == "member"]
        if n is None:
            n = max(named) + 1 if named else 0
        if not _is_int(n) or not 0 <= n <= PM_DQN_POP_MAX:
            raise ValueError(f"League: n {n!r} (0..{PM_DQN_POP_MAX})")
        n = int(n)
        for q, k in enumerate(kinds):
            if k[0] == "member" and k[1] >= n:
                raise ValueError(f"League: player {q}: member {k[1]} of a population of {n}")
        for k, pr in enumerate(pairs):
            if len(pr) != 3 or not all(_is_int(x) for x in pr):
                raise ValueError(f"League: pair {k}: {pr!r} is not (player_A, player_B, episodes)")
            a, b, ep = pr
            if not (0 <= a < len(players) and 0 <= b < len(players)):
                raise ValueError(f"League: pair {k}: player index outside [0, {len(players)})")
            if ep < 1:
                raise ValueError(f"League: pair {k}: episodes {ep} (>= 1)")
            if a == b and kinds[a][0] == "member":
                raise ValueError(f"League: pair {k}: member player {a} against itself")
        if per_block is not None and (not _is_int(per_block) or not 1 <= per_block <= MAX_SLOTS):
            raise ValueError(f"League: per_block {per_block!r} (1..{MAX_SLOTS})")
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError(f"League: max_steps {max_steps} (>= 0)")
        episodes = np.array([pr[2] for pr in pairs], np.int64)
        E = int(episodes.sum())
        if E > 2**31 - 1:
            raise ValueError(f"League: {E} episodes (at most 2^31 - 1)")
        self.params_env = env_params(**env_kw)
        # ---- the host plan
        net_of = np.array([k[1] if k[0] == "member" else FOLLOWER if k[0] == "follower" else n + k[1] for k in kinds],
                          np.int64)
        pa = np.array([pr[0] for pr in pairs], np.int64)
        pb = np.array([pr[1] for pr in pairs], np.int64)
        self.pair_first = np.concatenate([[0], np.cumsum(episodes)]).astype(np.int32)
        self.net_A = np.repeat(net_of[pa], episodes) if len(pairs) else np.zeros(0, np.int64)
        self.net_B = np.repeat(net_of[pb], episodes) if len(pairs) else np.zeros(0, np.int64)
        if per_block is None and len(pairs) and int(episodes.max()) < COLUMNS:
            per_block = int(episodes.max())
        self.blk_nets, self.blk_range, self.order = plan_blocks(self.net_A, self.net_B, per_block)
        within = np.arange(E, dtype=np.int64) - np.repeat(self.pair_first[:-1].astype(np.int64), episodes)
        self.serve_idx = (within[self.order] if crn else self.order).astype(np.int32)
        # a player's pair list: 2 * pair + side, pairs ascending, side A before side B
        entry = np.stack([2 * np.arange(len(pairs)), 2 * np.arange(len(pairs)) + 1], 1).reshape(-1)
        owner = np.stack([pa, pb], 1).reshape(-1)
        by_owner = np.argsort(owner, kind="stable")
        self.player_pairs = entry[by_owner].astype(np.int32)
        self.player_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(players)))]).astype(np.int32)
        per_col = -(-int(self.blk_range[:, 1].max(initial=0)) // COLUMNS)
        self.wave_steps = min(max_steps * per_col + per_col, 2**31 - 1)
        self.env_kw, self.players, self.pairs, self.kinds = dict(env_kw), players, pairs, kinds
        self.n, self.n_players, self.n_pairs, self.E, self.n_blocks = n, len(players), len(pairs), E, len(self.blk_nets)
        self.n_nets, self.crn, self.max_steps, self.per_block = n + len(fixed), bool(crn), max_steps, per_block
        # select() ranks the first n entries of the fitness: they must be the members, in order
        self.members_first = len(kinds) >= n and all(kinds[p] == ("member", p) for p in range(n))
        # ---- nothing above allocates
        self.device = dev = torch.device(device)
        parts = [self.blk_nets.reshape(-1), self.blk_range.reshape(-1), self.order, self.serve_idx, self.pair_first,
                 self.player_off, self.player_pairs]
        self._int = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)  # one copy
        cuts = np.cumsum([0] + [p.size for p in parts])
        (self.d_blk_nets, self.d_blk_range, self.d_order, self.d_serve_idx, self.d_pair_first, self.d_player_off,
         self.d_player_pairs) = (self._int[cuts[i]:cuts[i + 1]] for i in range(len(parts)))
        self.w = torch.zeros((max(self.n_nets, 1), PM_QNET_NW), dtype=torch.float32, device=dev)  # pads stay 0
        for j, net in enumerate(fixed):
            if not isinstance(net, torch.Tensor):
                from .evaluate import folded_weights
                net = folded_weights(net, dev)
            self.w[n + j].copy_(net.reshape(-1))
        i32 = dict(dtype=torch.int32, device=dev)
        self.score_A, self.score_B = torch.zeros(E, **i32), torch.zeros(E, **i32)
        self.length = torch.full((E,), -1, **i32)
        self.last = torch.zeros(E, dtype=torch.int8, device=dev)
        self.status = torch.zeros(1, **i32)
        self.serves = torch.zeros((E, 3), dtype=torch.float64, device=dev)  # slot order
        self.pair_stats = torch.zeros((self.n_pairs, PM_LEAGUE_STATS), dtype=torch.int64, device=dev)
        self.player_stats = torch.zeros((self.n_players, PM_LEAGUE_STATS), dtype=torch.int64, device=dev)
        self.fitness = torch.zeros(self.n_players, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def round_robin(cls, env_kw, n, episodes, both_sides=True, **kw):
        """The n members against each other: every ordered pair (i, j), i != j, or with both_sides=False every
        unordered pair i < j, `episodes` each."""
        n = int(n)
        pairs = [(i, j, episodes) for i in range(n) for j in range(n) if (i != j if both_sides else i < j)]
        return cls(env_kw, [("member", p) for p in range(n)], pairs, n=n, **kw)

    @classmethod
    def versus(cls, env_kw, n, opponents, episodes, **kw):
        """Every member as B against every opponent as A (the evaluators' sides, train_iterative.py:176-180):
        players = the n members, then the opponents (fixed nets or FOLLOWER); pairs opponent-major."""
        n, opponents = int(n), list(opponents)
        for o in opponents:
            if _is_member(o) or (_is_int(o) and o != FOLLOWER):
                raise ValueError("League.versus: an opponent is a fixed net or FOLLOWER")
        pairs = [(n + o, p, episodes) for o in range(len(opponents)) for p in range(n)]
        return cls(env_kw, [("member", p) for p in range(n)] + opponents, pairs, n=n, **kw)

    def column_share(self):
        """The share of k_play's columns that start with a slot: sum(episodes) / (128 * blocks)."""
        return self.E / (COLUMNS * self.n_blocks) if self.n_blocks else 0.0

    # ------------------------------------------------------------------ the device path
    def evaluate(self, params, round, seed=0, stream=None):
        """Play every pair's episodes with the members' nets as `params` holds them now (the stacked [n, PM_QNET_NP]
        blocks, e.g. DQNPopulation.params, read in place and folded in eval mode on every call) and serves
        (seed, round). Enqueues the fold, the serves, the fills of length / status, pm_play and the reduction; reads
        nothing back. Returns `fitness` (wins / games per player, the object's own device tensor); score_A, score_B,
        length, last (per arena), serves (per slot), pair_stats, player_stats and status stay on the object.
        Arenas cut by max_steps keep length -1 and the scores of the call before."""
        n = self.n
        if n:
            if not isinstance(params, torch.Tensor) or tuple(params.shape) != (n, PM_QNET_NP) or \
                    params.dtype != torch.float32 or not params.is_contiguous():
                raise ValueError(f"League.evaluate: params must be a contiguous float32 [n={n}, {PM_QNET_NP}] tensor")
            _lib.require_device(params, "params")
        lib = _lib.load()
        st = stream_ptr(stream)
        if n:
            check(lib.pm_qnet_fold(ptr(params), None, _lib.PM_FOLD_EVAL, 0, 0, None, ptr(self.w), n, st), "pm_qnet_fold")
        prm = ctypes.byref(self.params_env)
        check(lib.pm_league_serves(prm, ptr(self.d_serve_idx), int(seed) & _MASK64, int(round) & 0xFFFFFFFF,
                                   ptr(self.serves), self.E, st), "pm_league_serves")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            self.length.fill_(-1)
            self.status.zero_()
        check(lib.pm_play(prm, ptr(self.w), self.n_nets, ptr(self.d_blk_nets), ptr(self.d_blk_range), self.n_blocks,
                          ptr(self.d_order), ptr(self.serves), self.E, self.wave_steps, ptr(self.score_A),
                          ptr(self.score_B), ptr(self.length), ptr(self.last), ptr(self.status), st), "pm_play")
        check(lib.pm_league_reduce(ptr(self.score_A), ptr(self.score_B), ptr(self.length), ptr(self.d_pair_first),
                                   self.n_pairs, ptr(self.d_player_off), ptr(self.d_player_pairs), self.n_players,
                                   ptr(self.pair_stats), ptr(self.player_stats), ptr(self.fitness), st),
              "pm_league_reduce")
        return self.fitness

    def results(self):
        """The last evaluate's outputs as host arrays, in a dict: the only call here that synchronises. Raises
        play's RuntimeError if an episode did not finish or the kernel counted an invalid id."""
        out = {k: getattr(self, k).cpu().numpy() for k in ("score_A", "score_B", "length", "last", "pair_stats",
                                                           "player_stats", "fitness", "serves")}
        st = int(self.status.item())
        if st or (out["length"] < 0).any():
            raise RuntimeError(f"pm_play: {int((out['length'] < 0).sum())} arenas did not finish within "
                               f"{self.max_steps} steps ({st} invalid ids or cut episodes)")
        out["status"] = st
        return out

    def select(self, fitness, round, *, bottom=0.25, top=0.25, seed=0, stream=None):
        """Truncation selection over the members, the first n entries of `fitness` (pm_pbt_select): the
        floor(bottom * n) worst members each get a source drawn among the max(1, floor(top * n)) best. Returns the
        device tensors (src_of int64 [n], rank int32 [n], draw int32 [n]: the bits of the uint32 draw that
        explore() consumes). Enqueues one launch."""
        n = self.n
        if not self.members_first or n < 1:
            raise ValueError("League.select: the first n players must be the members 0..n-1")
        n_bottom, n_top = selection_counts(n, bottom, top)
        if not isinstance(fitness, torch.Tensor) or fitness.dtype != torch.float32 or fitness.numel() < n or \
                not fitness.is_contiguous():
            raise ValueError(f"League.select: fitness must be a contiguous float32 tensor of at least n = {n} entries")
        _lib.require_device(fitness, "fitness")
        dev = fitness.device
        rank = torch.empty(n, dtype=torch.int32, device=dev)
        src_of = torch.empty(n, dtype=torch.int64, device=dev)
        draw = torch.empty(n, dtype=torch.int32, device=dev)
        check(_lib.load().pm_pbt_select(ptr(fitness), n, n_bottom, n_top, int(seed) & _MASK64, int(round) & _MASK64,
                                        ptr(rank), ptr(src_of), ptr(draw), stream_ptr(stream)), "pm_pbt_select")
        return src_of, rank, draw


def selection_counts(n, bottom, top):
    """(n_bottom, n_top) = (floor(bottom * n), max(1, floor(top * n))); ValueError if they overlap."""
    if not (0.0 <= bottom <= 1.0 and 0.0 <= top <= 1.0):
        raise ValueError(f"select: bottom {bottom} / top {top} (fractions of the population)")
    n_bottom, n_top = int(math.floor(bottom * n)), max(1, int(math.floor(top * n)))
    if n_bottom + n_top > n:
        raise ValueError(f"select: {n_bottom} bottom + {n_top} top members of {n}")
    return n_bottom, n_top


def select_host(fitness, n_bottom, n_top, seed, round):
    """The numpy model of pm_pbt_select, on the oracle's Philox restatement: (src_of int64, rank int32, draw
    uint32). A NaN fitness is -inf; a is better than b iff f[a] > f[b] or (f[a] == f[b] and a < b); rank[p] = the
    members better than p; bottom members (rank >= n - n_bottom) draw a source among the n_top best."""
    from oracle import oracle as orc
    f = np.asarray(fitness, np.float32).reshape(-1).copy()
    n = f.size
    if not (1 <= n <= PM_DQN_POP_MAX and n_bottom >= 0 and n_top >= 1 and n_bottom + n_top <= n):
        raise ValueError(f"select_host: n={n} n_bottom={n_bottom} n_top={n_top}")
    f[np.isnan(f)] = -np.inf
    idx = np.arange(n)
    better = (f[:, None] > f[None, :]) | ((f[:, None] == f[None, :]) & (idx[:, None] < idx[None, :]))  # [a, p]
    rank = better.sum(0).astype(np.int32)
    who = np.empty(n, np.int64)
    who[rank] = idx
    r = orc.philox64(idx, TAG_PBT, np.full(n, int(round) & _MASK64, np.uint64), int(seed) & _MASK64)
    src_of = np.where(rank >= n - n_bottom, who[orc.below(r[0], n_top)], idx).astype(np.int64)
    return src_of, rank, r[1].astype(np.uint32)


TAG_PBT = 10  # pm_dev.h's purpose tag of the selection draw


def explore(population, src_of, draw, factors=None):
    """PBT's explore step, on the host: every replaced member p (src_of[p] != p) takes, for the j-th key of
    `factors` in sorted order, its source's value of that hyper-parameter times factors[key][(draw[p] >> j) & 1],
    applied through population.set_hyper. src_of and draw (select()'s tensors, or host sequences) are read in ONE
    transfer of 12 n bytes: the step's one synchronisation. Returns the replaced members."""
    factors = {"lr": (0.8, 1.25)} if factors is None else dict(factors)
    keys = sorted(factors)
    if len(keys) > 32:
        raise ValueError("explore: at most 32 factors (one bit of the draw each)")
    for k in keys:
        if k not in population.hyper:
            raise ValueError(f"explore: unknown hyper-parameter {k!r}")
        if len(factors[k]) != 2:
            raise ValueError(f"explore: factors[{k!r}] must be a pair")
    src_t = torch.as_tensor(src_of).reshape(-1).to(torch.int64)
    draw_t = torch.as_tensor(np.asarray(draw).view(np.int32) if isinstance(draw, np.ndarray) and draw.dtype == np.uint32
                             else draw).reshape(-1).to(device=src_t.device, dtype=torch.int32)
    n = population.n
    if src_t.numel() != n or draw_t.numel() != n:
        raise ValueError(f"explore: {src_t.numel()} sources and {draw_t.numel()} draws for {n} members")
    host = torch.cat([src_t.view(torch.int32), draw_t]).cpu().numpy()  # the one read
    src = host[:2 * n].view(np.int64)
    bits = host[2 * n:].view(np.uint32)
    replaced = [p for p in range(n) if src[p] != p]
    if not replaced:
        return replaced
    new = {}
    for j, k in enumerate(keys):
        old = list(population.hyper[k])
        vals = list(old)
        for p in replaced:
            vals[p] = old[int(src[p])] * factors[k][(int(bits[p]) >> j) & 1]
        new[k] = vals
    population.set_hyper(**new)
    return replaced


class PBTTrainer:
    """Population-based training around a pongmi.dqn.PopulationTrainer: per generation

        trainer.run(iterations); fitness = league.evaluate(population.params, g, seed)
        src_of, rank, draw = league.select(fitness, g, bottom=, top=, seed=); population.exploit(src_of)
        explore(population, src_of, draw, factors)

    with g the generation count kept across run() calls. Between trainer.run's closing read of its stats and
    explore's read of (src_of, draw) nothing synchronises. run() returns the fitness of every generation as a host
    array [generations, players], read once at the end."""

    def __init__(self, trainer, league, *, bottom=0.25, top=0.25, factors=None, seed=0):
        if league.n != trainer.population.n:
            raise ValueError(f"PBTTrainer: a league of {league.n} members for a population of {trainer.population.n}")
        selection_counts(league.n, bottom, top)
        self.trainer, self.league, self.population = trainer, league, trainer.population
        self.bottom, self.top, self.seed = float(bottom), float(top), int(seed)
        self.factors = {"lr": (0.8, 1.25)} if factors is None else dict(factors)
        self.generation = 0

    def run(self, generations, iterations):
        fits = []
        for _ in range(int(generations)):
            self.trainer.run(iterations)
            g = self.generation
            fitness = self.league.evaluate(self.population.params, g, self.seed)
            fits.append(fitness.clone())  # the league overwrites its tensor in the next generation
            src_of, _, draw = self.league.select(fitness, g, bottom=self.bottom, top=self.top, seed=self.seed)
            self.population.exploit(src_of)
            explore(self.population, src_of, draw, self.factors)
            self.generation += 1
        if not fits:
            return np.zeros((0, self.league.n_players), np.float32)
        return torch.stack(fits).cpu().numpy()
