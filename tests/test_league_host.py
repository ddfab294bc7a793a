"""Host-only checks of pongmi.league: the static plan a League builds (block schedule, serve indices, the players'
pair lists, the constructors' shapes), every ValueError of its arguments, the argument checks of pm_league_serves /
pm_league_reduce / pm_pbt_select (made before any HIP call, so they answer without a GPU), the numpy model of the
selection kernel, and explore() on a host hyper-parameter table. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)
PM_E_ARG, PM_E_SIZE = -1, -2


def _league(players, pairs, **kw):
    from pongmi.league import League
    return League(ENV_KW, players, pairs, device="cpu", **kw)


def _fixed(seed=0):
    from pongmi._lib import PM_QNET_NW
    return torch.randn(PM_QNET_NW, generator=torch.Generator().manual_seed(seed))


def _mixed():
    from pongmi.play import FOLLOWER
    players = [("member", 0), ("member", 1), ("member", 2), _fixed(), FOLLOWER, ("member", 3)]
    pairs = [(0, 1, 5), (1, 0, 5), (3, 2, 130), (4, 4, 7), (4, 0, 1), (0, 1, 3)]
    return players, pairs


@pytest.mark.parametrize("per_block", [None, 128, 64, 1024])
def test_schedule_is_plan_blocks_of_the_expanded_episodes(per_block):
    from pongmi.play import COLUMNS, plan_blocks
    players, pairs = _mixed()
    L = _league(players, pairs, per_block=per_block, max_steps=500)
    net_of = [0, 1, 2, 4, -1, 3]  # members keep their index, the fixed net follows the n = 4 members
    netA = np.concatenate([np.full(e, net_of[a]) for a, _, e in pairs])
    netB = np.concatenate([np.full(e, net_of[b]) for _, b, e in pairs])
    assert np.array_equal(L.net_A, netA) and np.array_equal(L.net_B, netB)
    bn, br, order = plan_blocks(netA, netB, per_block)  # a pair has 130 episodes: None is play's rule
    assert np.array_equal(L.blk_nets, bn) and np.array_equal(L.blk_range, br) and np.array_equal(L.order, order)
    assert L.n == 4 and L.n_nets == 5 and L.E == 151 and L.n_pairs == 6 and L.n_players == 6
    assert np.array_equal(L.pair_first, [0, 5, 10, 140, 147, 148, 151])
    per_col = -(-int(br[:, 1].max()) // COLUMNS)
    assert L.wave_steps == 500 * per_col + per_col
    # the one upload holds the plan, in the plan's order
    assert np.array_equal(L.d_blk_nets.numpy(), bn.reshape(-1)) and np.array_equal(L.d_order.numpy(), order)
    assert np.array_equal(L.d_pair_first.numpy(), L.pair_first)
    assert np.array_equal(L.d_player_pairs.numpy(), L.player_pairs)
    assert abs(L.column_share() - 151 / (128 * len(bn))) < 1e-12


def test_default_per_block_is_the_largest_pair_below_128_episodes():
    from pongmi.play import plan_blocks
    L = _league([0, 1, 2], [(0, 1, 16), (1, 2, 77), (2, 0, 3)])
    assert L.per_block == 77
    bn, br, order = plan_blocks(L.net_A, L.net_B, 77)
    assert np.array_equal(L.blk_range, br) and len(br) == 3
    L = _league([0, 1, 2], [(0, 1, 16), (1, 2, 128)])
    assert L.per_block is None
    assert np.array_equal(L.blk_range, plan_blocks(L.net_A, L.net_B, None)[1])


def test_serve_idx_under_both_crn_settings():
    players, pairs = _mixed()
    first = np.cumsum([0] + [e for _, _, e in pairs])
    within = np.concatenate([np.arange(e) for _, _, e in pairs])
    for per_block in (None, 64):
        L = _league(players, pairs, per_block=per_block, crn=True)
        assert np.array_equal(L.serve_idx, within[L.order])
        assert np.array_equal(np.sort(L.order), np.arange(L.E))
        # (0, 1) and (1, 0): the same serve index episode by episode
        slot_of = np.argsort(L.order)
        assert np.array_equal(L.serve_idx[slot_of[first[0]:first[1]]], L.serve_idx[slot_of[first[1]:first[2]]])
        L = _league(players, pairs, per_block=per_block, crn=False)
        assert np.array_equal(L.serve_idx, L.order)
        assert np.array_equal(L.d_serve_idx.numpy(), L.serve_idx)


def test_player_lists_hold_every_pair_once_per_side():
    players, pairs = _mixed()
    L = _league(players, pairs)
    off, lst = L.player_off, L.player_pairs
    assert off[0] == 0 and off[-1] == 2 * len(pairs) and len(off) == len(players) + 1
    assert sorted(lst.tolist()) == list(range(2 * len(pairs)))  # every (pair, side) exactly once
    for q in range(len(players)):
        mine = lst[off[q]:off[q + 1]].tolist()
        want = sorted([2 * k for k, pr in enumerate(pairs) if pr[0] == q] + [2 * k + 1 for k, pr in enumerate(pairs) if pr[1] == q])
        assert mine == want, q
    assert off[5] == off[6]  # member 3 plays in no pair: an empty list
    assert lst[off[4]:off[5]].tolist() == [6, 7, 8]  # the follower meets itself: both sides of pair 3


def test_round_robin_and_versus_shapes():
    from pongmi.league import League
    from pongmi.play import FOLLOWER
    L = League.round_robin(ENV_KW, 4, 16, device="cpu")
    assert L.n == 4 and L.n_players == 4 and L.n_pairs == 12 and L.E == 192 and L.members_first
    assert [(a, b) for a, b, _ in L.pairs] == [(i, j) for i in range(4) for j in range(4) if i != j]
    assert L.per_block == 16 and L.n_blocks == 12
    assert np.diff(L.player_off).tolist() == [6, 6, 6, 6]
    L = League.round_robin(ENV_KW, 4, 16, both_sides=False, device="cpu")
    assert [(a, b) for a, b, _ in L.pairs] == [(i, j) for i in range(4) for j in range(i + 1, 4)]
    L = League.versus(ENV_KW, 3, [_fixed(1), FOLLOWER], 128, device="cpu")
    assert L.n == 3 and L.n_players == 5 and L.n_nets == 4 and L.members_first
    assert L.pairs == [(3, 0, 128), (3, 1, 128), (3, 2, 128), (4, 0, 128), (4, 1, 128), (4, 2, 128)]
    assert np.array_equal(L.net_A[::128], [3, 3, 3, -1, -1, -1]) and np.array_equal(L.net_B[::128], [0, 1, 2, 0, 1, 2])
    assert L.n_blocks == 6 and L.column_share() == 1.0
    assert torch.equal(L.w[3], _fixed(1)) and not L.w[:3].any()
    with pytest.raises(ValueError):
        League.versus(ENV_KW, 3, [("member", 1)], 8, device="cpu")


@pytest.mark.parametrize("players,pairs,kw", [
    ([0, 1], [(0, 2, 4)], {}),                       # a player index out of range
    ([0, 1], [(-1, 1, 4)], {}),
    ([0, 1], [(0, 1, 0)], {}),                       # episodes < 1
    ([0, 1], [(0, 0, 4)], {}),                       # a member against itself
    ([("member", 0), ("member", 2)], [(0, 1, 4)], dict(n=2)),  # a member index >= n
    ([0, 1], [(0, 1, 4)], dict(per_block=0)),
    ([0, 1], [(0, 1, 4)], dict(per_block=1025)),
    ([0, -2], [(0, 1, 4)], {}),                      # neither a member nor FOLLOWER
    ([0, 1], [(0, 1)], {}),                          # not a triple
    ([0, torch.zeros(5)], [(0, 1, 4)], {}),          # a fixed net of the wrong size
])
def test_bad_arguments_raise_value_error(players, pairs, kw):
    with pytest.raises(ValueError):
        _league(players, pairs, **kw)


def test_self_pairs_of_follower_and_fixed_nets_are_allowed():
    from pongmi.play import FOLLOWER
    L = _league([FOLLOWER, _fixed()], [(0, 0, 3), (1, 1, 2)])
    assert L.n == 0 and L.n_nets == 1 and L.E == 5
    assert L.player_pairs.tolist() == [0, 1, 2, 3] and L.player_off.tolist() == [0, 2, 4]


def test_entry_points_check_their_arguments_without_a_gpu():
    from pongmi import _lib
    from pongmi.env import env_params
    L = _lib.load()
    prm = env_params(**ENV_KW)
    p = ctypes.byref(prm)
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)  # a non-null address: every call below is rejected before it is used
    # pm_league_serves
    assert L.pm_league_serves(p, a, 0, 0, a, -1, None) == PM_E_SIZE
    assert L.pm_league_serves(None, None, 0, 0, None, 0, None) == 0  # m == 0: a no-op
    assert L.pm_league_serves(None, a, 0, 0, a, 4, None) == PM_E_ARG
    assert L.pm_league_serves(p, None, 0, 0, a, 4, None) == PM_E_ARG
    assert L.pm_league_serves(p, a, 0, 0, None, 4, None) == PM_E_ARG
    bad = env_params(**ENV_KW)
    bad.speed_scale_every = 0
    assert L.pm_league_serves(ctypes.byref(bad), a, 0, 0, a, 4, None) == PM_E_ARG
    assert b"speed_scale_every" in L.pm_last_error()
    # pm_league_reduce
    assert L.pm_league_reduce(a, a, a, a, -1, a, a, 1, a, a, a, None) == PM_E_SIZE
    assert L.pm_league_reduce(a, a, a, a, 1, a, a, -1, a, a, a, None) == PM_E_SIZE
    for k in (0, 1, 2, 3, 8):  # scoreA, scoreB, length, pair_first, pair_stats with n_pairs > 0
        args = [a, a, a, a, 2, a, a, 0, a, a, a, None]
        args[k] = None
        assert L.pm_league_reduce(*args) == PM_E_ARG, k
    for k in (5, 6, 9, 10):  # player_off, player_pairs, player_stats, fitness with n_players > 0
        args = [a, a, a, a, 2, a, a, 3, a, a, a, None]
        args[k] = None
        assert L.pm_league_reduce(*args) == PM_E_ARG, k
    assert L.pm_league_reduce(None, None, None, None, 0, None, None, 0, None, None, None, None) == 0
    # pm_pbt_select
    for n, nb, nt in ((0, 0, 1), (_lib.PM_DQN_POP_MAX + 1, 0, 1), (-3, 0, 1), (8, -1, 1), (8, 0, 0), (8, 5, 4), (1, 1, 1)):
        assert L.pm_pbt_select(a, n, nb, nt, 0, 0, a, a, a, None) == PM_E_SIZE, (n, nb, nt)
    for k in (0, 6, 7, 8):
        args = [a, 8, 2, 2, 0, 0, a, a, a, None]
        args[k] = None
        assert L.pm_pbt_select(*args) == PM_E_ARG, k


def _fitness_cases(n, rng):
    yield "equal", np.full(n, 0.5, np.float32)
    yield "ties", (rng.integers(0, 4, n) / 4).astype(np.float32)
    f = rng.random(n).astype(np.float32)
    f[n // 2] = np.nan
    yield "nan", f


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_select_host_properties(n):
    from pongmi.league import select_host
    rng = np.random.default_rng(n)
    for name, f in _fitness_cases(n, rng):
        for n_bottom, n_top in {(0, 1), (n // 4, max(1, n // 4)), (n - max(1, n // 2), max(1, n // 2))}:
            src, rank, draw = select_host(f, n_bottom, n_top, seed=5, round=3)
            assert sorted(rank.tolist()) == list(range(n)), name  # a permutation
            assert src.dtype == np.int64 and rank.dtype == np.int32 and draw.dtype == np.uint32
            g = np.where(np.isnan(f), -np.inf, f)
            order = np.argsort(rank)
            assert (np.diff(g[order]) <= 0).all(), name  # better first
            same = np.diff(g[order]) == 0
            assert (np.diff(order)[same] > 0).all(), name  # ties by index
            if name == "nan":
                assert rank[n // 2] == n - 1  # the NaN ranks last (it is the only -inf)
            bottom = rank >= n - n_bottom
            assert np.array_equal(src[~bottom], np.arange(n)[~bottom])
            assert (rank[src[bottom]] < n_top).all()
            if n_bottom == 0:
                assert np.array_equal(src, np.arange(n))
            assert bottom.sum() == n_bottom
    # the draws move with round and seed, and not with the fitness
    f = rng.random(n).astype(np.float32)
    d0 = select_host(f, 0, 1, 5, 3)[2]
    assert np.array_equal(d0, select_host(f[::-1], 0, 1, 5, 3)[2])
    if n >= 64:
        assert not np.array_equal(d0, select_host(f, 0, 1, 5, 4)[2])
        assert not np.array_equal(d0, select_host(f, 0, 1, 6, 3)[2])


def test_select_host_is_the_stated_rule_on_a_small_case():
    from oracle import oracle as orc
    from pongmi.league import TAG_PBT, select_host
    f = np.array([0.5, 0.75, 0.5, np.nan, 0.75, 0.0], np.float32)
    src, rank, draw = select_host(f, 2, 2, seed=9, round=(1 << 32) + 7)
    assert rank.tolist() == [2, 0, 3, 5, 1, 4]
    r = orc.philox(np.arange(6), TAG_PBT, 7, 1, 9)  # the round's low and high word
    assert np.array_equal(draw, r[1])
    top = np.array([1, 4])  # the members of rank 0 and 1
    assert src.tolist() == [0, 1, 2, int(top[orc.below(r[0][3], 2)]), 4, int(top[orc.below(r[0][5], 2)])]
    for bad in ((0, 0), (5, 2), (-1, 1)):
        with pytest.raises(ValueError):
            select_host(f, bad[0], bad[1], 0, 0)


def test_selection_counts():
    from pongmi.league import selection_counts
    assert selection_counts(4, 0.25, 0.25) == (1, 1)
    assert selection_counts(7, 0.25, 0.25) == (1, 1)
    assert selection_counts(3, 0.25, 0.0) == (0, 1)  # top is at least 1
    assert selection_counts(64, 0.5, 0.5) == (32, 32)
    with pytest.raises(ValueError):
        selection_counts(4, 0.75, 0.5)


class _HyperTable:
    """What explore() needs of a DQNPopulation: n, the hyper table and set_hyper."""

    def __init__(self, **hyper):
        self.hyper = {k: list(v) for k, v in hyper.items()}
        self.n = len(next(iter(self.hyper.values())))
        self.calls = []

    def set_hyper(self, **kw):
        self.calls.append(sorted(kw))
        for k, v in kw.items():
            assert len(v) == self.n
            self.hyper[k] = list(v)


def test_explore_on_a_host_hyper_table():
    from pongmi.league import explore
    pop = _HyperTable(lr=[1e-3, 2e-3, 4e-3, 8e-3], gamma=[0.9, 0.95, 0.99, 0.999], seed=[0, 1, 2, 3])
    src = torch.tensor([0, 3, 2, 0])  # members 1 and 3 are replaced
    draw = np.array([3, 0b10, 1, 0xFFFFFFFD], np.uint32)  # bit 0 -> gamma (sorted first), bit 1 -> lr
    out = explore(pop, src, draw, {"lr": (0.5, 2.0), "gamma": (0.9, 1.0)})
    assert out == [1, 3] and pop.calls == [["gamma", "lr"]]
    assert pop.hyper["gamma"] == [0.9, 0.999 * 0.9, 0.99, 0.9 * 1.0]
    assert pop.hyper["lr"] == [1e-3, 8e-3 * 2.0, 4e-3, 1e-3 * 0.5]
    assert pop.hyper["seed"] == [0, 1, 2, 3]
    # the default factors touch lr only; nobody replaced: set_hyper is not called
    pop = _HyperTable(lr=[1e-3, 2e-3])
    assert explore(pop, [0, 1], [7, 7]) == [] and pop.calls == []
    assert explore(pop, [1, 1], torch.tensor([1, 0], dtype=torch.int32)) == [0]
    assert pop.hyper["lr"] == [2e-3 * 1.25, 2e-3]
    with pytest.raises(ValueError):
        explore(pop, [0, 1], [0, 0], {"momentum": (1, 2)})
    with pytest.raises(ValueError):
        explore(pop, [0, 1, 1], [0, 0, 0])
