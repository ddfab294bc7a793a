"""Host-only checks of pongmi.matchmaking: the argument checks of pm_league_match / pm_league_rate (made before any HIP
call, so they answer without a GPU), match_host on a case worked out by hand, the order of its pick frequencies,
Matchmaker's ValueErrors, and rate_host (monotone on a transitive league; against the same iteration in float64).
No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)
PM_E_ARG, PM_E_SIZE = -1, -2


def test_entry_points_check_their_arguments_without_a_gpu():
    from pongmi import _lib
    L = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)  # a non-null, 16-byte aligned address: every call below is rejected before it is used
    assert a % 16 == 0
    far = a + (1 << 30)        # a second table that overlaps nothing (never dereferenced)

    def match(**kw):
        args = dict(pair_stats=a, pair_players=a, n_pairs=3, player_off=a, player_pairs=a, n_players=4, net_of=a, w=a,
                    n_nets=4, n=2, mode=_lib.PM_MATCH_HARD, power=2, seed=0, round=0, wA_out=far, opp=a, total=a,
                    stream=None)
        args.update(kw)
        return L.pm_league_match(*args.values())

    for bad in (dict(n=0), dict(n=-1), dict(n=_lib.PM_DQN_POP_MAX + 1), dict(n=5), dict(n_pairs=-1), dict(n_nets=0),
                dict(power=9), dict(power=-1), dict(mode=2), dict(mode=-1)):
        assert match(**bad) == PM_E_SIZE, bad
        assert b"pm_league_match" in L.pm_last_error()
    for name in ("pair_stats", "pair_players", "player_off", "player_pairs", "net_of", "w", "wA_out", "opp", "total"):
        assert match(**{name: None}) == PM_E_ARG, name
        assert b"null" in L.pm_last_error()
    for name, off in (("w", 4), ("wA_out", 8), ("pair_stats", 4), ("opp", 2), ("net_of", 1)):
        assert match(**{name: (far if name == "wA_out" else a) + off}) == PM_E_ARG, name
    row = 4 * _lib.PM_QNET_NW
    for out in (a, a + 16, a + 4 * row - 16, a - 2 * row + 16):  # wA_out [2 rows] against w [4 rows]
        assert match(wA_out=out) == PM_E_ARG, out - a
        assert b"overlaps" in L.pm_last_error()

    def rate(**kw):
        args = dict(pair_stats=a, pair_players=a, n_pairs=3, player_off=a, player_pairs=a, n_players=4, iterations=8,
                    prior=1.0, rating=a, stream=None)
        args.update(kw)
        return L.pm_league_rate(*args.values())

    for bad in (dict(n_players=-1), dict(n_players=_lib.PM_LEAGUE_RATE_MAX + 1), dict(n_pairs=-1), dict(iterations=-1)):
        assert rate(**bad) == PM_E_SIZE, bad
        assert b"pm_league_rate" in L.pm_last_error()
    for bad in (dict(prior=0.0), dict(prior=-1.0), dict(prior=float("nan")), dict(prior=float("inf"))):
        assert rate(**bad) == PM_E_ARG, bad
    for name in ("pair_stats", "pair_players", "player_off", "player_pairs", "rating"):
        assert rate(**{name: None}) == PM_E_ARG, name
    assert rate(rating=a + 2) == PM_E_ARG
    # the documented no-op size: no player
    assert L.pm_league_rate(None, None, 0, None, None, 0, 32, 1.0, None, None) == 0


# One member (player 0) and three fixed nets (players 1..3): pairs (0, 1), (2, 0), (0, 3) of 4 games each. The member
# lost all four to player 1 (x = 0), took a win, a loss and two draws from player 2 as side B (s = 2 * 1 + 2 = 4 of
# 8: x = 0.5) and won all four against player 3 (x = 1).
HAND = dict(pair_stats=np.array([[4, 0, 4, 0, 0, 12, 99, 0], [4, 1, 1, 2, 5, 5, 99, 0], [4, 4, 0, 0, 12, 0, 99, 0]], np.int64),
            pair_players=np.array([[0, 1], [2, 0], [0, 3]], np.int32),
            player_off=np.array([0, 3, 4, 5, 6], np.int32), player_pairs=np.array([0, 3, 4, 1, 2, 5], np.int32),
            n_players=4, net_of=np.array([0, 1, 2, 3], np.int32), n_nets=4)


@pytest.mark.parametrize("mode,power,want", [
    ("hard", 1, [65536, 32768, 1]),   # f = 1, 0.5, 0: 65535 + 1, trunc(32767.5) + 1, 0 + 1
    ("hard", 2, [65536, 16384, 1]),   # f = 1, 0.25, 0: trunc(16383.75) + 1
    ("hard", 0, [65536, 65536, 65536]),
    ("even", 1, [1, 65536, 1]),       # 4 x (1 - x) = 0, 1, 0
    ("even", 2, [1, 65536, 1]),       # the power is not used
])
def test_match_host_on_a_case_worked_by_hand(orc, mode, power, want):
    from pongmi.matchmaking import TAG_MATCH, match_host, match_weights_host
    q, o = match_weights_host(**HAND, p=0, mode=mode, power=power)
    assert q.tolist() == want and o.tolist() == [1, 2, 3]
    seen = set()
    for rnd in range(48):
        opp, total = match_host(**HAND, n=1, mode=mode, power=power, seed=5, round=rnd)
        assert opp.dtype == np.int32 and total.dtype == np.int32 and total.tolist() == [sum(want)]
        d = orc.philox(np.array([0]), TAG_MATCH, rnd, 0, 5)[0]
        t = (int(d[0]) * sum(want)) >> 32
        pick = 1 if t < want[0] else 2 if t < want[0] + want[1] else 3  # the first inclusive prefix above t
        assert opp.tolist() == [pick], rnd
        seen.add(pick)
    assert len(seen) >= (1 if mode == "even" else 2)
    # a chosen draw: round 0 of seed 5 under hard / 1 lands where the thresholds 65536 and 98304 say
    if (mode, power) == ("hard", 1):
        d0 = int(orc.philox(np.array([0]), TAG_MATCH, 0, 0, 5)[0][0])
        t0 = (d0 * 98305) >> 32
        assert match_host(**HAND, n=1, mode="hard", power=1, seed=5, round=0)[0][0] == (1 if t0 < 65536 else 2 if t0 < 98304 else 3)


def test_match_host_ineligible_entries_and_empty_lists():
    from pongmi.matchmaking import match_host, match_weights_host
    c = dict(HAND, net_of=np.array([0, -1, 4, 3], np.int32))  # player 1 is the follower, player 2's net is n_nets
    c["player_pairs"] = np.array([0, 3, 4, 6, -2, 1, 1, 2, 5], np.int32)  # + pair 3 = n_pairs, a negative entry, itself
    c["player_off"] = np.array([0, 7, 7, 8, 9], np.int32)
    q, o = match_weights_host(**c, p=0, mode="hard", power=1)
    assert q.tolist() == [0, 0, 1, 0, 0, 0, 0]  # only player 3 is left (entry 1 names pair 0's A: the member itself)
    opp, total = match_host(**c, n=1, mode="hard", power=1, seed=0, round=0)
    assert opp.tolist() == [3] and total.tolist() == [1]
    c["net_of"] = np.array([0, -1, 4, -1], np.int32)
    opp, total = match_host(**c, n=2, mode="hard", power=1, seed=0, round=0)  # player 1's list is empty
    assert opp.tolist() == [-1, -1] and total.tolist() == [0, 0]
    with pytest.raises(ValueError):
        match_host(**HAND, n=1, mode="soft", power=1, seed=0, round=0)
    with pytest.raises(ValueError):
        match_host(**HAND, n=1, mode="hard", power=9, seed=0, round=0)


def test_pick_frequencies_order_as_the_weights():
    """x = 0, 0.5 and 0.75 under hard / 1: weights 65536 : 32768 : 16384, so about 2341, 1170 and 585 of 4096."""
    from pongmi.matchmaking import match_host, match_weights_host
    c = dict(HAND)
    c["pair_stats"] = HAND["pair_stats"].copy()
    c["pair_stats"][2] = [4, 3, 1, 0, 0, 0, 0, 0]
    assert match_weights_host(**c, p=0, mode="hard", power=1)[0].tolist() == [65536, 32768, 16384]
    picks = np.array([match_host(**c, n=1, mode="hard", power=1, seed=11, round=r)[0][0] for r in range(4096)])
    count = np.bincount(picks, minlength=4)
    assert count[0] == 0 and count.sum() == 4096
    assert count[1] > count[2] > count[3] > 0
    # and within five standard deviations of the weights' shares
    for k, share in ((1, 4 / 7), (2, 2 / 7), (3, 1 / 7)):
        assert abs(count[k] - 4096 * share) < 5 * (4096 * share * (1 - share)) ** 0.5, (k, count[k])


def _cpu_league(players, pairs, **kw):
    from pongmi.league import League
    L = League(ENV_KW, players, pairs, device="cpu", **kw)
    L.device = "no-such-device"  # an allocation now raises something that is not a ValueError
    return L


def test_matchmaker_raises_before_it_allocates():
    from pongmi._lib import PM_LEAGUE_MATCH_MAX, PM_QNET_NW
    from pongmi.matchmaking import Matchmaker, league_tables
    from pongmi.play import FOLLOWER
    fixed = torch.zeros(PM_QNET_NW)
    good = _cpu_league([0, 1, fixed, FOLLOWER], [(0, 1, 2), (2, 0, 2), (3, 1, 2)])
    pp, net_of = league_tables(good)
    assert pp.tolist() == [[0, 1], [2, 0], [3, 1]] and net_of.tolist() == [0, 1, 2, -1]
    assert pp.dtype == np.int32 and net_of.dtype == np.int32
    with pytest.raises(Exception) as ok:  # valid arguments reach the allocation
        Matchmaker(good)
    assert not isinstance(ok.value, ValueError)
    for kw in (dict(mode="soft"), dict(mode=2), dict(power=9), dict(power=-1), dict(power=2.0), dict(power=True),
               dict(initial=torch.zeros(5)), dict(initial=torch.zeros(PM_QNET_NW, dtype=torch.float64)),
               dict(initial=[fixed]), dict(initial=[fixed, 3])):
        with pytest.raises(ValueError):
            Matchmaker(good, **kw)
    with pytest.raises(ValueError, match="members"):
        Matchmaker(_cpu_league([FOLLOWER, 0], [(0, 1, 2)]))  # the member is not player 0
    with pytest.raises(ValueError, match="members"):
        Matchmaker(_cpu_league([FOLLOWER, fixed], [(0, 1, 2)]))  # no member at all
    # a member list over the cap: the plan's offsets are all the check reads
    off = np.array([0, 3, PM_LEAGUE_MATCH_MAX + 4, PM_LEAGUE_MATCH_MAX + 4], np.int32)
    long_ = SimpleNamespace(n=2, members_first=True, player_off=off, device="no-such-device")
    with pytest.raises(ValueError, match=str(PM_LEAGUE_MATCH_MAX)):
        Matchmaker(long_)
    # ... and the longest list it takes is a member's, not another player's
    long_.player_off = np.array([0, 3, 6, PM_LEAGUE_MATCH_MAX + 7], np.int32)
    with pytest.raises(Exception) as ok:
        Matchmaker(long_)
    assert not isinstance(ok.value, ValueError)


def test_matchmaker_on_a_host_league_keeps_initial_rows():
    """On a CPU league the object can be built (nothing is launched): wA's shape, alignment and initial rows."""
    from pongmi._lib import PM_QNET_NW
    from pongmi.league import League
    from pongmi.matchmaking import Matchmaker
    L = League(ENV_KW, [0, 1, torch.ones(PM_QNET_NW)], [(0, 1, 2), (2, 0, 2), (2, 1, 2)], device="cpu")
    net = torch.arange(PM_QNET_NW, dtype=torch.float32)
    mm = Matchmaker(L, mode="even", initial=net)
    assert mm.wA.shape == (2, PM_QNET_NW) and mm.wA.is_contiguous() and mm.wA.data_ptr() % 16 == 0
    assert torch.equal(mm.wA[0], net) and torch.equal(mm.wA[1], net)
    mm = Matchmaker(L, initial=[net, 2 * net])
    assert torch.equal(mm.wA[1], 2 * net) and mm.d_net_of.tolist() == [0, 1, 2]
    assert mm.d_pair_players.tolist() == [0, 1, 2, 0, 2, 1]
    assert not Matchmaker(L).wA.any()


def _transitive(n, games=16):
    """Every pair i < j, player i as A, scoring 0.75: 12 wins and 4 losses of 16."""
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    ps = np.zeros((len(pairs), 8), np.int64)
    ps[:, 0], ps[:, 1], ps[:, 2] = games, 3 * games // 4, games // 4
    owner = np.array(pairs).reshape(-1)
    by = np.argsort(owner, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int32)
    return dict(pair_stats=ps, pair_players=np.array(pairs, np.int32), player_off=off,
                player_pairs=np.arange(2 * len(pairs))[by].astype(np.int32), n_players=n)


def _random_league(n, seed):
    """Every ordered pair of n players with random results of 1..40 games, draws included."""
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    g = rng.integers(1, 41, len(pairs))
    wa = rng.integers(0, g + 1)
    wb = rng.integers(0, g - wa + 1)
    ps = np.zeros((len(pairs), 8), np.int64)
    ps[:, 0], ps[:, 1], ps[:, 2], ps[:, 3] = g, wa, wb, g - wa - wb
    owner = np.array(pairs).reshape(-1)
    by = np.argsort(owner, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int32)
    return dict(pair_stats=ps, pair_players=np.array(pairs, np.int32), player_off=off,
                player_pairs=np.arange(2 * len(pairs))[by].astype(np.int32), n_players=n)


def test_rate_host_decreases_down_a_transitive_league():
    from pongmi.matchmaking import rate_host
    r = rate_host(**_transitive(6), iterations=32, prior=1.0)
    assert r.dtype == np.float32 and r.shape == (6,)
    assert (np.diff(r) < 0).all() and r[0] > 1.0 > r[-1] > 0.0
    assert np.array_equal(rate_host(**_transitive(6), iterations=0, prior=1.0), np.ones(6, np.float32))
    # one step by hand for player 0: S = 5 pairs * 24 points, W = 0.5 * 120 + 0.5; D = 1 / 2 + 5 * 16 / 2
    r1 = rate_host(**_transitive(6), iterations=1, prior=1.0)
    assert r1[0] == np.float32(60.5) / np.float32(40.5)
    # a player in no pair keeps the prior's fixed point: W = prior / 2, D = prior / (r + 1), r = 1
    c = _transitive(6)
    c["player_off"] = np.concatenate([c["player_off"], c["player_off"][-1:]])
    c["n_players"] = 7
    assert rate_host(**c, iterations=32, prior=0.5)[6] == 1.0


RATE_F64_MEASURED = 3.9e-7  # the largest relative difference over the fixtures below, as measured (3.854e-07)


def test_rate_host_agrees_with_the_iteration_in_float64():
    """rate_host in float32 (the kernel's arithmetic and addition order) against the same iteration in float64, 32
    steps, priors 1.0 and 0.5, on a transitive league of 6 (lists of 5), a transitive league of 130 (lists of 129:
    three passes of a wave) and a random league of 70 with draws (lists of 138). The largest relative difference
    measured over them is 3.9e-7 (prior 1.0 / 0.5: 1.4e-7 / 3.2e-7, 2.8e-7 / 2.7e-7 and 2.4e-7 / 3.9e-7); the bound is four
    times that, 1.56e-6, for float32 accumulation over the longest list."""
    from pongmi.matchmaking import rate_host
    worst = 0.0
    for c in (_transitive(6), _transitive(130), _random_league(70, 3)):
        for prior in (1.0, 0.5):
            r32 = rate_host(**c, iterations=32, prior=prior)
            r64 = rate_host(**c, iterations=32, prior=prior, dtype=np.float64)
            assert r64.dtype == np.float64 and np.isfinite(r64).all() and (r64 > 0).all()
            rel = float(np.max(np.abs(r32.astype(np.float64) - r64) / r64))
            print(f"n {c['n_players']} prior {prior}: max relative difference {rel:.3e}")
            worst = max(worst, rel)
    assert worst <= 4 * RATE_F64_MEASURED, worst
