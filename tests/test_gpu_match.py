"""pongmi.matchmaking on the MI355X: pm_league_match against match_host (opponents and totals as integers, the copied
rows as bits) and pm_league_rate against rate_host (float32 bits) on synthetic pair_stats written from numpy with
hand-built pair lists; then a League, a Matchmaker and a PopulationRollout end to end, and SelfPlayPBTTrainer against
the same generations written out by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_gpu_league.py's ENV_KW
ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)
LENGTHS = (0, 1, 63, 64, 65, 129)  # around the wave's chunk of 64 entries
FILL = -3.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(rng, k):
    """k pairs' stats: no games, all wins of A, all wins of B, all draws, and random splits of 1..40 games."""
    kind = rng.integers(0, 7, k)
    g = np.where(kind == 0, 0, rng.integers(1, 41, k))
    wa = np.where(kind == 1, g, np.where((kind == 2) | (kind == 3), 0, rng.integers(0, g + 1)))
    wb = np.where(kind == 2, g, np.where((kind == 1) | (kind == 3), 0, rng.integers(0, g - wa + 1)))
    ps = rng.integers(0, 1000, (k, 8)).astype(np.int64)  # points, ticks, unfinished: not read
    ps[:, 0], ps[:, 1], ps[:, 2], ps[:, 3] = g, wa, wb, g - wa - wb
    return ps


def _match_case(n, seed):
    """n members, three fixed nets, the follower (net_of -1) and a player whose net_of is n_nets (one past the
    table). Member p's list has LENGTHS[p % 6] entries (n = 1: 65; n = 2: 2046 against the three fixed nets, and
    129), one pair per entry, the member on a random side, the opponent anyone, itself included. The first list of at
    least 63 entries also names pair index n_pairs and meets the net-less player in a pair it lost outright; with n
    >= 65 member 5 only has entries that are not eligible. pair_stats, pair_players and w carry one guard row that a
    missing range check would read: a lost pair against a fixed net, and a net of its own."""
    from pongmi._lib import PM_QNET_NW
    rng = np.random.default_rng(seed)
    n_nets, n_players = n + 3, n + 5
    follower, beyond = n + 3, n + 4
    net_of = np.concatenate([np.arange(n + 3), [-1, n_nets]]).astype(np.int32)
    lengths = [65] if n == 1 else [2046, 129] if n == 2 else [LENGTHS[p % 6] for p in range(n)]
    dead = 5 if n >= 65 else None
    pairs, lists = [], []
    for p in range(n):
        k = lengths[p]
        if n == 2 and p == 0:
            o = n + np.arange(k) % 3
        elif p == dead:
            o = rng.choice([follower, beyond, p], k)
        else:
            o = np.where(rng.random(k) < 0.75, rng.integers(0, n + 3, k), rng.choice([follower, beyond, p], k))
        side = rng.integers(0, 2, k)
        first = len(pairs)
        pairs += [(p, int(o[j])) if side[j] == 0 else (int(o[j]), p) for j in range(k)]
        lists.append(2 * (first + np.arange(k)) + side)
    n_pairs = len(pairs)
    special = next(p for p in range(n) if lengths[p] >= 63 and p != dead)
    ps = np.concatenate([_stats(rng, n_pairs), [[8, 0, 8, 0, 0, 0, 0, 0]]]).astype(np.int64)
    pp = np.array(pairs + [(special, n)], np.int32).reshape(-1, 2)  # the guard pair: lost outright to fixed net n
    lists[special][0] = 2 * n_pairs  # one past the last pair
    j = int(lists[special][1]) >> 1
    pp[j] = (special, beyond)
    lists[special][1] = 2 * j
    ps[j, :4] = (8, 0, 8, 0)
    if dead is not None:
        lists[dead][:3] = (2 * n_pairs, -1, 2 * n_pairs + 7)  # and entries that name no pair at all
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists]), ]).astype(np.int32)
    off = np.concatenate([off, np.full(n_players - n, off[-1])]).astype(np.int32)  # the others' lists are empty
    w = torch.randn((n_nets + 1, PM_QNET_NW), generator=torch.Generator().manual_seed(seed))
    case = dict(pair_stats=ps[:n_pairs], pair_players=pp[:n_pairs], player_off=off,
                player_pairs=np.concatenate(lists + [np.zeros(0, np.int64)]).astype(np.int32), n_players=n_players,
                net_of=net_of, n_nets=n_nets)  # what the host model sees: no guard rows
    return case, dict(case, pair_stats=ps, pair_players=pp), w, dead, special


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_match_equals_match_host(n):
    from pongmi import _lib
    from pongmi._lib import PM_QNET_NW
    from pongmi.matchmaking import MODES, match_host, match_weights_host
    case, guarded, w, dead, special = _match_case(n, 100 + n)
    n_pairs = len(case["pair_players"])
    lib = _lib.load()
    d = {k: _dev(guarded[k]) for k in ("pair_stats", "pair_players", "player_off", "player_pairs", "net_of")}
    d_w = w.cuda()
    assert d["pair_stats"].shape[0] == n_pairs + 1 and d_w.shape[0] == case["n_nets"] + 1
    # what the fixture promises
    lens = np.diff(case["player_off"][:n + 1])
    if n == 2:
        assert lens.tolist() == [2046, 129]
        assert set(match_weights_host(**case, p=0, mode="hard", power=0)[1][2:].tolist()) == {2, 3, 4}
    if n >= 65:
        assert set(lens.tolist()) == set(LENGTHS)
    q_sp = match_weights_host(**case, p=special, mode="hard", power=1)[0]
    assert q_sp[0] == 0 and q_sp[1] == 0  # the entry past the last pair, and the player whose net is n_nets
    seen_none = False
    for mode, power in (("hard", 0), ("hard", 1), ("hard", 2), ("hard", 8), ("even", 1)):
        for seed, rnd in ((0, 0), (0, (1 << 32) + 5), ((1 << 63) + 9, 0), ((1 << 63) + 9, (1 << 32) + 5)):
            wA = torch.full((n + 1, PM_QNET_NW), FILL, device="cuda")  # a guard row behind the n rows
            opp = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
            total = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
            _lib.check(lib.pm_league_match(_lib.ptr(d["pair_stats"]), _lib.ptr(d["pair_players"]), n_pairs,
                                           _lib.ptr(d["player_off"]), _lib.ptr(d["player_pairs"]), case["n_players"],
                                           _lib.ptr(d["net_of"]), _lib.ptr(d_w), case["n_nets"], n, MODES[mode], power, seed,
                                           rnd, _lib.ptr(wA), _lib.ptr(opp), _lib.ptr(total), _lib.stream_ptr()),
                       "pm_league_match")
            w_opp, w_total = match_host(**case, n=n, mode=mode, power=power, seed=seed, round=rnd)
            key = (mode, power, seed, rnd)
            g_opp, g_total = opp.cpu().numpy(), total.cpu().numpy()
            assert np.array_equal(g_total[:n], w_total), key
            assert np.array_equal(g_opp[:n], w_opp), key
            assert g_opp[n] == -5 and g_total[n] == -5, key
            drew = w_opp >= 0
            rows = torch.from_numpy(case["net_of"][np.where(drew, w_opp, 0)].astype(np.int64)).cuda()
            want = torch.where(torch.from_numpy(drew).cuda()[:, None], d_w[rows], torch.full_like(d_w[rows], FILL))
            assert torch.equal(wA[:n].view(torch.int32), want.view(torch.int32)), key
            assert (wA[n] == FILL).all(), key
            assert ((w_opp >= 0) == (w_total > 0)).all() and (w_opp < n + 3).all()  # never the net-less players
            assert (w_opp != np.arange(n)).all()
            seen_none |= bool((~drew).any())
            if dead is not None:
                assert w_opp[dead] == -1 and w_total[dead] == 0 and lens[dead] > 0
    assert seen_none == (n >= 65)  # members with an empty list, and the one with nobody eligible
    if n == 2:  # the draws moved with seed and round
        a = [match_host(**case, n=n, mode="hard", power=0, seed=s, round=r)[0][0] for s in range(4) for r in range(4)]
        assert len(set(a)) == 3


def _rate_case(P, seed):
    """P players: every player but the last meets a few random others (player 0 about 200 of them, with repeats:
    four passes of its wave), in pairs with and without games; player 1 (player 0 when alone) also meets itself,
    and the last player of three or more plays nobody. Player 0's list also names pair index n_pairs: a guard row
    holds a pair that a missing range check would count."""
    rng = np.random.default_rng(seed)
    pairs = []
    busy = P if P < 3 else P - 1
    if busy > 1:
        for i in range(busy):
            for _ in range(200 if i == 0 else 4):
                j = int(rng.integers(0, busy - 1))
                j += j >= i
                pairs.append((i, j) if rng.random() < 0.5 else (j, i))
    me = min(1, P - 1)
    pairs.append((me, me))
    n_pairs = len(pairs)
    ps = np.concatenate([_stats(rng, n_pairs), [[8, 8, 0, 0, 0, 0, 0, 0]]]).astype(np.int64)
    ps[n_pairs - 1, :4] = (6, 3, 2, 1)  # the self-pair has games
    pp = np.array(pairs + [(0, busy - 1)], np.int32).reshape(-1, 2)  # the guard pair: won outright
    lists = [[] for _ in range(P)]
    for k, (a, b) in enumerate(pairs):
        lists[a].append(2 * k)
        lists[b].append(2 * k + 1)
    lists[0].insert(len(lists[0]) // 2, 2 * n_pairs)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    case = dict(pair_stats=ps[:n_pairs], pair_players=pp[:n_pairs], player_off=off,
                player_pairs=np.concatenate([np.array(x, np.int64) for x in lists]).astype(np.int32), n_players=P)
    return case, dict(case, pair_stats=ps, pair_players=pp)


@pytest.mark.parametrize("P", [1, 2, 65, 300])
def test_rate_equals_rate_host(P):
    from pongmi import _lib
    from pongmi.matchmaking import rate_host
    case, guarded = _rate_case(P, 200 + P)
    n_pairs = len(case["pair_players"])
    lib = _lib.load()
    d = {k: _dev(guarded[k]) for k in ("pair_stats", "pair_players", "player_off", "player_pairs")}
    for iterations in (0, 1, 32):
        for prior in (1.0, 0.5):
            rating = torch.full((P + 1,), FILL, device="cuda")
            _lib.check(lib.pm_league_rate(_lib.ptr(d["pair_stats"]), _lib.ptr(d["pair_players"]), n_pairs,
                                          _lib.ptr(d["player_off"]), _lib.ptr(d["player_pairs"]), P, iterations, prior,
                                          _lib.ptr(rating), _lib.stream_ptr()), "pm_league_rate")
            want = rate_host(**case, iterations=iterations, prior=prior)
            got = rating.cpu().numpy()
            assert np.array_equal(got[:P].view(np.int32), want.view(np.int32)), (iterations, prior)
            assert got[P] == FILL
            assert np.isfinite(want).all() and (want > 0).all()
            if iterations == 0:
                assert (want == 1.0).all()
            if P == 1 or (P >= 3 and iterations):
                assert want[-1] == 1.0  # nobody met (its own pair aside): the prior's fixed point
    if P >= 65:
        assert len(set(want.tolist())) > P // 2 and int(np.diff(case["player_off"])[0]) > 192


# ------------------------------------------------------------------------------------------- end to end
N, M = 3, 32


def _nets(k, seed):
    from models.qnet import QNet
    torch.manual_seed(seed)
    return [QNet(7, 3) for _ in range(k)]


def _fixed_w(seed):
    from models.qnet import QNet
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict
    torch.manual_seed(seed)
    return fold(pack_state_dict(QNet(7, 3).state_dict()), _lib.PM_FOLD_TRAIN).reshape(-1)


def _league(fixed):
    """Three members and one fixed net; every member meets the two others and the fixed net: three candidates."""
    from pongmi.league import League
    players = [("member", p) for p in range(N)] + [fixed]
    pairs = [(0, 1, 8), (2, 0, 8), (1, 2, 8), (3, 0, 8), (3, 1, 8), (2, 3, 8)]
    return League(ENV_KW, players, pairs)


def _replays():
    from pongmi.replay import DeviceReplay
    return [DeviceReplay(M * 16, "cuda") for _ in range(N)]


def _env():
    from pongmi.env import PongEnv2PBatch
    env = PongEnv2PBatch(N * M, seed=9, autoreset=True)
    env.reset()
    return env


def test_league_matchmaker_and_collector_end_to_end():
    from pongmi.matchmaking import Matchmaker, match_host
    from pongmi.qnet import pack_state_dict
    from pongmi.rollout import STATS_PUSH, PopulationRollout
    params = torch.stack([pack_state_dict(net.state_dict()).reshape(-1) for net in _nets(N, 60)]).cuda().contiguous()
    fixed, first = _fixed_w(61), _fixed_w(62)
    L = _league(fixed)
    assert np.diff(L.player_off).tolist() == [3, 3, 3, 3]
    mm = Matchmaker(L, mode="hard", power=2, seed=4, initial=first)
    assert torch.equal(mm.wA.cpu(), first.cpu().expand(N, -1))
    env, replays = _env(), _replays()
    R = PopulationRollout(env, mm.wA, params, n=N, replays=replays, steps_max=4)
    for p in range(N):  # the collector plays the matchmaker's rows in place
        assert R.wA[p].data_ptr() == mm.wA[p].data_ptr()
    L.evaluate(params, 0, seed=1)
    opp, total = mm.assign(0)
    assert opp.is_cuda and total.is_cuda and opp.dtype == torch.int32 and total.dtype == torch.int32
    ps = L.pair_stats.cpu().numpy()
    assert (ps[:, 0] == 8).all()
    w_opp, w_total = match_host(ps, mm.pair_players, L.player_off, L.player_pairs, L.n_players, mm.net_of, L.n_nets, N,
                                "hard", 2, 4, 0)
    assert np.array_equal(opp.cpu().numpy(), w_opp) and np.array_equal(total.cpu().numpy(), w_total)
    assert (w_opp >= 0).all() and (w_opp != np.arange(N)).all()
    for p in range(N):
        assert torch.equal(mm.wA[p].view(torch.int32), L.w[int(mm.net_of[w_opp[p]])].view(torch.int32)), p
        assert R.wA[p].data_ptr() == mm.wA[p].data_ptr()
    assert not torch.equal(mm.wA.cpu(), first.cpu().expand(N, -1))
    # the next collect plays the assigned nets: equal to a fresh collector given those rows as a list
    got = R.collect(4)
    env2, replays2 = _env(), _replays()
    R2 = PopulationRollout(env2, [mm.wA[p].clone() for p in range(N)], params, n=N, replays=replays2, steps_max=4)
    want = R2.collect(4)
    for k in STATS_PUSH:
        assert np.array_equal(got[k], want[k]), k
    assert torch.equal(R.stats, R2.stats)
    for p in range(N):
        a, b = replays[p], replays2[p]
        assert (a.pos, a.size) == (b.pos, b.size) == ((4 * M) % a.cap, 4 * M)
        assert torch.equal(a.trans.view(torch.int32), b.trans.view(torch.int32)), p
        assert torch.equal(a.prios.view(torch.int32), b.prios.view(torch.int32)), p
        assert a.work is not None and torch.equal(a.work, b.work), p
    # and not equal to what the first opponent would have given (the rows matter)
    env3, replays3 = _env(), _replays()
    PopulationRollout(env3, first, params, n=N, replays=replays3, steps_max=4).collect(4)
    assert any(not torch.equal(replays[p].trans, replays3[p].trans) for p in range(N))
    # a rating is a fitness select() takes
    rating = mm.rate()
    assert rating.shape == (N + 1,) and rating.dtype == torch.float32 and rating.is_cuda
    src_of, rank, _ = L.select(rating, 0, bottom=0.34, top=0.34)
    r = rating.cpu().numpy()
    assert int(rank.cpu().numpy()[int(np.argmax(r[:N]))]) == 0 and np.isfinite(r).all()


def _self_play_setup(seed_nets):
    from pongmi.dqn import DQNPopulation, PopulationTrainer
    from pongmi.matchmaking import Matchmaker
    L = _league(_fixed_w(71))
    mm = Matchmaker(L, mode="hard", power=2, seed=4, initial=_fixed_w(72))
    pop = DQNPopulation(_nets(N, seed_nets), batch=64, lr=[1e-3, 2e-3, 3e-3], train_features=True,
                        target_update_interval=3, seed=[1, 2, 3])
    trainer = PopulationTrainer(_env(), mm.wA, pop, _replays(), collect_steps=8, updates=2)
    return L, mm, pop, trainer


@pytest.mark.parametrize("fitness", ["wins", "rating"])
def test_self_play_pbt_trainer_equals_the_sequence_by_hand(fitness):
    from pongmi.league import explore
    from pongmi.matchmaking import SelfPlayPBTTrainer, match_host
    kw = dict(bottom=0.34, top=0.34, seed=7)
    factors = {"lr": (0.8, 1.25)}
    L, mm, pop, trainer = _self_play_setup(80)
    T = SelfPlayPBTTrainer(trainer, L, mm, factors=factors, fitness=fitness, **kw)
    fits = T.run(2, 3)
    assert fits.shape == (2, N + 1) and T.generation == 2 and len(T.opponents) == 2
    # by hand, on objects of their own
    L2, mm2, pop2, trainer2 = _self_play_setup(80)
    for g in range(2):
        trainer2.run(3)
        fit = L2.evaluate(pop2.params, g, 7)
        if fitness == "rating":
            fit = mm2.rate(32, 1.0)
        assert np.array_equal(fit.cpu().numpy().view(np.int32), fits[g].view(np.int32)), g
        opp, _ = mm2.assign(g)
        assert torch.equal(opp, T.opponents[g]), g
        ps = L2.pair_stats.cpu().numpy()
        w_opp, _ = match_host(ps, mm2.pair_players, L2.player_off, L2.player_pairs, L2.n_players, mm2.net_of, L2.n_nets,
                              N, "hard", 2, 4, g)
        assert np.array_equal(opp.cpu().numpy(), w_opp), g
        # the rows are the nets as evaluated: copied before exploit replaces anybody
        for p in range(N):
            assert torch.equal(mm2.wA[p].view(torch.int32), L2.w[int(mm2.net_of[w_opp[p]])].view(torch.int32)), (g, p)
        src_of, _, draw = L2.select(fit, g, **kw)
        pop2.exploit(src_of)
        replaced = explore(pop2, src_of, draw, factors)
        assert len(replaced) == 1
    for k in ("params", "target", "adam_m", "adam_v"):
        assert torch.equal(getattr(pop, k).view(torch.int32), getattr(pop2, k).view(torch.int32)), k
    assert pop.hyper["lr"] == pop2.hyper["lr"] and pop.hyper["lr"] != [1e-3, 2e-3, 3e-3]
    assert torch.equal(mm.wA.view(torch.int32), mm2.wA.view(torch.int32))
    for p in range(N):
        assert trainer.rollout.wA[p].data_ptr() == mm.wA[p].data_ptr()
    from pongmi.matchmaking import Matchmaker
    with pytest.raises(ValueError, match="in place"):  # a collector that plays other rows would never see an assignment
        SelfPlayPBTTrainer(trainer, L, Matchmaker(L), **kw)
    with pytest.raises(ValueError, match="another league"):
        SelfPlayPBTTrainer(trainer, L, mm2, **kw)
    with pytest.raises(ValueError):
        SelfPlayPBTTrainer(trainer, L, mm, fitness="elo", **kw)
