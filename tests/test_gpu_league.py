"""pongmi.league on the MI355X: the device serves against oracle.philox_serve, a League's matches against
pongmi.play.play on the same serves, the reduction against a numpy recomputation, pm_pbt_select against select_host,
the per-call eval fold, and a PBTTrainer end to end. Everything is compared exactly: the serves bit for bit (ENV_KW's
angle intervals lie within +-60 degrees, so no serve takes the OCML branch), integers as integers, the fitness as
float32 bits."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_gpu_play.py's ENV_KW
ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)


def _params(n, seed):
    """n random QNets as stacked [n, PM_QNET_NP] parameter blocks on the device."""
    from models.qnet import QNet
    from pongmi.qnet import pack_state_dict
    torch.manual_seed(seed)
    return torch.stack([pack_state_dict(QNet(7, 3).state_dict()).reshape(-1) for _ in range(n)]).cuda().contiguous()


def _fixed(seed):
    from models.qnet import QNet
    from pongmi import _lib
    torch.manual_seed(seed)
    return (QNet(7, 3).state_dict(), _lib.PM_FOLD_TRAIN)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _split(m):
    """m episodes over up to three pairs of two followers (so that crn has something to repeat)."""
    if m < 3:
        return [(0, 1, m)]
    a = m // 3
    return [(0, 1, a), (1, 0, a), (0, 0, m - 2 * a)]


@pytest.mark.parametrize("crn", [True, False])
@pytest.mark.parametrize("m", [1, 63, 65, 300])
def test_serves_equal_the_oracle_bit_for_bit(orc, m, crn):
    from pongmi import _lib
    from pongmi.league import League
    from pongmi.play import FOLLOWER
    L = League(ENV_KW, [FOLLOWER, FOLLOWER], _split(m), crn=crn)
    assert L.E == m
    lib = _lib.load()
    pv = orc.env_params_from_kwargs(**ENV_KW)
    out = torch.full((m + 1, 3), -7.0, dtype=torch.float64, device="cuda")  # a guard row behind the m slots
    for rnd in (0, 123456):
        for seed in (0, (1 << 63) + 5):
            _lib.check(lib.pm_league_serves(ctypes.byref(L.params_env), _lib.ptr(L.d_serve_idx), seed, rnd, _lib.ptr(out),
                                            m, _lib.stream_ptr()), "pm_league_serves")
            got = out.cpu().numpy()
            vx, vy, spin, far = orc.philox_serve(pv, L.serve_idx, np.full(m, rnd), seed, want_far=True)
            assert not far.any()
            want = np.stack([vx, vy, spin], 1)
            assert np.array_equal(_bits(got[:m]), _bits(want)), (rnd, seed)
            assert (got[m] == -7.0).all()
    if crn and m >= 3:  # pairs (0, 1) and (1, 0) face the same serves, episode by episode
        slot_of = np.argsort(L.order)
        a = m // 3
        assert np.array_equal(got[slot_of[:a]], got[slot_of[a:2 * a]])


@pytest.mark.parametrize("per_block", [128, 1024])
def test_matches_equal_play_on_the_same_serves(per_block):
    """5 members, a fixed net and the follower; pairs of 1, 16, 77 and 130 episodes, the 130 as two blocks
    (per_block 128) and as one block whose columns refill (1024); a follower-follower pair."""
    from pongmi import _lib
    from pongmi.evaluate import folded_weights
    from pongmi.league import League
    from pongmi.play import FOLLOWER, play
    from pongmi.qnet import fold
    params = _params(5, 100)
    fx = _fixed(200)
    players = [("member", p) for p in range(5)] + [fx, FOLLOWER]
    pairs = [(0, 1, 1), (1, 0, 16), (2, 5, 77), (5, 3, 130), (6, 4, 16), (6, 6, 16), (3, 6, 77)]
    L = League(ENV_KW, players, pairs, per_block=per_block)
    assert int(L.blk_range[:, 1].max()) == (128 if per_block == 128 else 130)
    fit = L.evaluate(params, 3, seed=11)
    assert isinstance(fit, torch.Tensor) and fit.is_cuda and fit.shape == (7,)
    assert int(L.status.item()) == 0
    res = L.results()
    serves = np.empty((L.E, 3))
    serves[L.order] = res["serves"]  # slot order -> arena order
    w = torch.cat([fold(params, _lib.PM_FOLD_EVAL), folded_weights(fx, "cuda").reshape(1, -1)])
    sA, sB, length, last = play(ENV_KW, w, L.net_A, L.net_B, serves)
    assert np.array_equal(res["score_A"], sA) and np.array_equal(res["score_B"], sB)
    assert np.array_equal(res["length"], length) and np.array_equal(res["last"], last)
    assert (length > 0).all() and (np.maximum(sA, sB) == 3).all()


def _reduce_host(sA, sB, length, pair_first, pairs, n_players):
    """pair_stats, player_stats and fitness recomputed in numpy from the per-arena arrays."""
    ps = np.zeros((len(pairs), 8), np.int64)
    for k in range(len(pairs)):
        a, b, ln = (x[pair_first[k]:pair_first[k + 1]].astype(np.int64) for x in (sA, sB, length))
        ok = ln >= 0
        ps[k] = [ok.sum(), (a > b)[ok].sum(), (b > a)[ok].sum(), (a == b)[ok].sum(), a[ok].sum(), b[ok].sum(), ln[ok].sum(),
                 (~ok).sum()]
    pl = np.zeros((n_players, 8), np.int64)
    for k, (a, b, _) in enumerate(pairs):
        g, wa, wb, d, pa, pb, t, u = ps[k]
        pl[a] += [g, wa, wb, d, pa, pb, t, u]
        pl[b] += [g, wb, wa, d, pb, pa, t, u]
    fit = np.zeros(n_players, np.float32)
    nz = pl[:, 0] > 0
    fit[nz] = pl[nz, 1].astype(np.float32) / pl[nz, 0].astype(np.float32)
    return ps, pl, fit


@pytest.mark.parametrize("max_steps", [1_000_000, 40])
def test_reduction_equals_numpy(max_steps):
    """Pairs of 1, 33 and 257 arenas and a player in no pair. With max_steps=40 episodes are cut: `unfinished` and
    status agree with the count of length < 0, and results() raises."""
    from pongmi.league import League
    from pongmi.play import FOLLOWER
    params = _params(4, 300)
    players = [("member", 0), ("member", 1), ("member", 2), FOLLOWER, ("member", 3)]
    pairs = [(0, 1, 1), (1, 2, 33), (3, 0, 257), (2, 0, 33)]
    L = League(ENV_KW, players, pairs, max_steps=max_steps)
    L.evaluate(params, 0, seed=1)
    sA, sB, length = (t.cpu().numpy() for t in (L.score_A, L.score_B, L.length))
    ps, pl, fit = _reduce_host(sA, sB, length, L.pair_first, pairs, 5)
    assert np.array_equal(L.pair_stats.cpu().numpy(), ps)
    assert np.array_equal(L.player_stats.cpu().numpy(), pl)
    assert np.array_equal(_bits(L.fitness.cpu().numpy()), _bits(fit))
    assert not pl[4].any() and fit[4] == 0.0
    cut = int((length < 0).sum())
    assert int(ps[:, 7].sum()) == cut and int(L.status.item()) == cut
    if max_steps == 40:
        assert cut > 0
        with pytest.raises(RuntimeError, match="did not finish"):
            L.results()
    else:
        assert cut == 0 and ps[:, 0].tolist() == [1, 33, 257, 33] and (ps[:, 3] == 0).all()
        assert L.results()["status"] == 0


def test_reduce_kernels_on_synthetic_results():
    """pm_league_reduce alone, on arrays no match produces: draws, unfinished arenas anywhere, a pair of 1000
    arenas (four passes of its workgroup), a player with 70 pairs (two passes of its wave), an empty pair."""
    from pongmi import _lib
    rng = np.random.default_rng(5)
    sizes = [1, 33, 257, 1000, 0] + [3] * 70
    pair_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    E = int(pair_first[-1])
    sA, sB = rng.integers(0, 4, E).astype(np.int32), rng.integers(0, 4, E).astype(np.int32)
    length = np.where(rng.random(E) < 0.2, -1, rng.integers(1, 5000, E)).astype(np.int32)
    # players: 0 is B of every pair; 1..4 are A of the first four; 5 is A of the rest; 6 plays nothing
    pairs = [(min(k + 1, 5), 0, s) for k, s in enumerate(sizes)]
    n_players = 7
    owner = np.array([[a, b] for a, b, _ in pairs]).reshape(-1)
    entry = np.arange(2 * len(pairs))
    by = np.argsort(owner, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n_players))]).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = [dev(x) for x in (sA, sB, length, pair_first, off, entry[by].astype(np.int32))]
    ps = torch.full((len(pairs), 8), -1, dtype=torch.int64, device="cuda")
    pl = torch.full((n_players, 8), -1, dtype=torch.int64, device="cuda")
    fit = torch.full((n_players,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().pm_league_reduce(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), len(pairs),
                                            _lib.ptr(d[4]), _lib.ptr(d[5]), n_players, _lib.ptr(ps), _lib.ptr(pl),
                                            _lib.ptr(fit), _lib.stream_ptr()), "pm_league_reduce")
    want_ps, want_pl, want_fit = _reduce_host(sA, sB, length, pair_first, pairs, n_players)
    assert np.array_equal(ps.cpu().numpy(), want_ps) and np.array_equal(pl.cpu().numpy(), want_pl)
    assert np.array_equal(_bits(fit.cpu().numpy()), _bits(want_fit))
    assert want_ps[:, 3].sum() > 0 and want_ps[:, 7].sum() > 0 and not want_ps[4].any()


def _fitness_cases(n, rng):
    yield "equal", np.full(n, 0.5, np.float32)
    yield "ties", (rng.integers(0, 4, n) / 4).astype(np.float32)
    f = rng.random(n).astype(np.float32)
    f[n // 2] = np.nan
    yield "nan", f
    yield "distinct", rng.permutation(n).astype(np.float32) / n


@pytest.mark.parametrize("n", [1, 2, 64, 65, 300, 1024])
def test_select_equals_select_host(n):
    from pongmi import _lib
    from pongmi.league import select_host
    lib = _lib.load()
    rng = np.random.default_rng(n)
    counts = sorted({(0, 1), (n // 4, max(1, n // 4)), (n - max(1, n // 2), max(1, n // 2)), (n - 1, 1) if n > 1 else (0, 1)})
    for name, f in _fitness_cases(n, rng):
        d_f = torch.from_numpy(f).cuda()
        for n_bottom, n_top in counts:
            for seed, rnd in ((0, 0), ((1 << 63) + 9, (1 << 32) + 5)):
                rank = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")   # guard entries behind n
                src = torch.full((n + 1,), -5, dtype=torch.int64, device="cuda")
                draw = torch.full((n + 1,), -5, dtype=torch.int32, device="cuda")
                _lib.check(lib.pm_pbt_select(_lib.ptr(d_f), n, n_bottom, n_top, seed, rnd, _lib.ptr(rank), _lib.ptr(src),
                                             _lib.ptr(draw), _lib.stream_ptr()), "pm_pbt_select")
                w_src, w_rank, w_draw = select_host(f, n_bottom, n_top, seed, rnd)
                key = (name, n_bottom, n_top, seed)
                assert np.array_equal(rank[:n].cpu().numpy(), w_rank), key
                assert np.array_equal(src[:n].cpu().numpy(), w_src), key
                assert np.array_equal(draw[:n].cpu().numpy().view(np.uint32), w_draw), key
                assert int(rank[n]) == -5 and int(src[n]) == -5 and int(draw[n]) == -5


def test_eval_fold_is_redone_on_every_call():
    """params changes in place (member 0 copied over member 3): the next evaluate gives member 3 member 0's results
    against the common opponents, serve for serve (crn)."""
    from pongmi.league import League
    from pongmi.play import FOLLOWER
    params = _params(5, 400)
    L = League.versus(ENV_KW, 5, [_fixed(401), FOLLOWER], 16)

    def arenas_of(member):  # the member's arenas against both opponents
        idx = [k for k, (_, b, _) in enumerate(L.pairs) if b == member]
        return np.concatenate([np.arange(L.pair_first[k], L.pair_first[k + 1]) for k in idx])

    L.evaluate(params, 2, seed=3)
    before = {k: getattr(L, k).cpu().numpy().copy() for k in ("score_A", "score_B", "length", "last")}
    a0, a3 = arenas_of(0), arenas_of(3)
    assert not np.array_equal(before["length"][a0], before["length"][a3])  # two different nets to begin with
    params[3].copy_(params[0])
    fit = L.evaluate(params, 2, seed=3)
    after = L.results()
    for k in before:
        assert np.array_equal(after[k][a0], before[k][a0]), k  # member 0 plays as before
        assert np.array_equal(after[k][a3], after[k][a0]), k   # member 3 is member 0 now
    assert np.array_equal(after["player_stats"][3], after["player_stats"][0])
    assert float(fit[3]) == float(fit[0])


def test_pbt_trainer_end_to_end(monkeypatch):
    """4 members of 32 arenas, two generations: after each exploit every replaced member holds its source's params,
    target, Adam moments and counters from before it; evaluate and select hand over device tensors and results()
    is never called (no host read between trainer.run's closing read and explore's)."""
    from models.qnet import QNet
    from pongmi import league as lg
    from pongmi.dqn import DQNPopulation, PopulationTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.play import FOLLOWER
    from pongmi.qnet import fold, pack_state_dict
    from pongmi.replay import DeviceReplay
    n, m, cap = 4, 32, 32 * 16
    torch.manual_seed(50)
    nets = [QNet(7, 3) for _ in range(n)]
    wA = fold(pack_state_dict(QNet(7, 3).state_dict()), 1).reshape(-1)
    env = PongEnv2PBatch(n * m, seed=9, autoreset=True)
    env.reset()
    pop = DQNPopulation(nets, batch=64, lr=[1e-3, 2e-3, 3e-3, 4e-3], train_features=True, target_update_interval=3,
                        seed=[1, 2, 3, 4])
    trainer = PopulationTrainer(env, wA, pop, [DeviceReplay(cap, "cuda") for _ in range(n)], collect_steps=8, updates=2)
    L = lg.League.versus(ENV_KW, n, [FOLLOWER], 16)
    seen = dict(results=0, exploits=[], handed=[])
    monkeypatch.setattr(lg.League, "results", lambda self: seen.__setitem__("results", seen["results"] + 1))
    evaluate, select, exploit = L.evaluate, L.select, pop.exploit

    def spy_evaluate(*a, **kw):
        out = evaluate(*a, **kw)
        seen["handed"].append(out)
        return out

    def spy_select(*a, **kw):
        out = select(*a, **kw)
        seen["handed"].extend(out)
        return out

    def spy_exploit(src_of):
        names = ("params", "target", "adam_m", "adam_v")
        old = {k: getattr(pop, k).clone() for k in names}
        old_ctr = pop.stats_buf.view(torch.int64)[:, :2].clone()
        old_lr = list(pop.hyper["lr"])
        exploit(src_of)
        src = src_of.cpu().numpy()
        for p in range(n):
            for k in names:
                assert torch.equal(getattr(pop, k)[p], old[k][src[p]]), (p, k)
            assert torch.equal(pop.stats_buf.view(torch.int64)[p, :2], old_ctr[src[p]]), p
        seen["exploits"].append((src, old_lr))

    monkeypatch.setattr(L, "evaluate", spy_evaluate)
    monkeypatch.setattr(L, "select", spy_select)
    monkeypatch.setattr(pop, "exploit", spy_exploit)
    T = lg.PBTTrainer(trainer, L, bottom=0.25, top=0.25, factors={"lr": (0.8, 1.25)}, seed=7)
    fits = T.run(2, 3)
    assert fits.shape == (2, n + 1) and fits.dtype == np.float32 and T.generation == 2
    assert seen["results"] == 0 and len(seen["exploits"]) == 2
    assert len(seen["handed"]) == 8 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in seen["handed"])
    for g, (src, old_lr) in enumerate(seen["exploits"]):
        w_src, w_rank, w_draw = lg.select_host(fits[g][:n], 1, 1, 7, g)
        assert np.array_equal(src, w_src)
        replaced = [p for p in range(n) if src[p] != p]
        assert len(replaced) == 1 and w_rank[replaced[0]] == n - 1 and w_rank[src[replaced[0]]] == 0
    # the last explore: the replaced member's lr is its source's times the factor its draw picked
    p = replaced[0]
    assert pop.hyper["lr"][p] == old_lr[src[p]] * (0.8, 1.25)[int(w_draw[p]) & 1]
    assert all(pop.hyper["lr"][q] == old_lr[q] for q in range(n) if q != p)
    assert (pop.stats()["steps"] > 0).all()
