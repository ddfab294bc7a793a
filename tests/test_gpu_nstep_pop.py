"""N-step returns for a population: three members with windows (1, 3, 8) and discounts of their own, 64 arenas
each. Member p of PopulationRollout.collect equals the solo n-step collector with member p's nstep and gamma,
member p of DQNPopulation.update / update_from equals the solo DQNLearner with member p's nstep, bit for bit; and
one PopulationTrainer(nstep=3) runs end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, M = 3, 64
NSTEP, GAMMA = (1, 3, 8), (0.99, 0.97, 0.9)
CFG = dict(paddle_width=0.1, paddle_speed=0.02, max_score=1, ball_speed_range=[0.2, 0.3], speed_scale_every=1,
           speed_increment=0.1)  # episodes a few ticks long (tests/test_gpu_nstep_rollout.py)
LEARNER = ("params", "target", "adam_m", "adam_v", "grad", "stats_buf", "td", "q", "s", "ns", "act", "rew", "done", "isw",
           "idx")


def _sds(n, seed):
    from models.qnet import QNet
    torch.manual_seed(seed)
    return [QNet(7, 3).state_dict() for _ in range(n)]


def _wA():
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict
    return fold(pack_state_dict(_sds(1, 5)[0]), _lib.PM_FOLD_TRAIN).reshape(-1)


def _collectors(params, cap, steps_max):
    """The population collector and three solo collectors on copies of the members' slices, each with its ring."""
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import PopulationRollout, SelfPlayRollout
    env = PongEnv2PBatch(N * M, seed=77, autoreset=True, **CFG)
    env.reset()
    wA = _wA()
    Rp = [DeviceReplay(cap, "cuda") for _ in range(N)]
    Rs = [DeviceReplay(cap, "cuda") for _ in range(N)]
    solo = []
    for p in range(N):
        e = PongEnv2PBatch(M, seed=77 + p, autoreset=True, **CFG)
        e.f64.copy_(env.f64[:, p * M:(p + 1) * M])
        e.i32.copy_(env.i32[:, p * M:(p + 1) * M])
        e.obsA.copy_(env.obsA[p * M:(p + 1) * M])
        e.obsB.copy_(env.obsB[p * M:(p + 1) * M])
        solo.append(SelfPlayRollout(e, wA, params[p].clone(), epsilon=0.3, seed_net=9 + p))
    pop = PopulationRollout(env, wA, params, n=N, replays=Rp, epsilon=0.3, seed_net=[9 + p for p in range(N)],
                            steps_max=steps_max, nstep=NSTEP, gamma=GAMMA)
    return env, pop, Rp, solo, Rs


def test_collect_equals_the_solo_nstep_collectors():
    from pongmi.qnet import pack_state_dict
    from pongmi.rollout import STATS_PUSH
    params = torch.stack([pack_state_dict(sd).reshape(-1) for sd in _sds(N, 21)]).contiguous()
    cap = M * 20 + 7
    env, pop, Rp, solo, Rs = _collectors(params, cap, 12)
    for steps in (12, 9):  # the second collect wraps every ring and starts with empty windows
        got = pop.collect(steps)
        for p in range(N):
            ref = solo[p].run(steps, replay=Rs[p], nstep=NSTEP[p], gamma=GAMMA[p])
            assert [int(got[k][p]) for k in STATS_PUSH] == [ref[k] for k in STATS_PUSH], (p, steps)
    for p in range(N):
        e, sl = solo[p].env, slice(p * M, (p + 1) * M)
        assert torch.equal(env.f64[:, sl], e.f64) and torch.equal(env.i32[:3, sl], e.i32[:3]), p
        assert torch.equal(env.obsA[sl], e.obsA) and torch.equal(env.obsB[sl], e.obsB), p
        assert torch.equal(pop.ep_reward[sl], solo[p].ep_reward), p
        a, b = Rp[p], Rs[p]
        assert (a.pos, a.size, a.max_horizon) == (b.pos, b.size, NSTEP[p]), p
        assert torch.equal(a.trans.view(torch.int32), b.trans.view(torch.int32)), p
        assert torch.equal(a.prios, b.prios) and torch.equal(a.work, b.work), p
        k = ((a.trans[:a.size, 15].view(torch.int32) >> 16) & 7) + 1
        assert sorted(set(k.cpu().tolist())) == list(range(1, NSTEP[p] + 1)), p  # the member's own window
        assert int(((a.trans[:a.size, 15].view(torch.int32) >> 8) & 1).sum()) > 0, p


def _population(sds, batch, **kw):
    from pongmi.dqn import DQNLearner, DQNPopulation
    common = dict(batch=batch, train_features=True, loss="huber", max_norm=10.0, **kw)
    pop = DQNPopulation(sds, n=N, gamma=list(GAMMA), seed=[5 + p for p in range(N)], nstep=list(NSTEP), **common)
    solo = [DQNLearner(sds[p], gamma=GAMMA[p], seed=5 + p, nstep=NSTEP[p], **common) for p in range(N)]
    return pop, solo


def _same_member(pop, p, L, rows):
    m = pop.member(p)
    for name in LEARNER:
        a, b = getattr(m, name), getattr(L, name)
        if name in ("td", "q", "s", "ns", "act", "rew", "done", "isw", "idx"):
            a, b = a[:rows], b[:rows]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (p, name)
    assert torch.equal(pop.norm[p:p + 1], L.norm), p


def test_update_equals_the_solo_learners():
    batch = 33
    sds = _sds(N, 31)
    pop, solo = _population(sds, batch)
    rng = np.random.default_rng(4)
    for p in range(N):
        s, ns = rng.random((batch, 7), dtype=np.float32), rng.random((batch, 7), dtype=np.float32)
        a, r = rng.integers(0, 3, batch), rng.integers(-1, 2, batch).astype(np.float32)
        d, iw = rng.random(batch) < 0.2, rng.uniform(0.2, 1.0, batch).astype(np.float32)
        h = rng.integers(1, NSTEP[p] + 1, batch) if NSTEP[p] > 1 else None
        pop.load_batch(p, s, a, r, ns, d, isw=iw, horizon=h)
        solo[p].update(s, a, r, ns, d, isw=iw, horizon=h)
    pop.update()
    torch.cuda.synchronize()
    for p in range(N):
        _same_member(pop, p, solo[p], batch)
        if NSTEP[p] > 1:
            assert torch.equal(pop.horizon[p, :batch], solo[p].horizon)
    assert pop.stats()["steps"].tolist() == [1] * N


def test_update_from_equals_the_solo_learners():
    from pongmi.qnet import pack_state_dict
    batch, updates = 64, 3
    sds = _sds(N, 41)
    params = torch.stack([pack_state_dict(sd).reshape(-1) for sd in sds]).contiguous()
    _, coll, Rp, solo_coll, Rs = _collectors(params, M * 16, 16)
    coll.collect(16)
    for p in range(N):
        solo_coll[p].run(16, replay=Rs[p], nstep=NSTEP[p], gamma=GAMMA[p])
    pop, solo = _population(sds, batch)
    u = np.random.default_rng(6).random((N, updates, batch))
    pop.update_from(Rp, updates, beta_frames=1000, seed=3, uniforms=u)
    for p in range(N):
        solo[p].update_from(Rs[p], updates, beta_frames=1000, seed=3, uniforms=u[p])
    torch.cuda.synchronize()
    for p in range(N):
        _same_member(pop, p, solo[p], batch)
        assert torch.equal(Rp[p].prios, Rs[p].prios) and torch.equal(Rp[p].work, Rs[p].work), p
        if NSTEP[p] > 1:
            assert torch.equal(pop.horizon[p, :batch], solo[p].horizon), p
            assert int(pop.horizon[p, :batch].max()) > 1, p
    assert pop.stats()["status"].tolist() == [0] * N


def test_population_trainer_end_to_end():
    from pongmi.dqn import DQNPopulation, PopulationTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    env = PongEnv2PBatch(N * M, seed=3, autoreset=True, **CFG)
    env.reset()
    pop = DQNPopulation(_sds(N, 51), n=N, batch=64, train_features=True, nstep=3)
    Rs = [DeviceReplay(M * 8, "cuda") for _ in range(N)]
    T = PopulationTrainer(env, _wA(), pop, Rs, collect_steps=8, updates=2, epsilon=0.3, nstep=3)
    before = pop.params.clone()
    st = T.run(2)
    s = pop.stats()
    assert s["status"].tolist() == [0] * N and s["steps"].tolist() == [4] * N
    assert (st["episodes"] > 0).all() and not torch.equal(before, pop.params)
    assert [r.max_horizon for r in Rs] == [3] * N
    k = ((Rs[0].trans[:, 15].view(torch.int32) >> 16) & 7) + 1
    assert sorted(set(k.cpu().tolist())) == [1, 2, 3]


def test_population_calls_name_the_offending_member():
    """The C entries' own validation, on live handles: a bad window or discount names its member, and a horizon
    buffer that two members share breaks the aliasing rule."""
    import ctypes
    from pongmi import _lib
    from pongmi.dqn import DQNPopulation
    from pongmi.qnet import pack_state_dict
    params = torch.stack([pack_state_dict(sd).reshape(-1) for sd in _sds(N, 21)]).contiguous()
    _, coll, _, _, _ = _collectors(params, M * 16, 4)
    coll.collect(1)  # creates the handle
    L = coll.lib
    i32, f64 = ctypes.c_int32 * N, ctypes.c_double * N
    err = lambda: L.pm_last_error().decode()  # noqa: E731
    assert L.pm_rollout_nstep_pop_set(coll._handle, i32(1, 9, 2), f64(0.9, 0.9, 0.9), _lib.stream_ptr()) == -2
    assert "pm_rollout_nstep_pop_set: member 1: nstep=9 (1..8)" in err()
    assert L.pm_rollout_nstep_pop_set(coll._handle, i32(1, 2, 2), f64(0.9, 0.9, float("inf")), _lib.stream_ptr()) == -1
    assert "pm_rollout_nstep_pop_set: member 2: gamma is not finite" in err()
    assert L.pm_rollout_nstep_pop_set(coll._handle, i32(1, 2, 2), None, _lib.stream_ptr()) == -1
    assert L.pm_rollout_nstep_pop_set(coll._handle, None, None, _lib.stream_ptr()) == 0  # every member one step again
    pop = DQNPopulation(_sds(N, 31), n=N, batch=32, nstep=2)
    pop.update()  # creates the handle and attaches the members' own horizon rows
    ns = (_lib.DqnNstep * N)()
    for p in range(N):
        ns[p].horizon = pop.horizon[0 if p == 2 else p].data_ptr()
    assert L.pm_dqn_nstep_pop_set(pop._handle, ns, _lib.stream_ptr()) == -1
    assert "member 2: its horizon overlaps member 0's horizon" in err()
    assert L.pm_dqn_nstep_pop_set(pop._handle, pop._ns, _lib.stream_ptr()) == 0
