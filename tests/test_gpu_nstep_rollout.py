"""The n-step collector (pm_rollout_push_n / SelfPlayRollout.run(nstep=)) against the one-step collector.

The one-step launch (pm_rollout_push, pinned to the stepped composition and the oracle by test_gpu_rollout.py) and
the n-step launch run on identically seeded envs. The n-step rows, horizon bits included, must equal
pongmi.rollout.nstep_fold_host of the one-step rows bit for bit, and everything that does not depend on the
window must be equal between the two runs: prios, the whole sum-tree workspace (leaves and both node levels),
the env state, the observations, ep_reward and the stats.

The env parameters make episodes a few ticks long (max_score 1, a fast ball, narrow paddles: on the CPU oracle,
oracle.cpu_selfplay.PhiloxRollout, 64 arenas x 40 steps end 640 episodes, 121 of them on the last 7 steps, and
every arena has two ends fewer than 8 steps apart), so windows are cut by a done at every age.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(paddle_width=0.1, paddle_speed=0.02, max_score=1, ball_speed_range=[0.2, 0.3], speed_scale_every=1,
           speed_increment=0.1)
GAMMA, EPS, SEED_ENV, SEED_NET = 0.97, 0.3, 0x5757, 17
NS = (1, 2, 3, 8)


@functools.lru_cache(maxsize=None)
def _models():
    from models.qnet import QNet
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict
    torch.manual_seed(1234)
    mA, mB = QNet(7, 3), QNet(7, 3)
    return fold(pack_state_dict(mA.state_dict()), _lib.PM_FOLD_TRAIN).reshape(-1), pack_state_dict(mB.state_dict()).reshape(-1)


def _collect(n, launches, cap, pos0, nstep, entry_n=None):
    """Run `launches` (a tuple of step counts) from a fresh env into a ring whose write slot starts at pos0. Returns
    per launch a dict of host arrays: the launch's rows in launch order, the whole prios / work buffers, the env
    state, observations, ep_reward and stats. entry_n: go through pm_rollout_push_n even for nstep 1."""
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import STATS_PUSH, SelfPlayRollout
    wA, paramsB = _models()
    env = PongEnv2PBatch(n, seed=SEED_ENV, autoreset=True, **CFG)
    env.reset()
    replay = DeviceReplay(cap, env.device)
    replay.pos = replay.size = pos0
    roll = SelfPlayRollout(env, wA, paramsB, epsilon=EPS, seed_net=SEED_NET)
    out = []
    for steps in launches:
        pos = replay.pos
        if entry_n:
            roll.reserve(steps)
            roll.stats.zero_()
            roll._push(steps, replay, nstep, GAMMA)
            env.counter += steps
            st = dict(zip(STATS_PUSH, roll.stats.cpu().tolist()))
        else:
            st = roll.run(steps, replay=replay, nstep=nstep, gamma=GAMMA)
        idx = (pos + np.arange(steps * n)) % cap
        state = env.get_state()
        out.append(dict(rows=replay.trans.cpu().numpy()[idx], prios=replay.prios.cpu().numpy(),
                        work=replay.work.cpu().numpy(), obsA=env.obsA.cpu().numpy(), obsB=env.obsB.cpu().numpy(),
                        ep=roll.ep_reward.cpu().numpy(), stats=[st[k] for k in STATS_PUSH],
                        state={k: state[k] for k in ("x", "y", "vx", "vy", "spin", "top", "bot", "scoreA", "scoreB",
                                                     "bounces")},
                        pos=replay.pos, size=replay.size, max_horizon=replay.max_horizon))
    return out


@functools.lru_cache(maxsize=None)
def _one_step(n, launches, cap, pos0):
    return _collect(n, launches, cap, pos0, 1)


def _check(n, launches, cap, pos0, N, entry_n=None):
    from pongmi.rollout import nstep_fold_host
    ref = _one_step(n, launches, cap, pos0)
    got = _collect(n, launches, cap, pos0, N, entry_n)
    for steps, a, b in zip(launches, ref, got):
        want = nstep_fold_host(a["rows"], n, steps, N, GAMMA)
        assert np.array_equal(b["rows"].view(np.int32), want.view(np.int32))
        for k in ("prios", "work", "obsA", "obsB", "ep"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        for k, v in a["state"].items():
            assert np.array_equal(v, b["state"][k]), k
        assert a["stats"] == b["stats"] and (a["pos"], a["size"]) == (b["pos"], b["size"])
        assert b["max_horizon"] == N
    return ref, got


def _short_cases():
    return sorted({(n, N, s) for n in (33, 64) for N in NS for s in (1, N - 1, N, N + 1) if s >= 1})


@pytest.mark.parametrize("n,N,steps", _short_cases())
def test_short_launches_equal_the_folded_one_step_rows(n, N, steps):
    _check(n, (steps,), n * 16, 0, N)


@pytest.mark.parametrize("N", NS)
def test_long_launch_with_short_episodes(N):
    n, steps = 64, 40
    ref, got = _check(n, (steps,), n * steps, 0, N)
    bits = ref[0]["rows"][:, 15].view(np.int32).reshape(steps, n)
    done = (bits >> 8) & 1
    assert done.sum() >= 8
    assert done[steps - (N - 1):].sum() >= 1 or N == 1  # a done on the launch's last N - 1 steps
    if N == 8:
        assert any((np.diff(np.nonzero(done[:, i])[0]) < N).any() for i in range(n))  # two dones < N steps apart
    k = ((got[0]["rows"][:, 15].view(np.int32) >> 16) & 7) + 1
    assert sorted(set(k.tolist())) == list(range(1, N + 1))  # every horizon up to N occurs
    assert not (bits >> 16).any()  # the one-step rows leave bits 16 and up zero


@pytest.mark.parametrize("N", (3, 8))
def test_launch_that_wraps_the_ring(N):
    n, steps = 33, 12
    cap = n * steps + 5
    _check(n, (steps,), cap, cap - 7 * n - 3, N)  # the ring's end falls inside step 7's rows


@pytest.mark.parametrize("N", (2, 8))
def test_second_launch_starts_with_an_empty_window(N):
    n = 64
    _check(n, (9, 11), n * 24, 0, N)


@pytest.mark.parametrize("n", (33, 64))
def test_one_step_through_the_n_entry_is_the_one_step_launch(n):
    _check(n, (10, 6), n * 16 + 9, n * 16 - 40, 1, entry_n=True)


def test_bad_window_is_rejected_before_the_launch():
    from pongmi import _lib
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import SelfPlayRollout
    wA, paramsB = _models()
    env = PongEnv2PBatch(8, seed=1, autoreset=True, **CFG)
    env.reset()
    roll, replay = SelfPlayRollout(env, wA, paramsB), DeviceReplay(64, env.device)
    for kw, word in ((dict(nstep=0), "nstep=0"), (dict(nstep=9), "nstep=9"), (dict(nstep=2, gamma=float("nan")), "gamma")):
        with pytest.raises(_lib.PongmiError, match=word):
            roll.run(2, replay=replay, **kw)
    assert replay.size == 0 and env.counter == 0
