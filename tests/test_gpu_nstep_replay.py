"""The replay path with per-row horizons (pm_dqn_replay_update_n / DQNLearner(nstep=).update_from) and
DeviceReplay.push(horizon=), in the pattern of tests/test_gpu_dqn_replay.py: one call of several updates against
the loop of separate pieces (the oracle's draw, a host gather that decodes the horizon bits, update(horizon=),
update_priorities), bit for bit, on a cap-4096 ring filled by the n-step collector with a window of 3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA, BETA_START, BETA_FRAMES = 0.6, 0.4, 1000
CFG = dict(paddle_width=0.1, paddle_speed=0.02, max_score=1, ball_speed_range=[0.2, 0.3], speed_scale_every=1,
           speed_increment=0.1)  # episodes a few ticks long (tests/test_gpu_nstep_rollout.py)
STATE = ("params", "target", "adam_m", "adam_v", "grad", "td", "q", "stats_buf", "s", "ns", "act", "rew", "done", "isw",
         "idx")


@pytest.fixture(scope="module")
def nets():
    from models.qnet import QNet
    torch.manual_seed(11)
    return QNet(7, 3).state_dict(), QNet(7, 3).state_dict()


def _np(t):
    return t.detach().cpu().numpy()


def _collected(nets, nstep, cap=4096, n=64):
    """A full ring from four 16-step launches of the collector; the priorities spread as a learner would leave them."""
    from pongmi import _lib
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import fold, pack_state_dict
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import SelfPlayRollout
    env = PongEnv2PBatch(n, seed=77, autoreset=True, **CFG)
    env.reset()
    wA = fold(pack_state_dict(nets[1]), _lib.PM_FOLD_TRAIN).reshape(-1)
    roll = SelfPlayRollout(env, wA, pack_state_dict(nets[0]).reshape(-1), epsilon=0.3, seed_net=3)
    R = DeviceReplay(cap, env.device, alpha=ALPHA)
    for _ in range(cap // (16 * n)):
        roll.run(16, replay=R, nstep=nstep, gamma=0.99)
    R.prios.copy_(torch.from_numpy(np.random.default_rng(5).uniform(0.01, 3.0, cap).astype(np.float32)))
    R.refresh()
    assert R.size == cap and R.max_horizon == nstep
    return R


def _beta(steps):
    b = BETA_START + (steps + 1) * (1.0 - BETA_START) / BETA_FRAMES
    return min(b, 1.0)


def _learner(nets, batch, tf, **kw):
    from pongmi.dqn import DQNLearner
    return DQNLearner(nets[0], nets[1], batch=batch, train_features=tf, seed=5, **kw)


def _same(orc, A, B, what, names=STATE):
    for name in names:
        assert orc.bits_equal(_np(getattr(A, name)), _np(getattr(B, name))), f"{what}: {name}"


def _tree_is_rebuild(orc, R):
    from pongmi import _lib
    fresh = torch.zeros_like(R.work)
    _lib.check(_lib.load().pm_per_build(R.prios.data_ptr(), R.cap, R.alpha, fresh.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(R.work, fresh)


@pytest.mark.parametrize("tf", [False, True])
def test_one_call_equals_the_loop_of_pieces(orc, nets, tf):
    batch, updates = 256, 4
    R = _collected(nets, 3)
    trans, prios = _np(R.trans).copy(), _np(R.prios).copy()
    u = np.random.default_rng(9).random((updates, batch))
    L = _learner(nets, batch, tf, nstep=3, loss="huber", max_norm=10.0)
    idx_last, td_last = L.update_from(R, updates, beta_start=BETA_START, beta_frames=BETA_FRAMES, uniforms=u)
    torch.cuda.synchronize()

    C = _learner(nets, batch, tf, nstep=3, loss="huber", max_norm=10.0)
    seen = set()
    for k in range(updates):
        idx, w = orc.per_sample_tree(prios, R.size, R.cap, _beta(k), u[k], alpha=ALPHA)
        w = (w / w.max()).astype(np.float32)
        rows = trans[idx]
        bits = rows[:, 15].copy().view(np.int32)
        h = ((bits >> 16) & 7) + 1
        seen |= set(h.tolist())
        td = C.update(rows[:, 0:7], bits & 0xFF, rows[:, 7], rows[:, 8:15], (bits >> 8) & 1, isw=w, horizon=h)
        torch.cuda.synchronize()
        orc.per_update(prios, idx, _np(td))
    assert seen == {1, 2, 3}  # every horizon of the window was drawn
    C.idx.copy_(torch.from_numpy(idx))
    _same(orc, L, C, f"train_features {tf}")
    assert np.array_equal(_np(L.horizon), h)  # the gather wrote the rows' horizons next to act / done
    assert orc.bits_equal(_np(R.prios), prios)
    _tree_is_rebuild(orc, R)
    assert L.stats()["steps"] == updates and L.stats()["status"] == 0
    assert torch.equal(idx_last, L.idx) and torch.equal(td_last, L.td)


def test_pushed_horizons_round_trip_through_the_gather(orc, nets):
    from pongmi.replay import DeviceReplay
    cap, batch = 300, 33
    rng = np.random.default_rng(3)
    s, ns = rng.random((cap, 7), dtype=np.float32), rng.random((cap, 7), dtype=np.float32)
    a, r = rng.integers(0, 3, cap), rng.integers(-1, 2, cap).astype(np.float32)
    d, h = rng.random(cap) < 0.2, rng.integers(1, 9, cap)
    R = DeviceReplay(cap, "cuda", alpha=ALPHA)
    R.push(s[:200], a[:200], r[:200], ns[:200], d[:200], horizon=h[:200])
    assert R.max_horizon == int(h[:200].max())
    R.push(s[200:], a[200:], r[200:], ns[200:], d[200:])  # rows without a horizon are one step
    h[200:] = 1
    bits = _np(R.trans)[:, 15].copy().view(np.int32)
    assert np.array_equal(bits, a | (d.astype(np.int64) << 8) | ((h - 1) << 16))
    with pytest.raises(ValueError, match="horizons"):
        R.push(s[:2], a[:2], r[:2], ns[:2], d[:2], horizon=[1, 9])
    L = _learner(nets, batch, False, nstep=8)
    idx, _ = L.update_from(R, 1, beta_start=BETA_START, beta_frames=BETA_FRAMES, uniforms=rng.random((1, batch)))
    i = _np(idx)
    assert np.array_equal(_np(L.horizon), h[i]) and np.array_equal(_np(L.act), a[i])
    assert np.array_equal(_np(L.done), d[i].astype(np.uint8)) and orc.bits_equal(_np(L.rew), r[i])
    assert set(h[i].tolist()) > {1}


def test_ring_of_one_step_rows_gives_the_plain_paths_results(orc, nets):
    from pongmi import _lib
    batch, updates = 255, 3
    u = np.random.default_rng(2).random((updates, batch))
    out = []
    for nstep in (1, 3):
        R = _collected(nets, 1)
        L = _learner(nets, batch, True, nstep=nstep)
        L.update_from(R, updates, beta_start=BETA_START, beta_frames=BETA_FRAMES, uniforms=u)
        torch.cuda.synchronize()
        out.append((L, R))
    _same(orc, out[0][0], out[1][0], "one-step ring")
    assert torch.equal(out[0][1].prios, out[1][1].prios) and torch.equal(out[0][1].work, out[1][1].work)
    assert _np(out[1][0].horizon).tolist() == [1] * batch
    # and a learner built with nstep=1 refuses a ring that holds longer horizons
    R3 = _collected(nets, 3)
    with pytest.raises(_lib.PongmiError, match="nstep=1"):
        out[0][0].update_from(R3, 1)
