"""Actions ahead (ABI 26): in the fused U = 1 step the learner launch's feature blocks take the next
step's acting heads from the learner and leave modelB's greedy action per arena in sp.gB; k_actenv's
env blocks read that byte instead of 256 B of features and a head pass. Everything a step leaves is
bit for bit what the featB path, the full forward in k_actenv and the plain step leave, also when
the hand-off times out (the fallback stores the features as before).

    python tests/test_gpu_actions_ahead.py forced    # the forced-timeout leg, run by its test in a
                                                     # child process under PONGMI_AHEAD_FORCE_TIMEOUT=1
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_KW = dict(paddle_speed=0.03, max_score=3, magnus_factor=0.025, restitution=1, friction=0.6,
              ball_speed_range=[0.03, 0.05], spin_range=[-5, 5], speed_scale_every=1, speed_increment=0.1)
# test_features_ahead_is_bitwise_identical's list; aA only between overlapped learners (after a plain
# step it holds the actions taken, after an overlapped one the next step's)
TENSORS = ("paramsB", "paramsT", "adam_m", "adam_v", "prios", "trans", "f64", "i32", "opp", "w_B", "learn_heads",
           "per_work", "idx", "isw", "aB", "obsA", "obsB", "ep_reward")
SENTINEL = 3


def _qnet_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "qnet.npz"), allow_pickle=False))


def _sd(g, who):
    return {k[len(who) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(who + ".") and "q_" not in k}


def _random_qnet_sd(seed):
    from models.qnet import QNet
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in QNet(7, 3).state_dict().items()}


def _learner(g, n, batch, cap, n_pool, seed, **kw):
    from pongmi.selfplay import SelfPlayLearner
    pool = [_random_qnet_sd(100 + k) for k in range(n_pool)]
    return SelfPlayLearner(ENV_KW, n, _sd(g, "modelB"), _sd(g, "modelA"), pool, batch=batch, memory_size=cap,
                           epsilon=0.3, target_update_interval=3, seed=seed, **kw)


def _ahead(L):
    """The library's own answer: would this learner's fused learner launch leave actions in gB?"""
    import ctypes
    from pongmi import _lib
    return L.lib.pm_selfplay_act_ahead(ctypes.byref(L.sp), _lib.PM_UPD_FIRST | _lib.PM_UPD_LAST, 1)


def _greedy_B(L):
    """What k_act_sp(PM_ACT_B) writes into aB for the observations now in obsB: the full forward's
    argmax (k_env applies the epsilon draw later). Its outputs (aB, and the PER sample it also draws)
    go to scratch buffers, so the learner's state is as before."""
    from pongmi import _lib
    keep = (L.sp.aB, L.sp.idx, L.sp.isw)
    aB, idx, isw = torch.full_like(L.aB, 9), torch.zeros_like(L.idx), torch.zeros_like(L.isw)
    L.sp.aB, L.sp.idx, L.sp.isw = _lib.ptr(aB), _lib.ptr(idx), _lib.ptr(isw)
    try:
        L.act(_lib.PM_ACT_B)
        torch.cuda.synchronize()
    finally:
        L.sp.aB, L.sp.idx, L.sp.isw = keep
    return aB


@pytest.mark.parametrize("n_pool", [0, 3])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 3000])
def test_gB_is_the_full_forwards_greedy_action(n, n_pool):
    """After L.step() gB holds no sentinel and equals, arena by arena, the greedy action of the full
    forward (k_act_sp(PM_ACT_B)) on the same observations and weights: partial tiles, partial env
    blocks, one and several feature blocks. n = 1 cannot hold a learner at all (the library requires
    batch >= 1 and n > batch, include/pongmi.h): there the case checks that refusal."""
    from pongmi import _lib
    g = _qnet_golden()
    if n == 1:
        with pytest.raises(_lib.PongmiError):
            _learner(g, n, 1, 64, n_pool, seed=31)
        return
    L = _learner(g, n, min(32, n // 2), max(4 * n, 256), n_pool, seed=31)
    assert L.gB is not None and bool((L.gB == SENTINEL).all()) and _ahead(L) == 1
    for k in range(4):
        L.step()
        torch.cuda.synchronize()
        assert L._gB_ready and L.sp.gB_ready == (k > 0)  # the first step's k_actenv read featB
        gB = L.gB.clone()
        assert not bool((gB == SENTINEL).any()), (n, k)
        assert torch.equal(gB, _greedy_B(L)), (n, n_pool, k)
    L.check_status()
    assert L.counters()["train_steps"] > 0


def _run_equal(g, n, batch, steps=20, expect_gB=True):
    """Default learner (actions ahead, driven through step() and the piecewise API) against
    features_ahead=False (k_actenv's full forward) and overlap=False (the plain step)."""
    from pongmi import _lib
    kw = dict(n=n, batch=batch, cap=16384, n_pool=3, seed=23)
    A = _learner(g, **kw)
    B = _learner(g, features_ahead=False, **kw)
    C = _learner(g, overlap=False, **kw)
    assert A.featB is not None and A.gB is not None and B.featB is None and B.gB is None
    used = 0
    for k in range(steps):
        if k == 4:
            for L in (A, B, C):
                L.set_epsilon(0.11)
        if k == 6:
            sd = _random_qnet_sd(77)
            for L in (A, B, C):
                L.set_modelA(sd)
        if k == 11:
            sd = _random_qnet_sd(91)
            for L in (A, B, C):
                L.reset_B(sd, epsilon=0.2)
        if k % 4 in (1, 3):  # the piecewise API
            if not A._aA_ready:
                A.act(_lib.PM_ACT_A)
            if k % 4 == 1:
                A.actenv()
            else:
                A.act(_lib.PM_ACT_B)
                A.env_step()
            A.learn(act_next=True)
            A.apply()
        else:
            A.step()
        used += int(A._gB_ready)
        B.step()
        C.step()
    torch.cuda.synchronize()
    for name in TENSORS + ("aA",):
        assert torch.equal(getattr(A, name), getattr(B, name)), (n, batch, "features_ahead=False", name)
    for name in TENSORS:
        assert torch.equal(getattr(A, name), getattr(C, name)), (n, batch, "overlap=False", name)
    ca = A.counters()
    assert ca == B.counters() and ca == C.counters()
    assert ca["train_steps"] > 0 and ca["status"] == 0
    A.check_status()
    assert used == (steps if expect_gB else 0)  # every learner launch of A took (or did not take) the new path
    return A


@pytest.mark.parametrize("batch", [32, 256])
@pytest.mark.parametrize("n", [3000, 4096])
def test_actions_ahead_is_bitwise_identical(n, batch):
    A = _run_equal(_qnet_golden(), n, batch)
    assert not bool((A.gB == SENTINEL).any())


def test_switched_off_is_bitwise_identical(monkeypatch):
    """PONGMI_ACT_AHEAD=0 (read per launch) keeps the featB path from the same library: the same
    results, gB never written."""
    monkeypatch.setenv("PONGMI_ACT_AHEAD", "0")
    g = _qnet_golden()
    for n, batch in ((3000, 32), (4096, 256)):
        A = _run_equal(g, n, batch, expect_gB=False)
        assert bool((A.gB == SENTINEL).all())


def _forced_main():
    """Child process, PONGMI_AHEAD_FORCE_TIMEOUT=1: every feature block's poll expires at once, so
    every tile takes the fallback (features to featB, the sentinel to gB): the same bits, status 0."""
    assert os.environ.get("PONGMI_AHEAD_FORCE_TIMEOUT") == "1"
    g = _qnet_golden()
    for n, batch in ((3000, 32), (4096, 256)):
        A = _run_equal(g, n, batch)  # the path is on (gB_ready) and falls back tile by tile
        assert bool((A.gB == SENTINEL).all()), "the fallback did not run"
    print("FORCED_TIMEOUT_OK")


def test_forced_timeout_falls_back_bitwise():
    env = dict(os.environ, PONGMI_AHEAD_FORCE_TIMEOUT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "forced"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "FORCED_TIMEOUT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_two_tiles_per_wave_at_the_workloads_size():
    """65 536 arenas, pool 8 (the bench's shape): the only size at which a feature block's wave parks
    two tiles (18 tiles on 16 waves)."""
    g = _qnet_golden()
    kw = dict(n=65536, batch=256, cap=131072, n_pool=8, seed=37)
    A = _learner(g, **kw)
    B = _learner(g, features_ahead=False, **kw)
    assert _ahead(A) == 1
    for _ in range(6):
        A.step()
        B.step()
    torch.cuda.synchronize()
    assert A._gB_ready and not bool((A.gB == SENTINEL).any())
    for name in TENSORS + ("aA",):
        assert torch.equal(getattr(A, name), getattr(B, name)), name
    assert A.counters() == B.counters() and A.counters()["train_steps"] > 0
    A.check_status()


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert sys.argv[1:] == ["forced"], sys.argv
    _forced_main()
