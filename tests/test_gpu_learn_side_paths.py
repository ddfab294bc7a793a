"""The learner launch's side paths: the side-A act blocks (run_tiles on 16 waves: whole rounds of 32-row
tiles and a partial last round) and the feature blocks, whose acting heads run as v_mfma_f32_4x4x1 chains
(tile_heads_mfma), one or two tiles per wave. The production step() against the plain step
(overlap=False: k_act_sp's 256-thread blocks, which round differently, k_env, k_learn without side
blocks): everything a step leaves is bit for bit equal after each of 6 steps, and gB equals the full
forward's greedy action.

    python tests/test_gpu_learn_side_paths.py forced   # the forced-timeout leg, run by its test in a
                                                       # child process under PONGMI_AHEAD_FORCE_TIMEOUT=1
"""
import hashlib
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
# compared after every step; per_work is the sum tree. aA and gB are compared in _twin (an overlapped
# step leaves the NEXT step's actions there, a plain one the actions it took)
ARRAYS = ("aB", "obsA", "obsB", "trans", "prios", "per_work", "paramsB", "learn_heads", "w_B")
SENTINEL = 3
STEPS, BATCH = 6, 32
WAVES = 16  # of a learner-launch side block


def _qnet_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "qnet.npz"), allow_pickle=False))


def _sd(g, who):
    return {k[len(who) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(who + ".") and "q_" not in k}


def _random_qnet_sd(seed):
    from models.qnet import QNet
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in QNet(7, 3).state_dict().items()}


def _learner(g, n, n_pool, seed, **kw):
    from pongmi.selfplay import SelfPlayLearner
    pool = [_random_qnet_sd(100 + k) for k in range(n_pool)]
    return SelfPlayLearner(ENV_KW, n, _sd(g, "modelB"), _sd(g, "modelA"), pool, batch=BATCH, memory_size=max(4 * n, 256),
                           epsilon=0.3, target_update_interval=3, seed=seed, **kw)


def _ahead(L):
    import ctypes
    from pongmi import _lib
    return L.lib.pm_selfplay_act_ahead(ctypes.byref(L.sp), _lib.PM_UPD_FIRST | _lib.PM_UPD_LAST, 1)


def _greedy_B(L):
    """k_act_sp(PM_ACT_B)'s greedy actions for the observations now in obsB, into scratch buffers."""
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


def _modelA_rows(L, chunk):
    """Rows of net 0 per side-A act block of `chunk` arenas, from the env blocks' opponent lists."""
    nets = L.n_pool + 1
    cnt = (L.opp_cnt.cpu().numpy().reshape(-1, nets)[:, 0] & 0xFFFF).astype(np.int64)
    seg = chunk // 256
    return [int(cnt[k:k + seg].sum()) for k in range(0, len(cnt), seg)]


def _twin(n, n_pool, seed, forced=False, digest=None, **kw):
    """step() (actions ahead, side blocks) against the plain step; returns the overlapped learner."""
    g = _qnet_golden()
    A = _learner(g, n, n_pool, seed, **kw)
    C = _learner(g, n, n_pool, seed, overlap=False, **kw)
    assert A.gB is not None and _ahead(A) == 1
    next_aA = None
    for k in range(STEPS):
        A.step()
        C.step()
        torch.cuda.synchronize()
        for name in ARRAYS:
            assert torch.equal(getattr(A, name), getattr(C, name)), (n, n_pool, k, name)
        if next_aA is not None:  # the actions A's side blocks left for this step are the ones C took
            assert torch.equal(next_aA, C.aA), (n, n_pool, k, "aA")
        next_aA = A.aA.clone()
        gB = A.gB.clone()
        if forced:
            assert bool((gB == SENTINEL).all()), "the fallback did not run"
        else:
            assert not bool((gB == SENTINEL).any()), (n, n_pool, k)
            assert torch.equal(gB, _greedy_B(A)), (n, n_pool, k, "gB")
        if digest is not None:
            for name in ARRAYS + ("aA",):
                digest.update(getattr(A, name).cpu().numpy().tobytes())
    assert A.counters() == C.counters() and A.counters()["train_steps"] > 0 and A.counters()["status"] == 0
    A.check_status()
    return A


@pytest.mark.parametrize("n", [1, 33, 512, 513, 544, 1000])
def test_tile_counts_around_a_full_block(n):
    """No pool: every arena plays net 0 and a side-A block takes 512 arenas, 16 tiles on 16 waves: a
    partial round, the whole round exactly, a second block of one row, of one tile, and a ragged one.
    n = 1 cannot hold a learner (the library requires n > batch >= 1): there the case checks that
    refusal."""
    from pongmi import _lib
    if n == 1:
        with pytest.raises(_lib.PongmiError):
            _learner(_qnet_golden(), n, 0, seed=41)
        return
    _twin(n, 0, seed=41)


@pytest.mark.parametrize("n", [768, 3000])
def test_more_tiles_than_waves(n):
    """Pool of 3 at ratio 0.1: modelA's side-A block takes 768 arenas, about 690 rows = 22 tiles on 16
    waves, so 6 waves run a second round (the pool nets' blocks hold a few rows: a partial round).
    3000: several blocks and a ragged last one."""
    A = _twin(n, 3, seed=43, pool_ratio=0.1)
    rows = _modelA_rows(A, 768)
    assert len(rows) == (n + 767) // 768
    assert max((r + 31) // 32 for r in rows) > WAVES, rows


@pytest.mark.parametrize("n_pool", [0, 3])
@pytest.mark.parametrize("n", [3000, 4096, 4100])
def test_feature_blocks(n, n_pool):
    """Feature blocks of kFeatTilesLearn = 16 tiles, one per wave: whole blocks (4096), a last block
    with idle waves and a partial tile (3000: 94 tiles, 24 rows in the last), n no multiple of 32 past
    whole blocks (4100)."""
    _twin(n, n_pool, seed=47)


def test_feature_blocks_with_two_tiles_per_wave():
    """65 536 arenas with a pool of 8 (the bench's shape) is the size at which the feature blocks get 18
    tiles, so two of a block's 16 waves run two head chains in one sweep (tile_heads_mfma2); modelA's act
    blocks hold about 515 rows there, 16 or 17 tiles."""
    A = _twin(65536, 8, seed=53)
    tiles = [(r + 31) // 32 for r in _modelA_rows(A, 768)]
    assert max(tiles) > WAVES and min(tiles) <= WAVES, tiles


def _digest_of(cases):
    d = hashlib.sha256()
    for n, n_pool in cases:
        _twin(n, n_pool, seed=59, forced=os.environ.get("PONGMI_AHEAD_FORCE_TIMEOUT") == "1", digest=d)
    return d.hexdigest()


FORCED_CASES = ((3000, 3), (4096, 0))


def test_forced_timeout_is_bitwise_the_unforced_run():
    """PONGMI_AHEAD_FORCE_TIMEOUT=1 in a fresh child process: every feature block's poll expires at once
    and every tile takes the fallback (features to featB, the sentinel to gB). Every array after every
    step is what the un-forced run here leaves (one digest over all of them)."""
    env = dict(os.environ, PONGMI_AHEAD_FORCE_TIMEOUT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "forced"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "FORCED_DIGEST " in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    forced = r.stdout.split("FORCED_DIGEST ")[1].split()[0]
    assert os.environ.get("PONGMI_AHEAD_FORCE_TIMEOUT") != "1"
    assert forced == _digest_of(FORCED_CASES)


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert sys.argv[1:] == ["forced"], sys.argv
    assert os.environ.get("PONGMI_AHEAD_FORCE_TIMEOUT") == "1"
    print("FORCED_DIGEST", _digest_of(FORCED_CASES))
