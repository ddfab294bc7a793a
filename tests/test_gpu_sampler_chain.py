"""k_actenv's sampler blocks (sample_fwd_block32: one control-block read, straight-line level 0, the IS
weight formed behind the replay-row loads) against the two-launch first half of the plain step
(k_act_sp's sampler blocks + k_env's forward blocks), compared before any learner launch runs."""
import numpy as np
import pytest
import torch

from test_gpu_selfplay import _learner

pytestmark = pytest.mark.gpu

STEPS, SYNC = 6, 3  # one target sync among the compared steps
GUARD, GUARD_VALUE = 256, -7  # PM_MAX_BATCH entries past the batch: where a store gated on the thread index lands

# (batch, n, cap). (., 512, 2048): both sides of the 32-sample sampler block and of the wave boundary of
# the lanes that own a sample's weight (4 lanes per sample: 16 samples per wave, waves 0-1 of a block).
# n + 1 = cap + 1 > batch with cap = n: every sample lies in the push range, isw is the only output.
# (100, 300, 1000): a capacity that is no multiple of 64, the lo + 16 > cap leaf path; its n is also no
# multiple of 256, so the first fused step's env blocks take their feature tiles from a ragged featB.
SHAPES = [(b, 512, 2048) for b in (1, 31, 32, 33, 64, 255, 256)] + [(33, 34, 34), (255, 256, 256), (100, 300, 1000)]
SEED = 21


def _guard_batch_tails(L):
    """Re-point the learner's idx / isw (ABI: [batch]) at buffers GUARD entries longer whose tails hold
    a sentinel (test_gpu_selfplay.py's idiom)."""
    from pongmi._lib import ptr
    L.idx = torch.cat([L.idx, torch.full((GUARD,), GUARD_VALUE, dtype=L.idx.dtype, device=L.idx.device)])
    L.isw = torch.cat([L.isw, torch.full((GUARD,), GUARD_VALUE, dtype=L.isw.dtype, device=L.isw.device)])
    L.sp.idx, L.sp.isw = ptr(L.idx), ptr(L.isw)
    return L


def _assert_batch_tails(*learners):
    for L in learners:
        assert L.idx.numel() == L.batch + GUARD
        assert bool((L.idx[L.batch:] == GUARD_VALUE).all()), "idx written past batch"
        assert bool((L.isw[L.batch:] == GUARD_VALUE).all()), "isw written past batch"


def _half(L):
    """idx, isw, the sample rows of hfeat (as bits) and the counters, right after a step's first half."""
    torch.cuda.synchronize()
    _assert_batch_tails(L)
    B = L.batch
    return (L.idx[:B].cpu().numpy().copy(), L.isw[:B].cpu().numpy().view(np.uint32).copy(),
            L.hfeat[:B, :75].cpu().numpy().view(np.uint32).copy(), L.counters())


@pytest.mark.parametrize("batch,n,cap", SHAPES)
def test_actenv_sampler_equals_act_plus_env_before_the_learner(golden, batch, n, cap):
    """Twin learners on one seed. A's step is actenv() + the learner launch (the production step), B's
    is act(PM_ACT_B) + env_step() + learn(). After the first half of each of 6 steps, before any learner
    launch: idx and isw bit for bit (nothing past `batch` written), and floats 0..74 of every hfeat row
    whose sample lies outside the step's push range (the rows the first half computes; the rest are
    k_learn's). Precondition of the (., 512, 2048) cases from batch 31 up, from B's idx and counters
    alone: in some compared step a sample lies inside the push range and another outside, so both the
    `mine` rows and the skipped ones are exercised (seed 21: on the CPU port, oracle/cpu_selfplay.py,
    steps 2..6 are mixed at every one of these batch sizes; step 1 has the whole fill in the range)."""
    from pongmi import _lib
    kw = dict(n=n, batch=batch, cap=cap, seed=SEED, n_pool=2, target_update_interval=SYNC)
    A = _guard_batch_tails(_learner(golden, **kw))
    B = _guard_batch_tails(_learner(golden, overlap=False, **kw))
    mixed, rows = 0, 0
    for step in range(STEPS):
        if not A._aA_ready:
            A.act(_lib.PM_ACT_A)
        A.actenv()
        B.act(_lib.PM_ACT_A)
        B.act(_lib.PM_ACT_B)
        B.env_step()
        ia, wa, ha, ca = _half(A)
        ib, wb, hb, cb = _half(B)
        assert ca == cb, step
        assert np.array_equal(ia, ib), (step, "idx")
        assert np.array_equal(wa, wb), (step, "isw")
        inside = (ib - cb["pos"]) % cap < n  # the push this step makes: [pos, pos + n) mod cap
        assert ((ib >= 0) & (ib < min(cb["size"] + n, cap))).all(), step
        mixed += bool(inside.any() and not inside.all())
        rows += int((~inside).sum())
        assert np.array_equal(ha[~inside], hb[~inside]), (step, "hfeat")
        A.learn(act_next=True)
        A.apply()
        B.learn()
        B.apply()
    torch.cuda.synchronize()
    _assert_batch_tails(A, B)
    print(f"batch {batch} n {n} cap {cap}: {mixed} of {STEPS} steps mixed, {rows} stable rows compared")
    if cap == n:
        assert rows == 0  # isw (and idx) are the only outputs
    if (n, cap) == (512, 2048) and batch >= 31:
        assert mixed >= 1, "precondition: no step with samples on both sides of the push range"
    c = A.counters()
    assert c == B.counters() and c["train_steps"] == STEPS and c["status"] == 0
