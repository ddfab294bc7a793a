"""k_actenv's sampler blocks on 16-column matrix-core tiles (sample_fwd_block16: 8 samples per block,
columns 0-7 their s rows, columns 8-15 their s' rows) against the two-launch first half of the plain
step (k_act_sp's sampler blocks + k_env's forward blocks on 32-row tiles), compared before any learner
launch runs, at the batch sizes where the 8-sample block and the 16-column tile change shape."""
import numpy as np
import pytest
import torch

from test_gpu_selfplay import _learner

pytestmark = pytest.mark.gpu

STEPS, SYNC = 6, 3  # one target sync among the compared steps
GUARD, GUARD_VALUE = 256, -7  # PM_MAX_BATCH entries past the batch: where a store gated on the thread index lands

# (batch, n, cap). (., 512, 2048): both sides of the 8-sample block (7, 8, 9; 15, 16, 17; 24), so also of
# the tile's s / s' column boundary with a part-filled and a full last tile, and a last block with one
# (249) and two (250) live samples behind 31 full ones. (9, 10, 10): n + 1 = cap + 1 > batch with cap = n,
# every sample lies in the push range and idx / isw are the only outputs. (20, 300, 1000): a capacity
# that is no multiple of 64 (the lo + 16 > cap leaf path) and an n that is no multiple of 256 (the first
# fused step's env blocks take their feature tiles from a ragged featB).
SHAPES = [(b, 512, 2048) for b in (7, 8, 9, 15, 16, 17, 24, 249, 250)] + [(9, 10, 10), (20, 300, 1000)]
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


def _arm_hfeat(L):
    """hfeat's rows past the batch before a first half. Rows [batch, 2 batch) are the learner launch's
    push-row payload, written and read inside one launch under its flag, so a sentinel there disturbs
    nothing; they are where a sampler block's store that is not gated on j < batch lands (a block's
    columns reach sample 8 ceil(batch / 8) - 1 <= batch + 6). The rows from 2 batch on carry the
    learner's flag, epochs and tagged granules from launch to launch: those are compared with a copy."""
    B = L.batch
    assert L.hfeat.shape[0] >= 2 * B + 1
    L.hfeat[B:2 * B] = float(GUARD_VALUE)
    torch.cuda.synchronize()
    return L.hfeat[2 * B:].clone()


def _assert_hfeat_tail(L, kept):
    B = L.batch
    assert bool((L.hfeat[B:2 * B] == float(GUARD_VALUE)).all()), "hfeat written past batch"
    assert torch.equal(L.hfeat[2 * B:].view(torch.int32), kept.view(torch.int32)), "hfeat hand-off rows written"


def _half(L):
    """idx, isw, the sample rows of hfeat (as bits) and the counters, right after a step's first half."""
    torch.cuda.synchronize()
    _assert_batch_tails(L)
    B = L.batch
    return (L.idx[:B].cpu().numpy().copy(), L.isw[:B].cpu().numpy().view(np.uint32).copy(),
            L.hfeat[:B, :75].cpu().numpy().view(np.uint32).copy(), L.counters())


@pytest.mark.parametrize("batch,n,cap", SHAPES)
def test_actenv_tile16_equals_act_plus_env_before_the_learner(golden, batch, n, cap):
    """Twin learners on one seed. A's step is actenv() + the learner launch (the production step), B's
    is act(PM_ACT_B) + env_step() + learn(). After the first half of each of 6 steps, before any learner
    launch: idx and isw bit for bit (nothing past `batch` written), floats 0..74 of every hfeat row whose
    sample lies outside the step's push range (the rows the first half computes; the rest are k_learn's),
    the counters, and A's hfeat rows from `batch` on as they were before the half. Preconditions, from
    B's outputs alone: at every (., 512, 2048) shape some compared step has samples on both sides of the
    push range (from step 2 on half or more of the priority mass lies in the range, so an unmixed batch
    of 7 has probability below 2 % per step; seed 21), and in some compared step the Q_T slots differ in
    bits from the Q_B(s') slots, i.e. the target heads are not the online ones there."""
    from pongmi import _lib
    kw = dict(n=n, batch=batch, cap=cap, seed=SEED, n_pool=2, target_update_interval=SYNC)
    A = _guard_batch_tails(_learner(golden, **kw))
    B = _guard_batch_tails(_learner(golden, overlap=False, **kw))
    mixed, rows, qt_differs = 0, 0, 0
    for step in range(STEPS):
        if not A._aA_ready:
            A.act(_lib.PM_ACT_A)
        kept = _arm_hfeat(A)
        A.actenv()
        B.act(_lib.PM_ACT_A)
        B.act(_lib.PM_ACT_B)
        B.env_step()
        ia, wa, ha, ca = _half(A)
        ib, wb, hb, cb = _half(B)
        _assert_hfeat_tail(A, kept)
        assert ca == cb, step
        assert np.array_equal(ia, ib), (step, "idx")
        assert np.array_equal(wa, wb), (step, "isw")
        inside = (ib - cb["pos"]) % cap < n  # the push this step makes: [pos, pos + n) mod cap
        assert ((ib >= 0) & (ib < min(cb["size"] + n, cap))).all(), step
        mixed += bool(inside.any() and not inside.all())
        rows += int((~inside).sum())
        qt_differs += bool((hb[~inside][:, 72:75] != hb[~inside][:, 68:71]).any())
        assert np.array_equal(ha[~inside], hb[~inside]), (step, "hfeat")
        A.learn(act_next=True)
        A.apply()
        B.learn()
        B.apply()
    torch.cuda.synchronize()
    _assert_batch_tails(A, B)
    print(f"batch {batch} n {n} cap {cap}: {mixed} of {STEPS} steps mixed, {rows} stable rows compared, "
          f"Q_T != Q_B(s') in {qt_differs} steps")
    if cap == n:
        assert rows == 0  # idx and isw are the only outputs
    if (n, cap) == (512, 2048):
        assert mixed >= 1, "precondition: no step with samples on both sides of the push range"
    if rows:
        assert qt_differs >= 1, "precondition: the target heads never differed from the online ones"
    c = A.counters()
    assert c == B.counters() and c["train_steps"] == STEPS and c["status"] == 0


def _final(L):
    torch.cuda.synchronize()
    return L.paramsB.cpu().numpy().view(np.uint32).copy(), L.prios.cpu().numpy().view(np.uint32).copy(), L.counters()


def test_six_full_steps_equal_the_plain_step(golden):
    """Update-complete: 6 full step()s of twin learners at (17, 512, 2048), the fused step (k_actenv with
    the 16-column sampler tile + the learner launch) against the plain one: the final paramsB, the
    priorities and the counters are equal bit for bit and the status is 0."""
    kw = dict(n=512, batch=17, cap=2048, seed=SEED, n_pool=2, target_update_interval=SYNC)
    A = _learner(golden, **kw)
    B = _learner(golden, overlap=False, **kw)
    for _ in range(STEPS):
        A.step()
        B.step()
    pa, ra, ca = _final(A)
    pb, rb, cb = _final(B)
    assert ca == cb and ca["status"] == 0 and ca["train_steps"] == STEPS
    assert np.array_equal(pa, pb), "paramsB"
    assert np.array_equal(ra, rb), "prios"
