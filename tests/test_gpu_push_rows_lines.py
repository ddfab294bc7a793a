"""The env blocks' replay push as whole-line stores (pm_dev.h store_ring_rows16: lane l stores piece
l & 3 of row (l >> 2) + 16 k of its wave, the slot taken per stored row): every step of the production
step (k_actenv) and of the plain step (k_env) against the oracle, and every ring row, priority and PER
leaf outside the step's push range bit-equal to what it was, so a row landing in a wrong slot shows
both where it is missing and where it landed."""
import numpy as np
import pytest
import torch

from test_gpu_selfplay import _check_rollout, _learner, _snap

pytestmark = pytest.mark.gpu

STEPS = 6
# (batch, n, cap): both sides of one 256-arena block, a ragged second block, a ring that wraps inside a
# wave of block 0 (300 / 1000) and of a later block at a row that is no multiple of 4 or 16 (513 / 1300),
# and n = cap (the push range is the whole ring, pos stays 0).
SHAPES = [(8, 255, 1000), (8, 256, 1000), (8, 257, 1000), (8, 300, 1000), (8, 513, 1300), (33, 34, 34)]
# (n, cap) -> {step (1-based): first arena whose row wraps to slot 0}, asserted from the counters
WRAPS = {(300, 1000): {4: 100}, (513, 1300): {3: 274, 6: 35}}


def _leaves(L):
    """The PER leaves in per_work (csrc/pm_per.h: level-2 sums, level-1 sums, leaves; each section
    padded to 256 bytes), as bits."""
    pad = lambda doubles: (doubles * 8 + 255) // 256 * 256  # noqa: E731
    off = pad((L.cap + 1023) // 1024) + pad((L.cap + 63) // 64)
    return L.per_work[off:off + 4 * L.cap].view(torch.float32).cpu().numpy().view(np.uint32).copy()


def _ring(L):
    torch.cuda.synchronize()
    return (L.trans.cpu().numpy().view(np.uint32).copy(), L.prios.cpu().numpy().view(np.uint32).copy(), _leaves(L))


def _check_push(orc, L, step, first_half, seen):
    """One step's first half (acting, env tick, push) on L: the oracle's rollout check, the untouched
    rest of the ring, and the wrap preconditions of this shape."""
    n, cap = L.n, L.cap
    pre, ring0 = _snap(L), _ring(L)
    first_half()
    post, ring1 = _snap(L), _ring(L)
    _check_rollout(orc, L, pre, post)
    pos = pre["ctrl"]["pos"]
    assert pos == (step - 1) * n % cap  # (the learner launch advances it)
    inside = (np.arange(cap) - pos) % cap < n
    for name, a, b in zip(("trans", "prios", "leaf"), ring0, ring1):
        assert np.array_equal(a[~inside], b[~inside]), (step, name, "written outside the push range")
    # the pushed leaves: one value for the whole push (max_prio ** alpha), never the zero of an empty slot
    lv = ring1[2][inside]
    assert (lv == lv[0]).all() and lv[0] != 0, (step, "leaf")
    want = WRAPS.get((n, cap), {}).get(step)
    if want is not None:
        assert cap - pos == want and 0 < want < n, (step, pos)
        seen.append((step, want, want // 256, want % 256))


@pytest.mark.parametrize("batch,n,cap", SHAPES)
def test_production_and_plain_push_match_oracle_and_touch_nothing_else(orc, golden, batch, n, cap):
    from pongmi import _lib
    kw = dict(n=n, batch=batch, cap=cap, seed=17, n_pool=2, target_update_interval=3)
    A = _learner(golden, **kw)                 # the production step: actenv() + the learner launch
    B = _learner(golden, overlap=False, **kw)  # the plain step: act + env_step, then learn
    seenA, seenB = [], []

    def half_a():
        A.actenv()

    def half_b():
        B.act()
        B.env_step()

    for step in range(1, STEPS + 1):
        if not A._aA_ready:  # before the snapshot: aA of the observations the step acts on
            A.act(_lib.PM_ACT_A)
        _check_push(orc, A, step, half_a, seenA)
        A.learn(act_next=True)
        A.apply()
        _check_push(orc, B, step, half_b, seenB)
        B.learn()
        B.apply()
    torch.cuda.synchronize()
    for name in ("trans", "prios", "per_work", "f64", "i32", "opp", "aB", "obsA", "obsB", "ep_reward", "paramsB"):
        assert torch.equal(getattr(A, name), getattr(B, name)), name
    assert A.counters() == B.counters() and A.counters()["status"] == 0
    wraps = WRAPS.get((n, cap), {})
    assert seenA == seenB and [s for s, *_ in seenA] == sorted(wraps)
    if (n, cap) == (300, 1000):
        # a wrap inside wave 1 of block 0, at a row that is a multiple of 4 but not of 16
        assert seenA == [(4, 100, 0, 100)] and 100 % 64 != 0 and 100 % 16 != 0
    if (n, cap) == (513, 1300):
        # block 1, row 18 (no multiple of 4 or 16, inside wave 0) and block 0, row 35 (odd, inside wave 0)
        assert seenA == [(3, 274, 1, 18), (6, 35, 0, 35)] and 18 % 4 != 0 and 35 % 4 != 0
    if n == cap:
        assert A.counters()["pos"] == 0
