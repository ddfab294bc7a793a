"""store_ring_rows16's staging (pm_dev.h: lane l's four pieces cross the wave's LDS and leave as whole
lines), written for a bank-spread form of it (piece k of lane l's row in slot k ^ ((l >> 1) & 3), undone
inside the lane quad on the read) that passed this file and was left out because the step did not get
faster (DESIGN.md "k_actenv's two ends"); it pins the staging for the next attempt. Six steps of the production
step (k_actenv) and of the plain step (k_env) as twins. Both run the same staging, so beside the twins'
equality every pushed row is rebuilt from what the step read and wrote elsewhere (the observations
before and after it and the action taken: a piece in a wrong slot or row shows, the observations differ
in every arena), and every ring row outside the push range is bit-equal to a snapshot. The ring wraps
inside a wave, at a 16-row instruction boundary and at row 0 of a block; one case runs the workload's
65 536 arenas, where two blocks share a CU (the small shapes never put two blocks on one).

No episode ends in six steps (a serve starts at x = 0.5 with at most 0.05 per tick), so a pushed row's
next observation is the observation the step stored and its done flag is 0; both are asserted."""
import pytest
import torch

from test_gpu_selfplay import _learner

pytestmark = pytest.mark.gpu

STEPS = 6
# (n, cap) -> {step (1-based): first arena whose row wraps to slot 0}; pos = (step - 1) n mod cap
SHAPES = {
    (65, 146): {3: 16, 5: 32},       # 16-row instruction boundaries of wave 0
    (100, 237): {3: 37, 5: 74},      # inside wave 0 at a row that is no multiple of 4; wave 1, row 10
    (256, 592): {3: 80, 5: 160},     # wave 1, row 16 and wave 2, row 32: instruction boundaries past wave 0
    (300, 856): {3: 256, 6: 212},    # row 0 of block 1; block 0, wave 3, row 20
    (65536, 132072): {3: 1000, 5: 2000},  # block 3, wave 3, row 40; block 7, wave 3, row 16
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _first_half(L, half, step, wraps):
    """One step's acting, env tick and push on L, and the checks of the ring. Returns the wrap seen."""
    n, cap = L.n, L.cap
    torch.cuda.synchronize()
    pos = L.counters()["pos"]
    assert pos == (step - 1) * n % cap
    obs0, ring0 = L.obsB.clone(), _bits(L.trans).clone()
    half()
    torch.cuda.synchronize()
    ring1 = _bits(L.trans)
    slot = (pos + torch.arange(n, device=ring1.device)) % cap
    rows = ring1[slot]
    assert torch.equal(rows[:, 0:7], _bits(obs0)), (step, "s")
    assert torch.equal(rows[:, 8:15], _bits(L.obsB)), (step, "s'")
    assert torch.equal(rows[:, 15], L.aB.to(torch.int32)), (step, "action | done << 8, done = 0")
    outside = torch.ones(cap, dtype=torch.bool, device=ring1.device)
    outside[slot] = False
    assert torch.equal(ring1[outside], ring0[outside]), (step, "written outside the push range")
    want = wraps.get(step)
    if want is not None:
        assert cap - pos == want and 0 < want < n, (step, pos)
    return want


@pytest.mark.parametrize("n,cap", sorted(SHAPES))
def test_staging_stores_every_row_whole_and_in_place(golden, n, cap):
    from pongmi import _lib
    wraps = SHAPES[(n, cap)]
    kw = dict(n=n, batch=8 if n < 65536 else 256, cap=cap, seed=19, n_pool=2 if n < 65536 else 8)
    A = _learner(golden, **kw)                 # the production step: actenv() + the learner launch
    B = _learner(golden, overlap=False, **kw)  # the plain step: act + env_step, then learn

    def half_b():
        B.act()
        B.env_step()

    seen = []
    for step in range(1, STEPS + 1):
        if not A._aA_ready:
            A.act(_lib.PM_ACT_A)
        wa = _first_half(A, A.actenv, step, wraps)
        A.learn(act_next=True)
        A.apply()
        wb = _first_half(B, half_b, step, wraps)
        B.learn()
        B.apply()
        assert wa == wb
        seen += [step] if wa is not None else []
        assert torch.equal(_bits(A.trans), _bits(B.trans)), (step, "twins")
    torch.cuda.synchronize()
    assert seen == sorted(wraps)
    for name in ("prios", "per_work", "f64", "i32", "opp", "aB", "obsA", "obsB", "ep_reward", "paramsB"):
        assert torch.equal(getattr(A, name), getattr(B, name)), name
    assert A.counters() == B.counters() and A.counters()["status"] == 0
