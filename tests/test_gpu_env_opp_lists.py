"""The per-block opponent lists the env blocks leave for the next act (pm_mfma.h write_opp_lists in
env_block's tail): after the fused step's k_actenv and after the plain step's k_env, at arena counts
on both sides of a 256-arena block and of a wave, with pools of 0, 1, 2, 63 and 64 nets (65 lists are above kListNets: no lists are written)."""
import numpy as np
import pytest
import torch

from test_gpu_selfplay import _learner

pytestmark = pytest.mark.gpu

SENTINEL = -7
K_LIST_NETS = 64


def _host_lists(opp, nn):
    """Per 256-arena block: nets ascending, arenas ascending within a net; offset << 16 | count per net.
    Returns (list entries per block, cnt)."""
    n = len(opp)
    neb = (n + 255) // 256
    lists, cnt = [], np.zeros(neb * nn, np.int32)
    for e in range(neb):
        ids = opp[e * 256:(e + 1) * 256]
        off, lst = 0, []
        for k in range(nn):
            sel = np.nonzero(ids == k)[0] + e * 256
            lst.extend(sel.tolist())
            cnt[e * nn + k] = (off << 16) | len(sel)
            off += len(sel)
        assert off == len(ids)
        lists.append(np.array(lst, np.int32))
    return lists, cnt


def _check(L, what):
    torch.cuda.synchronize()
    nn = L.n_pool + 1
    opp = L.opp.cpu().numpy()
    lst, cnt = L.opp_list.cpu().numpy(), L.opp_cnt.cpu().numpy()
    assert opp.min() >= 0 and opp.max() < nn
    if nn > K_LIST_NETS:
        assert (lst == SENTINEL).all() and (cnt == SENTINEL).all(), (what, "lists written above kListNets")
        return
    want, wcnt = _host_lists(opp, nn)
    assert np.array_equal(cnt, wcnt), (what, "opp_cnt")
    for e, w in enumerate(want):
        got = lst[e * 256:(e + 1) * 256]
        assert np.array_equal(got[:len(w)], w), (what, "opp_list", e)
        assert (got[len(w):] == SENTINEL).all(), (what, "opp_list written past the block's arenas", e)


@pytest.mark.parametrize("n_pool", [0, 1, 2, 63, 64])
@pytest.mark.parametrize("n", [255, 256, 257, 300, 1000])
def test_env_blocks_write_grouped_opponent_lists(golden, n, n_pool):
    from pongmi import _lib
    kw = dict(n=n, batch=8, cap=4 * n, seed=41, n_pool=n_pool, pool_ratio=0.7)
    A = _learner(golden, **kw)                 # k_actenv
    B = _learner(golden, overlap=False, **kw)  # k_env
    rng = np.random.RandomState(n * 100 + n_pool)
    used = set()
    for step in range(3):
        # The acts run first, on the lists the step before left (consistent with the nets it left). Then
        # any net for any arena (the serve's own draw changes few of them per step) and a sentinel in
        # both buffers: the env blocks must rebuild every list from the nets they store.
        if not A._aA_ready:
            A.act(_lib.PM_ACT_A)
        B.act()
        opp = torch.from_numpy(rng.randint(0, n_pool + 1, n).astype(np.int32)).cuda()
        for L in (A, B):
            L.opp.copy_(opp)
            L.opp_list.fill_(SENTINEL)
            L.opp_cnt.fill_(SENTINEL)
        A.actenv()
        _check(A, ("actenv", step))
        A.learn(act_next=True)
        A.apply()
        B.env_step()
        _check(B, ("env_step", step))
        B.learn()
        B.apply()
        assert torch.equal(A.opp, B.opp) and torch.equal(A.opp_list, B.opp_list) and torch.equal(A.opp_cnt, B.opp_cnt)
        used |= set(A.opp.cpu().numpy().tolist())
    if n_pool + 1 <= n // 8:
        assert len(used) == n_pool + 1  # every net's list was non-empty somewhere
    assert A.counters()["status"] == 0 and B.counters()["status"] == 0
