"""write_opp_lists' packed scan (pm_mfma.h: up to 16 nets, byte fields of four words, one wave scan
per word, one barrier) and the ballot loop it left for 17-64 nets, against a numpy stable grouping:
after the plain step's k_env (env_step()) and the fused step's k_actenv, at arena counts on both sides
of a wave and of a 256-arena block, with net counts on both sides of a packed word's four fields and
of the packed path's limit, and with forced assignments that put a whole wave (64) and a whole block
(256) on one net, the sums a 7-bit field and an 8-bit field would lose.

The self-play learner's ABI wants more arenas than the batch (n > batch >= 1), so one arena runs
through the QNetRNN self-play learner's env_step() (k_rsp_env shares the function), which also runs a
ragged second block.

No episode ends in the steps taken here (a serve starts at x = 0.5 with at most 0.05 per tick, and
an episode is three points), so the forced nets are the nets the env blocks store, checked below."""
import numpy as np
import pytest
import torch

from test_gpu_selfplay import _learner

SENTINEL = -7
ARENAS = [1, 63, 64, 65, 255, 256, 257, 300]
POOLS = [0, 1, 3, 4, 7, 8, 15, 16, 63]  # + modelA: 1, 2, 4, 5, 8, 9, 16 nets packed; 17 and 64 the loop
PATTERNS = ["one net: 0", "one net: top field of word 0", "one net: the last", "alternating", "one arena per net",
            "random"]


def _forced(pattern, n, nn, rng):
    i = np.arange(n)
    if pattern == "one net: 0":
        opp = np.zeros(n)
    elif pattern == "one net: top field of word 0":
        opp = np.full(n, min(3, nn - 1))
    elif pattern == "one net: the last":
        opp = np.full(n, nn - 1)
    elif pattern == "alternating":  # consecutive lanes on consecutive nets
        opp = i % nn
    elif pattern == "one arena per net":
        # nets 1 .. nn - 1 hold one arena of every block each (as far as the block has rows), in
        # descending arena order, so the list's order is not the arenas'; the rest play net 0
        r = i % 256
        rows = np.minimum(256, n - (i - r))
        k = rows - 1 - r
        opp = np.where((k >= 1) & (k < nn), k, 0)
    else:
        opp = rng.randint(0, nn, n)
    return opp.astype(np.int32)


def _group(opp, nn):
    """numpy's stable grouping: per 256-arena block the arenas sorted by net with a stable sort (equal
    nets keep arena order), and offset << 16 | count per net. Returns (list [n], cnt [blocks * nn])."""
    n = len(opp)
    lst = np.empty(n, np.int32)
    cnt = np.empty(((n + 255) // 256) * nn, np.int32)
    for e in range((n + 255) // 256):
        ids = opp[e * 256:(e + 1) * 256]
        lst[e * 256:e * 256 + len(ids)] = e * 256 + np.argsort(ids, kind="stable")
        c = np.bincount(ids, minlength=nn)
        cnt[e * nn:(e + 1) * nn] = ((np.cumsum(c) - c) << 16) | c
    return lst, cnt


def _rule(opp, nn):
    """The ordering rule spelt out: nets ascending, arenas ascending within a net, one arena at a time."""
    n = len(opp)
    lst, cnt = [], []
    for e in range((n + 255) // 256):
        off = 0
        for k in range(nn):
            members = [i for i in range(e * 256, min(n, e * 256 + 256)) if opp[i] == k]
            assert members == sorted(members)
            lst += members
            cnt.append((off << 16) | len(members))
            off += len(members)
    return np.array(lst, np.int32), np.array(cnt, np.int32)


@pytest.mark.parametrize("n_pool", POOLS)
def test_numpy_grouping_is_the_ordering_rule(n_pool):
    """CPU: the reference of the GPU test below restates "ascending within a net" for every input it sees."""
    nn = n_pool + 1
    for n in ARENAS:
        rng = np.random.RandomState(n * 100 + n_pool)
        for pattern in PATTERNS:
            opp = _forced(pattern, n, nn, rng)
            assert opp.min() >= 0 and opp.max() < nn
            lst, cnt = _group(opp, nn)
            wl, wc = _rule(opp, nn)
            assert np.array_equal(lst, wl) and np.array_equal(cnt, wc), (n, pattern)
            if pattern.startswith("one net") and n >= 256:
                assert (cnt & 0xffff).max() == 256  # a block's count past 8 bits
            if pattern == "one arena per net" and min(n, 256) >= nn:
                c = cnt[:nn] & 0xffff
                assert (c[1:] == 1).all() and (np.diff(lst[c[0]:c[0] + nn - 1]) < 0).all()  # block 0: descending arenas


def _pad_lists(L):
    """The lists in buffers longer than the kernels may write: a store past the valid arenas shows. They
    keep what the init kernel wrote: the next act reads its rows through them (offsets and counts of a
    sentinel would send it out of bounds)."""
    from pongmi._lib import ptr
    torch.cuda.synchronize()
    neb = (L.n + 255) // 256
    lst, cnt = L.opp_list, L.opp_cnt
    assert lst.numel() == L.n and cnt.numel() == neb * (L.n_pool + 1)
    L.opp_list = torch.full((neb * 256 + 256,), SENTINEL, dtype=torch.int32, device=L.opp.device)
    L.opp_cnt = torch.full((cnt.numel() + 64,), SENTINEL, dtype=torch.int32, device=L.opp.device)
    L.opp_list[:L.n] = lst
    L.opp_cnt[:cnt.numel()] = cnt
    L.sp.opp_list, L.sp.opp_cnt = ptr(L.opp_list), ptr(L.opp_cnt)
    torch.cuda.synchronize()


def _check(L, forced, nn, what):
    torch.cuda.synchronize()
    n = L.n
    assert np.array_equal(L.opp.cpu().numpy(), forced), (what, "an episode ended: the forced nets were redrawn")
    lst, cnt = L.opp_list.cpu().numpy(), L.opp_cnt.cpu().numpy()
    wl, wc = _group(forced, nn)
    assert np.array_equal(cnt[:len(wc)], wc), (what, "opp_cnt")
    assert (cnt[len(wc):] == SENTINEL).all(), (what, "opp_cnt written past the last block's nets")
    assert np.array_equal(lst[:n], wl), (what, "opp_list")
    assert (lst[n:] == SENTINEL).all(), (what, "opp_list written past the valid arenas")


@pytest.mark.gpu
@pytest.mark.parametrize("n_pool", POOLS)
@pytest.mark.parametrize("n", ARENAS[1:])
def test_packed_and_looped_lists_match_numpy_grouping(golden, n, n_pool):
    from pongmi import _lib
    nn = n_pool + 1
    kw = dict(n=n, batch=8, cap=max(4 * n, 64), seed=43, n_pool=n_pool, pool_ratio=0.7)
    A = _learner(golden, **kw)                 # k_actenv
    B = _learner(golden, overlap=False, **kw)  # k_env
    _pad_lists(A)
    _pad_lists(B)
    rng = np.random.RandomState(n * 100 + n_pool)
    for pattern in PATTERNS:
        # the acts first, on the lists the step before left; then the forced nets and the sentinel
        if not A._aA_ready:
            A.act(_lib.PM_ACT_A)
        B.act()
        forced = _forced(pattern, n, nn, rng)
        opp = torch.from_numpy(forced).cuda()
        for L in (A, B):
            L.opp.copy_(opp)
            L.opp_list.fill_(SENTINEL)
            L.opp_cnt.fill_(SENTINEL)
        A.actenv()
        _check(A, forced, nn, ("actenv", pattern))
        A.learn(act_next=True)
        A.apply()
        B.env_step()
        _check(B, forced, nn, ("env_step", pattern))
        B.learn()
        B.apply()
        assert torch.equal(A.opp_list, B.opp_list) and torch.equal(A.opp_cnt, B.opp_cnt), pattern
    assert A.counters()["status"] == 0 and B.counters()["status"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_pool", POOLS)
@pytest.mark.parametrize("n", [ARENAS[0], 257])
def test_rnn_env_lists_match_numpy_grouping(golden, n, n_pool):
    from test_gpu_rnn_selfplay import _learner as _rnn_learner
    nn = n_pool + 1
    L = _rnn_learner(golden, n=n, n_pool=n_pool, seed=43)
    _pad_lists(L)
    rng = np.random.RandomState(n * 100 + n_pool)
    for pattern in PATTERNS:
        forced = _forced(pattern, n, nn, rng)
        L.opp.copy_(torch.from_numpy(forced).cuda())
        L.opp_list.fill_(SENTINEL)
        L.opp_cnt.fill_(SENTINEL)
        L.env_step()
        _check(L, forced, nn, ("rnn env_step", pattern))
