"""K4's stand-alone entry points (pm_per_sample / pm_per_update / pm_per_build) at every shape they
branch on: batch sizes around the 64-sample sampler block and the 1024-thread normalise stride, buffer
sizes around a 64-entry node and a 1024-entry chunk, other alpha / beta, uniforms at 0 and 1 - 2^-53
and on runs of zero priorities, more than one 1024-chunk prefix round, duplicate updates across
256-thread blocks, and the tree pm_per_build leaves in its workspace. Indices, priorities and tree
nodes are compared bit for bit with the oracle's restatement of the device's summation order; the
sampler is tied to np.random.choice's own algorithm outside the CDF rounding band."""
import numpy as np
import pytest
import torch

from oracle.oracle import bits_equal

pytestmark = pytest.mark.gpu

U_LAST = 1.0 - 2.0 ** -53  # the largest uniform random_sample() returns
PM_E_ARG, PM_E_SIZE = -1, -2  # include/pongmi.h


def random_prios(rng, size):
    pr = rng.uniform(0, 3, size).astype(np.float32)
    pr[rng.rand(size) < 0.1] = 0.0  # zero-priority entries are never drawn
    pr[0] = 0.5
    return pr


def check_sample(orc, pr, size, bs, alpha, beta, u, choice=True):
    """One pm_per_sample call against the restatement (indices exact, weights at the tolerances of
    test_per_sample_matches_oracle_at_scale) and, with `choice`, np.random.choice's algorithm outside
    the boundary band. Returns the indices."""
    from pongmi.replay import per_sample

    assert len(u) == bs
    idx, w = per_sample(torch.from_numpy(pr).cuda(), size, bs, beta, alpha=alpha, uniforms=u)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    b32 = float(np.float32(beta))  # the ABI takes beta as a float
    tidx, tw = orc.per_sample_tree(pr, size, size, b32, u, alpha=alpha)
    assert np.array_equal(idx, tidx), f"{(idx != tidx).sum()} of {bs} indices differ"
    assert np.all(idx >= 0) and np.all(idx < size) and np.all(pr[idx] > 0)
    np.testing.assert_allclose(w, tw / tw.max(), rtol=5e-7)  # the device normalises by its own float32 max
    if beta == 0:
        assert np.all(w == 1.0)
    if choice:
        ref_idx, ref_w = orc.per_sample(pr, size, bs, b32, u, alpha=alpha)
        band = orc.per_boundary_band(pr, size, u, alpha=alpha)
        assert np.array_equal(idx[~band], ref_idx[~band])
        if not band.any():
            np.testing.assert_allclose(w, ref_w, rtol=2e-5)
    return idx


# ------------------------------------------------------------------ sampler shapes
SHAPES = [(5000, bs) for bs in (1, 63, 64, 65, 255, 257, 1025, 2049)] + \
         [(size, 256) for size in (63, 64, 65, 1024, 1025, 16_384, 65_537)]


@pytest.mark.parametrize("alpha,beta", [(0.6, 0.4), (1.0, 1.0), (0.3, 0.0)])
@pytest.mark.parametrize("size,bs", SHAPES)
def test_per_sample_shapes(orc, size, bs, alpha, beta):
    """Batch sizes below, at and beside the 64-sample block and past the 1024-thread stride of the
    normalise kernel; sizes beside a 64-entry node, a 1024-entry chunk and 64 chunks; alpha 1 and beta 1,
    and beta 0 (weights exactly 1)."""
    rng = np.random.RandomState(size * 7 + bs)
    check_sample(orc, random_prios(rng, size), size, bs, alpha, beta, rng.random_sample(bs))


# ------------------------------------------------------------------ edge uniforms
def _layout(kind, size, rng):
    if kind == "last_leaf":  # all mass in one leaf at the far end
        pr = np.zeros(size, np.float32)
        pr[size - 1] = 2.5
    elif kind == "head_zero":  # the first 70 % zero
        pr = rng.uniform(0.1, 3, size).astype(np.float32)
        pr[:int(0.7 * size)] = 0.0
    elif kind == "tail_zero":  # the last 70 % zero
        pr = rng.uniform(0.1, 3, size).astype(np.float32)
        pr[int(0.3 * size):] = 0.0
    else:  # all equal: every CDF boundary is j / size
        pr = np.full(size, 0.75, np.float32)
    return pr


@pytest.mark.parametrize("kind", ["last_leaf", "head_zero", "tail_zero", "equal"])
@pytest.mark.parametrize("size", [1000, 5000, 65_537])
def test_per_sample_edge_uniforms(orc, size, kind):
    """u = 0, u = 1 - 2^-53 and its neighbours (u * total lands an ulp below the total, in front of
    which only zero priorities may be left), the exact CDF boundaries j / size, and random ones, over
    layouts with long zero runs. Every draw has a positive priority, lies below size and equals the
    restatement. (With priorities of ordinary range the plain search settles all of these; the
    fallback itself is forced in test_per_sample_last_nonzero_child_decides.)"""
    rng = np.random.RandomState(size + len(kind))
    pr = _layout(kind, size, rng)
    edge = [0.0, 2.0 ** -53, 2.0 ** -1074, 0.3, 0.5, U_LAST, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -51, 1.0 - 2.0 ** -40]
    bounds = np.arange(0, 64) / 64.0 if kind != "equal" else rng.randint(0, size, 64) / size
    u = np.concatenate([edge, bounds, np.nextafter(bounds, 2.0), rng.random_sample(256 - len(edge) - 128)])
    assert len(u) == 256 and u.max() < 1.0
    idx = check_sample(orc, pr, size, 256, 0.6, 0.4, u)
    nz = np.nonzero(pr)[0]
    assert idx[0] == nz[0] and idx[5] == nz[-1]  # u = 0 takes the first entry with mass, the last u the last


def test_per_sample_last_nonzero_child_decides(orc):
    """Layouts built so that u * total lands past every running sum of a node's children, on a run of
    trailing zeros, and the "last nonzero child" fallback decides the draw (alpha = 1, so a leaf is
    its priority, and 2^53 absorbs a 1 added to it).
    One node of 64 leaves: its sum takes the quarter 1 + 1 = 2 whole (2^53 + 2), the search's running
    sum adds the ones one by one and stays at 2^53 = u * total for u = 1 - 2^-53: no child exceeds
    it, and leaf 49, the last with mass, is taken.
    One chunk of 16 nodes: the chunk sum runs 1 + 1 + 2^53 + 2 = 2^53 + 4, the search starts the third
    lane at (1) + (1 + 2^53) = 2^53 and reaches 2^53 + 2 = u * total: node 8, the last with mass, is
    taken by the fallback, and inside it leaf 517 by the fallback again.
    The restatement reports which levels' fallback settled a draw (1 the leaves, 2 the nodes); the other
    uniforms take the plain path."""
    big = np.float32(2.0 ** 53)
    u = np.array([U_LAST, 0.5, 0.0, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -50, 0.25, 0.75, 2.0 ** -60])
    leaves = np.zeros(64, np.float32)
    leaves[[0, 48, 49]] = big, 1, 1
    nodes = np.zeros(1024, np.float32)
    nodes[[0, 256, 320, 517]] = 1, 1, big, 2
    for pr, last, plain, levels in ((leaves, 49, 0, 1), (nodes, 517, 320, 3)):
        size = len(pr)
        idx = check_sample(orc, pr, size, len(u), 1.0, 0.4, u)
        fell = orc.per_sample_tree(pr, size, size, 0.4, u, alpha=1.0, want_fallback=True)[2]
        assert fell.tolist() == [levels, 0, 0, levels, 0, 0, 0, 0]
        assert np.all(idx[fell > 0] == last) and np.all(idx[[1, 4, 5, 6]] == plain) and np.all(pr[idx] > 0)
        assert np.all(pr[last + 1:] == 0)  # the draw landed on the zeros behind it


# ------------------------------------------------------------------ more than one prefix round
ROUND_ENTRIES = 1024 * 1024  # entries whose chunk sums fill one prefix round (PER_ROUND chunks of PER_CHUNK)
ROUND_CASES = [(ROUND_ENTRIES, "random"), (ROUND_ENTRIES + 1, "random"), (ROUND_ENTRIES + 1, "round0_zero"),
               (ROUND_ENTRIES + 1, "later_zero"), (2 * ROUND_ENTRIES + 1, "random"),
               (2 * ROUND_ENTRIES + 1, "round0_zero"), (2 * ROUND_ENTRIES + 1, "later_zero")]


@pytest.mark.parametrize("size,kind", ROUND_CASES)
def test_per_sample_prefix_rounds(orc, size, kind):
    """1024 chunks (the last single-round size), 1025 (a second round of one chunk holding one entry)
    and 2049 (three rounds): per_sample_block's separate total pass and its per-round search with the
    carried running total. Random priorities with 10 % zeros; the same with round 0 all zero (the
    search has to skip a round without mass); and with every round after the first all zero. 256 draws,
    u = 0 and 1 - 2^-53 among them, indices exact. With priorities of this range every draw has a hit
    in some round; the chunk-level fallback and its carry across rounds are forced in
    test_per_sample_chunk_fallback_decides."""
    rng = np.random.RandomState(size % 100_003)
    pr = random_prios(rng, size)
    if kind == "round0_zero":
        pr[:ROUND_ENTRIES] = 0.0
        pr[size - 1] = 0.25  # the one-entry last round keeps mass
    elif kind == "later_zero":
        pr[ROUND_ENTRIES:] = 0.0
    u = np.concatenate([[0.0, U_LAST, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -30, 0.5, 2.0 ** -60], rng.random_sample(250)])
    idx = check_sample(orc, pr, size, 256, 0.6, 0.4, u)
    nz = np.nonzero(pr)[0]
    assert idx[0] == nz[0] and idx[1] == nz[-1]
    if kind == "round0_zero":
        assert idx.min() >= ROUND_ENTRIES
    elif kind == "later_zero":
        assert idx.max() < ROUND_ENTRIES
    elif size > ROUND_ENTRIES + 1:
        assert idx.min() < ROUND_ENTRIES <= idx.max()  # draws from more than one round


CH = 1024  # entries per chunk
BIG = 2.0 ** 53
# name: (size, {entry: priority}, the entry u = 1 - 2^-53 draws, the levels whose fallback settles it)
CHUNK_FALLBACK = {
    # one round of 773 chunks. Chunk 0 holds 2^53; the ones in chunks 768 and 772 (two threads of the
    # block's last wave) are absorbed when the prefix adds them one by one, but the round's end value
    # takes the wave's 1 + 1 = 2 whole: total 2^53 + 2, u * total = 2^53, every prefix entry is 2^53.
    # No entry exceeds it, and the first to reach the end value is chunk 0.
    "one_round": (773 * CH, {5: BIG, 768 * CH + 3: 1, 772 * CH + 9: 1}, 5, 7),
    # three rounds, the same in round 0 (chunks 1019 and 1023), nothing behind it: rounds 1 and 2 have
    # no mass, and the `lastnz` / `lastbef` carried out of round 0 are taken after the last round.
    "carried": (2 * CH * CH + 1, {0: BIG, 1019 * CH: 1, 1023 * CH: 1}, 0, 7),
    # two rounds; round 1 holds 0.75, which the running total 2^53 + 2 absorbs even in the end value:
    # a round whose end does not exceed its start is skipped, and round 0's fallback stays.
    "absorbed_round": (CH * CH + 1, {7: BIG, 1019 * CH + 1: 1, 1023 * CH + 2: 1, 1024 * CH: 0.75}, 7, 7),
    # round 1 has mass the end value sees (0.25 + 0.75 + 0.75 on top of 2^53 + 2 gives 2^53 + 4;
    # u * total = 2^53 + 2) and no prefix entry shows (each stays at 2^53 + 2): its fallback, chunk 1024
    # with `lastbef` = the running total, replaces the one carried out of round 0. Inside the chunk the
    # remainder is 0 and the plain search takes the entry with mass.
    "replaced": (2 * CH * CH + 1, {7: BIG, 1019 * CH + 1: 1, 1023 * CH + 2: 1, 1024 * CH + 70: 0.25,
                                   2043 * CH: 0.75, 2047 * CH + 3: 0.75}, 1024 * CH + 70, 4),
}


@pytest.mark.parametrize("name", list(CHUNK_FALLBACK))
def test_per_sample_chunk_fallback_decides(orc, name):
    """The chunk-level fallback of per_sample_block (no prefix entry of any round exceeds u * total:
    the last round with mass gives its "first chunk to reach the round's end value") and its
    `lastnz` / `lastbef` carry across rounds, forced with alpha = 1 and a 2^53 leaf that absorbs what
    is added to it piecewise (see CHUNK_FALLBACK). The restatement says which level's fallback
    settled each draw; indices are exact, every draw has a positive priority, and the uniforms away
    from 1 take the plain path to the 2^53 leaf."""
    size, entries, last, levels = CHUNK_FALLBACK[name]
    pr = np.zeros(size, np.float32)
    for e, v in entries.items():
        pr[e] = v
    u = np.array([U_LAST, 0.5, 0.0, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -50, 0.25, 0.75, 2.0 ** -60])
    idx = check_sample(orc, pr, size, len(u), 1.0, 0.4, u)
    fell = orc.per_sample_tree(pr, size, size, 0.4, u, alpha=1.0, want_fallback=True)[2]
    assert fell.tolist() == [levels, 0, 0, levels, 0, 0, 0, 0]
    assert np.all(fell[[0, 3]] & 4)  # the chunk level's fallback decided
    big = int(np.argmax(pr))
    assert idx.tolist() == [last, big, big, last, big, big, big, big]


# ------------------------------------------------------------------ pm_per_update
@pytest.mark.parametrize("pattern", ["distinct", "equal", "far_duplicates", "adjacent_duplicates"])
@pytest.mark.parametrize("bs", [1, 64, 256, 257, 1000])
def test_per_update_duplicates_and_blocks(orc, bs, pattern):
    """prios[idx[j]] = |err[j]| + 1e-6 in sequential order (the last duplicate wins) against
    oracle.per_update: all indices distinct, all equal, and duplicates whose first and last
    occurrence sit in different 256-thread blocks (bs > 256) or far apart in one, and duplicates
    right next to each other. Negative and zero errors included; every untouched priority keeps its
    bits."""
    from pongmi.replay import per_update

    cap = 4096
    rng = np.random.RandomState(10 * bs + len(pattern))
    pr = rng.uniform(0, 3, cap).astype(np.float32)
    if pattern == "distinct":
        idx = rng.permutation(cap)[:bs]
    elif pattern == "equal":
        idx = np.full(bs, 1234)
    elif pattern == "far_duplicates":
        idx = rng.permutation(cap)[:bs]
        k = min(max(bs // 8, 1), bs - 256) if bs > 256 else max(bs // 8, 1)
        idx[bs - k:] = idx[:k]  # the last k repeat the first k: in the last block and the first for bs > 256
        if bs > 256:
            assert bs - k >= 256 and k <= 256
    else:  # pairs next to each other, the pairs at 63 | 64 and 255 | 256 across a wave and a block
        idx = rng.permutation(cap)[:bs]
        idx[2:bs:2] = idx[1:bs - 1:2]
    err = rng.uniform(-2, 2, bs).astype(np.float32)
    err[::5] = 0.0
    err[-1] = -1.5 if bs > 1 else 0.0
    exp = pr.copy()
    orc.per_update(exp, idx, err)
    dev = torch.from_numpy(pr.copy()).cuda()
    per_update(dev, torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(err))
    got = dev.cpu().numpy()
    assert bits_equal(got, exp), f"{(got != exp).sum()} priorities differ"
    untouched = np.ones(cap, bool)
    untouched[idx] = False
    assert bits_equal(got[untouched], pr[untouched]) and untouched.sum() >= cap - bs
    assert np.all(got[idx] > 0)
    if pattern == "distinct":
        assert np.all(got[idx[err == 0]] == np.float32(1e-6)) and (err == 0).any()
    if pattern != "distinct" and bs > 1:  # the winner is the last occurrence, not the first
        assert got[idx[-1]] == np.float32(abs(err[-1])) + np.float32(1e-6)


# ------------------------------------------------------------------ pm_per_build
def _work(cap):
    from pongmi import _lib

    return torch.zeros(int(_lib.load().pm_per_work_bytes(cap)) + 64, dtype=torch.uint8, device="cuda")


def _build(prios_dev, cap, alpha, work):
    from pongmi import _lib

    return _lib.load().pm_per_build(_lib.ptr(prios_dev), cap, alpha, _lib.ptr(work), _lib.stream_ptr())


def _read_tree(work, cap):
    """chunk, sub, leaf out of a tree workspace (csrc/pm_per.h per_tree: chunk sums, level-1 sums and
    leaves, each section padded to 256 bytes)."""
    pad = lambda n: ((n * 8 + 255) // 256) * 256  # noqa: E731
    nsub, nch = -(-cap // 64), -(-cap // 1024)
    raw = work.cpu().numpy()
    chunk = raw[:8 * nch].view(np.float64)
    sub = raw[pad(nch):pad(nch) + 8 * nsub].view(np.float64)
    leaf = raw[pad(nch) + pad(nsub):pad(nch) + pad(nsub) + 4 * cap].view(np.float32)
    return chunk, sub, leaf


@pytest.mark.parametrize("alpha", [0.6, 1.0])
@pytest.mark.parametrize("cap", [1, 63, 65, 1023, 1025, 100_000])
def test_per_build_tree_bit_exact(orc, cap, alpha):
    """pm_per_build's leaves, level-1 and level-2 nodes read back from the workspace equal
    oracle.per_tree bit for bit, with zero, negative and NaN priorities (zero leaves) in the array; a
    rebuild after pm_per_update equals a build of a fresh copy."""
    from pongmi import _lib
    from pongmi.replay import per_update

    rng = np.random.RandomState(cap)
    pr = rng.uniform(0, 3, cap).astype(np.float32)
    kind = rng.randint(0, 12, cap)
    pr[kind == 0] = 0.0
    pr[kind == 1] = -rng.uniform(0.1, 2, cap).astype(np.float32)[kind == 1]
    pr[kind == 2] = np.nan
    if cap >= 63:
        assert (kind == 0).any() and (kind == 1).any() and (kind == 2).any()
    dev = torch.from_numpy(pr.copy()).cuda()
    work = _work(cap)
    _lib.check(_build(dev, cap, alpha, work), "pm_per_build")

    def same_tree(work, prios):
        chunk, sub, leaf = _read_tree(work, cap)
        echunk, esub, eleaf = orc.per_tree(prios, cap, alpha)
        assert bits_equal(leaf, eleaf), f"{(leaf != eleaf).sum()} leaves differ"
        assert bits_equal(sub, esub) and bits_equal(chunk, echunk)
        assert np.all(leaf[~(prios > 0)] == 0)  # zero, negative and NaN priorities: a zero leaf

    same_tree(work, pr)
    bs = min(cap, 300)
    idx = rng.randint(0, cap, bs)
    err = rng.uniform(-2, 2, bs).astype(np.float32)
    per_update(dev, torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(err))
    upd = pr.copy()
    orc.per_update(upd, idx, err)
    assert bits_equal(dev.cpu().numpy(), upd)
    _lib.check(_build(dev, cap, alpha, work), "pm_per_build")
    fresh = _work(cap)
    _lib.check(_build(torch.from_numpy(upd.copy()).cuda(), cap, alpha, fresh), "pm_per_build")
    for a, b in zip(_read_tree(work, cap), _read_tree(fresh, cap)):
        assert bits_equal(a, b)
    same_tree(work, upd)


def test_per_build_bad_arguments():
    """A workspace that is not 16-byte aligned is PM_E_ARG and cap <= 0 is PM_E_SIZE, for pm_per_build;
    the same workspace rule holds for pm_per_sample. Nothing is launched."""
    from pongmi import _lib

    lib = _lib.load()
    pr = torch.ones(128, dtype=torch.float32, device="cuda")
    work = _work(128)
    assert work.data_ptr() % 16 == 0
    assert _build(pr, 128, 0.6, work[8:]) == PM_E_ARG
    assert _build(pr, 0, 0.6, work) == PM_E_SIZE and _build(pr, -5, 0.6, work) == PM_E_SIZE
    assert lib.pm_per_build(None, 128, 0.6, _lib.ptr(work), _lib.stream_ptr()) == PM_E_ARG
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    w = torch.zeros(4, dtype=torch.float32, device="cuda")
    rc = lib.pm_per_sample(_lib.ptr(pr), 128, 0.6, 0.4, None, 0, 0, _lib.ptr(idx), _lib.ptr(w), 4, _lib.ptr(work[8:]),
                           _lib.stream_ptr())
    assert rc == PM_E_ARG
    with pytest.raises(_lib.PongmiError):
        _lib.check(rc, "pm_per_sample")
    assert _build(pr, 128, 0.6, work) == 0  # and the aligned call goes through
    torch.cuda.synchronize()
