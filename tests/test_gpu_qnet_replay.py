"""K2 (QNet fold / Q / fused two-player act) and K4 (PER sample / update) against the reference's
golden outputs and the oracle, on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sd(g, who):
    return {k[len(who) + 1:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(who + ".") and "q_" not in k}


def _obs(rng, n):
    lo = np.array([0, 0, -0.08, -0.08, 0, 0, -5], np.float32)
    hi = np.array([1, 1, 0.08, 0.08, 1, 1, 5], np.float32)
    return (lo + (hi - lo) * rng.random_sample((n, 7))).astype(np.float32)


def test_qnet_q_matches_reference_golden(golden):
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict, q_values

    g = golden("qnet")
    x = torch.from_numpy(g["obs"]).cuda()
    for who in ("modelB", "modelA"):
        blk = pack_state_dict(_sd(g, who))
        for mode, key in ((_lib.PM_FOLD_EVAL, "q_eval"), (_lib.PM_FOLD_TRAIN, "q_train")):
            q = q_values(fold(blk, mode)[0], x).cpu().numpy()
            np.testing.assert_allclose(q, g[f"{who}.{key}"], rtol=0, atol=2e-5)


def test_qnet_q_matches_oracle_at_scale(orc, golden):
    """65 536 rows: the device's Q equals the float32 restatement of its evaluation order bit for bit
    (oracle.qnet_forward_f32), the folded weights equal torch's mu + sigma*eps float32 fold bit for
    bit, and the float64 forward of the reference's formula stays within 3e-5."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict, q_values

    g = golden("qnet")
    sd = _sd(g, "modelB")
    x = _obs(np.random.RandomState(3), 65536)
    sdn = {k: v.numpy() for k, v in sd.items()}
    for mode, name in ((_lib.PM_FOLD_TRAIN, "train"), (_lib.PM_FOLD_EVAL, "eval")):
        w = fold(pack_state_dict(sd), mode)[0]
        assert np.array_equal(w[:4932].cpu().numpy(), orc.fold_heads_f32(sdn, name)), name
        q = q_values(w, torch.from_numpy(x).cuda()).cpu().numpy()
        q32 = orc.qnet_forward_f32(w.cpu().numpy(), x)
        assert np.array_equal(q.view(np.int32), q32.view(np.int32)), f"{name}: {(q != q32).sum()} Q values differ"
        ref = orc.qnet_forward(orc.qnet_effective(sdn, noisy=name == "train"), x)
        np.testing.assert_allclose(q, ref, rtol=0, atol=3e-5)


def test_fold_fresh_noise_matches_restatement(orc, golden):
    """reset_noise on the device: eps_w = f(out) (x) f(in), eps_b = f(out) with f = sign*sqrt|.|,
    values equal to the Philox restatement; written back into the block's epsilon slots."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict, unpack_state_dict

    g = golden("qnet")
    blk = pack_state_dict(_sd(g, "modelB"))
    out = blk.clone()
    seed, ctr = 77, 5
    w = fold(blk, _lib.PM_FOLD_TRAIN_FRESH, seed=seed, counter=ctr, params_out=out)
    sd = unpack_state_dict(out)
    fVi, fVo, fAi, fAo = orc.philox_noise(seed, orc.TAG_NOISE_ACT, ctr)
    assert np.array_equal(sd["fc_V.weight_epsilon"].numpy(), np.outer(fVo, fVi))  # the draws bit for bit
    assert np.array_equal(sd["fc_A.weight_epsilon"].numpy(), np.outer(fAo, fAi))
    assert np.array_equal(sd["fc_A.bias_epsilon"].numpy(), fAo)
    # effective heads = mu + sigma*eps from the written-back eps
    sd0 = unpack_state_dict(blk)
    wh = w[0, 4672:4672 + 256].cpu().numpy().reshape(4, 64)
    expA = sd0["fc_A.weight_mu"].numpy() + sd0["fc_A.weight_sigma"].numpy() * sd["fc_A.weight_epsilon"].numpy()
    assert np.array_equal(wh[1:], expA.astype(np.float32))
    # the raw draws are N(0,1): recover them over many counters
    raws = []
    for c in range(40):
        fold(blk, _lib.PM_FOLD_TRAIN_FRESH, seed=seed, counter=1000 + c, params_out=out)
        e = unpack_state_dict(out)["fc_V.weight_epsilon"].numpy()[0] / unpack_state_dict(out)["fc_V.bias_epsilon"].numpy()[0]
        raws.append(np.sign(e) * e ** 2)
    r = np.concatenate(raws)
    assert abs(r.mean()) < 0.1 and abs(r.var() - 1) < 0.15


def test_act_both_players(orc, golden):
    """A greedy on its per-arena opponent, B eps-greedy; the eps draws and random actions are
    the Philox restatement's, the greedy ones argmax of the oracle Q (first index on ties)."""
    from pongmi import _lib
    from pongmi.qnet import act, fold, pack_state_dict

    g = golden("qnet")
    sdB, sdA = _sd(g, "modelB"), _sd(g, "modelA")
    n = 50000
    rng = np.random.RandomState(9)
    oA, oB = _obs(rng, n), _obs(rng, n)
    opp = rng.randint(0, 3, n).astype(np.int32)
    w_opp = torch.cat([fold(pack_state_dict(sdA), _lib.PM_FOLD_TRAIN), fold(pack_state_dict(sdB), _lib.PM_FOLD_EVAL),
                       fold(pack_state_dict(sdA), _lib.PM_FOLD_EVAL)])
    w_B = fold(pack_state_dict(sdB), _lib.PM_FOLD_TRAIN)[0]
    effs = [orc.qnet_effective({k: v.numpy() for k, v in s.items()}, noisy=m)
            for s, m in ((sdA, True), (sdB, False), (sdA, False))]
    # the float32 restatement of the device's order: every Q bitwise, so every action exactly
    qa32 = np.zeros((n, 3), np.float32)
    for k in range(3):
        sel = opp == k
        qa32[sel] = orc.qnet_forward_f32(w_opp[k].cpu().numpy(), oA[sel])
    qb32 = orc.qnet_forward_f32(w_B.cpu().numpy(), oB)
    qa_ref = np.zeros((n, 3))
    for k in range(3):
        sel = opp == k
        qa_ref[sel] = orc.qnet_forward(effs[k], oA[sel])
    for eps in (0.0, 0.3, 1.0):
        seed, ctr = 11, 3
        aA, aB, qA, qB = act(w_opp, torch.from_numpy(opp), w_B, torch.from_numpy(oA).cuda(), torch.from_numpy(oB).cuda(),
                             epsilon=eps, seed=seed, counter=ctr, want_q=True)
        aA, aB = aA.cpu().numpy(), aB.cpu().numpy()
        assert np.array_equal(qA.cpu().numpy(), qa32) and np.array_equal(qB.cpu().numpy(), qb32)
        np.testing.assert_allclose(qA.cpu().numpy(), qa_ref, atol=3e-5)  # the reference's formula, float64
        assert np.array_equal(aA, np.argmax(qa32, 1))  # first max on ties, every arena
        r = orc.philox64(np.arange(n), orc.TAG_ACT, np.full(n, ctr, np.uint64), seed)
        explore = orc.u53(r[0], r[1]) < eps
        rnd = orc.below(r[2], 3)
        assert np.array_equal(aB, np.where(explore, rnd, np.argmax(qb32, 1)))
        assert abs(explore.mean() - eps) < 0.01
        if eps == 1.0:
            counts = np.bincount(aB, minlength=3)
            assert np.all(np.abs(counts / n - 1 / 3) < 0.01)


# ------------------------------------------------------------------ K2 at ragged sizes
TAIL = 64  # rows allocated past n and filled with a sentinel: nothing may write them, no result may depend on them
Q_SENTINEL, A_SENTINEL = -12345.0, 77


def _with_tail(a, fill):
    """Host array [n, ...] -> device tensor [n + TAIL, ...], the tail rows filled with `fill`."""
    a = np.ascontiguousarray(a)
    out = np.full((a.shape[0] + TAIL,) + a.shape[1:], fill, a.dtype)
    out[:a.shape[0]] = a
    return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1000])
def test_qnet_q_ragged_n(orc, golden, n):
    """pm_qnet_q below, at and beside the 32-row tile and the 256-row block: q[:n] equals the float32
    restatement bit for bit, rows past n are neither written nor read."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict

    lib = _lib.load()
    w = fold(pack_state_dict(_sd(golden("qnet"), "modelB")), _lib.PM_FOLD_TRAIN)[0].contiguous()
    x = _obs(np.random.RandomState(100 + n), n)
    ref = orc.qnet_forward_f32(w.cpu().numpy(), x) if n else np.zeros((0, 3), np.float32)
    for tail in (0.5, 1e30, np.nan):
        xd = _with_tail(x, np.float32(tail))
        q = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
        _lib.check(lib.pm_qnet_q(_lib.ptr(w), _lib.ptr(xd), _lib.ptr(q), n, _lib.stream_ptr()), "pm_qnet_q")
        q = q.cpu().numpy()
        assert np.array_equal(q[:n].view(np.int32), ref.view(np.int32)), f"{(q[:n] != ref).sum()} Q values differ"
        assert np.all(q[n:] == Q_SENTINEL)


def _act_raw(w_opp, opp, n_opp, w_B, oA, oB, n, eps=0.0, seed=0, counter=0, eps_dev=None, counter_dev=None,
             chunk0=0, chunk1=0):
    """pm_qnet_act through the C ABI on buffers TAIL rows longer than n: observations with NaN tails,
    outputs with sentinel tails (checked here). Returns host aA, aB, qA, qB of the n rows."""
    from pongmi import _lib

    lib = _lib.load()
    oAd, oBd = _with_tail(oA, np.float32(np.nan)), _with_tail(oB, np.float32(np.nan))
    oppd = _with_tail(opp.astype(np.int32), np.int32(1)) if opp is not None else None
    aA = torch.full((n + TAIL,), A_SENTINEL, dtype=torch.int8, device="cuda")
    aB = torch.full((n + TAIL,), A_SENTINEL, dtype=torch.int8, device="cuda")
    qA = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
    qB = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
    p = _lib.ptr
    _lib.check(lib.pm_qnet_act(p(w_opp), p(oppd), n_opp, p(w_B), p(oAd), p(oBd), float(eps), p(eps_dev), int(seed),
                               int(counter), p(counter_dev), p(aA), p(aB), p(qA), p(qB), n, int(chunk0), int(chunk1),
                               _lib.stream_ptr()), "pm_qnet_act")
    out = [t.cpu().numpy() for t in (aA, aB, qA, qB)]
    assert np.all(out[0][n:] == A_SENTINEL) and np.all(out[1][n:] == A_SENTINEL)
    assert np.all(out[2][n:] == Q_SENTINEL) and np.all(out[3][n:] == Q_SENTINEL)
    return [o[:n] for o in out]


def _many_nets(golden, count, seed):
    """`count` distinct nets: modelA's block with perturbed parameters, eval-folded -> [count, NW]."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict

    base = pack_state_dict(_sd(golden("qnet"), "modelA"), "cpu")
    gen = torch.Generator().manual_seed(seed)
    blocks = base[None, :] + 0.05 * torch.randn((count, base.numel()), generator=gen)
    return fold(blocks.cuda().contiguous(), _lib.PM_FOLD_EVAL).contiguous()


ACT_CASES = [(cfg, n) for n in (1, 33, 257, 1000, 5000) for cfg in ("none", "zero", "skip2")] + [("many", 257)]


@pytest.mark.parametrize("cfg,n", ACT_CASES)
def test_act_ragged_sizes_nets_and_chunks(orc, golden, cfg, n):
    """pm_qnet_act at ragged n, for opp_id NULL / all net 0 / a net that owns no row / 70 nets with
    a few rows each, under four chunkings (a chunk below a tile row count, unaligned chunks, one
    chunk for everything) and eps 0 / 0.3: actions and Q of both players equal the float32 restatement
    and the Philox draw bit for bit, hence are equal across chunkings; nothing is written past n."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict

    rng = np.random.RandomState(1000 + n)
    oA, oB = _obs(rng, n), _obs(rng, n)
    n_opp = {"none": 3, "zero": 3, "skip2": 5, "many": 70}[cfg]
    w_opp = _many_nets(golden, n_opp, seed=n_opp)
    w_B = fold(pack_state_dict(_sd(golden("qnet"), "modelB")), _lib.PM_FOLD_TRAIN)[0].contiguous()
    if cfg == "none":
        opp, net = None, np.zeros(n, np.int64)
    elif cfg == "zero":
        opp = net = np.zeros(n, np.int64)
    elif cfg == "skip2":
        opp = net = np.array([0, 1, 3, 4])[rng.randint(0, 4, n)]
    else:
        opp = net = np.where(rng.random_sample(n) < 0.3, 0, rng.randint(0, n_opp, n))  # net 0 owns ~a third
        assert (np.bincount(net, minlength=n_opp) < 4).sum() > n_opp // 2  # most nets own fewer than four rows
    qa32 = np.zeros((n, 3), np.float32)
    w_host = w_opp.cpu().numpy()
    for k in np.unique(net):
        qa32[net == k] = orc.qnet_forward_f32(w_host[k], oA[net == k])
    qb32 = orc.qnet_forward_f32(w_B.cpu().numpy(), oB)
    seed, ctr = 11, 3
    r = orc.philox64(np.arange(n), orc.TAG_ACT, np.full(n, ctr, np.uint64), seed)
    for eps in (0.0, 0.3):
        expB = np.where(orc.u53(r[0], r[1]) < eps, orc.below(r[2], 3), np.argmax(qb32, 1))
        first = None
        for chunk0, chunk1 in ((0, 0), (64, 64), (100, 300), (4096, 4096)):
            got = _act_raw(w_opp, opp, n_opp, w_B, oA, oB, n, eps=eps, seed=seed, counter=ctr, chunk0=chunk0,
                           chunk1=chunk1)
            where = (cfg, n, eps, chunk0, chunk1)
            assert np.array_equal(got[2].view(np.int32), qa32.view(np.int32)), where
            assert np.array_equal(got[3].view(np.int32), qb32.view(np.int32)), where
            assert np.array_equal(got[0], np.argmax(qa32, 1)), where
            assert np.array_equal(got[1], expB), where
            if first is None:
                first = got
            for a, b in zip(first, got):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), where


def test_act_device_side_epsilon_and_counter(golden):
    """*eps_dev replaces epsilon, *counter_dev is added to counter: the same actions as the same
    values passed as host arguments."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict

    n = 1000
    rng = np.random.RandomState(5)
    oA, oB = _obs(rng, n), _obs(rng, n)
    opp = rng.randint(0, 3, n)
    w_opp = _many_nets(golden, 3, seed=3)
    w_B = fold(pack_state_dict(_sd(golden("qnet"), "modelB")), _lib.PM_FOLD_TRAIN)[0].contiguous()
    eps_dev = torch.tensor([0.3], dtype=torch.float64, device="cuda")
    ctr_dev = torch.tensor([41], dtype=torch.int64, device="cuda")
    host = _act_raw(w_opp, opp, 3, w_B, oA, oB, n, eps=0.3, seed=9, counter=48)
    other = _act_raw(w_opp, opp, 3, w_B, oA, oB, n, eps=0.3, seed=9, counter=7)
    assert not np.array_equal(host[1], other[1])  # the counter matters
    assert not np.array_equal(host[1], _act_raw(w_opp, opp, 3, w_B, oA, oB, n, eps=0.0, seed=9, counter=48)[1])
    for kw in (dict(eps=0.9, eps_dev=eps_dev, counter=48),                    # eps_dev wins over epsilon
               dict(eps=0.3, counter=0, counter_dev=ctr_dev + 7),             # the counter from the device alone
               dict(eps=0.9, eps_dev=eps_dev, counter=7, counter_dev=ctr_dev)):  # counter + *counter_dev
        got = _act_raw(w_opp, opp, 3, w_B, oA, oB, n, seed=9, **kw)
        for a, b in zip(host, got):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), sorted(kw)


def test_act_exact_ties_take_first_index(orc, golden):
    """Exact ties (random weights never produce one): a net whose advantage rows 1 and 2 are
    identical, and one with all three identical (eval fold, sigma 0). The restatement's Q ties on
    every row, and both players' greedy action is the first maximal index, in every lane group of a
    tile (n = 100: three full tiles and a ragged one)."""
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict

    n = 100
    rng = np.random.RandomState(17)
    oA, oB = _obs(rng, n), _obs(rng, n)

    def tied(rows):
        sd = {k: v.clone() for k, v in _sd(golden("qnet"), "modelB").items()}
        for k in ("fc_A.weight_mu", "fc_A.bias_mu"):
            for r in rows[1:]:
                sd[k][r] = sd[k][rows[0]]
        for k in ("fc_A.weight_sigma", "fc_A.bias_sigma", "fc_V.weight_sigma", "fc_V.bias_sigma"):
            sd[k] = torch.zeros_like(sd[k])
        return fold(pack_state_dict(sd), _lib.PM_FOLD_EVAL)[0].contiguous()

    for rows in ((1, 2), (0, 1, 2)):
        w = tied(rows)
        for obs in (oA, oB):
            q = orc.qnet_forward_f32(w.cpu().numpy(), obs)
            assert all(np.array_equal(q[:, rows[0]], q[:, r]) for r in rows[1:])  # exact ties on every row
        aA, aB, qA, qB = _act_raw(w, None, 1, w, oA, oB, n, eps=0.0)
        for a, q, obs in ((aA, qA, oA), (aB, qB, oB)):
            ref = orc.qnet_forward_f32(w.cpu().numpy(), obs)
            assert np.array_equal(q.view(np.int32), ref.view(np.int32))
            exp = np.argmax(ref, 1)  # numpy: the first maximal index
            assert np.array_equal(a, exp)
            assert not np.any(a == rows[-1])  # a tied later index never wins
            print(f"tied rows {rows}: action counts {np.bincount(a, minlength=3)}")
            if len(rows) == 3:
                assert np.all(a == 0)


def test_per_matches_reference_golden(golden):
    from pongmi.replay import per_sample, per_update

    g = golden("per")
    for ph in range(int(g["n_phases"])):
        u = 0
        while f"p{ph}.u{u}.idxs" in g:
            k = f"p{ph}.u{u}."
            prios = torch.from_numpy(g[k + "prios_before"].copy()).cuda()
            idx, w = per_sample(prios, int(g[k + "size"]), 64, float(g[k + "beta"]), uniforms=g[k + "uniforms"])
            assert np.array_equal(idx.cpu().numpy(), g[k + "idxs"])
            np.testing.assert_allclose(w.cpu().numpy(), g[k + "weights"], rtol=2e-5)
            per_update(prios, torch.from_numpy(g[k + "upd_idx"]), torch.from_numpy(g[k + "upd_err"]))
            assert np.array_equal(prios.cpu().numpy(), g[k + "prios_after"])
            u += 1


@pytest.mark.parametrize("size", [1, 1023, 1025, 700_000, 1_000_000])
def test_per_sample_matches_oracle_at_scale(orc, size):
    from pongmi.replay import per_sample

    cap = 1_000_000
    rng = np.random.RandomState(size)
    pr = rng.uniform(0, 3, cap).astype(np.float32)
    pr[rng.rand(cap) < 0.1] = 0.0  # unfilled / zero-priority entries are never drawn
    if size == 1:
        pr[0] = 0.5
    u = rng.random_sample(256)
    idx, w = per_sample(torch.from_numpy(pr).cuda(), size, 256, 0.55, uniforms=u)
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    # the device's descent restated in its own summation order: every index and weight exactly
    tidx, tw = orc.per_sample_tree(pr, size, size, 0.55, u)
    assert np.array_equal(idx, tidx)
    np.testing.assert_allclose(w, tw / tw.max(), rtol=5e-7)  # the device normalises by its own float32 max
    # np.random.choice's own algorithm (float32-normalised CDF): identical on every draw outside the
    # rounding band of a CDF boundary (oracle.per_boundary_band); the band's size is reported
    ref_idx, ref_w = orc.per_sample(pr, size, 256, 0.55, u)
    band = orc.per_boundary_band(pr, size, u)
    assert np.array_equal(idx[~band], ref_idx[~band])
    print(f"size {size}: {band.sum()} of 256 draws in the boundary band, {(idx != ref_idx).sum()} differ there")
    assert np.all(pr[idx] > 0) and np.all(idx < size)
    np.testing.assert_allclose(w, ref_w, rtol=2e-5)


def test_per_philox_sampling_distribution():
    """Production uniforms: sampled frequencies follow p_i^alpha (chi-square)."""
    from pongmi.replay import per_sample

    pr = torch.tensor([0.0, 1.0, 2.0, 0.5, 4.0, 0.0, 1e-6, 3.0], device="cuda")
    counts = np.zeros(8)
    for c in range(400):
        idx, _ = per_sample(pr, 8, 256, 0.4, counter=c, seed=99)
        counts += np.bincount(idx.cpu().numpy(), minlength=8)
    p = pr.cpu().numpy().astype(np.float64) ** 0.6
    p /= p.sum()
    exp = p * counts.sum()
    assert counts[0] == 0 and counts[5] == 0
    m = exp > 5
    chi2 = ((counts[m] - exp[m]) ** 2 / exp[m]).sum()
    assert chi2 < 30, (counts, exp)
