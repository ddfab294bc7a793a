"""K5 — QNetRNN on the matrix cores (pm_rnn_fold / pm_rnn_q / pm_rnn_act) against the reference's
own outputs (tests/golden/rnn.npz, produced by models/qnet_rnn.py on checkpoints_rnn/rnn_pong_soul_3.pth)
and the float64 oracle (oracle.rnn_forward).

Tolerance: the kernel computes in fp32 (exact-f32 MFMA, a different summation order than torch's
CPU GEMMs); Q / h / c agree with the reference to rtol 1e-4, atol 1e-5 (|values| <= ~5) over one
step, the 8-step sequence and the 12-step carried roll-out. Integer actions: identical to the
argmax (first max) of the same kernel's Q values; the two entry points (pm_rnn_q, pm_rnn_act)
are bit-identical on the same rows.

Every size the ABI accepts (the second half of this file, through the C ABI on buffers with
sentinel tails): pm_rnn_q at n = 0, 1, 31 ... 300 and pm_rnn_act at n = 1 ... 1000 with no opponent
ids, one net, a net that owns no arena, a net that owns exactly one or two 128-row groups, 64 nets
and 65 nets (the lists dropped), under four chunkings, the packed per-256-arena lists and the
compaction, eps 0 / 0.3 and reset rows — each against the float64 oracle (rtol 1e-4, atol 5e-5,
actions outside the oracle's tie band exact, the epsilon branch exact) and bit for bit against
pm_rnn_q on the same rows padded to whole 128-row groups; nothing is written past n. Device-side
epsilon / counter, exact ties (first index), the argument errors, and pm_rnn_fold's fresh noise
for every net of a count = 3 fold against the Philox restatement.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5


def _sd(g):
    return {k[7:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("params.")}


def _w(g, mode):
    from pongmi import _lib, rnn
    m = _lib.PM_FOLD_TRAIN if mode == "train" else _lib.PM_FOLD_EVAL
    return rnn.fold(rnn.pack_state_dict(_sd(g)), m)[0]


def _close(a, b, what):
    np.testing.assert_allclose(a.detach().cpu().numpy() if torch.is_tensor(a) else a, b, rtol=RTOL, atol=ATOL,
                               err_msg=what)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_rnn_step_matches_reference(golden, mode):
    from pongmi import rnn
    g = golden("rnn")
    w = _w(g, mode)
    h = torch.from_numpy(g["act_h0"][0]).cuda().contiguous()
    c = torch.from_numpy(g["act_c0"][0]).cuda().contiguous()
    q = rnn.q_step(w, torch.from_numpy(g["act_x"][:, 0]).cuda(), h, c)
    _close(q, g[f"act_q_{mode}"], "q")
    _close(h, g[f"act_h1_{mode}"][0], "h")
    _close(c, g[f"act_c1_{mode}"][0], "c")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_rnn_sequence_matches_reference(golden, mode):
    from pongmi import rnn
    g = golden("rnn")
    q, h, c = rnn.forward(_w(g, mode), torch.from_numpy(g["seq_x"]).cuda())
    _close(q, g[f"seq_q_{mode}"], "q")
    _close(h, g[f"seq_h_{mode}"][0], "h")
    _close(c, g[f"seq_c_{mode}"][0], "c")


def test_rnn_rollout_matches_reference(golden):
    """12 acting steps with the state carried (select_action_for_model, train_rnn_iterative.py:371-389)."""
    from pongmi import rnn
    g = golden("rnn")
    w = _w(g, "train")
    h, c = rnn.init_state(16)
    for t in range(12):
        q = rnn.q_step(w, torch.from_numpy(g["roll_x"][t]).cuda(), h, c)
        _close(q, g["roll_q"][t], f"q at step {t}")
    _close(h, g["roll_h"][0], "h")
    _close(c, g["roll_c"][0], "c")


def test_dropin_module_matches_reference(golden):
    """models.qnet_rnn.QNetRNN on the device (HIP path) and with autograd (torch path)."""
    from models.qnet_rnn import QNetRNN
    g = golden("rnn")
    net = QNetRNN(7, 3).cuda()
    net.load_state_dict(_sd(g))
    x = torch.from_numpy(g["seq_x"]).cuda()
    for mode in ("train", "eval"):
        net.train(mode == "train")
        with torch.no_grad():
            q, (h, c) = net(x, net.init_hidden(16, "cuda"))
        assert h.shape == (1, 16, 128) and c.shape == (1, 16, 128)
        _close(q, g[f"seq_q_{mode}"], "q (HIP path)")
        _close(h[0], g[f"seq_h_{mode}"][0], "h (HIP path)")
    net.train(True)
    q, _ = net(x, net.init_hidden(16, "cuda"))  # autograd: the torch path
    assert q.requires_grad
    _close(q, g["seq_q_train"], "q (torch path)")


def test_rnn_against_oracle_random_states(golden, orc):
    """4096 rows of random observations and warm states against the float64 oracle."""
    from pongmi import rnn
    g = golden("rnn")
    sd = {k[7:]: v for k, v in g.items() if k.startswith("params.")}
    rng = np.random.default_rng(11)
    n = 4096
    x = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
    x[:, 6] *= 5
    h0 = rng.normal(0, 0.4, (n, 128)).astype(np.float32)
    c0 = rng.normal(0, 0.8, (n, 128)).astype(np.float32)
    for mode in ("train", "eval"):
        h, c = torch.from_numpy(h0).cuda(), torch.from_numpy(c0).cuda()
        q = rnn.q_step(_w(g, mode), torch.from_numpy(x).cuda(), h, c)
        eff = orc.rnn_effective(sd, mode == "train")
        qo, ho, co = orc.rnn_forward(eff, x[:, None, :], h0, c0)
        # fp32 vs float64 on warm random states (pre-activations up to ~20): one fp32 K = 256 gate
        # dot product carries ~256 * 2^-24 * sum|w x| of rounding, up to ~2e-5 on c
        for a, b, what in ((q, qo, "q"), (h, ho, "h"), (c, co, "c")):
            np.testing.assert_allclose(a.cpu().numpy(), b, rtol=RTOL, atol=5e-5, err_msg=what)


def test_rnn_reset_rows_start_from_zero(golden):
    from pongmi import rnn
    g = golden("rnn")
    w = _w(g, "train")
    n = 300  # ragged: not a multiple of the 32-arena tile or the 128-row block
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(0, 1, (n, 7)).astype(np.float32)).cuda()
    h0 = torch.from_numpy(rng.normal(0, 0.4, (n, 128)).astype(np.float32)).cuda()
    c0 = torch.from_numpy(rng.normal(0, 0.8, (n, 128)).astype(np.float32)).cuda()
    reset = torch.from_numpy(rng.random(n) < 0.3).cuda()
    h, c = h0.clone(), c0.clone()
    q = rnn.q_step(w, x, h, c, reset=reset)
    hz, cz = h0.clone(), c0.clone()
    hz[reset] = 0
    cz[reset] = 0
    q2 = rnn.q_step(w, x, hz, cz)
    assert torch.equal(q, q2) and torch.equal(h, hz) and torch.equal(c, cz)


def _host_lists(opp, nn):
    """Per-256-arena-block opponent lists as the env kernels write them (write_opp_lists)."""
    n = len(opp)
    neb = (n + 255) // 256
    lst = np.zeros(n, np.int32)
    cnt = np.zeros(neb * nn, np.int32)
    for e in range(neb):
        ids = opp[e * 256:(e + 1) * 256]
        off = 0
        for k in range(nn):
            sel = np.nonzero(ids == k)[0] + e * 256
            lst[e * 256 + off:e * 256 + off + len(sel)] = sel
            cnt[e * nn + k] = (off << 16) | len(sel)
            off += len(sel)
    return lst, cnt


@pytest.mark.parametrize("n,n_opp,lists", [(1000, 1, False), (5000, 3, False), (257, 9, False), (5000, 3, True),
                                           (33000, 5, True), (300, 9, True)])
def test_rnn_act_matches_q_step(golden, n, n_opp, lists):
    """The fused two-player act: A greedy with its opponent's net, B greedy (eps = 0) — actions are
    the first-max argmax of the same Q values pm_rnn_q returns, states advance identically."""
    from pongmi import _lib, rnn
    from models.qnet_rnn import QNetRNN
    g = golden("rnn")
    wB = _w(g, "train")
    torch.manual_seed(7)
    nets = [QNetRNN(7, 3) for _ in range(n_opp)]
    w_opp = rnn.fold(torch.stack([rnn.pack_state_dict(m.state_dict()) for m in nets]), _lib.PM_FOLD_EVAL)
    rng = np.random.default_rng(n)
    obsA = torch.from_numpy(rng.uniform(0, 1, (n, 7)).astype(np.float32)).cuda()
    obsB = torch.from_numpy(rng.uniform(0, 1, (n, 7)).astype(np.float32)).cuda()
    opp = torch.from_numpy(rng.integers(0, n_opp, n).astype(np.int32)).cuda() if n_opp > 1 else None
    stA = [torch.from_numpy(rng.normal(0, 0.4, (n, 128)).astype(np.float32)).cuda() for _ in range(2)]
    stB = [torch.from_numpy(rng.normal(0, 0.4, (n, 128)).astype(np.float32)).cuda() for _ in range(2)]
    refA = [t.clone() for t in stA]
    refB = [t.clone() for t in stB]
    kw = {}
    if lists:  # side A packed over per-block lists (the self-play loop's path)
        oid_h = opp.cpu().numpy() if opp is not None else np.zeros(n, np.int32)
        if opp is None:
            opp = torch.zeros(n, dtype=torch.int32, device="cuda")
        lst, cnt = _host_lists(oid_h, n_opp)
        kw = dict(opp_list=torch.from_numpy(lst).cuda(), opp_cnt=torch.from_numpy(cnt).cuda())
    aA, aB, qA, qB = rnn.act(w_opp, opp, wB, obsA, obsB, stA, stB, epsilon=0.0, want_q=True, chunk1=1024, **kw)
    qB_ref = rnn.q_step(wB, obsB, *refB)
    qA_ref = torch.empty_like(qA)
    hA, cA = torch.empty_like(refA[0]), torch.empty_like(refA[1])
    oid = opp.long() if opp is not None else torch.zeros(n, dtype=torch.long, device="cuda")
    for k in range(n_opp):
        sel = (oid == k).nonzero().flatten()
        if sel.numel() == 0:
            continue
        hk, ck = refA[0][sel].contiguous(), refA[1][sel].contiguous()
        qA_ref[sel] = rnn.q_step(w_opp[k], obsA[sel], hk, ck)
        hA[sel], cA[sel] = hk, ck
    assert torch.equal(qB, qB_ref) and torch.equal(qA, qA_ref)
    assert torch.equal(stB[0], refB[0]) and torch.equal(stB[1], refB[1])
    assert torch.equal(stA[0], hA) and torch.equal(stA[1], cA)
    assert torch.equal(aB.long(), qB.argmax(1)) and torch.equal(aA.long(), qA.argmax(1))


def test_rnn_act_epsilon_and_reset(golden):
    """eps = 1: B acts uniformly at random in {0, 1, 2} but its forward still advances (h, c)
    (train_rnn_iterative.py:379-383); reset zeroes both players' state first."""
    from pongmi import rnn
    g = golden("rnn")
    w = _w(g, "train")
    n = 4096
    rng = np.random.default_rng(1)
    obs = torch.from_numpy(rng.uniform(0, 1, (n, 7)).astype(np.float32)).cuda()
    st = [torch.from_numpy(rng.normal(0, 0.4, (n, 128)).astype(np.float32)).cuda() for _ in range(4)]
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    reset[::5] = True
    ref = [t.clone() for t in st]
    for t in ref:
        t[reset] = 0
    pre = [t.clone() for t in ref]
    aA, aB = rnn.act(w.reshape(1, -1), None, w, obs, obs, st[:2], st[2:], reset=reset, epsilon=1.0, seed=5, counter=9)
    qA = rnn.q_step(w, obs, ref[0], ref[1])
    qB = rnn.q_step(w, obs, ref[2], ref[3])
    for a, b in zip(st, ref):
        assert torch.equal(a, b)
    assert torch.equal(aA.long(), qA.argmax(1))
    counts = torch.bincount(aB.long(), minlength=3).cpu().numpy()
    assert counts.min() > n / 3 - 5 * np.sqrt(n * 2 / 9), counts
    assert (aB.long() != qB.argmax(1)).any()
    aA2, aB2 = rnn.act(w.reshape(1, -1), None, w, obs, obs, pre[:2], pre[2:], epsilon=1.0, seed=5, counter=9)
    assert torch.equal(aB, aB2)  # Philox(seed, counter): reproducible


def test_rnn_fold_fresh_noise_writes_buffers(golden):
    """train_fresh: reset_noise() on the device (factorised Gaussian, models/qnet_rnn.py:33-41) —
    weight_epsilon = outer(f(e_out), f(e_in)), bias_epsilon = f(e_out), written back, and the
    folded weights equal a train-mode fold of the written-back block."""
    from pongmi import _lib, rnn
    g = golden("rnn")
    p = rnn.pack_state_dict(_sd(g))
    out = p.clone()
    w = rnn.fold(p, _lib.PM_FOLD_TRAIN_FRESH, seed=3, counter=4, params_out=out)[0]
    sd = rnn.unpack_state_dict(out)
    for m in ("fc_shared_head.0", "fc_V", "fc_A"):
        we, be = sd[f"{m}.weight_epsilon"], sd[f"{m}.bias_epsilon"]
        assert not torch.equal(be, torch.from_numpy(g[f"params.{m}.bias_epsilon"]))
        r = int(be.abs().argmax())
        e_in = we[r] / be[r]
        torch.testing.assert_close(we, torch.outer(be, e_in), rtol=1e-5, atol=1e-6)
    assert torch.equal(rnn.fold(out, _lib.PM_FOLD_TRAIN)[0], w)
    w2 = rnn.fold(p, _lib.PM_FOLD_TRAIN_FRESH, seed=3, counter=5)[0]
    assert not torch.equal(w, w2)


# ------------------------------------------------------------------ K5 at every size the ABI accepts
TAIL = 64  # rows allocated past n and filled with a sentinel: nothing may write them, no result may depend on them
S_SENTINEL, Q_SENTINEL, A_SENTINEL = 1234.5, -12345.0, 77
# fp32 device vs the float64 oracle on warm random states: the bound of
# test_rnn_against_oracle_random_states (one fp32 K = 256 gate dot product carries up to ~2e-5 on c)
O_RTOL, O_ATOL = 1e-4, 5e-5
EPS32 = float(np.float32(0.3))  # pm_rnn_act takes epsilon as a float: the value the device compares with


def _with_tail(a, fill):
    """Host array [n, ...] -> device tensor [n + TAIL, ...], the tail rows filled with `fill`."""
    a = np.ascontiguousarray(a)
    out = np.full((a.shape[0] + TAIL,) + a.shape[1:], fill, a.dtype)
    out[:a.shape[0]] = a
    return torch.from_numpy(out).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _split_tail(t, n, fill, what):
    """Device tensor [n + TAIL, ...] -> its n rows on the host; the tail must be bit-unchanged."""
    a = t.cpu().numpy()
    assert _same(a[n:], np.full_like(a[n:], fill)), f"{what}: rows past n were written"
    return a[:n]


def _ragged_inputs(seed, n):
    """x U(0, 1), warm (h, c) N(0, 0.4), ~30 % of the rows reset (the last row always, row 0 never)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (n, 7)).astype(np.float32)
    h = rng.normal(0, 0.4, (n, 128)).astype(np.float32)
    c = rng.normal(0, 0.4, (n, 128)).astype(np.float32)
    reset = rng.random(n) < 0.3
    if n:
        reset[n - 1] = True
    if n > 1:
        reset[0] = False
    return x, h, c, reset


def _golden_sd_np(g):
    return {k[7:]: v for k, v in g.items() if k.startswith("params.")}


def _pack_np(sd):
    from pongmi import rnn
    return rnn.pack_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


_NETS = {}


def _rand_sds(count):
    """The first `count` of 65 QNetRNN(7, 3) state dicts drawn under torch.manual_seed(7) (numpy)."""
    if "sds" not in _NETS:
        from models.qnet_rnn import QNetRNN
        torch.manual_seed(7)
        _NETS["sds"] = [{k: v.detach().clone().numpy() for k, v in QNetRNN(7, 3).state_dict().items()}
                        for _ in range(65)]
    return _NETS["sds"][:count]


def _rand_nets(count, orc):
    """(eval-folded device weights [count, NW], the oracle's effective weights) of _rand_sds(count)."""
    from pongmi import _lib, rnn
    sds = _rand_sds(count)
    if "w" not in _NETS:
        blocks = torch.stack([_pack_np(sd) for sd in _NETS["sds"]])
        _NETS["w"] = rnn.fold(blocks, _lib.PM_FOLD_EVAL).contiguous()
        _NETS["eff"] = {}
    for k in range(count):
        if k not in _NETS["eff"]:
            _NETS["eff"][k] = orc.rnn_effective(sds[k], False)
    return _NETS["w"][:count].contiguous(), [_NETS["eff"][k] for k in range(count)]


def _oracle_step(orc, eff, x, h0, c0, reset):
    """One float64 QNetRNN step from (h0, c0), the reset rows from zero state."""
    h, c = h0.astype(np.float64), c0.astype(np.float64)
    if reset is not None:
        h[reset] = 0.0
        c[reset] = 0.0
    return orc.rnn_forward(eff, x[:, None, :], h, c)


def _vs_oracle(who, dev, ref):
    """(q, h, c) of the device against the oracle's within O_RTOL / O_ATOL; returns the worst
    error / tolerance of the three."""
    worst = 0.0
    for a, b, what in zip(dev, ref, "qhc"):
        tol = O_ATOL + O_RTOL * np.abs(b)
        err = np.abs(a - b)
        assert np.all(err <= tol), f"{who}: {what} off by {err.max():.3g} ({(err / tol).max():.2f} x the tolerance)"
        worst = max(worst, float((err / tol).max()) if err.size else 0.0)
    return worst


def _band(q_or):
    """Rows whose top-2 oracle gap lies within twice the Q tolerance (either may win on the device)."""
    tol = (O_ATOL + O_RTOL * np.abs(q_or)).max(axis=1)
    srt = np.sort(q_or, axis=1)
    return srt[:, 2] - srt[:, 1] <= 2.0 * tol, srt, tol


def _band_cap(n):
    return max(1, -(-n // 100))


def _check_actions(who, a, q_dev, q_or, eps, seed, ctr, orc):
    """Actions against the launch's own Q (first max), the oracle's argmax outside the tie band, the
    restated Philox draw on the epsilon branch. Returns (in-band rows, explored rows)."""
    n = len(a)
    want, explore = orc.rnn_act_decision(q_or, eps, seed, ctr, np.arange(n))
    assert np.array_equal(a[explore], want[explore]), f"{who}: epsilon-branch actions"
    g = ~explore
    assert np.array_equal(a[g], orc.argmax_first(q_dev)[g]), f"{who}: action != first-max argmax of the launch's own Q"
    band, srt, tol = _band(q_or)
    clear = g & ~band
    assert np.array_equal(a[clear], want[clear]), f"{who}: greedy actions differ from the oracle's argmax"
    inb = g & band
    pick = q_or[np.arange(n), a.astype(np.int64)]
    assert np.all(pick[inb] >= srt[inb, 2] - 2.0 * tol[inb]), f"{who}: in-band pick not a near-max"
    assert int(band.sum()) <= _band_cap(n), f"{who}: {int(band.sum())} rows in the tie band (cap {_band_cap(n)})"
    return int(band.sum()), int(explore.sum())


def _rnn_q_raw(w, x, h0, c0, reset, n):
    """pm_rnn_q through the C ABI on buffers TAIL rows longer than n (x tail NaN, reset tail 1,
    h / c / q tails sentinels, checked here). Returns host (q, h, c) of the n rows."""
    from pongmi import _lib
    lib = _lib.load()
    xd = _with_tail(x, np.float32(np.nan))
    hd, cd = _with_tail(h0, np.float32(S_SENTINEL)), _with_tail(c0, np.float32(S_SENTINEL))
    rd = _with_tail(reset.astype(np.uint8), np.uint8(1)) if reset is not None else None
    q = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
    p = _lib.ptr
    _lib.check(lib.pm_rnn_q(p(w), p(xd), p(hd), p(cd), p(rd), p(q), n, _lib.stream_ptr()), "pm_rnn_q")
    return _split_tail(q, n, Q_SENTINEL, "q"), _split_tail(hd, n, S_SENTINEL, "h"), _split_tail(cd, n, S_SENTINEL, "c")


def _q_padded(w, x, h0, c0, reset, seed=99):
    """The same rows through pm_rnn_q padded with other rows to whole 128-row groups: host (q, h, c)
    of the first n rows. A row's result depends on its inputs and its net only."""
    from pongmi import rnn
    n = len(x)
    if n == 0:
        return np.zeros((0, 3), np.float32), h0.copy(), c0.copy()
    pad = -n % 128
    fx, fh, fc, fr = _ragged_inputs(seed, pad)
    xd = torch.from_numpy(np.concatenate([x, fx])).cuda()
    hd = torch.from_numpy(np.concatenate([h0, fh])).cuda()
    cd = torch.from_numpy(np.concatenate([c0, fc])).cuda()
    rd = torch.from_numpy(np.concatenate([reset, fr])).cuda() if reset is not None else None
    q = rnn.q_step(w, xd, hd, cd, reset=rd)
    return q.cpu().numpy()[:n], hd.cpu().numpy()[:n], cd.cpu().numpy()[:n]


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300])
def test_rnn_q_ragged_n(orc, golden, n, mode):
    """pm_rnn_q below, at and beside the 32-row tile and the 128-row group, without and with reset
    rows: (q, h, c) within the float64 oracle's tolerance (reset rows: the oracle from zero state) and
    equal bit for bit to the same rows inside a launch padded to whole groups; rows past n are neither
    written nor read; n = 0 is PM_OK and writes nothing."""
    g = golden("rnn")
    w = _w(g, mode).contiguous()
    eff = orc.rnn_effective(_golden_sd_np(g), mode == "train")
    x, h0, c0, reset = _ragged_inputs(1000 + n, n)
    for rs in (None, reset):
        q, h, c = _rnn_q_raw(w, x, h0, c0, rs, n)
        if n == 0:
            continue
        for a, b, what in zip((q, h, c), _q_padded(w, x, h0, c0, rs), "qhc"):
            assert _same(a, b), f"{what}: {np.count_nonzero(a != b)} values differ from the padded launch"
        ref = _oracle_step(orc, eff, x, h0, c0, rs)
        worst = _vs_oracle(f"n={n} {mode}", (q, h, c), ref)
        band = int(_band(ref[0])[0].sum())
        print(f"\npm_rnn_q n={n} {mode} reset={'set' if rs is not None else 'null'}: max error / tolerance "
              f"{worst:.3f}, {band} rows in the tie band")
        assert band <= _band_cap(n)
        if rs is not None:  # a reset row ignores its (h, c): the same bytes from any other state
            q2, h2, c2 = _rnn_q_raw(w, x, np.where(rs[:, None], 7.0, h0).astype(np.float32),
                                    np.where(rs[:, None], np.nan, c0).astype(np.float32), rs, n)
            assert _same(q, q2) and _same(h, h2) and _same(c, c2)


def _rnn_act_raw(w_opp, opp, n_opp, w_B, oA, oB, st, n, reset=None, eps=0.0, seed=0, counter=0, eps_dev=None,
                 counter_dev=None, chunk0=0, chunk1=0, lists=None):
    """pm_rnn_act through the C ABI on buffers TAIL rows longer than n: observations with NaN tails,
    opponent-id and reset tails 1, states / actions / Q with sentinel tails (checked here). st = host
    (hA, cA, hB, cB). Returns a dict of the n rows of aA, aB, qA, qB, hA, cA, hB, cB (host)."""
    from pongmi import _lib
    lib = _lib.load()
    oAd, oBd = _with_tail(oA, np.float32(np.nan)), _with_tail(oB, np.float32(np.nan))
    oppd = _with_tail(opp.astype(np.int32), np.int32(1)) if opp is not None else None
    rd = _with_tail(reset.astype(np.uint8), np.uint8(1)) if reset is not None else None
    sd = [_with_tail(s, np.float32(S_SENTINEL)) for s in st]
    aA = torch.full((n + TAIL,), A_SENTINEL, dtype=torch.int8, device="cuda")
    aB = torch.full((n + TAIL,), A_SENTINEL, dtype=torch.int8, device="cuda")
    qA = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
    qB = torch.full((n + TAIL, 3), Q_SENTINEL, dtype=torch.float32, device="cuda")
    lst = cnt = None
    if lists is not None:
        lst, cnt = (torch.from_numpy(a).cuda() for a in lists)
    p = _lib.ptr
    _lib.check(lib.pm_rnn_act(p(w_opp), p(oppd), n_opp, p(w_B), p(oAd), p(oBd), p(sd[0]), p(sd[1]), p(sd[2]), p(sd[3]),
                              p(rd), float(eps), p(eps_dev), int(seed), int(counter), p(counter_dev), p(aA), p(aB),
                              p(qA), p(qB), n, int(chunk0), int(chunk1), p(lst), p(cnt), _lib.stream_ptr()),
               "pm_rnn_act")
    out = dict(aA=_split_tail(aA, n, A_SENTINEL, "aA"), aB=_split_tail(aB, n, A_SENTINEL, "aB"),
               qA=_split_tail(qA, n, Q_SENTINEL, "qA"), qB=_split_tail(qB, n, Q_SENTINEL, "qB"))
    for k, t in zip(("hA", "cA", "hB", "cB"), sd):
        out[k] = _split_tail(t, n, S_SENTINEL, k)
    return out


def _act_inputs(seed, n):
    rng = np.random.default_rng(seed)
    oA = rng.uniform(0, 1, (n, 7)).astype(np.float32)
    oB = rng.uniform(0, 1, (n, 7)).astype(np.float32)
    st = [rng.normal(0, 0.4, (n, 128)).astype(np.float32) for _ in range(4)]
    reset = rng.random(n) < 0.3
    reset[n - 1] = True
    if n > 1:
        reset[0] = False
    return oA, oB, st, reset


def _opp_config(cfg, n, seed):
    """(n_opp, opp_id or None, the net of every arena) of a named opponent configuration."""
    rng = np.random.default_rng(seed)
    if cfg == "none":
        return 3, None, np.zeros(n, np.int64)
    if cfg == "zero":
        return 3, np.zeros(n, np.int64), np.zeros(n, np.int64)
    if cfg == "skip2":  # 5 nets, net 2 owns no arena
        opp = np.array([0, 1, 3, 4])[rng.integers(0, 4, n)]
        return 5, opp, opp
    if cfg in ("own128", "own256"):  # net 1 owns exactly one / two whole 128-row groups
        k = int(cfg[3:])
        opp = np.where(rng.random(n) < 0.5, 0, 2)
        opp[rng.permutation(n)[:k]] = 1
        assert np.count_nonzero(opp == 1) == k
        return 3, opp, opp
    n_opp = {"nets64": 64, "nets65": 65}[cfg]
    opp = rng.integers(0, n_opp, n)
    opp[n - 1] = n_opp - 1  # the last net plays
    return n_opp, opp, opp


RNN_ACT_CASES = [(cfg, n) for n in (1, 33, 129, 257, 1000) for cfg in ("none", "zero", "skip2")] + \
                [(cfg, n) for n in (257, 1000) for cfg in ("own128", "own256")] + [("nets64", 300), ("nets65", 300)]
RNN_ACT_CHUNKS = ((0, 0), (32, 100), (256, 2048), (2048, 2048))
ACT_KEYS = ("aA", "aB", "qA", "qB", "hA", "cA", "hB", "cB")


@pytest.mark.parametrize("cfg,n", RNN_ACT_CASES)
def test_rnn_act_ragged_sizes_nets_and_chunks(orc, golden, cfg, n):
    """pm_rnn_act at ragged n for opp_id NULL / all arenas on net 0 / a net that owns no arena / a net
    that owns exactly 128 or 256 arenas / 64 nets / 65 nets (lists passed and ignored), under four
    chunkings, the compaction and the packed per-256-arena lists, eps 0 / 0.3, reset NULL / set: every
    variant gives the same bytes; both players' (q, h, c) are within the float64 oracle's tolerance
    and equal pm_rnn_q on the same rows (per net, padded to whole groups) bit for bit; actions are
    the first max of the launch's Q, the oracle's argmax outside its tie band, the restated Philox
    draw on the epsilon branch; nothing is written past n."""
    g = golden("rnn")
    w_B = _w(g, "train").contiguous()
    effB = orc.rnn_effective(_golden_sd_np(g), True)
    n_opp, opp, net = _opp_config(cfg, n, 50 + n)
    w_opp, effs = _rand_nets(n_opp, orc)
    oA, oB, st, reset = _act_inputs(2000 + n, n)
    lists = _host_lists(net.astype(np.int32), n_opp)
    seed, ctr = 11, 3
    for rs in (None, reset):
        # the references, once per reset setting: the oracle and pm_rnn_q on the same rows
        refB = _oracle_step(orc, effB, oB, st[2], st[3], rs)
        bitB = _q_padded(w_B, oB, st[2], st[3], rs)
        refA = [np.empty((n, 3)), np.empty((n, 128)), np.empty((n, 128))]
        bitA = [np.empty((n, 3), np.float32), np.empty((n, 128), np.float32), np.empty((n, 128), np.float32)]
        for k in np.unique(net):
            sel = net == k
            rk = rs[sel] if rs is not None else None
            for dst, src in zip(refA, _oracle_step(orc, effs[k], oA[sel], st[0][sel], st[1][sel], rk)):
                dst[sel] = src
            for dst, src in zip(bitA, _q_padded(w_opp[k], oA[sel], st[0][sel], st[1][sel], rk)):
                dst[sel] = src
        for eps in (0.0, EPS32):
            first = None
            for lst in (None, lists):
                for chunk0, chunk1 in RNN_ACT_CHUNKS:
                    got = _rnn_act_raw(w_opp, opp, n_opp, w_B, oA, oB, st, n, reset=rs, eps=eps, seed=seed, counter=ctr,
                                       chunk0=chunk0, chunk1=chunk1, lists=lst)
                    where = (cfg, n, rs is not None, eps, lst is not None, chunk0, chunk1)
                    if first is None:
                        first = got
                    for key in ACT_KEYS:
                        assert _same(first[key], got[key]), (key, where)
            got = first
            for key, b in zip(("qA", "hA", "cA", "qB", "hB", "cB"), bitA + list(bitB)):
                assert _same(got[key], b), f"{key}: {np.count_nonzero(got[key] != b)} values differ from pm_rnn_q"
            wA = _vs_oracle(f"A {where}", (got["qA"], got["hA"], got["cA"]), refA)
            wB = _vs_oracle(f"B {where}", (got["qB"], got["hB"], got["cB"]), refB)
            ibA, _ = _check_actions(f"A {where}", got["aA"], got["qA"], refA[0], 0.0, seed, ctr, orc)
            ibB, ex = _check_actions(f"B {where}", got["aB"], got["qB"], refB[0], eps, seed, ctr, orc)
            assert eps == 0.0 or n < 33 or ex > 0
            print(f"\npm_rnn_act {cfg} n={n} reset={'set' if rs is not None else 'null'} eps={eps:.1f}: max error / "
                  f"tolerance A {wA:.3f} B {wB:.3f}; rows in the tie band A {ibA} B {ibB}; {ex} epsilon-branch rows "
                  f"exact")


def test_rnn_act_device_side_epsilon_and_counter(orc):
    """*eps_dev replaces epsilon, *counter_dev is added to counter: the same bytes as the same values
    passed as host arguments, and other actions under another counter."""
    n = 300
    w_opp, _ = _rand_nets(3, orc)
    w_B = w_opp[2].contiguous()
    _, opp, _ = _opp_config("own128", n, 5)
    oA, oB, st, reset = _act_inputs(77, n)
    eps_dev = torch.tensor([EPS32], dtype=torch.float64, device="cuda")
    ctr_dev = torch.tensor([41], dtype=torch.int64, device="cuda")
    run = lambda **kw: _rnn_act_raw(w_opp, opp, 3, w_B, oA, oB, st, n, reset=reset, seed=9, **kw)  # noqa: E731
    host = run(eps=EPS32, counter=48)
    other = run(eps=EPS32, counter=7)
    assert not np.array_equal(host["aB"], other["aB"])  # the counter matters
    assert not np.array_equal(host["aB"], run(eps=0.0, counter=48)["aB"])
    for key in ACT_KEYS:
        if key != "aB":
            assert _same(host[key], other[key]), key  # only B's epsilon branch reads the counter
    for kw in (dict(eps=0.9, eps_dev=eps_dev, counter=48),                    # eps_dev wins over epsilon
               dict(eps=EPS32, counter=0, counter_dev=ctr_dev + 7),           # the counter from the device alone
               dict(eps=0.9, eps_dev=eps_dev, counter=7, counter_dev=ctr_dev)):  # counter + *counter_dev
        got = run(**kw)
        for key in ACT_KEYS:
            assert _same(host[key], got[key]), (key, sorted(kw))


def test_rnn_act_exact_ties_take_first_index(golden):
    """Exact ties (random weights never produce one): a net whose fc_A rows 1 and 2 are identical, and
    one with all three identical (eval fold, sigma 0). The head sums every advantage column in the
    same order, so the launch's own Q ties bit for bit on every row, and both players' action is the
    first maximal index, never the last tied one, in every tile (n = 100: three tiles and a ragged one)."""
    from pongmi import _lib, rnn
    n = 100
    oA, oB, st, _ = _act_inputs(17, n)

    def tied(rows):
        sd = {k: v.clone() for k, v in _sd(golden("rnn")).items()}
        for k in ("fc_A.weight_mu", "fc_A.bias_mu"):
            for r in rows[1:]:
                sd[k][r] = sd[k][rows[0]]
        for k in ("fc_A.weight_sigma", "fc_A.bias_sigma", "fc_V.weight_sigma", "fc_V.bias_sigma"):
            sd[k] = torch.zeros_like(sd[k])
        return rnn.fold(rnn.pack_state_dict(sd), _lib.PM_FOLD_EVAL)[0].contiguous()

    for rows in ((1, 2), (0, 1, 2)):
        w = tied(rows)
        got = _rnn_act_raw(w, None, 1, w, oA, oB, st, n, eps=0.0)
        for a, q in ((got["aA"], got["qA"]), (got["aB"], got["qB"])):
            for r in rows[1:]:
                assert _same(q[:, rows[0]], q[:, r]), f"columns {rows[0]} and {r} do not tie exactly"
            assert np.array_equal(a, np.argmax(q, 1))  # numpy: the first maximal index
            assert not np.any(a == rows[-1])  # a tied later index never wins
            print(f"\ntied rows {rows}: action counts {np.bincount(a, minlength=3)}")
            if len(rows) == 3:
                assert np.all(a == 0)
            else:
                assert np.any(a == 1)  # the tied pair is the maximum somewhere: the tie was decided


def test_rnn_q_and_act_argument_errors(orc):
    """Every argument error is rejected on the host before a launch: a null buffer, n < 0, n_opp = 0,
    a 4-byte-misaligned h / w_B (PM_E_ARG), chunk0 / chunk1 = 2049 (PM_E_SIZE); nothing is written and
    pm_last_error() says why."""
    from pongmi import _lib
    lib = _lib.load()
    PM_E_ARG, PM_E_SIZE = -1, -2
    n = 40
    w_opp, _ = _rand_nets(2, orc)
    w_B = w_opp[1].contiguous()
    oA, oB, st, reset = _act_inputs(3, n)
    x = torch.from_numpy(oA).cuda()
    xB = torch.from_numpy(oB).cuda()
    opp = torch.zeros(n, dtype=torch.int32, device="cuda")
    state = lambda: torch.full((n + 1, 128), S_SENTINEL, device="cuda")  # noqa: E731
    bufs = dict(h=state(), c=state(), hB=state(), cB=state(),
                q=torch.full((n, 3), Q_SENTINEL, device="cuda"), qB=torch.full((n, 3), Q_SENTINEL, device="cuda"),
                a=torch.full((n,), A_SENTINEL, dtype=torch.int8, device="cuda"),
                aB=torch.full((n,), A_SENTINEL, dtype=torch.int8, device="cuda"))
    before = {k: v.clone() for k, v in bufs.items()}
    p = _lib.ptr

    def rejected(rc, want, what):
        assert rc == want, f"{what}: rc {rc}, expected {want}"
        assert lib.pm_last_error(), what
        torch.cuda.synchronize()
        for k in bufs:
            assert torch.equal(bufs[k], before[k]), f"{what}: {k} was written"

    qargs = dict(w=p(w_B), x=p(x), h=p(bufs["h"]), c=p(bufs["c"]), reset=None, q=p(bufs["q"]), n=n)

    def q_call(**kw):
        a = dict(qargs, **kw)
        return lib.pm_rnn_q(a["w"], a["x"], a["h"], a["c"], a["reset"], a["q"], a["n"], _lib.stream_ptr())

    for name in ("w", "x", "h", "c", "q"):
        rejected(q_call(**{name: None}), PM_E_ARG, f"pm_rnn_q {name} = NULL")
    rejected(q_call(n=-1), PM_E_ARG, "pm_rnn_q n < 0")
    rejected(q_call(h=p(bufs["h"]) + 4), PM_E_ARG, "pm_rnn_q misaligned h")

    aargs = dict(w_opp=p(w_opp), opp=p(opp), n_opp=2, w_B=p(w_B), obsA=p(x), obsB=p(xB), hA=p(bufs["h"]),
                 cA=p(bufs["c"]), hB=p(bufs["hB"]), cB=p(bufs["cB"]), aA=p(bufs["a"]), aB=p(bufs["aB"]),
                 qA=p(bufs["q"]), qB=p(bufs["qB"]), n=n, chunk0=0, chunk1=0)

    def act_call(**kw):
        a = dict(aargs, **kw)
        return lib.pm_rnn_act(a["w_opp"], a["opp"], a["n_opp"], a["w_B"], a["obsA"], a["obsB"], a["hA"], a["cA"],
                              a["hB"], a["cB"], None, 0.0, None, 0, 0, None, a["aA"], a["aB"], a["qA"], a["qB"], a["n"],
                              a["chunk0"], a["chunk1"], None, None, _lib.stream_ptr())

    for name in ("w_opp", "w_B", "obsA", "obsB", "hA", "cA", "hB", "cB", "aA", "aB"):
        rejected(act_call(**{name: None}), PM_E_ARG, f"pm_rnn_act {name} = NULL")
    rejected(act_call(n=-1), PM_E_ARG, "pm_rnn_act n < 0")
    rejected(act_call(n_opp=0), PM_E_ARG, "pm_rnn_act n_opp = 0")
    rejected(act_call(hA=p(bufs["h"]) + 4), PM_E_ARG, "pm_rnn_act misaligned hA")
    rejected(act_call(w_B=p(w_B) + 4), PM_E_ARG, "pm_rnn_act misaligned w_B")
    rejected(act_call(chunk0=2049), PM_E_SIZE, "pm_rnn_act chunk0 = 2049")
    rejected(act_call(chunk1=2049), PM_E_SIZE, "pm_rnn_act chunk1 = 2049")
    assert act_call() == 0 and q_call(q=p(bufs["qB"])) == 0  # the same arguments unbroken are accepted
    torch.cuda.synchronize()


@pytest.mark.parametrize("cdev", [None, 1000])
def test_rnn_fold_fresh_noise_every_net(orc, golden, cdev):
    """count = 3, PM_FOLD_TRAIN_FRESH: net k draws with counter + *counter_dev + k * 0x10000 — its
    written-back epsilon buffers equal the Philox restatement bit for bit, nothing else of the block
    changes, and its effective weights equal a PM_FOLD_TRAIN fold of the written-back block.
    count = 0 is PM_OK; a misaligned w_eff is PM_E_ARG."""
    from pongmi import _lib, rnn
    lib = _lib.load()
    sds = [_golden_sd_np(golden("rnn"))] + _rand_sds(2)
    blocks = torch.stack([_pack_np(sd) for sd in sds]).contiguous()
    out = blocks.clone()
    seed, ctr = 21, 5
    cd = torch.tensor([cdev], dtype=torch.int64, device="cuda") if cdev is not None else None
    w = rnn.fold(blocks, _lib.PM_FOLD_TRAIN_FRESH, seed=seed, counter=ctr, counter_dev=cd, params_out=out)
    draws = []
    for k in range(3):
        sd = rnn.unpack_state_dict(out[k])
        ref = orc.rnn_philox_noise(seed, ctr + (cdev or 0) + k * 0x10000)
        for key, val in ref.items():
            assert _same(sd[key].numpy(), val), f"net {k}: {key}"
        draws.append(ref["fc_A.bias_epsilon"])
        assert torch.equal(out[k, :rnn.PM_RNN_NPARAM], blocks[k, :rnn.PM_RNN_NPARAM])  # parameters untouched
        assert torch.equal(rnn.fold(out[k], _lib.PM_FOLD_TRAIN)[0], w[k]), f"net {k}: w_eff"
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    if cdev is not None:  # *counter_dev is added: the same draws as the sum passed on the host
        w2 = rnn.fold(blocks, _lib.PM_FOLD_TRAIN_FRESH, seed=seed, counter=ctr + cdev)
        assert torch.equal(w, w2)
    # count = 0 and a misaligned w_eff: no launch
    keep = w.clone()
    p = _lib.ptr
    assert lib.pm_rnn_fold(p(blocks), None, _lib.PM_FOLD_TRAIN_FRESH, seed, ctr, None, p(w), 0, _lib.stream_ptr()) == 0
    rc = lib.pm_rnn_fold(p(blocks), None, _lib.PM_FOLD_TRAIN_FRESH, seed, ctr + 1, None, p(w) + 4, 1, _lib.stream_ptr())
    assert rc == -1 and lib.pm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(w, keep)
