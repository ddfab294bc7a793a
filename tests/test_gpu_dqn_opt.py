"""The stand-alone DQN learner's loss / clip options (pm_dqn_*_opt, DQNLearner(loss="huber", max_norm=)) on
the MI355X: Huber gradients at every batch edge in both modes, the clip's norm, coefficient and Adam step,
defaults that change no bit, split == fused and two summed replicas, the replay-driven update, and a
small ReplayTrainer run.

The reference is plain torch on the CPU: test_gpu_dqn.py's _autograd with its loss line replaced by
(iw * F.smooth_l1_loss(q, t, reduction='none', beta=beta)).mean(), then torch.nn.utils.clip_grad_norm_ and
torch.optim.Adam over the trained parameters (_Ref below), in float64 and, for the conditioned feature
bar, float32.

Bars: test_gpu_dqn.py's (head gradient rtol 2e-4 / atol 2e-6 x 256 / B; feature gradients against float64
rtol 5e-4 with atol max(1e-5 max|g|, 1.5 x the float32 autograd's own error); loss rtol 1e-4 with the
batch-1 allowance; td / q atol 3e-5; Adam rtol 1e-5 / atol 1e-7; the reference's norm at the gradient's
5e-4) and one derived here: the reported norm against the float64 norm of the device's own gradient,
rtol 1e-6. The squares are accumulated in fp64 from float32 values (each product of two float32 values is
exact in fp64, and 5 192 fp64 additions err by < 5 192 x 2^-53 < 1e-12 relative), so the only float32
roundings are the final conversion of the sum's square root (the fp64 sqrt itself is correctly rounded),
<= 2^-24 relative, and the conversion back for the comparison: together well under 2 x 2^-23 < 2.4e-7."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_dqn import BATCHES, FEATS, GAMMA, GRAD_RTOL, HEAD_OFF, LR, NPARAM, REF32_FACTOR, _batch, _conditioned_batch, \
    _learner, _np, nets  # noqa: F401  (nets: the module fixture)

pytestmark = pytest.mark.gpu

B1, B2 = 0.9, 0.999
MN = 0.02  # a max_norm that bites under the Huber loss too (its gradient is a bounded sign over most rows)


class _Ref:
    """modelB / targetB as models.qnet.QNet on the CPU with the block's own epsilon buffers (no reset_noise),
    the double-DQN target, the chosen loss, and optionally the clip and an Adam step."""

    def __init__(self, sd, tsd, dtype, tf, beta=None, max_norm=None):
        from models.qnet import QNet
        self.mB, self.mT = QNet(7, 3), QNet(7, 3)
        self.mB.load_state_dict(sd)
        self.mT.load_state_dict(tsd)
        self.mB.to(dtype).train()
        self.mT.to(dtype).eval()
        self.dtype, self.beta, self.max_norm = dtype, beta, max_norm
        self.trained = list(self.mB.parameters()) if tf else \
            list(self.mB.fc_V.parameters()) + list(self.mB.fc_A.parameters())
        self.opt = torch.optim.Adam(self.trained, lr=LR, betas=(B1, B2), eps=1e-8)

    def backward(self, batch, isw):
        dtype = self.dtype
        s, a, r, ns, d = batch
        s, ns, r = (torch.as_tensor(x).to(dtype) for x in (s, ns, r))
        a, d = torch.as_tensor(a).long(), torch.as_tensor(d).bool()
        iw = torch.ones(len(a), dtype=dtype) if isw is None else torch.as_tensor(isw).to(dtype)
        self.mB.zero_grad()
        q = self.mB(s).gather(1, a.unsqueeze(1)).squeeze(1)
        with torch.no_grad():
            qn = self.mB(ns)
            na = qn.argmax(1, keepdim=True)
            nq = self.mT(ns).gather(1, na).squeeze(1)
        t = r + GAMMA * nq * (~d)
        if self.beta is None:
            loss = (iw * (q - t).pow(2)).mean()
        else:
            loss = (iw * F.smooth_l1_loss(q, t, reduction='none', beta=self.beta)).mean()
        loss.backward()
        top2 = torch.sort(qn, dim=1, descending=True).values
        grads = np.concatenate([p.grad.numpy().ravel().astype(np.float64) for p in self.mB.parameters()])
        norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in self.trained)))
        return dict(loss=float(loss.detach()), grads=grads, norm=norm, gap=float((top2[:, 0] - top2[:, 1]).min()),
                    q=q.detach().numpy().astype(np.float64), diff=(q - t).detach().numpy().astype(np.float64),
                    td=(q - t).abs().detach().numpy().astype(np.float64))

    def step(self, batch, isw):
        out = self.backward(batch, isw)
        if self.max_norm is not None:
            out["norm_clip"] = float(torch.nn.utils.clip_grad_norm_(self.trained, self.max_norm))
        self.opt.step()
        return out

    def params(self):
        return np.concatenate([p.detach().numpy().ravel().astype(np.float64) for p in self.mB.parameters()])


def _assert_grads(grad, r64, r32, B, tf, what):
    """test_gpu_dqn.py's _check_case bars on a device gradient against the float64 / float32 references."""
    np.testing.assert_allclose(grad[HEAD_OFF:NPARAM], r64["grads"][HEAD_OFF:], rtol=2e-4, atol=2e-6 * 256 / B, err_msg=what)
    assert grad[NPARAM] == 1.0 and not grad[NPARAM + 1:].any()
    if tf:
        for name, lo, hi in FEATS:
            ref = r64["grads"][lo:hi]
            m = np.abs(ref).max()
            e32 = np.abs(r32["grads"][lo:hi] - ref).max()
            print(f"{what}: {name}: device {np.abs(grad[lo:hi] - ref).max() / max(m, 1e-30):.2e}, "
                  f"reference f32 {e32 / max(m, 1e-30):.2e} x max|g|")
            np.testing.assert_allclose(grad[lo:hi], ref, rtol=GRAD_RTOL, atol=max(1e-5 * m, REF32_FACTOR * e32) + 1e-12,
                                       err_msg=f"{what}: {name}")
    else:
        assert np.all(grad[:HEAD_OFF] == 7.0), what


def _check_huber(sd, tsd, batch, isw, tf, beta, what, min_gap=1e-4):
    """One gradient launch with the Huber loss against float64; returns the learner and the float64 reference."""
    B = len(batch[1])
    L = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf, loss="huber", huber_beta=beta)
    L.grad[:] = 7.0
    L.grads(*batch, isw=isw)
    torch.cuda.synchronize()
    r64 = _Ref(sd, tsd, torch.float64, tf, beta).backward(batch, isw)
    r32 = _Ref(sd, tsd, torch.float32, tf, beta).backward(batch, isw)
    assert r64["gap"] > min_gap or min_gap == 0, (what, r64["gap"])
    _assert_grads(_np(L.grad), r64, r32, B, tf, what)
    st = L.stats()
    loss_atol = 1.5 * abs(r32["loss"] - r64["loss"]) if B == 1 else 0.0  # test_gpu_dqn.py's batch-1 allowance
    print(f"{what}: loss {st['loss']:.7f} (ref {r64['loss']:.7f})")
    np.testing.assert_allclose(st["loss"], r64["loss"], rtol=1e-4, atol=loss_atol, err_msg=what)
    np.testing.assert_allclose(_np(L.q)[np.arange(B), batch[1]], r64["q"], rtol=0, atol=3e-5, err_msg=what)
    np.testing.assert_allclose(_np(L.td), r64["td"], rtol=0, atol=3e-5, err_msg=what)
    assert st["steps"] == 0 and "norm" not in st
    return L, r64


def _huber_batch(sd, tsd, B, beta):
    """_conditioned_batch rows on which, in float64, no row's branch hangs on float32 rounding (every | |d| - beta |
    > 1e-3) and, from batch 31 up, both branches hold at least 4 rows; the seed walks until they do."""
    for k in range(50):
        batch, iw = _conditioned_batch(sd, tsd, B, 100 + B + 17 * k)
        ad = _Ref(sd, tsd, torch.float64, True, beta).backward(batch, iw)["td"]
        nq = int((ad < beta).sum())
        if np.abs(ad - beta).min() > 1e-3 and (B < 31 or (nq >= 4 and B - nq >= 4)):
            return batch, iw, nq
    raise AssertionError(f"no conditioned Huber batch: B {B} beta {beta}")


def _plain_grads(sd, tsd, batch, isw, tf):
    L = _learner(sd, tsd, batch=len(batch[1]), fresh_noise=False, train_features=tf)
    L.grads(*batch, isw=isw)
    torch.cuda.synchronize()
    return L


# ----------------------------------------------------------------------------- 1. Huber at every batch edge
@pytest.mark.parametrize("tf", [0, 1])
@pytest.mark.parametrize("B", BATCHES)
def test_huber_gradients_at_every_batch_edge(nets, B, tf):
    """Batches 1, 31, 32, 33, 255, 256, heads only and whole net, beta 1 and 2 (batch 1: beta 1 puts the row
    in the linear zone, beta 4 in the quadratic): the gradient, loss, q and td bars against float64; isw None
    == ones bit for bit; td and q bit-identical to the plain learner's; a row with diff == 0 exactly
    contributes nothing."""
    sd, tsd = nets
    for beta in ((1.0, 4.0) if B == 1 else (1.0, 2.0)):
        batch, iw, nq = _huber_batch(sd, tsd, B, beta)
        what = f"batch {B}, train_features {tf}, beta {beta} ({nq} quadratic rows)"
        if B == 1:
            assert nq == (0 if beta == 1.0 else 1), what
        L, _ = _check_huber(sd, tsd, batch, iw, tf, beta, what)
        P = _plain_grads(sd, tsd, batch, iw, tf)
        assert torch.equal(L.td, P.td) and torch.equal(L.q, P.q), what  # the loss does not touch the forwards
        assert L.stats()["q_mean"] == P.stats()["q_mean"]
        assert not torch.equal(L.grad[HEAD_OFF:NPARAM], P.grad[HEAD_OFF:NPARAM])
        L0, _ = _check_huber(sd, tsd, batch, None, tf, beta, what + ", isw None")
        L1 = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf, loss="huber", huber_beta=beta)
        L1.grad[:] = 7.0
        L1.grads(*batch, isw=np.ones(B, np.float32))
        torch.cuda.synchronize()
        assert torch.equal(L0.grad, L1.grad) and torch.equal(L0.td, L1.td) and torch.equal(L0.q, L1.q), what
        assert L0.stats() == L1.stats()
    # diff == 0 exactly: both nets' heads zeroed (q = 0 and Q_T = 0 everywhere), the last row r = 0 and done
    batch, iw = _conditioned_batch(sd, tsd, B, 100 + B)
    s, a, r, ns, d = batch
    sd0, tsd0 = dict(sd), dict(tsd)
    for z in (sd0, tsd0):
        for k in list(z):
            if k.startswith(("fc_V.", "fc_A.")) and "epsilon" not in k:
                z[k] = torch.zeros_like(z[k])
    r0, d0 = r.copy(), d.copy()
    r0[:] = np.where(r0 == 0, 2.0, 2.0 * r0)  # every other row: t = r = +-2, q = 0: the linear zone of beta 1
    r0[B - 1], d0[B - 1] = 0.0, True
    bz = (s, a, r0, ns, d0)
    La, r64 = _check_huber(sd0, tsd0, bz, iw, tf, 1.0, f"batch {B}, train_features {tf}, zero diff", min_gap=0)
    assert r64["diff"][B - 1] == 0.0 and _np(La.td)[B - 1] == 0.0
    iw0 = iw.copy()
    iw0[B - 1] = 0.0  # the same batch with that row weighted out
    Lb = _learner(sd0, tsd0, batch=B, fresh_noise=False, train_features=tf, loss="huber", huber_beta=1.0)
    Lb.grad[:] = 7.0
    Lb.grads(*bz, isw=iw0)
    torch.cuda.synchronize()
    assert torch.equal(La.grad, Lb.grad)
    assert torch.isfinite(La.grad).all()
    if B == 1:
        assert not La.grad[HEAD_OFF:NPARAM].any()
    else:
        assert La.grad[HEAD_OFF:NPARAM].abs().max() > 0


# ----------------------------------------------------------------------------- 2. the clip
def _clip_batches(sd, tsd, B, tf):
    """Three _conditioned_batch batches on which the three clipped Adam steps are conditioned for float32 at all:
    torch's own float32 loop ends within half the Adam bar of its float64 loop (as _conditioned_batch keeps a*
    off float32 rounding: a parameter whose m / sqrt(v) hangs on a cancelling gradient element says nothing
    about the code under test). The condition is on the references alone; the seed walks until it holds."""
    off = 0 if tf else HEAD_OFF
    for j in range(20):
        batches = [_conditioned_batch(sd, tsd, B, 100 * k + B + 17 * j) for k in (1, 2, 3)]
        R64, R32 = _Ref(sd, tsd, torch.float64, tf, None, 1.0), _Ref(sd, tsd, torch.float32, tf, None, 1.0)
        for batch, iw in batches:
            R64.step(batch, iw)
            R32.step(batch, iw)
        p64, p32 = R64.params()[off:], R32.params()[off:]
        if (np.abs(p32 - p64) / (1e-7 + 1e-5 * np.abs(p64))).max() <= 0.5:
            return batches
    raise AssertionError(f"no conditioned clip batches: B {B} tf {tf}")


def _trained_norm(L, off):
    return float(np.sqrt((_np(L.grad)[off:NPARAM].astype(np.float64) ** 2).sum()))


@pytest.mark.parametrize("tf", [0, 1])
@pytest.mark.parametrize("B", BATCHES)
def test_clip_at_every_batch_edge(nets, B, tf):
    """max_norm = 1 under the squared loss (the float64 norms there are 2.0 .. 808.8: active everywhere): the
    norm against the device's own gradient and against float64; the moments after one update from zero;
    the parameters after three updates on three batches against the float64 torch loop; an inactive clip
    (max_norm = 2 x the norm) changes no bit; heads-only mode leaves [0, 4672) alone."""
    sd, tsd = nets
    off = 0 if tf else HEAD_OFF
    what = f"batch {B}, train_features {tf}"
    batches = _clip_batches(sd, tsd, B, tf)
    L = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf, max_norm=1.0)
    L.adam_m[:off] = 0.25
    L.adam_v[:off] = 0.5
    L.grad[:off] = 7.0
    p0 = L.params.clone()
    R = _Ref(sd, tsd, torch.float64, tf, None, 1.0)
    for k, (batch, iw) in enumerate(batches):
        L.update(*batch, isw=iw)
        torch.cuda.synchronize()
        ref = R.step(batch, iw)
        st = L.stats()
        n_dev = _trained_norm(L, off)
        print(f"{what}, update {k}: norm {st['norm']:.7g}, of the device's own gradient {n_dev:.7g}, float64 {ref['norm']:.7g}")
        assert abs(ref["norm_clip"] - ref["norm"]) <= 1e-12 * ref["norm"], what
        assert k > 0 or ref["norm"] > 1.5, what  # the first batch's clip bites for certain
        np.testing.assert_allclose(st["norm"], n_dev, rtol=1e-6, atol=0, err_msg=what)
        np.testing.assert_allclose(st["norm"], ref["norm"], rtol=5e-4, atol=0, err_msg=what)
        assert st["steps"] == k + 1 and st["adam_t"] == k + 1 and st["status"] == 0
        if k == 0:  # from zero moments: m = (1 - beta1) g coef, v = (1 - beta2) (g coef)^2, g the unclipped grad
            g = _np(L.grad)[off:NPARAM].astype(np.float64)
            coef = min(1.0, 1.0 / (n_dev + 1e-6))
            np.testing.assert_allclose(_np(L.adam_m)[off:], (1 - B1) * g * coef, rtol=1e-5, atol=1e-7, err_msg=what)
            np.testing.assert_allclose(_np(L.adam_v)[off:], (1 - B2) * (g * coef) ** 2, rtol=1e-5, atol=1e-7, err_msg=what)
            assert np.abs(_np(L.adam_m)[off:]).max() > 10 * 1e-7  # the bar can tell a clipped moment from an unclipped one
            assert np.abs(_np(L.adam_m)[off:] - (1 - B1) * g).max() > 10 * 1e-7
    got, want = _np(L.params)[off:NPARAM], R.params()[off:]
    print(f"{what}: parameters after three clipped updates: max |err| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, err_msg=what)
    if not tf:
        assert torch.equal(L.params[:HEAD_OFF], p0[:HEAD_OFF]) and torch.all(L.adam_m[:HEAD_OFF] == 0.25) and \
            torch.all(L.adam_v[:HEAD_OFF] == 0.5) and torch.all(L.grad[:HEAD_OFF] == 7.0), what
    # a clip that does not bite: the clamped coefficient is exactly 1.0f
    batch, iw = batches[0]
    n64 = _Ref(sd, tsd, torch.float64, tf).backward(batch, iw)["norm"]
    X = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf, max_norm=2.0 * n64)
    Y = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf)
    for Z in (X, Y):
        Z.update(*batch, isw=iw)
    torch.cuda.synchronize()
    for name in ("params", "target", "adam_m", "adam_v", "grad", "td", "q"):
        assert torch.equal(getattr(X, name), getattr(Y, name)), f"{what}: inactive clip: {name}"
    sx = X.stats()
    np.testing.assert_allclose(sx.pop("norm"), n64, rtol=5e-4)
    assert sx == Y.stats()


# ----------------------------------------------------------------------------- 3. defaults change nothing
def _drive_opt(L, entry, opt, *extra):
    from pongmi import _lib
    fn = getattr(_lib.load(), entry)
    _lib.check(fn(ctypes.byref(L.desc), ctypes.byref(opt) if opt is not None else None, *extra, _lib.stream_ptr()), entry)


def _same(X, Y, what, names=("params", "target", "adam_m", "adam_v", "grad", "td", "q")):
    for name in names:
        assert torch.equal(getattr(X, name), getattr(Y, name)), f"{what}: {name}"
    sx, sy = X.stats(), Y.stats()
    assert sx == sy, (what, sx, sy)


@pytest.mark.parametrize("tf", [0, 1])
def test_default_options_change_no_bit(nets, tf):
    """pm_dqn_update against pm_dqn_update_opt with a zeroed pm_dqn_opt and with a null one, three updates
    (fresh noise, a target sync inside); the same for grads / apply."""
    from pongmi import _lib
    sd, tsd = nets
    B = 33

    def fresh():
        return _learner(sd, tsd, batch=B, fresh_noise=True, seed=7, train_features=tf, target_update_interval=2)

    A, Z, N, S = fresh(), fresh(), fresh(), fresh()
    zero = _lib.DqnOpt()
    assert (zero.loss, zero.huber_beta, zero.max_norm, zero.norm) == (0, 0.0, 0.0, None)
    for k in range(3):
        batch, iw = _batch(np.random.RandomState(20 + k), B)
        A.update(*batch, isw=iw)
        for X in (Z, N, S):
            X.load_batch(*batch, isw=iw)
        _drive_opt(Z, "pm_dqn_update_opt", zero)
        _drive_opt(N, "pm_dqn_update_opt", None)
        _drive_opt(S, "pm_dqn_grads_opt", zero)
        _drive_opt(S, "pm_dqn_apply_opt", zero)
        torch.cuda.synchronize()
        _same(A, Z, f"update {k}: zeroed opt")
        _same(A, N, f"update {k}: null opt")
        _same(A, S, f"update {k}: grads_opt + apply_opt")
    assert A.stats()["steps"] == 3 and not torch.equal(A.target, A.params)


# ----------------------------------------------------------------------------- 4. split == fused, sharding
@pytest.mark.parametrize("tf", [0, 1])
def test_split_equals_fused_and_two_replicas_clip_on_the_averaged_gradient(nets, tf):
    sd, tsd = nets
    B, off = 33, 0 if tf else HEAD_OFF
    kw = dict(batch=B, fresh_noise=True, seed=7, train_features=tf, target_update_interval=2, loss="huber", huber_beta=1.0,
              max_norm=MN)
    A, C = _learner(sd, tsd, **kw), _learner(sd, tsd, **kw)
    for k in range(2):  # the second update syncs the target
        batch, iw = _batch(np.random.RandomState(30 + k), B)
        A.update(*batch, isw=iw)
        C.grads(*batch, isw=iw)
        C.apply()
        torch.cuda.synchronize()
        _same(A, C, f"update {k}: grads + apply vs update")
        assert A.stats()["norm"] > 1.5 * MN  # the clip was active
    assert A.stats()["steps"] == 2 and torch.equal(A.target, A.params)
    # two ranks, each with a batch of its own; the all-reduce by hand
    kw.update(fresh_noise=False)
    X, Y = _learner(sd, tsd, **kw), _learner(sd, tsd, **kw)
    (bx, wx), (by, wy) = _conditioned_batch(sd, tsd, B, 41), _conditioned_batch(sd, tsd, B, 42)
    X.grads(*bx, isw=wx)
    Y.grads(*by, isw=wy)
    total = X.grad + Y.grad
    assert total[NPARAM] == 2.0
    X.grad.copy_(total)
    Y.grad.copy_(total)
    X.apply()
    Y.apply()
    torch.cuda.synchronize()
    for name in ("params", "target", "adam_m", "adam_v", "grad", "norm"):
        assert torch.equal(getattr(X, name), getattr(Y, name)), f"two ranks: {name}"
    sx, sy = X.stats(), Y.stats()
    assert (sx["steps"], sx["adam_t"], sx["norm"]) == (sy["steps"], sy["adam_t"], sy["norm"]) == (1, 1, sx["norm"])
    R = _Ref(sd, tsd, torch.float64, tf, 1.0)
    g64 = 0.5 * (R.backward(bx, wx)["grads"] + R.backward(by, wy)["grads"])
    n64 = float(np.sqrt((g64[off:] ** 2).sum()))
    gavg = 0.5 * _np(total)[off:NPARAM].astype(np.float64)
    n_dev = float(np.sqrt((gavg ** 2).sum()))
    print(f"two ranks, train_features {tf}: norm {sx['norm']:.7g}, of the averaged device gradient {n_dev:.7g}, float64 {n64:.7g}")
    assert n64 > 1.5 * MN  # active
    np.testing.assert_allclose(sx["norm"], n_dev, rtol=1e-6, atol=0)
    np.testing.assert_allclose(sx["norm"], n64, rtol=5e-4, atol=0)
    np.testing.assert_allclose(gavg[HEAD_OFF - off:], g64[HEAD_OFF:], rtol=2e-4, atol=2e-6 * 256 / B)
    coef = min(1.0, MN / (n_dev + 1e-6))
    np.testing.assert_allclose(_np(X.adam_m)[off:], (1 - B1) * gavg * coef, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(_np(X.adam_v)[off:], (1 - B2) * (gavg * coef) ** 2, rtol=1e-5, atol=1e-7)
    assert torch.equal(X.grad, total)  # grad keeps the unclipped sum


# ----------------------------------------------------------------------------- 5. from the replay
def _replay_setup(orc, seed, zero_prios=False):
    import test_gpu_dqn_replay as tr
    cap = size = 512
    rng = np.random.default_rng(seed)
    trans = tr._rows(rng, cap)
    prios = np.zeros(cap, np.float32) if zero_prios else tr._prios(rng, cap, size)
    return tr, rng, trans, prios, tr._replay(trans, prios, size)


def _qnets():
    from models.qnet import QNet
    torch.manual_seed(11)
    return QNet(7, 3).state_dict(), QNet(7, 3).state_dict()


@pytest.mark.parametrize("tf", [False, True])
def test_update_from_with_options_equals_the_composition(orc, tf):
    """update_from(replay, 3, uniforms=u) with Huber and an active clip, cap 512, batch 32, against
    test_gpu_dqn_replay.py's composition (the draw, update() with the same options on those rows,
    update_priorities) bit for bit, the norm included; the tree equals a rebuild. And
    pm_dqn_replay_update_opt with a zeroed pm_dqn_opt against pm_dqn_replay_update."""
    from pongmi import _lib
    tr, rng, trans, prios, R = _replay_setup(orc, 50 + tf)
    batch, U = 32, 3
    kw = dict(target_update_interval=2, fresh_noise=True, loss="huber", huber_beta=1.0, max_norm=MN)
    A, C = tr._learner(_qnets(), batch, tf, **kw), tr._learner(_qnets(), batch, tf, **kw)
    u = rng.random((U, batch))
    tr._from(A, R, U, uniforms=u)
    for k in range(U):
        idx, w = tr._compose(orc, C, trans, prios, 512, k, u[k])
    tr._assert_batch_is_rows(orc, A, trans, idx, w, "last update")
    tr._same_learner(orc, A, C, f"tf {tf}: update_from vs the composition")
    assert torch.equal(A.norm, C.norm) and A.stats()["norm"] > 1.5 * MN  # active
    assert A.stats()["steps"] == U and A.stats()["status"] == 0
    assert orc.bits_equal(_np(R.prios), prios)
    tr._assert_tree_is_rebuild(orc, R, "options")
    # defaults: the _opt entry point with a zeroed opt against the plain one, given uniforms
    Rp, Rz = tr._replay(trans, prios, 512), tr._replay(trans, prios, 512)
    P, Z = tr._learner(_qnets(), batch, tf, target_update_interval=2), tr._learner(_qnets(), batch, tf, target_update_interval=2)
    u2 = rng.random((U, batch))
    tr._from(P, Rp, U, uniforms=u2)
    ud = torch.from_numpy(u2).cuda()
    Z.desc.isw = Z.isw.data_ptr()
    rp = _lib.DqnReplay(trans=Rz.trans.data_ptr(), prios=Rz.prios.data_ptr(), per_work=Rz.work.data_ptr(),
                        idx=Z.idx.data_ptr(), u=ud.data_ptr(), cap=512, size=512, alpha=Rz.alpha, beta_start=tr.BETA_START,
                        beta_frames=tr.BETA_FRAMES, seed=0)
    _drive_opt(Z, "pm_dqn_replay_update_opt", _lib.DqnOpt(), ctypes.byref(rp), U)
    torch.cuda.synchronize()
    tr._same_learner(orc, P, Z, f"tf {tf}: pm_dqn_replay_update vs _opt with a zeroed opt")
    assert torch.equal(P.idx, Z.idx) and torch.equal(P.isw, Z.isw)
    assert torch.equal(Rp.prios, Rz.prios) and torch.equal(Rp.work, Rz.work)


def test_void_update_with_options_touches_nothing(orc):
    tr, rng, trans, prios, R = _replay_setup(orc, 6, zero_prios=True)
    A = tr._learner(_qnets(), 32, True, loss="huber", max_norm=1.0)
    A.set_train_steps(4)
    A.norm.fill_(123.0)
    before = {n: _np(getattr(A, n)).copy() for n in ("params", "target", "adam_m", "adam_v", "s", "ns", "isw", "norm")}
    idx, _ = tr._from(A, R, 3)
    st = A.stats()
    assert st["status"] & 1 and st["steps"] == 4 and st["adam_t"] == 0 and st["norm"] == 123.0
    assert (_np(idx) == -1).all()
    for n, v in before.items():
        assert orc.bits_equal(_np(getattr(A, n)), v), n


# ----------------------------------------------------------------------------- 6. a small collect-and-train run
def test_replay_trainer_carries_the_options(nets):
    """test_toy_loop_trains_the_whole_net's nets through ReplayTrainer with train_features=True, loss="huber",
    max_norm=1.0 at 256 arenas: ReplayTrainer itself knows nothing of the options."""
    from pongmi import _lib
    from pongmi.dqn import ReplayTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import fold, pack_state_dict
    from pongmi.replay import DeviceReplay
    sd, tsd = nets
    env = PongEnv2PBatch(256, autoreset=True, seed=4)
    env.reset()
    L = _learner(sd, batch=256, train_features=True, seed=1, target_update_interval=8, loss="huber", max_norm=1.0)
    R = DeviceReplay(4096, "cuda", alpha=0.6)
    wA = fold(pack_state_dict(tsd), _lib.PM_FOLD_EVAL).reshape(-1)
    T = ReplayTrainer(env, wA, L, R, collect_steps=4, updates=2, epsilon=0.1, seed_net=1, seed=3)
    w2_before = L.state_dict()["features.2.weight"].clone()
    losses, norms = [], []
    for it in range(3):
        T.run(1)
        st = L.stats()
        losses.append(st["loss"])
        norms.append(st["norm"])
        assert st["steps"] == st["adam_t"] == 2 * (it + 1) and st["status"] == 0  # every update counted
    assert np.all(np.isfinite(losses)), losses
    assert np.all(np.isfinite(norms)) and min(norms) > 0, norms
    assert torch.isfinite(L.params).all()
    assert not torch.equal(L.state_dict()["features.2.weight"], w2_before)
