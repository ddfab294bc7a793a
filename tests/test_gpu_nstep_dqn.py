"""The learner's per-row horizon (pm_dqn_grads_n / pm_dqn_update_n, DQNLearner(nstep=)).

Bit for bit: a null pm_dqn_nstep, a null horizon and a horizon of all ones equal pm_dqn_update_opt; a uniform
horizon k with gamma = g equals the plain update with gamma = (double)disc(k), disc(k) the float32 product chain
computed here in numpy; with mixed horizons row j's td is row j's td of the uniform run with k = horizon[j]; rows
with done = 1 ignore their horizon. The mixed update's gradient and updated parameters are held to the float64
torch reference and the bars of tests/test_gpu_dqn.py (head gradients rtol 2e-4 / atol 2e-6 x 256 / batch,
feature gradients rtol 5e-4 with atol max(1e-5 max|g|, 1.5 x the float32 reference's own error), td atol 3e-5,
Adam rtol 1e-5 / atol 1e-7). The parameters after the step are compared with float64 Adam on the float64 gradient;
a first Adam step moves a parameter by lr g / (|g| + 1e-8), which no float32 gradient pins where |g| is near 1e-8,
so per element the atol is max(1e-7, 1.5 x the error of the same reference run in float32), that file's allowance
for its feature gradients. (At batch 32 with the Huber loss one head parameter has |g| = 7.5e-8: torch's own
float32 step is 2.57e-6 from the float64 one there, the device's 2.53e-6; every other element is inside 1e-7 +
1e-5 |p|.)"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA, LR = 0.99, 2.5e-4
HEAD_OFF, NPARAM = 4672, 5192
FEATS = (("features.0.weight", 0, 448), ("features.0.bias", 448, 512), ("features.2.weight", 512, 4608),
         ("features.2.bias", 4608, 4672))
GRAD_RTOL, REF32_FACTOR = 5e-4, 1.5
STATE = ("params", "target", "adam_m", "adam_v", "td", "grad", "stats_buf")


def _disc(k, gamma=GAMMA):
    g = np.float32(gamma)
    d = g
    for _ in range(k - 1):
        d = np.float32(d * g)
    return d


@pytest.fixture(scope="module")
def nets(golden):
    from pongmi.qnet import pack_state_dict, unpack_state_dict
    g = golden("dqn_full_steps")
    sd = {k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init.")}
    tblk = pack_state_dict(sd, "cpu")
    tblk[HEAD_OFF:NPARAM] += 0.05 * torch.randn(NPARAM - HEAD_OFF, generator=torch.Generator().manual_seed(8))
    return sd, unpack_state_dict(tblk)


def _reference(sd, tsd, batch, isw, disc, loss, tf, dtype):
    """train_iterative.py:152-158 with t = r + disc * nq * (~d), disc per row, autograd and one Adam step over
    models.qnet.QNet on the CPU."""
    from models.qnet import QNet
    mB, mT = QNet(7, 3), QNet(7, 3)
    mB.load_state_dict(sd)
    mT.load_state_dict(tsd)
    mB.to(dtype).train()
    mT.to(dtype).eval()
    s, a, r, ns, d = batch
    s, ns, r = (torch.as_tensor(x).to(dtype) for x in (s, ns, r))
    a, d = torch.as_tensor(a).long(), torch.as_tensor(d).bool()
    iw = torch.as_tensor(isw).to(dtype)
    params = list(mB.parameters())
    opt = torch.optim.Adam(params if tf else params[4:], lr=LR)
    q = mB(s).gather(1, a.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        qn = mB(ns)
        nq = mT(ns).gather(1, qn.argmax(1, keepdim=True)).squeeze(1)
    t = r + torch.as_tensor(np.asarray(disc, np.float64)).to(dtype) * nq * (~d)
    if loss == "huber":
        out = (iw * torch.nn.functional.smooth_l1_loss(q, t, reduction="none", beta=1.0)).mean()
    else:
        out = (iw * (q - t).pow(2)).mean()
    out.backward()
    top2 = torch.sort(qn, dim=1, descending=True).values
    grads = np.concatenate([p.grad.numpy().ravel().astype(np.float64) for p in params])
    td = (q - t).abs().detach().numpy().astype(np.float64)
    opt.step()
    after = np.concatenate([p.detach().numpy().ravel().astype(np.float64) for p in params])
    return dict(grads=grads, td=td, after=after, gap=float((top2[:, 0] - top2[:, 1]).min()))


def _batch(sd, tsd, B, seed):
    """Random rows (test_gpu_dqn.py's ranges) whose smallest top-2 gap of Q_B(s') is > 1e-4, with done rows."""
    lo = np.array([0, 0, -0.08, -0.08, 0, 0, -5], np.float32)
    hi = np.array([1, 1, 0.08, 0.08, 1, 1, 5], np.float32)
    for k in range(50):
        rng = np.random.RandomState(seed + 1000 * k)
        s = (lo + (hi - lo) * rng.random_sample((B, 7))).astype(np.float32)
        ns = (lo + (hi - lo) * rng.random_sample((B, 7))).astype(np.float32)
        a = rng.randint(0, 3, B).astype(np.int64)
        r = rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0], B).astype(np.float32)
        d = rng.rand(B) < 0.1
        if B > 1:
            d[B // 2] = True
        iw = rng.uniform(0.2, 1.0, B).astype(np.float32)
        iw /= iw.max()
        h = rng.randint(1, 9, B).astype(np.uint8)
        if B >= 32:
            h[:8] = np.arange(1, 9)  # every horizon occurs
        batch = (s, a, r, ns, d)
        if _reference(sd, tsd, batch, iw, np.full(B, GAMMA), "mse", 0, torch.float64)["gap"] > 1e-4:
            return batch, iw, h
    raise AssertionError("no conditioned batch")


def _learner(nets, B, tf, loss, **kw):
    from pongmi.dqn import DQNLearner
    kw.setdefault("gamma", GAMMA)
    return DQNLearner(nets[0], nets[1], batch=B, lr=LR, fresh_noise=False, train_features=tf, loss=loss,
                      max_norm=1e3 if loss == "huber" else None, **kw)


def _state(L):
    torch.cuda.synchronize()
    return {k: getattr(L, k).cpu().numpy().copy() for k in STATE}


def _same(a, b, what):
    for k in STATE:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _call(L, entry, *extra):
    from pongmi import _lib
    o = ctypes.byref(L.opt) if L.opt is not None else None
    _lib.check(getattr(L.lib, entry)(ctypes.byref(L.desc), o, *extra, _lib.stream_ptr()), entry)
    return _state(L)


@pytest.mark.parametrize("loss", ["mse", "huber"])
@pytest.mark.parametrize("tf", [0, 1])
@pytest.mark.parametrize("B", [1, 32, 33, 256])
def test_horizon_targets(nets, B, tf, loss):
    from pongmi import _lib
    sd, tsd = nets
    batch, iw, h = _batch(sd, tsd, B, 300 + B)
    what = f"batch {B}, train_features {tf}, {loss}"

    # ---- no horizon, a null horizon and all ones are pm_dqn_update_opt
    L = _learner(nets, B, tf, loss)
    L.load_batch(*batch, isw=iw)
    want = _call(L, "pm_dqn_update_opt")
    for name, ns in (("null struct", None), ("null horizon", _lib.DqnNstep(horizon=None))):
        L = _learner(nets, B, tf, loss)
        L.load_batch(*batch, isw=iw)
        _same(want, _call(L, "pm_dqn_update_n", ctypes.byref(ns) if ns is not None else None), f"{what}: {name}")
    L = _learner(nets, B, tf, loss, nstep=2)
    L.update(*batch, isw=iw, horizon=np.ones(B, np.uint8))
    _same(want, _state(L), f"{what}: all ones")
    assert want["stats_buf"].view(np.int64)[0] == 1  # a step was taken

    # ---- a uniform horizon k is the plain update with gamma = disc(k)
    td_of = {1: want["td"]}
    for k in (2, 3, 8):
        L = _learner(nets, B, tf, loss, nstep=k)
        L.update(*batch, isw=iw)  # horizon None: every row the learner's nstep
        got = _state(L)
        P = _learner(nets, B, tf, loss, gamma=float(_disc(k)))
        P.update(*batch, isw=iw)
        _same(_state(P), got, f"{what}: uniform {k}")
        td_of[k] = got["td"]
    for k in (4, 5, 6, 7):  # the other horizons the mixed batch holds
        L = _learner(nets, B, tf, loss, nstep=k)
        L.update(*batch, isw=iw)
        td_of[k] = _state(L)["td"]

    # ---- mixed horizons: rows are independent before the reduction
    L = _learner(nets, B, tf, loss, nstep=8)
    L.update(*batch, isw=iw, horizon=h)
    mixed = _state(L)
    for j in range(B):
        assert mixed["td"][j].view(np.int32) == td_of[int(h[j])][j].view(np.int32), (what, j, h[j])
    # rows with done = 1 ignore the horizon
    h2 = h.copy()
    h2[batch[4]] = (h2[batch[4]] % 8) + 1
    L2 = _learner(nets, B, tf, loss, nstep=8)
    L2.update(*batch, isw=iw, horizon=h2)
    _same(mixed, _state(L2), f"{what}: done rows")
    if B > 1:
        assert batch[4].any() and (h2 != h).any()

    # ---- the mixed update against the float64 reference, at test_gpu_dqn.py's bars
    disc = np.array([_disc(int(k)) for k in h], np.float64)
    r64 = _reference(sd, tsd, batch, iw, disc, loss, tf, torch.float64)
    grad = mixed["grad"]
    np.testing.assert_allclose(mixed["td"], r64["td"], rtol=0, atol=3e-5, err_msg=what)
    np.testing.assert_allclose(grad[HEAD_OFF:NPARAM], r64["grads"][HEAD_OFF:], rtol=2e-4, atol=2e-6 * 256 / B, err_msg=what)
    off = 0 if tf else HEAD_OFF
    r32 = _reference(sd, tsd, batch, iw, disc, loss, tf, torch.float32)
    if tf:
        for name, lo, hi in FEATS:
            ref = r64["grads"][lo:hi]
            m = np.abs(ref).max()
            e32 = np.abs(r32["grads"][lo:hi] - ref).max()
            np.testing.assert_allclose(grad[lo:hi], ref, rtol=GRAD_RTOL, atol=max(1e-5 * m, REF32_FACTOR * e32) + 1e-12,
                                       err_msg=f"{what}: {name}")
    err = np.abs(mixed["params"][off:NPARAM] - r64["after"][off:])
    print(f"{what}: params after Adam max|err| {err.max():.2e}")
    ref_err = np.abs(r32["after"][off:] - r64["after"][off:])  # the reference's own float32 step against float64
    bound = np.maximum(1e-7, REF32_FACTOR * ref_err) + 1e-5 * np.abs(r64["after"][off:])
    assert (err <= bound).all(), (what, int((err > bound).sum()), float((err - bound).max()))


def test_horizons_need_a_learner_built_for_them(nets):
    from pongmi import _lib
    batch, iw, h = _batch(nets[0], nets[1], 32, 1)
    L = _learner(nets, 32, 0, "mse")
    with pytest.raises(_lib.PongmiError, match="nstep=1"):
        L.update(*batch, isw=iw, horizon=h)
