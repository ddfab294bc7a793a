"""The stand-alone double-DQN learner (pm_dqn_grads / pm_dqn_apply / pm_dqn_update, pongmi.dqn.DQNLearner)
on the MI355X: the reference's own heads-only train_step run (dqn_steps.npz), whole-net training against
the reference's QNet with nothing frozen (dqn_full_steps.npz), every batch edge in both modes against
float64, the fresh-noise draw, determinism and the grads / apply split, and a small loop of one's own.

Bars (the ones the fused learner and the oracle are held to): head gradient rtol 2e-4 / atol 2e-6 (x 256 /
batch below batch 256), loss rtol 1e-4, q / td / targets atol 3e-5, Adam rtol 1e-5 / atol 1e-7. Feature
gradients in the form of test_gpu_drqn.py's _assert_grads_conditioned: against float64, rtol 5e-4 with
atol = max(1e-5 max|g|, 1.5 x the error of the reference's own float32 autograd against float64)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA, LR = 0.99, 2.5e-4
HEAD_OFF, NPARAM, EPS_OFF = 4672, 5192, 5192
FEATS = (("features.0.weight", 0, 448), ("features.0.bias", 448, 512), ("features.2.weight", 512, 4608),
         ("features.2.bias", 4608, 4672))
EPS_KEYS = ("fc_V.weight_epsilon", "fc_V.bias_epsilon", "fc_A.weight_epsilon", "fc_A.bias_epsilon")
GRAD_RTOL, REF32_FACTOR = 5e-4, 1.5
BATCHES = (1, 31, 32, 33, 255, 256)


def _init_sd(g):
    return {k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init.")}


def _set_eps(L, eps):
    """eps: {epsilon key: array} -> the block's epsilon buffers."""
    flat = np.concatenate([np.asarray(eps[k], np.float32).ravel() for k in EPS_KEYS])
    L.params[EPS_OFF:].copy_(torch.from_numpy(flat))


def _learner(sd, target=None, **kw):
    from pongmi.dqn import DQNLearner
    kw.setdefault("lr", LR)
    kw.setdefault("gamma", GAMMA)
    return DQNLearner(sd, target, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _check_step_outputs(orc, L, g, k, what):
    """After update k of a fixture replay: na (from the kernel's own Q_B(s') forward, taken before the
    update), loss, q, td and the targets against the reference's recorded run."""
    st = L.stats()
    a = g[f"s{k}.a"]
    q = _np(L.q)[np.arange(len(a)), a]
    td = _np(L.td)
    print(f"{what}: loss {st['loss']:.6f} (ref {float(g[f's{k}.loss']):.6f}), max |q err| "
          f"{np.abs(q - g[f's{k}.q']).max():.2e}, max |td err| {np.abs(td - g[f's{k}.errors']).max():.2e}")
    np.testing.assert_allclose(st["loss"], g[f"s{k}.loss"], rtol=1e-4, err_msg=what)
    np.testing.assert_allclose(q, g[f"s{k}.q"], rtol=0, atol=3e-5, err_msg=what)
    np.testing.assert_allclose(td, g[f"s{k}.errors"], rtol=0, atol=3e-5, err_msg=what)
    t_ref = g[f"s{k}.targets"]
    t_err = np.minimum(np.abs(q - td - t_ref), np.abs(q + td - t_ref))  # t = q -/+ |q - t|
    assert t_err.max() <= 3e-5, (what, t_err.max())
    np.testing.assert_allclose(st["q_mean"], q.astype(np.float64).mean(), rtol=1e-5, atol=1e-6)


def _na_of(orc, L, ns, a, r, d):
    """argmax Q_B(s') as the update's own forward computes Q_B: a gradient-only launch with s := s'."""
    L.grads(ns, a, r, ns, d)
    return orc.argmax_first(_np(L.q).astype(np.float64))


def _replay(orc, g, train_features):
    sd = _init_sd(g)
    L = _learner(sd, batch=256, target_update_interval=2, fresh_noise=False, train_features=train_features)
    if not train_features:  # the frozen part must keep every bit: params, Adam slots and grad
        L.adam_m[:HEAD_OFF] = 0.25
        L.adam_v[:HEAD_OFF] = 0.5
    p0, m0, v0 = L.params[:HEAD_OFF].clone(), L.adam_m[:HEAD_OFF].clone(), L.adam_v[:HEAD_OFF].clone()
    off = 0 if train_features else HEAD_OFF
    for k in range(3):
        what = f"{'whole net' if train_features else 'heads only'}, step {k}"
        _set_eps(L, {e: g[f"s{k}.noiseB.{e}"] for e in EPS_KEYS})
        batch = (g[f"s{k}.s"], g[f"s{k}.a"], g[f"s{k}.r"], g[f"s{k}.ns"], g[f"s{k}.d"])
        assert np.array_equal(_na_of(orc, L, batch[3], batch[1], batch[2], batch[4]), g[f"s{k}.na"]), what
        L.grad[:HEAD_OFF] = 7.0
        td = L.update(*batch, isw=g[f"s{k}.iw"])
        torch.cuda.synchronize()
        assert td.data_ptr() == L.td.data_ptr() and td.shape == (256,)
        _check_step_outputs(orc, L, g, k, what)
        grad = _np(L.grad)
        ref = g[f"s{k}.grads"]
        np.testing.assert_allclose(grad[HEAD_OFF:NPARAM], ref[HEAD_OFF - off:], rtol=2e-4, atol=2e-6, err_msg=what)
        assert grad[NPARAM] == 1.0 and not grad[NPARAM + 1:].any()
        if train_features:
            g64 = g[f"s{k}.grads64"]
            for name, lo, hi in FEATS:
                m = np.abs(g64[lo:hi]).max()
                e32 = np.abs(ref[lo:hi] - g64[lo:hi]).max()
                edev = np.abs(grad[lo:hi] - g64[lo:hi]).max()
                print(f"{what}: {name}: device {edev / m:.2e}, reference f32 {e32 / m:.2e} x max|g|")
                np.testing.assert_allclose(grad[lo:hi], g64[lo:hi], rtol=GRAD_RTOL,
                                           atol=max(1e-5 * m, REF32_FACTOR * e32), err_msg=f"{what}: {name}")
            np.testing.assert_allclose(_np(L.target)[:NPARAM], g[f"s{k}.target_after"], rtol=1e-5, atol=1e-7,
                                       err_msg=what)
        else:
            assert np.all(grad[:HEAD_OFF] == 7.0), what
            assert torch.equal(L.params[:HEAD_OFF], p0) and torch.equal(L.adam_m[:HEAD_OFF], m0) and \
                torch.equal(L.adam_v[:HEAD_OFF], v0), what
        np.testing.assert_allclose(_np(L.params)[off:NPARAM], g[f"s{k}.params_after"], rtol=1e-5, atol=1e-7,
                                   err_msg=what)
        np.testing.assert_allclose(_np(L.target)[HEAD_OFF:NPARAM], g[f"s{k}.target_heads_after"], rtol=1e-5,
                                   atol=1e-7, err_msg=what)
        st = L.stats()
        assert st["steps"] == k + 1 and st["adam_t"] == k + 1 and st["status"] == 0
    return L


def test_heads_only_replays_the_references_own_steps(orc, golden):
    """dqn_steps.npz (the reference's QNet, features frozen, Adam over the heads) with each step's recorded
    epsilon copied into the block, interval 2: na exact; loss, q, td, targets; gradient, parameters and
    target heads after each of the three steps; the frozen part bitwise untouched."""
    _replay(orc, golden("dqn_steps"), False)


def test_whole_net_matches_the_reference_with_nothing_frozen(orc, golden):
    """dqn_full_steps.npz (the reference's QNet, every parameter trainable, Adam over modelB.parameters()):
    the head tensors at the heads-only bars, the four feature tensors against the recorded float64
    gradient at the conditioned bar (device and reference float32 errors printed per tensor), all 5 192
    parameters and targetB after each step at Adam's bar."""
    g = golden("dqn_full_steps")
    assert min(float(g[f"s{k}.gap"]) for k in range(3)) > 1e-4
    L = _replay(orc, g, True)
    assert not torch.equal(L.params[:HEAD_OFF], torch.from_numpy(
        np.concatenate([g[f"init.{n}"].ravel() for n, _, _ in FEATS])).cuda())


# ----------------------------------------------------------------------------- batch edges
def _autograd(sd, tsd, batch, isw, dtype):
    """The reference's loss (train_iterative.py:152-158) with autograd over models.qnet.QNet on the CPU."""
    from models.qnet import QNet
    mB, mT = QNet(7, 3), QNet(7, 3)
    mB.load_state_dict(sd)
    mT.load_state_dict(tsd)
    mB.to(dtype).train()
    mT.to(dtype).eval()
    s, a, r, ns, d = batch
    s, ns, r = (torch.as_tensor(x).to(dtype) for x in (s, ns, r))
    a, d = torch.as_tensor(a).long(), torch.as_tensor(d).bool()
    iw = torch.ones(len(a), dtype=dtype) if isw is None else torch.as_tensor(isw).to(dtype)
    q = mB(s).gather(1, a.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        qn = mB(ns)
        na = qn.argmax(1, keepdim=True)
        nq = mT(ns).gather(1, na).squeeze(1)
    t = r + GAMMA * nq * (~d)
    loss = (iw * (q - t).pow(2)).mean()
    loss.backward()
    top2 = torch.sort(qn, dim=1, descending=True).values
    grads = np.concatenate([p.grad.numpy().ravel().astype(np.float64) for p in mB.parameters()])
    return dict(loss=float(loss.detach()), grads=grads, na=na.squeeze(1).numpy(), gap=float((top2[:, 0] - top2[:, 1]).min()),
                q=q.detach().numpy().astype(np.float64), td=(q - t).abs().detach().numpy().astype(np.float64))


def _batch(rng, B):
    lo = np.array([0, 0, -0.08, -0.08, 0, 0, -5], np.float32)
    hi = np.array([1, 1, 0.08, 0.08, 1, 1, 5], np.float32)
    s = (lo + (hi - lo) * rng.random_sample((B, 7))).astype(np.float32)
    ns = (lo + (hi - lo) * rng.random_sample((B, 7))).astype(np.float32)
    a = rng.randint(0, 3, B).astype(np.int64)
    r = rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0], B).astype(np.float32)
    d = rng.rand(B) < 0.1
    iw = rng.uniform(0.2, 1.0, B).astype(np.float32)
    return (s, a, r, ns, d), iw / iw.max()


@pytest.fixture(scope="module")
def nets(golden):
    """modelB = the fixture's initial net; targetB = the same features (oracle.dqn_loss_grads shares them, as
    the reference's frozen loop does) under perturbed heads, so Q_T is not Q_B. A target with features of
    its own is the whole-net fixture's step 1."""
    from pongmi.qnet import pack_state_dict, unpack_state_dict
    sd = _init_sd(golden("dqn_full_steps"))
    tblk = pack_state_dict(sd, "cpu")
    tblk[HEAD_OFF:NPARAM] += 0.05 * torch.randn(NPARAM - HEAD_OFF, generator=torch.Generator().manual_seed(8))
    return sd, unpack_state_dict(tblk)


def _check_case(orc, sd, tsd, batch, isw, tf, what, min_gap=1e-4, shared_features=True):
    """One gradient launch against float64: heads vs oracle.dqn_loss_grads, features vs float64 autograd of
    models.qnet.QNet at the conditioned bar; loss, q and td at the bars above. Returns the learner."""
    B = len(batch[1])
    L = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf)
    L.grad[:] = 7.0
    L.grads(*batch, isw=isw)
    torch.cuda.synchronize()
    r64 = _autograd(sd, tsd, batch, isw, torch.float64)
    assert r64["gap"] > min_gap or min_gap == 0, (what, r64["gap"])
    sdn = {k: _np(v) for k, v in sd.items()}
    tsdn = {k: _np(v) for k, v in tsd.items()}
    s, a, r, ns, d = batch
    res = orc.dqn_loss_grads(sdn, orc.pack_heads(sdn), orc.pack_heads(tsdn), sdn, s, a, r, ns, d,
                             np.ones(B) if isw is None else isw, GAMMA)
    grad = _np(L.grad)
    if shared_features:  # the oracle evaluates targetB on modelB's feature layers
        np.testing.assert_allclose(res["grads"], r64["grads"][HEAD_OFF:], rtol=1e-7, atol=1e-10)  # the references agree
    else:
        res = dict(grads=r64["grads"][HEAD_OFF:])
    np.testing.assert_allclose(grad[HEAD_OFF:NPARAM], res["grads"], rtol=2e-4, atol=2e-6 * 256 / B, err_msg=what)
    assert grad[NPARAM] == 1.0 and not grad[NPARAM + 1:].any()
    if tf:
        r32 = _autograd(sd, tsd, batch, isw, torch.float32)
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
    st = L.stats()
    # the loss bar holds from batch 2 up; at batch 1 the loss is one cancelling term (test_gpu_selfplay.py's
    # test_learn_matches_oracle_over_batch_sizes): there the reference's own float32 error is allowed 1.5 x
    loss_atol = 0.0
    if B == 1:
        loss_atol = 1.5 * abs(_autograd(sd, tsd, batch, isw, torch.float32)["loss"] - r64["loss"])
    np.testing.assert_allclose(st["loss"], r64["loss"], rtol=1e-4, atol=loss_atol, err_msg=what)
    np.testing.assert_allclose(_np(L.q)[np.arange(B), a], r64["q"], rtol=0, atol=3e-5, err_msg=what)
    np.testing.assert_allclose(_np(L.td), r64["td"], rtol=0, atol=3e-5, err_msg=what)
    assert st["steps"] == 0  # a gradient launch takes no step
    return L


def _conditioned_batch(sd, tsd, B, seed):
    """Random rows whose smallest top-2 gap of Q_B(s') is > 1e-4 (no a* hangs on float32 rounding)."""
    for k in range(50):
        rng = np.random.RandomState(seed + 1000 * k)
        batch, iw = _batch(rng, B)
        if _autograd(sd, tsd, batch, iw, torch.float64)["gap"] > 1e-4:
            return batch, iw
    raise AssertionError("no conditioned batch")


@pytest.mark.parametrize("tf", [0, 1])
@pytest.mark.parametrize("B", BATCHES)
def test_every_batch_edge(orc, nets, B, tf):
    """Batches 1, 31, 32, 33, 255, 256 (a partial tile, whole tiles, one row into the next tile), heads only
    and whole net: the gradient bars, and per case: a targetB whose feature layers differ from modelB's;
    isw None == isw of ones bit for bit; a whole batch of
    done rows; every action value present; an exact tie of Q_B(s') (fc_A zeroed: a* = 0); a row whose
    ReLUs are all dead contributes nothing to the feature gradient."""
    sd, tsd = nets
    batch, iw = _conditioned_batch(sd, tsd, B, 100 + B)
    s, a, r, ns, d = batch
    what = f"batch {B}, train_features {tf}"
    _check_case(orc, sd, tsd, batch, iw, tf, what)
    # isw = None is isw of ones
    L0 = _check_case(orc, sd, tsd, batch, None, tf, what + ", isw None")
    L1 = _learner(sd, tsd, batch=B, fresh_noise=False, train_features=tf)
    L1.grad[:] = 7.0
    L1.grads(*batch, isw=np.ones(B, np.float32))
    torch.cuda.synchronize()
    assert torch.equal(L0.grad, L1.grad) and torch.equal(L0.td, L1.td) and torch.equal(L0.q, L1.q)
    assert L0.stats() == L1.stats()
    # a targetB with feature layers of its own (between two syncs of whole-net training): heads against float64
    # autograd, as oracle.dqn_loss_grads shares the feature layers
    tsd2 = dict(tsd)
    tsd2["features.2.weight"] = tsd["features.2.weight"] + 0.01 * torch.randn(64, 64, generator=torch.Generator().manual_seed(B))
    _check_case(orc, sd, tsd2, batch, iw, tf, what + ", target features differ", shared_features=False)
    # every row done: t = r
    _check_case(orc, sd, tsd, (s, a, r, ns, np.ones(B, bool)), iw, tf, what + ", all done")
    # every action value appears (as far as the batch allows)
    _check_case(orc, sd, tsd, (s, (np.arange(B) % 3).astype(np.int64), r, ns, d), iw, tf, what + ", actions 0 1 2")
    # an exact tie: fc_A zeroed, every advantage equal, a* must be the first index
    sd0 = dict(sd)
    for k in list(sd0):
        if k.startswith("fc_A."):
            sd0[k] = torch.zeros_like(sd0[k])
    Lt = _check_case(orc, sd0, tsd, batch, iw, tf, what + ", tie", min_gap=0)
    qT = orc.qnet_forward(orc.qnet_effective({k: _np(v) for k, v in tsd.items()}, False), ns)
    q0 = _np(Lt.q)[np.arange(B), a].astype(np.float64)
    t0 = r + GAMMA * qT[:, 0] * (~d)
    np.testing.assert_allclose(_np(Lt.td), np.abs(q0 - t0), rtol=0, atol=3e-5)  # Q_T(s')[0], not [1] or [2]
    apart = (np.abs(qT[:, 0] - qT[:, 1]) > 1e-3) & (np.abs(qT[:, 0] - qT[:, 2]) > 1e-3)
    assert apart.mean() > 0.5  # another index would have shown in td
    # a dead row: W1 > 0, b1 < 0, b2 < 0 and s = -1 kill both ReLU layers of the last row
    sdd = dict(sd)
    sdd["features.0.weight"] = sd["features.0.weight"].abs()
    sdd["features.0.bias"] = -sd["features.0.bias"].abs() - 1e-3
    sdd["features.2.bias"] = -sd["features.2.bias"].abs() - 1e-3
    tsdd = dict(tsd)  # the oracle's target shares modelB's features
    tsdd.update({k: v for k, v in sdd.items() if k.startswith("features.")})
    s_dead = s.copy()
    s_dead[B - 1] = -1.0
    bd = (s_dead, a, r, ns, d)
    La = _check_case(orc, sdd, tsdd, bd, iw, tf, what + ", dead row", min_gap=0)
    iw0 = iw.copy()
    iw0[B - 1] = 0.0  # the same batch with the dead row weighted out
    Lb = _learner(sdd, tsdd, batch=B, fresh_noise=False, train_features=tf)
    Lb.grad[:] = 7.0
    Lb.grads(*bd, isw=iw0)
    torch.cuda.synchronize()
    assert torch.equal(La.grad[:HEAD_OFF], Lb.grad[:HEAD_OFF])  # the dead row's feature gradient is zero
    assert not torch.equal(La.grad[HEAD_OFF:NPARAM], Lb.grad[HEAD_OFF:NPARAM])  # its head bias gradient is not
    if tf and B > 1:
        assert La.grad[:HEAD_OFF].abs().max() > 0


# ----------------------------------------------------------------------------- noise, determinism, split
def test_fresh_noise_is_the_fused_learners_draw(orc, nets):
    """PM_FOLD_TRAIN_FRESH: the epsilon buffers after an update are philox_noise(seed, TAG_NOISE_TRAIN,
    steps_before + 1), bit for bit, the step count read on the device, for two consecutive updates."""
    from pongmi.qnet import unpack_state_dict
    sd, tsd = nets
    batch, iw = _batch(np.random.RandomState(5), 64)
    L = _learner(sd, tsd, batch=64, fresh_noise=True, seed=0x1234567890, train_features=True)
    L.set_train_steps(41)
    for steps_before in (41, 42):
        L.update(*batch, isw=iw)
        torch.cuda.synchronize()
        fVi, fVo, fAi, fAo = orc.philox_noise(0x1234567890, orc.TAG_NOISE_TRAIN, steps_before + 1)
        got = unpack_state_dict(L.params)
        assert np.array_equal(_np(got["fc_V.weight_epsilon"]), np.outer(fVo, fVi))
        assert np.array_equal(_np(got["fc_V.bias_epsilon"]), fVo)
        assert np.array_equal(_np(got["fc_A.weight_epsilon"]), np.outer(fAo, fAi))
        assert np.array_equal(_np(got["fc_A.bias_epsilon"]), fAo)
        assert L.stats()["steps"] == steps_before + 1
    # and the update used that noise: its q is the train-mode forward of the block as it now stands
    from pongmi import _lib
    from pongmi.qnet import q_values
    L.desc.noise = _lib.PM_FOLD_TRAIN
    L.grads(*batch, isw=iw)
    q_same_eps = L.q.clone()
    L.set_train_steps(42)  # the draw of update 43 again: the noise now in the block
    L.desc.noise = _lib.PM_FOLD_TRAIN_FRESH
    L.grads(*batch, isw=iw)
    torch.cuda.synchronize()
    assert torch.equal(L.q, q_same_eps)
    assert torch.equal(L.q, q_values(L.acting_weights(_lib.PM_FOLD_TRAIN), torch.from_numpy(batch[0]).cuda()))


@pytest.mark.parametrize("tf", [0, 1])
def test_deterministic_and_split_equals_update(nets, tf):
    """The same inputs twice give the same bits; grads + apply equals update; two replicas summed by hand
    (grad += grad, the count becomes 2) then apply equals the one-replica result; nothing is written past
    td[batch] or grad's 5 200 floats, and rows past batch in s / ns / a / r / done / isw are never read."""
    sd, tsd = nets
    B = 33
    batch, iw = _batch(np.random.RandomState(9), B)

    def fresh(cap=B):
        return _learner(sd, tsd, batch=cap, fresh_noise=True, seed=7, train_features=tf, target_update_interval=2)

    def same(X, Y):
        return torch.equal(X.grad, Y.grad) and torch.equal(X.td[:B], Y.td[:B]) and torch.equal(X.params, Y.params) and \
            torch.equal(X.target, Y.target) and torch.equal(X.adam_m, Y.adam_m) and torch.equal(X.adam_v, Y.adam_v) and \
            X.stats() == Y.stats()

    A, Bb, C, D = fresh(), fresh(), fresh(), fresh()
    for _ in range(2):  # the second update syncs the target
        A.update(*batch, isw=iw)
        Bb.update(*batch, isw=iw)
        C.grads(*batch, isw=iw)
        C.apply()
        D.grads(*batch, isw=iw)
        D.grad += D.grad  # world 2 by hand: every rank holds the same gradient, the count sums to 2
        assert D.grad[NPARAM] == 2.0
        D.apply()
        D.grad[:NPARAM + 1] *= 0.5
    torch.cuda.synchronize()
    assert same(A, Bb), "two runs differ"
    assert same(A, C), "grads + apply differs from update"
    assert same(A, D), "two summed replicas differ from one"
    assert A.stats()["steps"] == 2 and torch.equal(A.target, A.params)
    # canaries: a learner with room for 256 rows fed 33, poison behind them, guard floats behind grad
    E = fresh(cap=256)
    big = torch.full((NPARAM + 8 + 64,), 123.0, device="cuda")
    E.grad = big[:NPARAM + 8]
    E.desc.grad = big.data_ptr()
    E.grad.zero_()
    for buf in (E.s, E.ns, E.rew, E.isw):
        buf.fill_(float("nan"))
    E.act.fill_(7)
    E.done.fill_(1)
    E.td.fill_(123.0)
    E.q.fill_(123.0)
    for _ in range(2):
        E.update(*batch, isw=iw)
    torch.cuda.synchronize()
    assert torch.equal(E.grad, A.grad) and torch.equal(E.td[:B], A.td[:B]) and torch.equal(E.params, A.params)
    assert torch.all(big[NPARAM + 8:] == 123.0) and torch.all(E.td[B:] == 123.0) and torch.all(E.q[B:] == 123.0)
    assert torch.isnan(E.s[B:]).all() and torch.isnan(E.ns[B:]).all()
    assert np.isfinite(E.stats()["loss"]) and E.stats() == A.stats()


# ----------------------------------------------------------------------------- a loop of one's own
def test_toy_loop_trains_the_whole_net(nets):
    """INTEGRATION.md's "your own loop" at 512 arenas for 20 vector steps with train_features=True: the loss
    stays finite, features.2.weight moves, and the trained block acts like the QNet module it unpacks to."""
    from models.qnet import QNet
    from pongmi._lib import PM_FOLD_EVAL, PM_FOLD_TRAIN_FRESH
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import act, fold, pack_state_dict, q_values
    from pongmi.replay import per_sample, per_update
    sd, tsd = nets
    env = PongEnv2PBatch(512, autoreset=True, seed=4)
    env.reset()
    L = _learner(sd, batch=256, train_features=True, seed=1, target_update_interval=8)
    wA = fold(pack_state_dict(tsd), PM_FOLD_EVAL)
    n, cap, dev = env.n, 8192, env.obsB.device
    S, NS = torch.zeros(cap, 7, device=dev), torch.zeros(cap, 7, device=dev)
    A, R = torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(cap, device=dev)
    D, prios, pos, size = torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(cap, device=dev), 0, 0
    w2_before = L.state_dict()["features.2.weight"].clone()
    losses = []
    for step in range(20):
        wB = L.acting_weights(PM_FOLD_TRAIN_FRESH, seed=1, counter=step)
        aA, aB = act(wA, None, wB, env.obsA, env.obsB, epsilon=0.1, seed=2, counter=step)
        s = env.obsB.clone()
        _, (_, rB), done, info = env.step(aA, aB)
        idx = (pos + torch.arange(n, device=dev)) % cap
        S[idx], A[idx], R[idx], NS[idx], D[idx] = s, aB.int(), rB, info["term_obsB"], done.to(torch.uint8)
        prios[idx] = prios.max() if size else 1.0
        pos, size = (pos + n) % cap, min(cap, size + n)
        bi, w = per_sample(prios, size, 256, beta=0.4, seed=3, counter=step)
        td = L.update(S[bi], A[bi], R[bi], NS[bi], D[bi], isw=w)
        per_update(prios, bi, td)
        losses.append(L.stats()["loss"])
    assert np.all(np.isfinite(losses)), losses
    st = L.stats()
    assert st["steps"] == 20 and st["adam_t"] == 20 and st["status"] == 0
    assert not torch.equal(L.state_dict()["features.2.weight"], w2_before)
    assert torch.equal(L.target, L.params) is False and torch.isfinite(L.params).all()
    x = S[:256].clone()
    net = QNet(7, 3)
    net.load_state_dict(L.state_dict())
    net.eval()
    with torch.no_grad():
        ref = net(x.cpu())
    got = q_values(L.acting_weights(PM_FOLD_EVAL), x).cpu()
    assert (got - ref).abs().max() < 2e-5
