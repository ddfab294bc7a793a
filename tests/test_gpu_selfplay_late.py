"""The self-play learner from late-training states (tests/late_states.py): a learner is put into the
state by pm_selfplay_prepare's documented way in (overwrite priorities, Adam moments and the control
block, then prepare()), and the machinery of tests/test_gpu_selfplay.py judges what follows: the split
path against the oracle, the fast paths against the split path bit for bit.

What a fresh learner never shows and these states do: beta at and past its clamp, a target sync at
train step 100 000, Adam's bias corrections near 1 on moments whose sqrt(v) reaches down to adam_eps,
the Philox counters' carry into their high words, epsilon on its floor, and priority layouts (a
trained spread, a few giants, 1e30 entries that absorb their neighbours' sums) with a pending push
whose substituted value differs from every stored leaf, over rings that wrap, are no multiple of a
node, span 69 chunks or are not yet full."""
import numpy as np
import pytest
import torch

import late_states as ls
from test_gpu_selfplay import (_assert_same, _assert_tree_equals_rebuild, _check_per, _check_rollout, _check_update,
                               _drive_split, _learner, _snap)

pytestmark = pytest.mark.gpu

BATCH = 256
SYNC = 1000
EPS_WARM = 6  # eps_floor: plain steps before the injection, so that the first episodes end in the compared steps


def _set_ctrl(L, **fields):
    from pongmi import _lib
    c = _lib.Ctrl.from_buffer_copy(bytes(L.ctrl.cpu().numpy().tobytes()))
    for k, v in fields.items():
        setattr(c, k, v)
    L.ctrl.copy_(torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8))


def _inject(L, state, warm=0):
    """Put `L` into `state`: plain steps until every replay row the state can reach is a real
    transition (cap // n + 2 for a full ring, the pushes that cover [0, size) for the partial one; `warm`
    more where a test wants the arenas further into their episodes), then the state's priorities, Adam
    moments and control fields, then prepare() (sum tree from prios and ctrl, both noises from ctrl)."""
    n, cap = state["n"], state["cap"]
    assert (L.n, L.cap) == (n, cap)
    size = state["ctrl"]["size"]
    fill = cap // n + 2 if size == cap else -(-size // n)
    for _ in range(fill + warm):
        L.rollout()
        L.learn()
        L.apply()
    c = L.counters()
    assert c["status"] == 0 and c["size"] >= size
    L.prios.copy_(torch.from_numpy(state["prios"]))
    L.adam_m.copy_(torch.from_numpy(state["adam_m"]))
    L.adam_v.copy_(torch.from_numpy(state["adam_v"]))
    _set_ctrl(L, **state["ctrl"])
    L.prepare()
    torch.cuda.synchronize()
    got = L.counters()
    assert all(got[k] == (np.float32(v) if k == "max_prio" else v) for k, v in state["ctrl"].items()), got
    return L


def _make(golden, state, warm=0, batch=BATCH, **kw):
    return _inject(_learner(golden, n=state["n"], batch=batch, cap=state["cap"], seed=ls.LEARNER_SEED,
                            **state["learner_kw"], **kw), state, warm)


def _adam_of(state):
    return dict(m=state["adam_m"].astype(np.float64), v=state["adam_v"].astype(np.float64),
                t=state["ctrl"]["train_steps"])


def _state(orc, layout, geometry, scenario):
    """The state, with its preconditions re-asserted from the oracle's numbers."""
    st = ls.build_state(layout, geometry, scenario)
    n_in, _ = ls.check_preconditions(orc, st, BATCH)
    print(f"{layout} {geometry} {scenario}: oracle puts {n_in} of {BATCH} first draws inside the push range")
    return st


def _check_act_noise(orc, L, ctr):
    """w_B's head part = mu + sigma * eps with eps the fold of philox_noise(seed_net, TAG_NOISE_ACT, ctr)
    (test_fold_fresh_noise_matches_restatement's restatement), ctr the vector step the weights act in:
    gen_both_noises is keyed by ctrl.step in prepare and by step + 1 in the apply that ends a step."""
    from pongmi.qnet import unpack_state_dict
    sd = {k: v.numpy() for k, v in unpack_state_dict(L.paramsB).items()}
    fVi, fVo, fAi, fAo = orc.philox_noise(L.sp.seed_net, orc.TAG_NOISE_ACT, ctr)
    w = L.w_B.cpu().numpy()
    expV = sd["fc_V.weight_mu"] + sd["fc_V.weight_sigma"] * np.outer(fVo, fVi).astype(np.float32)
    expA = sd["fc_A.weight_mu"] + sd["fc_A.weight_sigma"] * np.outer(fAo, fAi).astype(np.float32)
    assert np.array_equal(w[4672:4736].reshape(1, 64), expV.astype(np.float32)), ctr
    assert np.array_equal(w[4736:4928].reshape(3, 64), expA.astype(np.float32)), ctr
    assert np.array_equal(w[4928:4929], sd["fc_V.bias_mu"] + sd["fc_V.bias_sigma"] * fVo), ctr
    assert np.array_equal(w[4929:4932], sd["fc_A.bias_mu"] + sd["fc_A.bias_sigma"] * fAo), ctr


def _split_step(orc, L, adam, figs, **kw):
    """One vector step of the split path, every part against the oracle. Returns the rollout's counts
    and the counters the update found."""
    pre = _snap(L)
    L.rollout()
    post = _snap(L)
    cnt = _check_rollout(orc, L, pre, post)
    _check_update(orc, L, post["ctrl"], post, "single", adam, sync=SYNC, loss_figs=figs, **kw)
    return cnt, post["ctrl"]


def _print_figs(what, figs):
    print(f"{what}: loss vs float64, worst update: device {max(d for d, _ in figs):.2e}, "
          f"reference float32 {max(r for _, r in figs):.2e} (relative)")


# ------------------------------------------------------------------ 3. the split path against the oracle
@pytest.mark.parametrize("scenario", list(ls.SCENARIOS))
def test_counter_scenarios_match_oracle(orc, golden, scenario):
    """Layout `trained` on the wrapping ring, four vector steps of rollout / learn / apply, every check
    of test_learn_and_apply_match_oracle (kind "single") and the rollout's.
      beta_clamp     frames 99 998 .. 100 001: the IS weights follow beta < 1 for two updates and are
                     (size P)^-1 exactly afterwards; train step 100 000 syncs the target, the others leave it;
      counter_carry  step, frame_idx + 1 and train_steps + 1 cross 2^32: the epsilon-greedy draws (TAG_ACT),
                     the PER uniforms (TAG_PER) and the update's noise (TAG_NOISE_TRAIN) are checked by the
                     oracle machinery with 64-bit counters, the acting noise (TAG_NOISE_ACT) here;
      eps_floor      epsilon 0.0203 follows the oracle's eps * 0.995^D until 0.995^D takes it below
                     min_epsilon (three finished episodes), is exactly 0.02 from that step on. EPS_WARM
                     more plain steps before the injection bring the first episodes' ends into the four
                     compared steps: the oracle's env tick finishes 0, 1, 12 and 15 of the 512 arenas'
                     episodes, so epsilon stays, decays once above the floor, meets it, and stays on it."""
    st = _state(orc, "trained", "wrap", scenario)
    L = _make(golden, st, warm=EPS_WARM if scenario == "eps_floor" else 0, fuse_apply=False, overlap=False)
    adam, figs = _adam_of(st), []
    c0 = st["ctrl"]
    if scenario == "counter_carry":
        _check_act_noise(orc, L, c0["step"])
    eps, floor_at, decayed_above = c0["epsilon"], None, 0
    for k in range(4):
        cnt, c = _split_step(orc, L, adam, figs)
        after = L.counters()
        frame = c["frame_idx"] + 1
        assert frame == c0["frame_idx"] + 1 + k and after["step"] == c0["step"] + 1 + k
        if scenario == "beta_clamp":
            beta = ls.beta_of(frame)
            assert (beta < 1.0) == (frame < 100_000) and (beta == 1.0) == (frame >= 100_000)
        if scenario == "counter_carry":
            _check_act_noise(orc, L, after["step"])
        if scenario == "eps_floor":
            raw = eps * 0.995 ** cnt["fin"]  # the oracle's decay over the episodes its own env tick finished
            if raw > 0.02:
                assert floor_at is None and after["epsilon"] > 0.02
                decayed_above += cnt["fin"] > 0
            else:
                floor_at = k if floor_at is None else floor_at
                assert after["epsilon"] == 0.02  # exactly
            eps = max(0.02, raw)
            print(f"eps_floor step {k}: {cnt['fin']} episodes finished, epsilon {after['epsilon']!r}")
    if scenario == "eps_floor":
        # preconditions, from the oracle's counts: a decay that stays above the floor, then the floor, then a
        # step that has to stay on it
        assert decayed_above >= 1 and floor_at is not None and floor_at < 3, (decayed_above, floor_at)
    if scenario == "beta_clamp":
        assert (st["ctrl"]["train_steps"] + 3) % SYNC == 0  # the third update synced (checked in _check_update)
    _print_figs(f"trained wrap {scenario}", figs)
    assert L.counters()["status"] == 0
    _assert_tree_equals_rebuild(L)


@pytest.mark.parametrize("geometry", list(ls.GEOMETRIES))
@pytest.mark.parametrize("layout", ["trained", "giants"])
def test_layouts_and_geometries_match_oracle(orc, golden, layout, geometry):
    """Layouts `trained` and `giants` at every ring geometry under beta_clamp, two vector steps each:
    the first draw sees the injected layout with the pending push substituted at its max_prio (for
    `giants` nearly the whole mass), the second what the first update's scatter left."""
    st = _state(orc, layout, geometry, "beta_clamp")
    L = _make(golden, st, fuse_apply=False, overlap=False)
    adam, figs = _adam_of(st), []
    for k in range(2):
        _split_step(orc, L, adam, figs)
        if geometry == "partial" and k == 0:  # the 36 slots past the first push are still empty
            c = L.counters()
            assert c["size"] == c["pos"] == 2012 and not L.prios[2012:].any().item()
    _print_figs(f"{layout} {geometry} beta_clamp", figs)
    c = L.counters()
    assert c["status"] == 0 and c["train_steps"] == st["ctrl"]["train_steps"] + 2
    _assert_tree_equals_rebuild(L)


def test_multi_update_step_across_clamp_and_sync(orc, golden):
    """U = 3 from beta_clamp: the first vector step's updates see frames 99 998, 99 999 and 100 000, so
    beta reaches its clamp and train step 100 000 syncs the target between updates of one step; the
    second step's run past both. Every update as test_multi_update_step_matches_oracle (kind "multi");
    after each commit max_prio is the array maximum and the sum tree equals a rebuild bit for bit."""
    from pongmi import _lib
    U = 3
    st = _state(orc, "trained", "wrap", "beta_clamp")
    L = _make(golden, st, fuse_apply=False, overlap=False, updates_per_step=U)
    adam, figs = _adam_of(st), []
    for step in range(2):
        c0 = L.counters()
        L.rollout()
        for u in range(U):
            mode = _lib.PM_UPD_FIRST if u == 0 else 0
            if u:
                L.resample()
            pre = _snap(L)
            c = pre["ctrl"]
            assert c["step"] == c0["step"] and c["pos"] == c0["pos"]
            assert c["frame_idx"] == c["train_steps"] == adam["t"] == st["ctrl"]["train_steps"] + step * U + u
            _check_update(orc, L, c, pre, "multi", adam, u=u, mode=mode, sync=SYNC, loss_figs=figs)
            synced = torch.equal(L.paramsT[:5192], L.paramsB[:5192])
            assert synced == ((step, u) == (0, 2)), (step, u)
        L.commit()
        torch.cuda.synchronize()
        c = L.counters()
        assert c["max_prio"] == L.prios.cpu().numpy().max() and c["max_bits"] == 0
        assert c["step"] == c0["step"] + 1 and c["pos"] == (c0["pos"] + L.n) % L.cap and c["status"] == 0
        _assert_tree_equals_rebuild(L)
    _print_figs("trained wrap beta_clamp U = 3", figs)


@pytest.mark.parametrize("geometry", list(ls.GEOMETRIES))
def test_absorbing_layout_draw_matches_oracle(orc, golden, geometry):
    """Layout `absorbing` (three 1e30 entries, the push substituted at 1e30): only the draw is checked,
    every index exact and every weight to one float32 ulp (_check_per); a loss whose weights span 1e18^beta
    is not a conditioned quantity. Two vector steps: the second draws after the first scatter has
    replaced the sampled absorbers."""
    st = _state(orc, "absorbing", geometry, "beta_clamp")
    L = _make(golden, st, fuse_apply=False, overlap=False)
    for k in range(2):
        L.rollout()
        snap = _snap(L)
        c = snap["ctrl"]
        L.learn()
        torch.cuda.synchronize()
        frame = c["frame_idx"] + 1
        size = min(c["size"] + L.n, L.cap)
        r = orc.philox64(np.arange(BATCH), orc.TAG_PER, np.full(BATCH, frame, np.uint64), L.sp.seed_env)
        idx = L.idx.cpu().numpy()
        if k == 0:  # the oracle's draw from the builders alone is the device's
            assert np.array_equal(idx, ls.first_draw(orc, st, BATCH)[0])
        _check_per(orc, snap["prios"], size, L.cap, ls.beta_of(frame), orc.u53(r[0], r[1]), idx, L.isw.cpu().numpy())
        L.apply()
    c = L.counters()
    assert c["status"] == 0 and c["train_steps"] == st["ctrl"]["train_steps"] + 2
    _assert_tree_equals_rebuild(L)


# ------------------------------------------------------ 4. the fast paths against the split path, bit for bit
FAST_U1 = [(lay, "wrap", sc) for lay in ("trained", "giants", "absorbing")
           for sc in ("beta_clamp", "counter_carry")] + \
          [("trained", geo, "beta_clamp") for geo in ("ragged", "chunks69", "partial")]


@pytest.mark.parametrize("layout,geometry,scenario", FAST_U1)
def test_production_step_equals_split_from_late_state(orc, golden, layout, geometry, scenario):
    """Twin learners from one injection: A's production step() (k_actenv's sampler blocks with the
    straight-line level 0, k_learn with side blocks, fused Adam, actions ahead) equals B's rollout /
    learn / apply after each of 6 steps: every array and counter of _assert_same."""
    st = _state(orc, layout, geometry, scenario)
    A = _make(golden, st)
    B = _make(golden, st, overlap=False, fuse_apply=False)
    _assert_same(A, B)  # byte-identical injections
    for k in range(6):
        A.step()
        B.rollout()
        B.learn()
        B.apply()
        _assert_same(A, B)
        assert A.counters()["status"] == 0, k
    c = A.counters()
    assert c["train_steps"] == st["ctrl"]["train_steps"] + 6 and c["step"] == st["ctrl"]["step"] + 6
    _assert_tree_equals_rebuild(A)


@pytest.mark.parametrize("layout", ["trained", "giants", "absorbing"])
def test_learn_multi_equals_split_from_late_state(orc, golden, layout):
    """U = 4 under beta_clamp: updates 1..3 of a step as one k_learn_multi launch (its descent with the
    tree's top level in LDS, the clamp, the sync and the epsilon floor's select inside the launch)
    against _drive_split (k_resample + learn_ex + apply_ex per update). prepare() makes k_learn_multi
    wait for a turn of the ring: cap // n + 5 steps, of which at least three compared ones ran it."""
    U = 4
    st = _state(orc, layout, "wrap", "beta_clamp")
    A = _make(golden, st, updates_per_step=U)
    B = _make(golden, st, updates_per_step=U, fuse_apply=False, overlap=False)
    assert A.frow is not None and B.frow is None
    _assert_same(A, B)
    ready = 0
    steps = st["cap"] // st["n"] + 5
    for k in range(steps):
        A.step()
        _drive_split(B, U)
        ready += A.sp.frow_ready == 1
        _assert_same(A, B)
        assert A.counters()["status"] == 0, k
    assert ready >= 3, ready
    assert A.counters()["train_steps"] == st["ctrl"]["train_steps"] + steps * U
    _assert_tree_equals_rebuild(A)


# ------------------------------------------------------------------------------------ 5. related checks
def test_running_max_prio_is_the_array_maximum(golden):
    """with one update per step the running max_prio equals max(prios) exactly (n > batch
    pushes at the old maximum survive every scatter). 40 production steps from a fresh learner: ten
    turns of the ring."""
    L = _learner(golden, n=512, batch=256, cap=2048, seed=ls.LEARNER_SEED, epsilon=0.5)
    for k in range(40):
        L.step()
        torch.cuda.synchronize()
        c = L.counters()
        assert c["max_prio"] == L.prios[:c["size"]].max().item(), k
    assert c["size"] == 2048 and c["step"] == 40 and c["status"] == 0


RESUMED_T = 50_000  # Adam's step count of the loaded optimiser state: both bias corrections round to 1


def test_dqn_learner_resumes_optimizer_state(orc, golden):
    """DQNLearner over the whole net: an Adam state of 50 000 steps with late_states' moments loaded
    through load_optimizer_state_dict, then two updates at batch 64 with interval 2 (the second syncs
    the target). Gradients against float64 at test_gpu_dqn.py's bars (heads rtol 2e-4 / atol
    2e-6 x 256 / B, features the conditioned bar), loss rtol 1e-4, and Adam from the loaded moments at
    step 50 001 / 50 002 against oracle.adam_step at rtol 1e-5 / atol 1e-7."""
    import test_gpu_dqn as dq
    from pongmi.checkpoint import adam_state_dict
    from pongmi.dqn import ALL_SHAPES
    from pongmi.qnet import pack_state_dict, unpack_state_dict
    B, NP, HO = 64, dq.NPARAM, dq.HEAD_OFF
    sd = dq._init_sd(golden("dqn_full_steps"))
    tblk = pack_state_dict(sd, "cpu")
    tblk[HO:NP] += 0.05 * torch.randn(NP - HO, generator=torch.Generator().manual_seed(8))  # Q_T is not Q_B
    L = dq._learner(sd, unpack_state_dict(tblk), batch=B, target_update_interval=2, fresh_noise=False,
                    train_features=True)
    m, v = ls.adam_moments_of(NP, 4)
    L.load_optimizer_state_dict(adam_state_dict(ALL_SHAPES, torch.from_numpy(m), torch.from_numpy(v), RESUMED_T, dq.LR))
    assert L.stats()["adam_t"] == RESUMED_T
    assert np.array_equal(dq._np(L.adam_m)[:NP], m) and np.array_equal(dq._np(L.adam_v)[:NP], v)
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    for k in range(2):
        what = f"resumed whole-net update {k}"
        cur, tcur = L.state_dict(), L.target_state_dict()
        batch, iw = dq._conditioned_batch(cur, tcur, B, 500 + k)
        p0, t0 = dq._np(L.params)[:NP].astype(np.float64), L.target.clone()
        L.update(*batch, isw=iw)
        torch.cuda.synchronize()
        r64, r32 = dq._autograd(cur, tcur, batch, iw, torch.float64), dq._autograd(cur, tcur, batch, iw, torch.float32)
        grad = dq._np(L.grad)
        np.testing.assert_allclose(grad[HO:NP], r64["grads"][HO:], rtol=2e-4, atol=2e-6 * 256 / B, err_msg=what)
        for name, lo, hi in dq.FEATS:
            ref = r64["grads"][lo:hi]
            mx, e32 = np.abs(ref).max(), np.abs(r32["grads"][lo:hi] - ref).max()
            print(f"{what}: {name}: device {np.abs(grad[lo:hi] - ref).max() / mx:.2e}, "
                  f"reference f32 {e32 / mx:.2e} x max|g|")
            np.testing.assert_allclose(grad[lo:hi], ref, rtol=dq.GRAD_RTOL, atol=max(1e-5 * mx, dq.REF32_FACTOR * e32),
                                       err_msg=f"{what}: {name}")
        st = L.stats()
        np.testing.assert_allclose(st["loss"], r64["loss"], rtol=1e-4, err_msg=what)
        assert st["steps"] == k + 1 and st["adam_t"] == RESUMED_T + k + 1 and st["status"] == 0
        p_ref, m64, v64 = orc.adam_step(p0, grad[:NP].astype(np.float64), m64, v64, RESUMED_T + k + 1, dq.LR)
        np.testing.assert_allclose(dq._np(L.params)[:NP], p_ref, rtol=1e-5, atol=1e-7, err_msg=what)
        np.testing.assert_allclose(dq._np(L.adam_m)[:NP], m64, rtol=1e-5, atol=1e-6 * np.abs(m64).max(), err_msg=what)
        np.testing.assert_allclose(dq._np(L.adam_v)[:NP], v64, rtol=1e-5, atol=1e-6 * np.abs(v64).max(), err_msg=what)
        if k == 0:
            assert torch.equal(L.target, t0), "the first update must leave the target"
        else:
            assert torch.equal(L.target[:NP], L.params[:NP]), "the second update syncs the target"


def test_drqn_learner_resumes_optimizer_state(orc, golden):
    """DRQNLearner at batch 64, T = 8: the same loaded Adam state, two updates with interval 2, each as
    test_gpu_drqn.py's _check_update: loss rtol 1e-4, gradients at the conditioned bar, clip + Adam at
    step 50 001 / 50 002 bit for bit against oracle.clip_adam_f32 from the loaded moments."""
    import test_gpu_drqn as dr
    from pongmi.checkpoint import adam_state_dict
    from pongmi.drqn import PARAM_SHAPES, DRQNLearner
    B, T = 64, 8
    sd = dr._np_sd(golden)
    rng = np.random.default_rng(B * 100 + T + 7)
    tsd = dr._perturbed(sd, rng)
    L = DRQNLearner(dr._tt(sd), dr._tt(tsd), batch=B, T=T, target_update_interval=2)
    count = sum(int(np.prod(s)) for s in PARAM_SHAPES)
    m, v = ls.adam_moments_of(count, 6)
    L.load_optimizer_state_dict(adam_state_dict(PARAM_SHAPES, torch.from_numpy(m), torch.from_numpy(v), RESUMED_T,
                                                L.desc.lr))
    assert L.stats()["adam_t"] == RESUMED_T
    assert np.array_equal(L.adam_m.cpu().numpy(), m) and np.array_equal(L.adam_v.cpu().numpy(), v)
    t0 = L.target.clone()
    for k in range(2):
        batch = dr._rand_batch(np.random.default_rng(90000 + 31 * k + B * 100 + T), B, T)
        dr._check_update(L, orc, tsd, batch, RESUMED_T + k + 1, f"resumed DRQN update {k}")
        st = L.stats()
        assert st["steps"] == k + 1 and st["adam_t"] == RESUMED_T + k + 1
        if k == 0:
            assert torch.equal(L.target, t0), "the first update must leave the target"
        else:
            assert torch.equal(L.params, L.target), "the second update syncs the target"
