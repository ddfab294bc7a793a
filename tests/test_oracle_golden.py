"""Pin the oracle (CPU restatement) against the reference's own outputs (tests/golden/*.npz,
generated from /root/reference by tests/golden/make_golden.py). CPU-only."""
import numpy as np
import pytest


def _param_values(g):
    return dict(zip([str(n) for n in g["param_names"]], g["param_values"].tolist()))


def _params(orc, g):
    vals = _param_values(g)
    return vals, orc.make_params(vals)


def test_collide_kat_bit_exact(orc, golden):
    g = golden("collide_kat")
    for row, exp in zip(g["inputs"], g["outputs"]):
        got = orc.collide(*row.tolist())
        assert np.array_equal(np.array(got), exp), (row, got, exp)
    # the +-0.0 vrel slide cases keep their sign through copysign
    assert np.array_equal(np.signbit(g["outputs"]), np.signbit(np.array([orc.collide(*r.tolist()) for r in g["inputs"]])))


def test_collide_div_bit_exact(orc, golden):
    """The collision over masses and radii whose reciprocals are inexact (m in {3, 0.7, 1.7, 0.1, 7,
    1e-3}, R in {0.03, 0.07, 0.0123, 0.5}: the divisions by m and I round), with the +-0 edge rows for
    m = 1 and m = 3: every output word and sign bit of the reference's."""
    g = golden("collide_div")
    assert {3.0, 0.7, 1.7, 0.1, 7.0, 1e-3} <= set(g["inputs"][:, 6].tolist()) and len(g["inputs"]) >= 4000
    got = np.array([orc.collide(*r.tolist()) for r in g["inputs"]])
    assert np.array_equal(got, g["outputs"])
    assert np.array_equal(np.signbit(got), np.signbit(g["outputs"]))
    assert np.any(np.signbit(g["outputs"]) & (g["outputs"] == 0))  # the table does hold a -0.0


ENV_SETS = ["cfg", "rnn", "default", "nospin", "wide", "heavy"]


@pytest.mark.parametrize("name", ENV_SETS)
def test_env_trajectories_bit_exact(orc, golden, name):
    """Oracle replays the reference trajectory: serves from a CPython-identical MT19937 stream
    seeded like random.seed(seed_i), steps with the recorded actions — every fp64 state word,
    every f32 obs, reward, done and score must be identical."""
    g = golden(f"env_{name}")
    pv, P = _params(orc, g)
    n, T = g["actA"].shape
    for i in range(n):
        mt = orc.MT(int(g["seeds"][i]))
        a = orc.new_arena(*mt.reset_draws(P))
        assert np.array_equal(orc.arena_state(a), g["init"][i])
        for t in range(T):
            oa, ob, r, d = orc.step(P, a, g["actA"][i, t], g["actB"][i, t])
            assert np.array_equal(orc.arena_state(a), g["state"][i, t]), (name, i, t)
            assert np.array_equal(oa, g["obsA"][i, t]) and np.array_equal(ob, g["obsB"][i, t])
            assert np.array_equal(r, g["rew"][i, t]) and d == bool(g["done"][i, t])
            if d:
                a = orc.new_arena(*mt.reset_draws(P))
                assert np.array_equal(orc.arena_state(a), g["reset_state"][i, t])
                oa, ob = orc.arena_obs(a)
                assert np.array_equal(oa, g["reset_obs"][i, t, 0]) and np.array_equal(ob, g["reset_obs"][i, t, 1])


def test_env_fixture_covers_edge_events(golden):
    """The trajectories must exercise stick and slide hits, speed-ups, misses with ghost play-on
    (scores keep counting after the first miss) and episode ends."""
    stick = sum(int(golden(f"env_{n}")["hits_stick"]) for n in ("cfg", "rnn", "default"))
    slide = sum(int(golden(f"env_{n}")["hits_slide"]) for n in ("cfg", "rnn", "default"))
    assert stick > 50 and slide > 20
    g = golden("env_cfg")
    assert g["done"].sum() > 20 and g["state"][..., 9].max() >= 5
    # the parameter-space fixtures: each ends episodes and hits paddles, `wide` (friction 0) slides,
    # `heavy` (friction 1.5) sticks
    for n in ("nospin", "wide", "heavy"):
        g = golden(f"env_{n}")
        assert g["done"].sum() >= 10, n
        assert int(g["hits_stick"]) + int(g["hits_slide"]) >= 1 and g["state"][..., 9].max() >= 1, n
    assert int(golden("env_wide")["hits_slide"]) > 0 and int(golden("env_heavy")["hits_stick"]) > 0
    # and each still holds what it is for
    pv = {n: _param_values(golden(f"env_{n}")) for n in ("nospin", "wide", "heavy")}
    assert pv["nospin"]["enable_spin"] == 0 and pv["nospin"]["magnus_factor"] != 0
    assert np.abs(golden("env_nospin")["state"][..., 4]).max() > 0  # spin is there, only its Magnus term is off
    w = golden("env_wide")["state"]  # both paddles clip at both walls
    assert w[..., 5].min() == 0.0 and w[..., 5].max() == 1.0 and w[..., 6].min() == 0.0 and w[..., 6].max() == 1.0
    assert pv["wide"]["friction"] == 0 and pv["wide"]["restitution"] < 1 and pv["wide"]["speed_increment"] < 0
    assert pv["heavy"]["ball_mass"] == 3.0 and pv["heavy"]["restitution"] > 1  # 1/3 is inexact; leftward, spinless serves
    assert np.all(golden("env_heavy")["init"][:, 2] < 0) and np.all(golden("env_heavy")["init"][:, 4] == 0)


def test_rollout_random_matches_reference_loop(orc, golden):
    """Config 1 (BASELINE.json configs[0]): random-vs-random loop on the CPython stream."""
    g = golden("rollout_random")
    for name in ("cfg", "rnn"):
        from oracle.oracle import env_params_from_kwargs
        import yaml, os
        cfgfile = {"cfg": "config.yaml", "rnn": "config_rnn.yaml"}[name]
        path = os.path.join(os.path.dirname(__file__), "..", "pingpong-selfplay-ai_amd", cfgfile)
        with open(path) as f:
            envkw = yaml.safe_load(f)["env"]
        P = orc.make_params(env_params_from_kwargs(**envkw))
        ep, ssum = orc.rollout_random(P, 0, int(g[f"{name}_steps"]))
        assert ep == int(g[f"{name}_episodes"]) and ssum == int(g[f"{name}_score_sum"])


def test_qnet_forward_matches_reference(orc, golden):
    g = golden("qnet")
    for who in ("modelB", "modelA"):
        sd = {k[len(who) + 1:]: v for k, v in g.items() if k.startswith(who + ".") and "q_" not in k}
        q_eval = orc.qnet_forward(orc.qnet_effective(sd, noisy=False), g["obs"])
        q_train = orc.qnet_forward(orc.qnet_effective(sd, noisy=True), g["obs"])
        np.testing.assert_allclose(q_eval, g[f"{who}.q_eval"], rtol=0, atol=2e-5)
        np.testing.assert_allclose(q_train, g[f"{who}.q_train"], rtol=0, atol=2e-5)
        gap = np.sort(q_eval, 1)
        clear = (gap[:, -1] - gap[:, -2]) > 1e-4
        assert np.array_equal(orc.argmax_first(q_eval)[clear], np.argmax(g[f"{who}.q_eval"], 1)[clear])


def test_noise_transform_matches_reference(orc, golden):
    g = golden("qnet")
    we, be = orc.noise_from_raw(g["noise.raw_in"], g["noise.raw_out"])
    assert np.array_equal(we, g["noise.weight_epsilon"]) and np.array_equal(be, g["noise.bias_epsilon"])


def test_per_matches_reference(orc, golden):
    g = golden("per")
    for ph in range(int(g["n_phases"])):
        u = 0
        while f"p{ph}.u{u}.idxs" in g:
            k = f"p{ph}.u{u}."
            idxs, w = orc.per_sample(g[k + "prios_before"], int(g[k + "size"]), 64, float(g[k + "beta"]),
                                     g[k + "uniforms"])
            assert np.array_equal(idxs, g[k + "idxs"])
            np.testing.assert_allclose(w, g[k + "weights"], rtol=1e-6)
            pr = g[k + "prios_before"].copy()
            orc.per_update(pr, g[k + "upd_idx"], g[k + "upd_err"])
            assert np.array_equal(pr, g[k + "prios_after"])
            u += 1


def test_dqn_steps_match_reference(orc, golden):
    g = golden("dqn_steps")
    sd = {k[5:]: v for k, v in g.items() if k.startswith("init.")}
    heads = orc.pack_heads(sd)
    target = heads.copy()
    m = np.zeros_like(heads)
    v = np.zeros_like(heads)
    for s in range(3):
        k = f"s{s}."
        eps = {kk[len(k) + 7:]: vv for kk, vv in g.items() if kk.startswith(k + "noiseB.")}
        res = orc.dqn_loss_grads(sd, heads, target, eps, g[k + "s"], g[k + "a"], g[k + "r"], g[k + "ns"],
                                 g[k + "d"], g[k + "iw"], 0.99)
        np.testing.assert_allclose(res["loss"], g[k + "loss"], rtol=2e-5)
        np.testing.assert_allclose(res["q"], g[k + "q"], atol=3e-5)
        np.testing.assert_allclose(res["targets"], g[k + "targets"], atol=3e-5)
        np.testing.assert_allclose(res["errors"], g[k + "errors"], atol=3e-5)
        np.testing.assert_allclose(res["grads"], g[k + "grads"], rtol=1e-4, atol=1e-6)
        heads, m, v = orc.adam_step(heads, res["grads"], m, v, s + 1, 2.5e-4)
        np.testing.assert_allclose(heads, g[k + "params_after"], rtol=3e-7, atol=2e-6)  # fp32 storage
        if (s + 1) % 2 == 0:
            target = heads.copy()
        np.testing.assert_allclose(target, g[k + "target_heads_after"], rtol=3e-7, atol=2e-6)


def test_rnn_forward_matches_reference(golden, orc):
    """QNetRNN restatement vs the reference module (act step, T=8 sequences, 12-step carry)."""
    g = golden("rnn")
    sd = {k[7:]: v for k, v in g.items() if k.startswith("params.")}
    for mode in ("train", "eval"):
        eff = orc.rnn_effective(sd, mode == "train")
        q, h, c = orc.rnn_forward(eff, g["act_x"], g["act_h0"][0], g["act_c0"][0])
        np.testing.assert_allclose(q, g[f"act_q_{mode}"], rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(h, g[f"act_h1_{mode}"][0], rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(c, g[f"act_c1_{mode}"][0], rtol=1e-4, atol=2e-6)
        z = np.zeros((16, 128))
        q, h, c = orc.rnn_forward(eff, g["seq_x"], z, z)
        np.testing.assert_allclose(q, g[f"seq_q_{mode}"], rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(h, g[f"seq_h_{mode}"][0], rtol=1e-4, atol=2e-6)
    eff = orc.rnn_effective(sd, True)
    h = c = np.zeros((16, 128))
    for t in range(12):
        q, h, c = orc.rnn_forward(eff, g["roll_x"][t][:, None, :], h, c)
        np.testing.assert_allclose(q, g["roll_q"][t], rtol=1e-4, atol=3e-6)
    np.testing.assert_allclose(c, g["roll_c"][0], rtol=1e-4, atol=3e-6)


def test_drqn_update_matches_reference(golden, orc):
    """The DRQN update restatement (hand-written BPTT + clip + Adam, float64) vs train_step_rnn run
    on the reference QNetRNN with torch autograd (tests/golden/drqn.npz)."""
    gr = golden("rnn")
    gd = golden("drqn")
    sd = {k[7:]: v.astype(np.float64) for k, v in gr.items() if k.startswith("params.")}
    target = dict(sd)
    batch = lambda k: tuple(gd[f"b{k}_{n}"] for n in ("obs", "act", "rew", "next", "done"))  # noqa: E731
    info = orc.drqn_grads(sd, target, *batch(0))
    np.testing.assert_allclose(info["q"], gd["u0_q"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(info["y"], gd["u0_target"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(info["loss"], gd["u0_loss"], rtol=1e-5)
    for k in orc.RNN_PARAM_KEYS:
        g = gd["u0_grad." + k]
        np.testing.assert_allclose(info["grads"][k], g, rtol=1e-3, atol=1e-5 * np.abs(g).max() + 1e-9, err_msg=k)
    adam = {}
    for k in range(3):
        sd, info = orc.drqn_update(sd, target, adam, k + 1, batch(k))
        np.testing.assert_allclose(info["loss"], gd[f"u{k}_loss"], rtol=1e-4)
        np.testing.assert_allclose(info["norm"], gd[f"u{k}_norm"], rtol=1e-4)
    for k in orc.RNN_PARAM_KEYS:
        np.testing.assert_allclose(np.ravel(sd[k])[::8], gd["final_sub." + k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_qnet_f32_order_restatement_matches_reference(orc, golden):
    """The float32 restatement of the device's evaluation order (what the GPU tests compare every
    action against) is itself a faithful QNet.forward: within float32 rounding of the reference's
    Q values, and equal argmax wherever the reference's top two Q differ by more than that rounding."""
    g = golden("qnet")
    for who in ("modelB", "modelA"):
        sd = {k[len(who) + 1:]: v for k, v in g.items() if k.startswith(who + ".") and "q_" not in k}
        for mode in ("eval", "train"):
            q = orc.qnet_forward_f32(orc.fold_heads_f32(sd, mode), g["obs"])
            ref = g[f"{who}.q_{mode}"]
            np.testing.assert_allclose(q, ref, rtol=0, atol=2e-5)
            gap = np.sort(ref, 1)
            clear = (gap[:, -1] - gap[:, -2]) > 4e-5
            assert np.array_equal(np.argmax(q, 1)[clear], np.argmax(ref, 1)[clear])


def test_per_tree_restatement_matches_reference(orc, golden):
    """The restatement of the device's sum-tree descent picks the reference's np.random.choice index
    on every draw of the golden PER fixture (the 2 draws that sit in the CDF rounding band included),
    and its IS weights equal the reference's."""
    g = golden("per")
    draws = 0
    for ph in range(int(g["n_phases"])):
        u = 0
        while f"p{ph}.u{u}.idxs" in g:
            k = f"p{ph}.u{u}."
            size = int(g[k + "size"])
            idx, w = orc.per_sample_tree(g[k + "prios_before"], size, size, float(g[k + "beta"]), g[k + "uniforms"])
            assert np.array_equal(idx, g[k + "idxs"])
            np.testing.assert_allclose(w / w.max(), g[k + "weights"], rtol=2e-6)
            draws += len(idx)
            u += 1
    assert draws >= 256


@pytest.mark.parametrize("size", [1, 1023, 1025, 4096, 200_000, 1_000_000, 1_048_577, 2_097_153])
def test_per_tree_restatement_vs_choice_outside_band(orc, size):
    """At every buffer size: the tree order and np.random.choice's float32-normalised CDF pick the same
    index for every uniform outside the CDF-boundary rounding band (per_boundary_band)."""
    rng = np.random.RandomState(size)
    pr = rng.uniform(0, 3, size).astype(np.float32)
    pr[rng.rand(size) < 0.1] = 0.0
    pr[0] = 0.5
    u = rng.random_sample(512)
    idx, _ = orc.per_sample_tree(pr, size, size, 0.5, u)
    ref, _ = orc.per_sample(pr, size, 512, 0.5, u)
    band = orc.per_boundary_band(pr, size, u)
    assert np.array_equal(idx[~band], ref[~band]) and np.all(pr[idx] > 0)


@pytest.mark.parametrize("alpha", [0.6, 0.4, 0.5, 1.0])
def test_det_pow_within_one_ulp_of_numpy_power(orc, alpha):
    """The PER leaf prio ** alpha (csrc/pm_per.h prio_pow, restated by oracle.det_pow_f32) against the
    reference's arithmetic, numpy's float32 power (scripts/train_iterative.py:67), over 1e-30 .. 1e30
    log-spaced (2e6 priorities): at most 1 ulp apart everywhere, and equal to the correctly rounded
    value (float64 pow rounded once to float32) on every input. Non-positive priorities give a 0 leaf
    (never sampled); a NaN priority gives a 0 leaf too, and the learner latches pm_ctrl.status bit 1
    (SelfPlayLearner.check_status raises), where numpy would propagate the NaN into the sample."""
    p = np.logspace(-30, 30, 2_000_001).astype(np.float32)
    d = orc.det_pow_f32(p, alpha)
    ref = np.power(p, np.float32(alpha))
    ulp = np.abs(d.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1
    exact = (p.astype(np.float64) ** np.float64(np.float32(alpha))).astype(np.float32)
    assert np.array_equal(d, exact)
    edge = orc.det_pow_f32(np.array([0.0, -1.0, np.nan], np.float32), alpha)
    assert np.array_equal(edge, np.zeros(3, np.float32))
