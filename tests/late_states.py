"""Late-training states for the self-play learner: priority layouts, ring geometries, counter
scenarios and Adam moments to inject into a SelfPlayLearner (numpy only: the host test of their
preconditions, tests/test_selfplay_late_host.py, and the GPU tests, tests/test_gpu_selfplay_late.py,
both import this module).

A state is a plain dict (build_state): `prios` float32 [cap] (0 past the filled part), `adam_m` /
`adam_v` float32 [520], and the control-block fields step, pos, size, train_steps, frame_idx, epsilon,
max_prio. `learner_kw` are the constructor arguments the scenario needs."""
import numpy as np

N_HEAD = 520
MASK64 = (1 << 64) - 1
LEARNER_SEED = 5  # the learners' seed: with a scenario's frame it fixes the first update's uniforms

# name -> (n, cap, pos, size): size == cap after a fill, except "partial" (36 slots stay empty after the push)
GEOMETRIES = {
    "wrap": (512, 2048, 1800, 2048),          # the push wraps the ring's end
    "ragged": (300, 1000, 777, 1000),         # cap no multiple of 64, n no multiple of 256
    "chunks69": (4096, 70_000, 69_000, 70_000),  # 69 chunks: past the level-2 search's stride of 64; wrapping push
    "partial": (512, 2048, 1500, 1500),       # the ring is not yet full
}

# name -> control-block fields and the learner's hyper-parameters
SCENARIOS = {
    # the next four updates see frames 99 998 .. 100 001: beta reaches 1.0 at frame 100 000 and is clamped
    # after it; train step 100 000 syncs the target, the three around it do not
    "beta_clamp": dict(ctrl=dict(step=99_997, train_steps=99_997, frame_idx=99_997, epsilon=0.3),
                       learner_kw=dict(beta_frames=100_000, target_update_interval=1000, epsilon=0.3)),
    # four steps cross the carry into the high word of all four Philox counters (TAG_ACT and
    # TAG_NOISE_ACT on step, TAG_PER on frame_idx + 1, TAG_NOISE_TRAIN on train_steps + 1)
    "counter_carry": dict(ctrl=dict(step=2 ** 32 - 2, train_steps=2 ** 32 - 3, frame_idx=2 ** 32 - 3, epsilon=0.3),
                          learner_kw=dict(beta_frames=100_000, target_update_interval=1000, epsilon=0.3)),
    # epsilon 0.0203 * 0.995^D falls below min_epsilon = 0.02 from D = 3 finished episodes on
    "eps_floor": dict(ctrl=dict(step=20_000, train_steps=20_000, frame_idx=20_000, epsilon=0.0203),
                      learner_kw=dict(beta_frames=100_000, target_update_interval=1000, epsilon=0.0203,
                                      min_epsilon=0.02)),
}

GIANT, TINY, ABSORBER = np.float32(1e4), np.float32(1e-6), np.float32(1e30)

# (layout, geometry) -> the builder's seed, chosen on the CPU (tests/test_selfplay_late_host.py asserts
# what each is for, under every scenario the GPU tests pair it with)
SEEDS = {(layout, geometry): 0 for layout in ("trained", "giants", "absorbing") for geometry in GEOMETRIES}
SEEDS[("giants", "wrap")] = 1  # seed 0 leaves no draw outside the push range under counter_carry


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def seed_env_of(seed, rank=0):
    """pongmi.dist.shard_seeds' env seed restated (the host test asserts they agree)."""
    return splitmix64((int(seed) * 0x100000001B3 + 1 + int(rank)) & MASK64)


def push_slots(n, cap, pos):
    """The ring slots of the coming push: [pos, pos + n) mod cap."""
    return (pos + np.arange(n)) % cap


def _log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def priorities(layout, geometry, seed):
    """float32 [cap] priorities of `layout` over the filled part [0, size) (0 past it)."""
    n, cap, pos, size = GEOMETRIES[geometry]
    rng = np.random.default_rng([seed, 1])
    pr = np.zeros(cap, np.float32)
    if layout in ("trained", "absorbing"):  # the spread |td| + 1e-6 produces
        pr[:size] = _log_uniform(rng, 1e-6, 1e2, size).astype(np.float32)
    if layout == "giants":  # the pending push at max_prio ** alpha carries almost all of the mass
        pr[:size] = TINY
        pr[rng.choice(size, max(4, cap // 500), replace=False)] = GIANT
    if layout == "absorbing":
        # three entries whose fp64 leaf sums absorb their neighbours: one in the last 1024-entry chunk
        # of the filled part, one inside the coming push range, one anywhere else; the first and the
        # last outside the push range, so the draw meets them as stored leaves
        slots = push_slots(n, cap, pos)
        free = np.setdiff1d(np.arange(size), slots)
        last = free[free >= (size - 1) // 1024 * 1024]
        if last.size == 0:  # the push covers the whole last chunk ("chunks69")
            last = np.arange((size - 1) // 1024 * 1024, size)
        a = int(rng.choice(last))
        b = int(rng.choice(slots))
        c = int(rng.choice(free[free != a]))
        pr[[a, b, c]] = ABSORBER
    if layout not in ("trained", "giants", "absorbing"):
        raise ValueError(layout)
    return pr


def adam_moments(seed):
    """Resumed optimiser moments: v = exp(U(ln 1e-16, ln 1e-2)), m = s * sqrt(v) * U(0, 1) with random
    signs s, so sqrt(v) runs from adam_eps = 1e-8, where eps is half of Adam's denominator, up to 0.1,
    where it is nothing. float32 [520] each."""
    return adam_moments_of(N_HEAD, seed)


def adam_moments_of(count, seed):
    rng = np.random.default_rng([seed, 2])
    v = _log_uniform(rng, 1e-16, 1e-2, count).astype(np.float32)
    s = np.where(rng.random(count) < 0.5, -1.0, 1.0)
    m = (s * np.sqrt(v.astype(np.float64)) * rng.random(count)).astype(np.float32)
    return m, v


def build_state(layout, geometry, scenario, seed=None):
    """The arrays and counters to inject: see the module docstring."""
    n, cap, pos, size = GEOMETRIES[geometry]
    seed = SEEDS[(layout, geometry)] if seed is None else seed
    pr = priorities(layout, geometry, seed)
    m, v = adam_moments(seed)
    ctrl = dict(SCENARIOS[scenario]["ctrl"])
    ctrl.update(pos=pos, size=size, max_prio=float(pr.max()))
    return dict(layout=layout, geometry=geometry, scenario=scenario, n=n, cap=cap, prios=pr, adam_m=m, adam_v=v,
                ctrl=ctrl, learner_kw=dict(SCENARIOS[scenario]["learner_kw"]))


def seen_priorities(state):
    """The priorities the first update's draw sees: the pending push substituted at max_prio, and the
    fill after it. Returns (prios float32 [cap], size)."""
    c = state["ctrl"]
    pr = state["prios"].copy()
    pr[push_slots(state["n"], state["cap"], c["pos"])] = np.float32(c["max_prio"])
    return pr, min(c["size"] + state["n"], state["cap"])


def first_uniforms(orc, state, batch, learner_seed=LEARNER_SEED, updates_ahead=0):
    """The uniforms of update `updates_ahead` after the injection: philox64(j, TAG_PER, frame, seed_env)."""
    frame = state["ctrl"]["frame_idx"] + 1 + updates_ahead
    r = orc.philox64(np.arange(batch), orc.TAG_PER, np.full(batch, frame, np.uint64), seed_env_of(learner_seed))
    return orc.u53(r[0], r[1])


def beta_of(frame, beta_start=0.4, beta_frames=100_000):
    """train_iterative.py:137: min(1, beta_start + frame * (1 - beta_start) / beta_frames), in the
    library's order of operations."""
    return min(1.0, beta_start + float(frame) * (1.0 - beta_start) / float(beta_frames))


def first_draw(orc, state, batch, learner_seed=LEARNER_SEED):
    """The oracle's first draw from the injected state: (idx, inside the push range, fallback mask)."""
    pr, size = seen_priorities(state)
    u = first_uniforms(orc, state, batch, learner_seed)
    beta = beta_of(state["ctrl"]["frame_idx"] + 1, beta_frames=state["learner_kw"]["beta_frames"])
    idx, _, fell = orc.per_sample_tree(pr, size, state["cap"], beta, u, want_fallback=True)
    inside = (idx - state["ctrl"]["pos"]) % state["cap"] < state["n"]
    return idx, inside, fell


def absorbed_nodes(orc, state):
    """How many level-1 nodes of the tree the first draw descends (oracle.per_tree on seen_priorities)
    hold an absorber beside smaller nonzero leaves and have lost part of those leaves to rounding: the
    node's fp64 sum less its absorbers differs from the other leaves' own sum by more than a quarter."""
    pr, _ = seen_priorities(state)
    _, sub, leaf = orc.per_tree(pr, state["cap"])
    top = leaf.max()
    lf = np.zeros(sub.shape[0] * 64)
    lf[:state["cap"]] = leaf.astype(np.float64)
    lf = lf.reshape(-1, 64)
    k = (lf == float(top)).sum(1)
    others = np.where(lf == float(top), 0.0, lf).sum(1)
    rest = sub - k * float(top)
    return int(((k > 0) & (others > 0) & (np.abs(rest - others) > 0.25 * others)).sum())


def check_preconditions(orc, state, batch, learner_seed=LEARNER_SEED):
    """What a layout is for, asserted from the builders and the oracle alone (no device value):
      trained    the first update draws inside the coming push range and outside it;
      giants     at least 90 % of its draws lie inside the push range, at least one outside;
      absorbing  the tree holds nodes whose fp64 sums have absorbed their small leaves, and draws fall
                 inside the push range (substituted at 1e30) -- see tests/test_selfplay_late_host.py on
                 the `last nonzero child' rule, which no Philox draw of this layout reaches.
    Returns (draws inside the push range, draws with a nonzero fallback mask)."""
    idx, inside, fell = first_draw(orc, state, batch, learner_seed)
    n_in, what = int(inside.sum()), (state["layout"], state["geometry"], state["scenario"])
    assert np.all((idx >= 0) & (idx < min(state["ctrl"]["size"] + state["n"], state["cap"]))), what
    assert state["ctrl"]["max_prio"] == state["prios"].max(), what
    if state["layout"] == "trained":
        assert 1 <= n_in <= batch - 1, (what, n_in)
    elif state["layout"] == "giants":
        assert 0.9 * batch <= n_in <= batch - 1, (what, n_in)
    else:
        assert absorbed_nodes(orc, state) >= 1 and n_in >= 1, what
    return n_in, int((fell != 0).sum())
