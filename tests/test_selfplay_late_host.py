"""The late-state builders (tests/late_states.py) do what they are for: checked on the host from the
builders and the oracle's sum-tree restatement alone, so the GPU tests of tests/test_gpu_selfplay_late.py
start from inputs whose properties do not hang on a device value."""
import numpy as np
import pytest

import late_states as ls

BATCH = 256
LAYOUTS = ("trained", "giants", "absorbing")
# every (layout, geometry, scenario) the GPU tests inject
CASES = sorted({(lay, "wrap", sc) for lay in LAYOUTS for sc in ls.SCENARIOS} |
               {(lay, geo, "beta_clamp") for lay in LAYOUTS for geo in ls.GEOMETRIES})


def test_seed_env_restatement_is_the_librarys():
    from pongmi.dist import shard_seeds
    for seed in (0, 5, 21, 2 ** 40 + 3):
        assert ls.seed_env_of(seed) == shard_seeds(seed, 0)[0]


@pytest.mark.parametrize("geometry", list(ls.GEOMETRIES))
def test_geometries_are_the_edges_they_name(geometry):
    n, cap, pos, size = ls.GEOMETRIES[geometry]
    slots = ls.push_slots(n, cap, pos)
    assert len(set(slots.tolist())) == n and size <= cap and pos <= size
    if geometry == "wrap":
        assert pos + n > cap and size == cap
    if geometry == "ragged":
        assert cap % 64 and n % 256 and size == cap
    if geometry == "chunks69":
        assert (cap + 1023) // 1024 == 69 > 64 and pos + n > cap and size == cap
    if geometry == "partial":
        assert size == pos < cap and cap - (size + n) == 36


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geometry", list(ls.GEOMETRIES))
def test_layouts_are_what_they_say(layout, geometry):
    n, cap, pos, size = ls.GEOMETRIES[geometry]
    st = ls.build_state(layout, geometry, "beta_clamp")
    pr = st["prios"]
    assert pr.dtype == np.float32 and pr.shape == (cap,) and np.all(pr[:size] > 0)
    past = np.flatnonzero(pr[size:]) + size  # only `absorbing`'s entry inside a push range that lies past the fill
    assert past.size == 0 or (layout == "absorbing" and past.size == 1 and (past[0] - pos) % cap < n)
    assert st["ctrl"]["max_prio"] == pr.max() and st["ctrl"]["pos"] == pos and st["ctrl"]["size"] == size
    assert np.array_equal(pr, ls.build_state(layout, geometry, "counter_carry")["prios"])  # twins: same bytes
    small = pr[:size][pr[:size] < 1e29]
    if layout == "giants":
        assert (pr == ls.GIANT).sum() == max(4, cap // 500) and np.all(small[small < 1e3] == ls.TINY)
    else:
        assert small.min() >= np.float32(1e-6) and small.max() <= np.float32(1e2)
        assert small.min() < 1e-5 and small.max() > 10  # the whole spread is there
    if layout == "absorbing":
        at = np.flatnonzero(pr == ls.ABSORBER)
        inside = (at - pos) % cap < n
        assert len(at) == 3 and inside.any() and (at >= (size - 1) // 1024 * 1024).any()
        if geometry != "chunks69":  # there the push covers the whole last chunk
            assert (~inside).sum() == 2  # two are met as stored leaves


def test_adam_moments_reach_down_to_eps():
    """sqrt(v) runs from adam_eps = 1e-8 (v = 1e-16) up to 0.1: in the lowest half decade eps is a
    quarter to a half of the denominator sqrt(v) / sqrt(bc2) + eps, seven decades up it is nothing."""
    m, v = ls.adam_moments(0)
    assert m.dtype == v.dtype == np.float32 and m.shape == v.shape == (520,)
    r = np.sqrt(v.astype(np.float64))
    assert (r < 3e-8).sum() > 20 and (r > 1e-3).sum() > 20 and np.all(np.abs(m) <= r * (1 + 1e-6))
    assert (m > 0).sum() > 100 and (m < 0).sum() > 100
    assert v.min() >= np.float32(1e-16) and v.max() <= np.float32(1e-2)


def test_counter_scenarios():
    c = ls.SCENARIOS["beta_clamp"]["ctrl"]
    frames = [c["frame_idx"] + 1 + k for k in range(4)]
    betas = [ls.beta_of(f) for f in frames]
    assert frames == [99_998, 99_999, 100_000, 100_001]
    assert betas[0] < betas[1] < 1.0 and betas[2] == 1.0 and betas[3] == 1.0
    assert 0.4 + 100_001 * (1.0 - 0.4) / 100_000 > 1.0  # frame 100 001 needs the clamp
    assert [(c["train_steps"] + 1 + k) % 1000 == 0 for k in range(4)] == [False, False, True, False]
    c = ls.SCENARIOS["counter_carry"]["ctrl"]
    for key, first in (("step", c["step"]), ("frame_idx", c["frame_idx"] + 1), ("train_steps", c["train_steps"] + 1)):
        used = [first + k for k in range(4)]  # the Philox counters of four steps
        assert used[0] >> 32 == 0 and used[-1] >> 32 == 1, key
    c, kw = ls.SCENARIOS["eps_floor"]["ctrl"], ls.SCENARIOS["eps_floor"]["learner_kw"]
    assert c["epsilon"] * 0.995 ** 2 > kw["min_epsilon"] > c["epsilon"] * 0.995 ** 3


@pytest.mark.parametrize("layout,geometry,scenario", CASES)
def test_first_draw_preconditions(orc, layout, geometry, scenario):
    """The first update's uniforms are philox64(j, TAG_PER, frame, seed_env): known on the host. With
    them and oracle.per_sample_tree: `trained` draws on both sides of the push range, `giants` puts at
    least 90 % of the batch inside it and at least one draw outside, `absorbing` draws from a tree
    whose node sums have absorbed their small leaves.

    `absorbing` and the `last nonzero child' rule: a level of the descent is settled by that rule only
    where u * total has been rounded onto or past the level's running total. The three 1e30 entries
    and the push at max_prio = 1e30 are equal float32 leaves (1e18), whose fp64 sums are exact in every
    association; the rule is then reached only by draws that land among the small leaves beside them,
    which hold 1e-18 of the mass. Over 250 880 first-update draws (every geometry, two scenarios, up
    to 150 builder seeds each) the oracle reports a nonzero fallback mask for none, and no choice of
    seed can change that, so this test does not assert one; the forced cases stay with
    tests/test_gpu_per.py and tests/test_gpu_per_level2.py (u = 1 - 2^-53, alpha = 1). The mask is
    still computed and printed, and the GPU tests compare every draw with the restatement exactly."""
    st = ls.build_state(layout, geometry, scenario)
    n_in, n_fell = ls.check_preconditions(orc, st, BATCH)
    print(f"{layout} {geometry} {scenario}: {n_in} of {BATCH} draws inside the push range, "
          f"{n_fell} settled by a last nonzero child, {ls.absorbed_nodes(orc, st)} absorbing nodes")
