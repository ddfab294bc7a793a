"""K1 at every variant it dispatches: the 12 k_env_step instantiations (autoreset mode x serve table
or Philox x write-through or not) on both sides of a 256-arena block and of the write-through switch,
with and without term rows; pm_env_reset with masks, wrapped serve tables, Philox serve counts and
null outputs; the step counter's high word; the parameter space the reference fixtures now pin the
oracle on; serve angles beyond 135 degrees; unaligned output rows. The expectation is always built
on the host alone (the C oracle's tick, the serve table or the Philox restatement) and compared bit
for bit, signed zeros included."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.oracle import bits_equal

pytestmark = pytest.mark.gpu

STATE_ORDER = ("x", "y", "vx", "vy", "spin", "top", "bot", "scoreA", "scoreB", "bounces")
K1_WT_MAX = 131072  # csrc/pm_env.hip kK1WtMax: the last arena count stepped by the write-through kernels
SENTINEL = -7.0
CAP = 3  # serve-table rows per arena: serves 0..7 wrap around it


def mid_game_state(rng, n, serves=None):
    """test_env_step_matches_oracle_at_scale's start states: mid-game, y beyond the lines, paddles at
    the walls."""
    return dict(x=rng.uniform(-0.02, 1.02, n), y=rng.uniform(-0.05, 1.05, n), vx=rng.uniform(-0.08, 0.08, n),
                vy=rng.uniform(-0.08, 0.08, n), spin=rng.uniform(-6, 6, n), top=rng.choice([0.0, 0.5, 1.0, 0.31], n),
                bot=rng.uniform(0, 1, n), scoreA=rng.randint(0, 3, n), scoreB=rng.randint(0, 3, n),
                bounces=rng.randint(0, 9, n), serves=np.zeros(n, np.int64) if serves is None else serves)


def assert_state(env, arr, serves, where):
    got = env.get_state()
    for k in STATE_ORDER:
        assert bits_equal(got[k], arr[k]), (where, k)
    assert np.array_equal(got["serves"], serves), (where, "serves")


def serve_table(rng, n):
    """[n, CAP, 3] serves (vx, vy, spin), every row distinct."""
    tab = np.empty((n, CAP, 3))
    tab[..., 0] = rng.uniform(-0.05, 0.05, (n, CAP))
    tab[..., 1] = rng.choice([-1.0, 1.0], (n, CAP)) * rng.uniform(0.01, 0.05, (n, CAP))
    tab[..., 2] = rng.uniform(-5, 5, (n, CAP))
    return tab


def host_serves(orc, p, arr, serves, which, table, seed, step=None):
    """Serve arenas `which` (indices) on the host: table row serves % CAP and serves += 1, or the
    Philox restatement (step-keyed with `step`, else keyed by the serve count, which then advances)."""
    if table is not None:
        vx, vy, sp = table[which, serves[which] % CAP].T
        serves[which] += 1
    else:
        vx, vy, sp = orc.philox_serve(p, which, serves[which], seed, step=step)
        if step is None:
            serves[which] += 1
    mask = np.zeros(arr.shape[0], bool)
    mask[which] = True
    orc.serve_arenas(arr, mask, vx, vy, sp)


# ------------------------------------------------------------------ the dispatch matrix
DISPATCH_KW = dict(paddle_speed=0.03, max_score=1, magnus_factor=0.025, restitution=1, friction=0.6,
                   ball_speed_range=[0.03, 0.05], spin_range=[-5, 5], speed_scale_every=1, speed_increment=0.1)
DISPATCH_TICKS = 12
DISPATCH_CASES = [(ar, inj, term, n) for n in (1, 255, 256, 257, 513, K1_WT_MAX, K1_WT_MAX + 1)
                  for ar in (0, 1, 2) for inj in (False, True) for term in (False, True)]


def dispatch_start(n):
    """Start state of a dispatch case. n = 1: the ball two ticks from the top line, the paddle far
    away, so the arena finishes in tick 2 and plays on from its serve."""
    rng = np.random.RandomState(n)
    st = mid_game_state(rng, n, serves=np.arange(n) % 8)
    if n == 1:
        st.update(serves=np.array([4]),
                  x=np.array([0.9]), y=np.array([0.06]), vx=np.array([0.0]), vy=np.array([-0.05]),
                  spin=np.array([0.0]), top=np.array([0.1]), scoreA=np.array([0]), scoreB=np.array([0]))
    return rng, st


@pytest.mark.parametrize("ar,inj,term,n", DISPATCH_CASES)
def test_env_step_dispatch_matrix(orc, ar, inj, term, n):
    """k_env_step<AR, INJ, WT> for AR 0 / 1 / 2, a serve table (INJ) or Philox, term rows given or
    null, at n = 1, beside a 256-arena block (255, 256, 257, 513: the full-block float4 copy-out next
    to the scalar tail), at the last write-through size and at the first size of the other six
    instantiations (131 073: a one-arena tail block). 12 ticks of random actions from random mid-game
    states with max_score = 1. Every arena, every tick: obs (post-reset), rewards, done, term rows,
    the ten state fields and serves[] equal the host's."""
    from pongmi.env import PongEnv2PBatch

    p = orc.env_params_from_kwargs(**DISPATCH_KW)
    P = orc.make_params(p)
    rng, st = dispatch_start(n)
    table = serve_table(rng, n) if inj else None
    seed = n
    env = PongEnv2PBatch(n, seed=seed, serve_table=table, autoreset={0: False, 1: True, 2: "done"}[ar], **DISPATCH_KW)
    assert env.autoreset == ar
    env.set_state(st)
    if term:
        env.term_obsA = torch.full((n, 7), SENTINEL, dtype=torch.float32, device="cuda")
        env.term_obsB = torch.full((n, 7), SENTINEL, dtype=torch.float32, device="cuda")
    else:
        env.term_obsA = env.term_obsB = None
    arr, serves = orc.arenas_from_soa(st), st["serves"].copy()
    eTA = eTB = np.full((n, 7), SENTINEL, np.float32)
    seen = wrapped = 0
    for t in range(DISPATCH_TICKS):
        where = (ar, inj, term, n, t)
        aA, aB = rng.randint(0, 3, n).astype(np.int8), rng.randint(0, 3, n).astype(np.int8)
        (oA, oB), (rA, rB), done, _ = env.step(torch.from_numpy(aA), torch.from_numpy(aB))
        assert env.counter == t + 1
        eA, eB, rew, ed = orc.step_arenas(P, arr, aA, aB)
        d = ed.astype(bool)
        seen += int(d.sum())
        assert np.array_equal(done.cpu().numpy(), ed), where
        assert bits_equal(rA.cpu().numpy(), rew[:, 0]) and bits_equal(rB.cpu().numpy(), rew[:, 1]), where
        if ar == 2:  # term rows of done arenas only; the others keep what they held
            eTA, eTB = np.where(d[:, None], eA, eTA), np.where(d[:, None], eB, eTB)
        else:  # the step's pre-reset observation (AR 0: there is no reset, so it equals obs)
            eTA, eTB = eA, eB
        if ar and d.any():
            wrapped += int((serves[d] >= CAP).sum())
            host_serves(orc, p, arr, serves, np.nonzero(d)[0], table, seed, step=t)
            sA, sB = orc.obs_of_arenas(arr)
            eA, eB = np.where(d[:, None], sA, eA), np.where(d[:, None], sB, eB)
        assert bits_equal(oA.cpu().numpy(), eA) and bits_equal(oB.cpu().numpy(), eB), where
        if term:
            assert bits_equal(env.term_obsA.cpu().numpy(), eTA), where
            assert bits_equal(env.term_obsB.cpu().numpy(), eTB), where
        assert_state(env, arr, serves, where)
    if not (ar and inj):
        assert np.array_equal(serves, st["serves"])  # only a table serve counts
    if ar:  # the reset was exercised: `seen` counts the oracle's own done flags
        assert seen >= (n / 16 if n >= 255 else 1), seen
        if inj:
            assert wrapped >= 1  # a served arena's count was past the table's end: the index wrapped


# ------------------------------------------------------------------ the counter's high word
def test_env_step_counter_high_word(orc):
    """Philox autoreset across the carry of the step counter: counter preset to 2^32 - 2, four ticks
    at n = 257. The serves of the arenas that finish equal philox_serve(step = counter) with the
    counter's high word 0 and then 1; every other arena ticks as the oracle."""
    from pongmi.env import PongEnv2PBatch

    n, seed = 257, 21
    p = orc.env_params_from_kwargs(**DISPATCH_KW)
    P = orc.make_params(p)
    rng = np.random.RandomState(4)
    st = mid_game_state(rng, n)
    env = PongEnv2PBatch(n, seed=seed, autoreset=True, **DISPATCH_KW)
    env.set_state(st)
    env.counter = 2 ** 32 - 2
    arr, serves = orc.arenas_from_soa(st), st["serves"].copy()
    for t in range(4):
        step = 2 ** 32 - 2 + t
        aA, aB = rng.randint(0, 3, n).astype(np.int8), rng.randint(0, 3, n).astype(np.int8)
        (oA, oB), _, done, _ = env.step(torch.from_numpy(aA), torch.from_numpy(aB))
        d = orc.step_arenas(P, arr, aA, aB)[3].astype(bool)
        assert np.array_equal(done.cpu().numpy().astype(bool), d)
        assert d.sum() >= 5, (t, d.sum())  # every tick serves, on both sides of the carry
        host_serves(orc, p, arr, serves, np.nonzero(d)[0], None, seed, step=step)
        eA, eB = orc.obs_of_arenas(arr)
        assert bits_equal(oA.cpu().numpy(), eA) and bits_equal(oB.cpu().numpy(), eB), t
        assert_state(env, arr, serves, t)
        # the high word matters: the serve keyed by the low word alone is another one
        lo = orc.philox_serve(p, np.nonzero(d)[0], None, seed, step=step & 0xFFFFFFFF)
        if step >> 32:
            assert not np.array_equal(lo[0], arr["vx"][d])
    assert env.counter == 2 ** 32 + 2


# ------------------------------------------------------------------ pm_env_reset
def _reset_raw(env, mask, obsA, obsB):
    from pongmi import _lib

    _lib.check(env.lib.pm_env_reset(ctypes.byref(env.params), ctypes.byref(env.state), _lib.ptr(mask),
                                    _lib.ptr(env.inject), env.inject_cap, env.seed, _lib.ptr(obsA), _lib.ptr(obsB),
                                    None, env.n, _lib.stream_ptr()), "pm_env_reset")


@pytest.mark.parametrize("mask_kind", ["random", "zeros", "ones", "none"])
@pytest.mark.parametrize("inj", [False, True])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_env_reset_masks_serve_counts_and_null_outputs(orc, n, inj, mask_kind):
    """pm_env_reset from mid-game states. Table mode: row serves[i] % 3 with serves preset to 0..7.
    Philox mode: philox_serve(i, serves[i]) with serves 0..5. Masked-in arenas are served and their
    serves[] advance; masked-out arenas keep every state word and serves[]; obs of every arena is the
    observation of its state after the call. With obsA, obsB or both null the state is the same and
    the output that is given is still right."""
    from pongmi.env import PongEnv2PBatch

    kw = dict(ball_speed_range=[0.03, 0.05], spin_range=[-5, 5])
    p = orc.env_params_from_kwargs(**kw)
    rng = np.random.RandomState(1000 * n + 10 * inj + len(mask_kind))
    st = mid_game_state(rng, n, serves=np.arange(n) % (8 if inj else 6))
    table = serve_table(rng, n) if inj else None
    seed = 31
    mask = {"random": rng.rand(n) < 0.5, "zeros": np.zeros(n, bool), "ones": np.ones(n, bool), "none": None}[mask_kind]
    if mask_kind == "random" and n > 1:
        assert 0 < mask.sum() < n
    arr, serves = orc.arenas_from_soa(st), st["serves"].copy()
    host_serves(orc, p, arr, serves, np.arange(n) if mask is None else np.nonzero(mask)[0], table, seed)
    eA, eB = orc.obs_of_arenas(arr)
    if mask is not None and not mask.all():  # the oracle left the others alone, and so must the device
        keep = ~mask
        assert np.array_equal(serves[keep], st["serves"][keep]) and bits_equal(arr["vx"][keep], st["vx"][keep])
    env = PongEnv2PBatch(n, seed=seed, serve_table=table, **kw)
    dmask = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda()
    for wantA, wantB in ((True, True), (False, True), (True, False), (False, False)):
        where = (n, inj, mask_kind, wantA, wantB)
        env.set_state(st)
        oA = torch.full((n, 7), SENTINEL, dtype=torch.float32, device="cuda")
        oB = torch.full((n, 7), SENTINEL, dtype=torch.float32, device="cuda")
        _reset_raw(env, dmask, oA if wantA else None, oB if wantB else None)
        assert_state(env, arr, serves, where)
        assert bits_equal(oA.cpu().numpy(), eA if wantA else np.full((n, 7), SENTINEL, np.float32)), where
        assert bits_equal(oB.cpu().numpy(), eB if wantB else np.full((n, 7), SENTINEL, np.float32)), where


# ------------------------------------------------------------------ the parameter space at scale
def _fixture_kw(golden, name):
    pv = dict(zip([str(k) for k in golden(f"env_{name}")["param_names"]], golden(f"env_{name}")["param_values"].tolist()))
    return dict(paddle_width=pv["paddle_width"], paddle_speed=pv["paddle_speed"], max_score=int(pv["max_score"]),
                enable_spin=bool(pv["enable_spin"]), magnus_factor=pv["magnus_factor"],
                restitution=pv["restitution"], friction=pv["friction"], ball_mass=pv["ball_mass"],
                world_ball_radius=pv["world_ball_radius"], ball_speed_range=(pv["speed_lo"], pv["speed_hi"]),
                spin_range=(pv["spin_lo"], pv["spin_hi"]),
                ball_angle_intervals=[[pv["ang0_lo"], pv["ang0_hi"]], [pv["ang1_lo"], pv["ang1_hi"]]],
                speed_scale_every=int(pv["speed_scale_every"]), speed_increment=pv["speed_increment"])


# two sets that need no fixture (the oracle is the yardstick): restitution 0 leaves -0.0 velocities
# behind every paddle hit, speed_scale_every = 1000 never scales
EXTRA_SETS = {"e0": dict(DISPATCH_KW, max_score=3, restitution=0.0),
              "noscale": dict(DISPATCH_KW, max_score=3, restitution=0.9, speed_scale_every=1000)}


@pytest.mark.parametrize("name", ["nospin", "wide", "heavy", "e0", "noscale"])
def test_env_step_parameter_space_at_scale(orc, golden, name):
    """4099 arenas, 40 ticks without reset, on the parameter sets of the three new reference fixtures
    (spin off; a wide fast paddle, friction 0, e < 1, scale < 1; mass 3, radius 0.07, e > 1) and on
    e = 0 and a scale period never reached: bit-exact with the C oracle, sign bits included, with at
    least 100 paddle hits (the oracle's bounce counters)."""
    from pongmi.env import PongEnv2PBatch

    n = 4099
    kw = EXTRA_SETS[name] if name in EXTRA_SETS else _fixture_kw(golden, name)
    P = orc.make_params(orc.env_params_from_kwargs(**kw))
    rng = np.random.RandomState(n)
    st = mid_game_state(rng, n)
    env = PongEnv2PBatch(n, **kw)
    env.set_state(st)
    arr = orc.arenas_from_soa(st)
    hits = negzero = 0
    for t in range(40):
        aA, aB = rng.randint(0, 3, n).astype(np.int8), rng.randint(0, 3, n).astype(np.int8)
        before = arr["bounces"].copy()
        (oA, oB), (rA, rB), done, _ = env.step(torch.from_numpy(aA), torch.from_numpy(aB))
        eA, eB, rew, ed = orc.step_arenas(P, arr, aA, aB)
        hits += int((arr["bounces"] - before).sum())
        negzero += int((np.signbit(arr["vy"]) & (arr["vy"] == 0)).sum())
        assert np.array_equal(done.cpu().numpy(), ed), (name, t)
        assert bits_equal(rA.cpu().numpy(), rew[:, 0]) and bits_equal(rB.cpu().numpy(), rew[:, 1]), (name, t)
        assert bits_equal(oA.cpu().numpy(), eA) and bits_equal(oB.cpu().numpy(), eB), (name, t)
        assert_state(env, arr, st["serves"], (name, t))
    assert hits >= 100, hits
    if name == "e0":
        assert negzero > 0  # -0.0 did occur, and compared equal bit for bit


# ------------------------------------------------------------------ serve angles beyond 135 degrees
FAR_KW = dict(ball_speed_range=[0.03, 0.05], spin_range=[-5, 5], max_score=1,
              ball_angle_intervals=[[120, 150], [-150, -120]])


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def test_serves_beyond_135_degrees(orc):
    """Angle intervals that straddle the 135 degree switch of serve_finish: a production reset of 4096
    arenas, then 30 autoreset ticks. Serves with |angle| < 135 degrees equal the restatement bit for
    bit; the others (redone with OCML's sincos, documented < 1 ulp, against numpy's here) lie within
    2 ulp of the oracle's speed * cos, speed * sin: each library's value is within an ulp of the true
    one, and the product is rounded once more. Spin is exact on both sides. At least 200 serves fall
    on each side."""
    from pongmi.env import PongEnv2PBatch

    n, seed = 4096, 55
    p = orc.env_params_from_kwargs(**FAR_KW)
    P = orc.make_params(p)
    env = PongEnv2PBatch(n, seed=seed, autoreset=True, **FAR_KW)
    env.reset()
    count = {"near": 0, "far": 0}
    worst = 0

    def check(st, idx, exp):
        nonlocal worst
        vx, vy, sp, far = exp
        assert bits_equal(st["spin"][idx], sp)
        assert bits_equal(st["vx"][idx][~far], vx[~far]) and bits_equal(st["vy"][idx][~far], vy[~far])
        if far.any():
            dist = max(_ulps(st["vx"][idx][far], vx[far]).max(), _ulps(st["vy"][idx][far], vy[far]).max())
            worst = max(worst, int(dist))
            assert dist <= 2, dist
        count["near"] += int((~far).sum())
        count["far"] += int(far.sum())

    st = env.get_state()
    check(st, np.arange(n), orc.philox_serve(p, np.arange(n), np.zeros(n, np.int64), seed, want_far=True))
    assert np.all(st["serves"] == 1) and np.all(st["vx"] < 0)
    rng = np.random.RandomState(6)
    for t in range(30):
        aA, aB = rng.randint(0, 3, n).astype(np.int8), rng.randint(0, 3, n).astype(np.int8)
        arr = orc.arenas_from_soa(st)
        _, _, done, _ = env.step(torch.from_numpy(aA), torch.from_numpy(aB))
        d = orc.step_arenas(P, arr, aA, aB)[3].astype(bool)
        assert np.array_equal(done.cpu().numpy().astype(bool), d)
        st = env.get_state()
        for k in STATE_ORDER:
            assert bits_equal(st[k][~d], arr[k][~d]), (t, k)
        idx = np.nonzero(d)[0]
        check(st, idx, orc.philox_serve(p, idx, None, seed, step=t, want_far=True))
        for k, v in (("x", 0.5), ("y", 0.5), ("top", 0.5), ("bot", 0.5), ("scoreA", 0), ("scoreB", 0), ("bounces", 0)):
            assert np.all(st[k][idx] == v), (t, k)
    print(f"serves with |angle| < 135 degrees: {count['near']} (exact); beyond: {count['far']}, "
          f"largest distance {worst} ulp")
    assert count["near"] >= 200 and count["far"] >= 200, count


# ------------------------------------------------------------------ unaligned output rows
def test_env_step_unaligned_outputs(orc):
    """obs and term rows that start one float into their buffers (the ABI asks for no alignment):
    copy_rows7 then takes its scalar path for full blocks too. n = 513, AR 1, Philox, 12 ticks: every
    output equals the aligned run's, and the floats in front of and behind each view keep a sentinel."""
    from pongmi.env import PongEnv2PBatch

    n, seed = 513, 8
    rng = np.random.RandomState(n + 1)
    st = mid_game_state(rng, n)
    ref = PongEnv2PBatch(n, seed=seed, autoreset=True, **DISPATCH_KW)
    env = PongEnv2PBatch(n, seed=seed, autoreset=True, **DISPATCH_KW)
    ref.set_state(st)
    env.set_state(st)
    names = ("obsA", "obsB", "term_obsA", "term_obsB")
    bufs = {}
    for k in names:
        bufs[k] = torch.full((n * 7 + 2,), SENTINEL, dtype=torch.float32, device="cuda")
        view = bufs[k][1:1 + n * 7].view(n, 7)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        setattr(env, k, view)
    seen = 0
    for t in range(DISPATCH_TICKS):
        aA, aB = rng.randint(0, 3, n).astype(np.int8), rng.randint(0, 3, n).astype(np.int8)
        _, (rA, rB), done, _ = ref.step(torch.from_numpy(aA), torch.from_numpy(aB))
        _, (qA, qB), qdone, _ = env.step(torch.from_numpy(aA), torch.from_numpy(aB))
        seen += int(done.sum())
        assert torch.equal(done, qdone) and torch.equal(rA, qA) and torch.equal(rB, qB)
        for k in names:
            assert bits_equal(getattr(env, k).cpu().numpy(), getattr(ref, k).cpu().numpy()), (t, k)
            host = bufs[k].cpu().numpy()
            assert host[0] == SENTINEL and host[-1] == SENTINEL, (t, k)
    got, exp = env.get_state(), ref.get_state()
    for k in STATE_ORDER:
        assert bits_equal(got[k], exp[k]), k
    assert seen >= n // 16
