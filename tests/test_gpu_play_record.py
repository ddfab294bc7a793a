"""Tick records of the match megakernels (pm_play_rec / pm_play_rnn_rec, pongmi.play.play / play_rnn
with record=, pongmi.tournament.play_matches with record=).

The yardstick is the stepped loop (`_stepped` below: PongEnv2PBatch + pongmi.qnet.q_values +
pongmi.rnn.q_step with its own (h, c) + the ball-follower comparison, one launch per player, side
and tick), keeping every tick's state, actions, q values, scores and bounce count of every arena.
The megakernels run the same tile_hidden / tile_heads and rnn_core chains and the same fp64 tick, so
every comparison is exact equality: states, q values bit for bit, actions and integers equal, a ball
follower's q values NaN. Players come from tests/golden (trained RNN_Gen1 and RNN_Soul3) plus a
random QNetRNN, two random QNets and the ball follower.

One stepped reference is computed per (env, plan, serves) and shared by the tests that need it.
"""
import itertools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)  # config.yaml
ENV_RNN_KW = dict(ENV_KW, speed_scale_every=5, speed_increment=0.2)                                    # config_rnn.yaml
ENVS = {"config": ENV_KW, "config_rnn": ENV_RNN_KW}
CKPT_KEY = {"RNN_Gen1": "modelB_state", "RNN_Soul3": "modelB_state", "Legacy4_12": "modelB", "Noisy5_5": "modelB"}
# player indices (see `players`)
GEN1, SOUL3, RNN_RAND, QNET_A, BOT, QNET_B = range(6)


def _serves(E, seed, env_kw, max_vy=None):
    """E serves drawn as reset() draws them; with max_vy, only the draws with |vy| < max_vy are kept."""
    from pongmi.env import draw_serve, env_config
    rng, cfg = random.Random(seed), env_config(**env_kw)
    out = []
    while len(out) < E:
        sv = draw_serve(rng, cfg)
        if max_vy is None or abs(sv[1]) < max_vy:
            out.append(sv)
    return np.array(out, np.float64).reshape(E, 3)


def _golden_state_dicts(golden):
    """name -> (type, state dict or None) of the five tournament participants in tests/golden."""
    g, gr = golden("tournament"), golden("rnn")
    out = {}
    for i, (name, typ) in enumerate(zip(g["names"].tolist(), g["types"].tolist())):
        if typ == "HardcodedBallFollower":
            out[name] = (typ, None)
        elif name == "RNN_Soul3":
            out[name] = (typ, {k[7:]: torch.from_numpy(v) for k, v in gr.items() if k.startswith("params.")})
        else:
            out[name] = (typ, {k[len(f"sd{i}."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"sd{i}.")})
    return out


@pytest.fixture(scope="module")
def players(golden):
    """Folded eval-mode weights [("rnn" | "qnet" | "bot", weights)]: 0 trained RNN_Gen1, 1 trained
    RNN_Soul3, 2 random QNetRNN, 3 random QNet, 4 ball follower, 5 another random QNet."""
    from models.qnet import QNet
    from models.qnet_rnn import QNetRNN
    from pongmi import _lib, qnet as _qnet, rnn as _rnn
    sds = _golden_state_dicts(golden)

    def rnn_weights(sd):
        m = QNetRNN(input_dim=7, output_dim=3, feature_dim=128, lstm_hidden_dim=128, lstm_layers=1, head_hidden_dim=128)
        if sd is not None:
            m.load_state_dict(sd)
        m.eval()
        return _rnn.fold(m.packed().cuda(), _lib.PM_FOLD_EVAL)[0]

    def qnet_weights(seed):
        torch.manual_seed(seed)
        return _qnet.fold(QNet(7, 3).eval().packed().cuda(), _lib.PM_FOLD_EVAL)[0]
    torch.manual_seed(7)
    w2 = rnn_weights(None)
    return [("rnn", rnn_weights(sds["RNN_Gen1"][1])), ("rnn", rnn_weights(sds["RNN_Soul3"][1])), ("rnn", w2),
            ("qnet", qnet_weights(8)), ("bot", None), ("qnet", qnet_weights(9))]


_REF = {}


def _stepped(env, players, pa, pb, seed, max_vy=None, max_ticks=1_000_000):
    """The stepped loop over every arena in lockstep, every tick kept. Returns a dict: serves; finals
    scoreA / scoreB / length / last [n]; per tick t (up to the longest episode) and arena i
    states [T, n, 7] f64, actions [T, n, 2], q [T, n, 2, 3] f32 (NaN: ball follower), ints [T, n, 3]
    (scoreA, scoreB, bounces), all after tick t. Rows past an arena's length are not meaningful."""
    key = (env, tuple(pa), tuple(pb), seed, max_vy)
    if key in _REF:
        return _REF[key]
    from pongmi import qnet as _qnet, rnn as _rnn
    from pongmi.env import PongEnv2PBatch
    env_kw = ENVS[env]
    n, dev = len(pa), "cuda"
    serves = _serves(n, seed, env_kw, max_vy)
    ta, tb = torch.tensor(pa, device=dev), torch.tensor(pb, device=dev)
    rows = [((ta == k).nonzero().flatten(), (tb == k).nonzero().flatten()) for k in range(len(players))]
    state = [[_rnn.init_state(int(r.numel()), dev) for r in rows[k]] if kind == "rnn" else None
             for k, (kind, _) in enumerate(players)]
    e = PongEnv2PBatch(n, device=dev, serve_table=serves.reshape(n, 1, 3), autoreset=False, **env_kw)
    obsA, obsB = e.reset()
    aA = torch.zeros(n, dtype=torch.int8, device=dev)
    aB = torch.zeros(n, dtype=torch.int8, device=dev)
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    score = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    length = torch.full((n,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(n, dtype=torch.int8, device=dev)
    tol = torch.tensor(0.01, dtype=torch.float32, device=dev)
    S, A, Q, I = [], [], [], []
    for t in range(max_ticks):
        q = torch.full((n, 2, 3), float("nan"), dtype=torch.float32, device=dev)
        for k, (kind, w) in enumerate(players):
            for side, (obs, out) in enumerate(((obsA, aA), (obsB, aB))):
                r = rows[k][side]
                if r.numel() == 0:
                    continue
                x = obs.index_select(0, r)
                if kind == "bot":
                    a = torch.where(x[:, 0] < x[:, 4] - tol, 0, torch.where(x[:, 0] > x[:, 4] + tol, 2, 1))
                else:
                    qv = _rnn.q_step(w, x, *state[k][side]) if kind == "rnn" else _qnet.q_values(w, x)
                    q[:, side].index_copy_(0, r, qv)
                    a = qv.argmax(1)
                out.index_copy_(0, r, a.to(out.dtype))
        A.append(torch.stack([aA, aB], 1).to(torch.int32))
        Q.append(q)
        (obsA, obsB), (rA, rB), done, _ = e.step(aA, aB)
        S.append(e.f64.t().clone())
        I.append(e.i32[0:3].t().clone())
        new = done.bool() & ~finished
        score = torch.where(new.unsqueeze(1), e.i32[0:2].t(), score)
        length = torch.where(new, torch.full_like(length, t + 1), length)
        last = torch.where(new, torch.sign(rB - rA).to(torch.int8), last)
        finished |= new
        if (t + 1) % 16 == 0 and bool(finished.all()):
            break
    assert bool(finished.all())
    s = score.cpu().numpy()
    ref = dict(serves=serves, scoreA=s[:, 0], scoreB=s[:, 1], length=length.cpu().numpy(), last=last.cpu().numpy(),
               states=torch.stack(S).cpu().numpy(), actions=torch.stack(A).cpu().numpy(),
               q=torch.stack(Q).cpu().numpy(), ints=torch.stack(I).cpu().numpy())
    _REF[key] = ref
    return ref


def _ids(players):
    """player index -> play / play_rnn id, and the stacked QNet and QNetRNN weights."""
    from pongmi.play import FOLLOWER, rnn_id
    ids, wq, wr = [], [], []
    for kind, w in players:
        if kind == "rnn":
            ids.append(rnn_id(len(wr)))
            wr.append(w)
        elif kind == "qnet":
            ids.append(len(wq))
            wq.append(w)
        else:
            ids.append(FOLLOWER)
    return ids, torch.stack(wq), torch.stack(wr)


def _fused(kernel, env, players, pa, pb, serves, **kw):
    """play (kernel "qnet") or play_rnn (kernel "rnn") on the same players."""
    from pongmi.play import play, play_rnn
    ids, wq, wr = _ids(players)
    ia, ib = [ids[k] for k in pa], [ids[k] for k in pb]
    if kernel == "qnet":
        return play(ENVS[env], wq, ia, ib, serves, **kw)
    return play_rnn(ENVS[env], wq, wr, ia, ib, serves, **kw)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same_q(got, ref, what):
    """Bit for bit where the reference has q values; NaN where the side is a ball follower."""
    none = np.isnan(ref)
    assert np.isnan(got[none]).all(), f"{what}: follower q values are not NaN"
    bad = np.nonzero(_bits(got)[~none] != _bits(ref)[~none])[0]
    assert bad.size == 0, f"{what}: {bad.size} q values differ in bits, first {bad[:5]}"


def _check_ticks(ref, i, F, f64, q, i32, what):
    """Ticks 0 .. F-1 of arena i as the kernel stored them against the stepped loop's."""
    assert np.array_equal(_bits(f64[:F]), _bits(ref["states"][:F, i])), f"{what}: states"
    assert np.array_equal(i32[:F, 0:2], ref["actions"][:F, i]), f"{what}: actions"
    assert np.array_equal(i32[:F, 2:5], ref["ints"][:F, i]), f"{what}: scores / bounces"
    _same_q(q[:F], ref["q"][:F, i], what)


def _check_record(rec, ref, i, ids=None, cap=4096):
    what = f"arena {i}"
    L = int(ref["length"][i])
    F = min(L, cap)
    assert rec.length == L and rec.frames == F and rec.truncated == (L > F), what
    sv = ref["serves"][i]
    assert np.array_equal(rec.serve, sv)
    assert np.array_equal(rec.states[0], [0.5, 0.5, sv[0], sv[1], sv[2], 0.5, 0.5]), f"{what}: frame 0"
    assert (rec.scores[0] == 0).all() and rec.bounces[0] == 0
    i32 = np.concatenate([rec.actions, rec.scores[1:], rec.bounces[1:, None]], 1)
    _check_ticks(ref, i, F, rec.states[1:], rec.q, i32, what)
    if not rec.truncated:
        assert (int(rec.scores[-1, 0]), int(rec.scores[-1, 1])) == (int(ref["scoreA"][i]), int(ref["scoreB"][i]))
        r = rec.rewards[-1]
        assert np.sign(r[1] - r[0]) == ref["last"][i]
    if ids is not None:
        assert rec.players == ids


def _same_finals(got, ref):
    for g, k in zip(got, ("scoreA", "scoreB", "length", "last")):
        diff = np.nonzero(np.asarray(g) != ref[k])[0]
        assert diff.size == 0, f"{k}: {diff.size} of {len(ref[k])} episodes differ, first {diff[:5]}"


def _expand(plan):
    return [a for a, _, e in plan for _ in range(e)], [b for _, b, e in plan for _ in range(e)]


PAIR = {"qnet": (QNET_A, QNET_B), "rnn": (GEN1, SOUL3)}


# ---------------------------------------------------------------- 1 / 4: smallest shapes
@pytest.mark.parametrize("E", [1, 129])
@pytest.mark.parametrize("env", ["config", "config_rnn"])
@pytest.mark.parametrize("kernel", ["qnet", "rnn"])
def test_one_recorded_episode(players, kernel, env, E):
    """One episode, recorded; 129 episodes of one pair with episode 128 (a second block of one slot)
    recorded."""
    pa, pb = [PAIR[kernel][0]] * E, [PAIR[kernel][1]] * E
    ref = _stepped(env, players, pa, pb, 100 + E)
    out = _fused(kernel, env, players, pa, pb, ref["serves"], record=[E - 1])
    _same_finals(out[:4], ref)
    assert len(out[4]) == 1
    ids = _ids(players)[0]
    _check_record(out[4][0], ref, E - 1, (ids[pa[0]], ids[pb[0]]))
    assert out[4][0].env_kw == ENVS[env]


# ---------------------------------------------------------------- 2 / 4: refill
@pytest.mark.parametrize("kernel,E", [("qnet", 300), ("rnn", 200)])
def test_refill_all_recorded_in_shuffled_order(players, kernel, E):
    """One pair, per_block = 1024: one block of E slots, so E - 128 episodes start in a refilled
    column. All are recorded, the indices shuffled: a row follows its arena, not the column or the
    slot. A refilled QNetRNN column starts its next episode from a zero (h, c): its tick-0 q values
    are the stepped loop's, which come from init_state."""
    env = "config" if kernel == "qnet" else "config_rnn"
    pa, pb = [PAIR[kernel][0]] * E, [PAIR[kernel][1]] * E
    ref = _stepped(env, players, pa, pb, 77)
    order = np.random.default_rng(5).permutation(E).tolist()
    out = _fused(kernel, env, players, pa, pb, ref["serves"], per_block=1024, record=order)
    _same_finals(out[:4], ref)
    assert len(out[4]) == E
    for rec, i in zip(out[4], order):
        _check_record(rec, ref, i)
    if kernel == "rnn":  # episodes differ from tick 0 on only through their serves: zero state in each
        q0 = np.stack([rec.q[0] for rec in out[4]])
        assert np.array_equal(_bits(q0), _bits(ref["q"][0, order]))


# ---------------------------------------------------------------- 3 / 4: subsets of ragged plans
QNET_PLAN = [(QNET_A, QNET_B, 77), (QNET_B, QNET_A, 40), (QNET_A, BOT, 130), (BOT, QNET_B, 5), (BOT, BOT, 64),
             (QNET_A, QNET_A, 33), (QNET_B, BOT, 20)]
# every pairing of kinds with a QNetRNN side, 200 episodes
RNN_PLAN = [(GEN1, GEN1, 20), (GEN1, SOUL3, 60), (RNN_RAND, QNET_A, 5), (QNET_A, SOUL3, 30), (SOUL3, BOT, 50),
            (BOT, RNN_RAND, 15), (RNN_RAND, GEN1, 20)]


@pytest.mark.parametrize("kernel,env", [("qnet", "config"), ("rnn", "config"), ("rnn", "config_rnn")])
def test_subset_of_a_ragged_plan(players, kernel, env):
    """Every seventh episode of a ragged plan over all pairings recorded: the recorded rows are exact
    and the results of all episodes equal a run with record=None."""
    pa, pb = _expand(QNET_PLAN if kernel == "qnet" else RNN_PLAN)
    ref = _stepped(env, players, pa, pb, 31)
    want = list(range(0, len(pa), 7))
    plain = _fused(kernel, env, players, pa, pb, ref["serves"])
    out = _fused(kernel, env, players, pa, pb, ref["serves"], record=want)
    assert len(plain) == 4 and len(out) == 5
    for a, b in zip(plain, out[:4]):
        assert np.array_equal(a, b)
    _same_finals(out[:4], ref)
    ids = _ids(players)[0]
    for rec, i in zip(out[4], want):
        _check_record(rec, ref, i, (ids[pa[i]], ids[pb[i]]))


# ---------------------------------------------------------------- 5: cap and untouched memory (C ABI)
F64_FILL, Q_FILL, I32_FILL = -12345.0, 54321.0, -999


def _raw(kernel, env, players, pa, pb, serves, rec_row, n_rec, cap):
    """pm_play_rec / pm_play_rnn_rec called directly on sentinel-filled record buffers. Returns
    (scoreA, scoreB, length, last, status, rec_f64, rec_q, rec_i32) as host arrays."""
    import ctypes
    from pongmi import _lib
    from pongmi._lib import ptr, stream_ptr
    from pongmi.env import env_params
    from pongmi.play import plan_blocks
    lib = _lib.load()
    ids, wq, wr = _ids(players)
    E = len(pa)
    blk_nets, blk_range, order = plan_blocks([ids[k] for k in pa], [ids[k] for k in pb], 128)
    nb = blk_nets.shape[0]
    dev = "cuda"
    host = np.concatenate([blk_nets.reshape(-1), blk_range.reshape(-1), order]).astype(np.int32)
    d_int = torch.from_numpy(host).to(dev)  # nets | ranges | order
    d_serves = torch.from_numpy(np.ascontiguousarray(serves[order])).to(dev)
    sA = torch.zeros(E, dtype=torch.int32, device=dev)
    sB = torch.zeros(E, dtype=torch.int32, device=dev)
    length = torch.full((E,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(E, dtype=torch.int8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = max(n_rec, 1)
    f64 = torch.full((rows, cap, 7), F64_FILL, dtype=torch.float64, device=dev)
    q = torch.full((rows, cap, 2, 3), Q_FILL, dtype=torch.float32, device=dev)
    i32 = torch.full((rows, cap, 5), I32_FILL, dtype=torch.int32, device=dev)
    d_row = torch.from_numpy(np.asarray(rec_row, np.int32)).to(dev)
    prm = env_params(**ENVS[env])
    head = (ctypes.byref(prm), ptr(wq), int(wq.shape[0]))
    plan = (ptr(d_int), ptr(d_int[2 * nb:]), nb, ptr(d_int[4 * nb:]), ptr(d_serves), E, 1_000_000)
    tail = (ptr(sA), ptr(sB), ptr(length), ptr(last), ptr(status), ptr(d_row), n_rec, cap, ptr(f64), ptr(q), ptr(i32),
            stream_ptr())
    if kernel == "qnet":
        _lib.check(lib.pm_play_rec(*head, *plan, *tail), "pm_play_rec")
    else:
        scratch = torch.empty(int(lib.pm_play_rnn_scratch_bytes(nb)) // 4, dtype=torch.float32, device=dev)
        _lib.check(lib.pm_play_rnn_rec(*head, ptr(wr), int(wr.shape[0]), *plan, ptr(scratch), *tail), "pm_play_rnn_rec")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (sA, sB, length, last, status, f64, q, i32))


def _untouched(f64, q, i32):
    return (f64 == F64_FILL).all() and (q == Q_FILL).all() and (i32 == I32_FILL).all()


@pytest.mark.parametrize("kernel", ["qnet", "rnn"])
def test_cap_and_untouched_memory(players, kernel):
    """rec_cap = 16 cuts every episode, a cap above the longest leaves each row's tail alone, rows of
    -1 write nothing, a row equal to n_rec is counted and writes nothing.

    Every episode has to be longer than 16 ticks for the first part. That does not hold for every
    serve of config.yaml: a serve with |vy| = 0.043 (speed 0.05 at 30 degrees) is past the paddle
    line after 12 ticks, and when the receiver misses it the episode is over at tick 16 (measured: several
    of 129 episodes of the two random QNets have length exactly 16). So this case keeps the draws with
    |vy| < 0.5 / 17: from y = 0.5 the ball is then inside [0, 1] through tick 17 whatever the players
    do (vy changes only at a paddle hit), no point is scored before tick 18, and length > 16 for
    every kept serve."""
    E = 129
    pa, pb = [PAIR[kernel][0]] * E, [PAIR[kernel][1]] * E
    ref = _stepped("config", players, pa, pb, 100 + E, max_vy=0.5 / 17)
    rows = np.random.default_rng(3).permutation(E).astype(np.int32)
    assert (ref["length"] > 16).all()
    out = _raw(kernel, "config", players, pa, pb, ref["serves"], rows, E, 16)
    _same_finals(out[:4], ref)  # length is the full length
    assert out[4][0] == 0
    for i in range(E):
        _check_ticks(ref, i, 16, out[5][rows[i]], out[6][rows[i]], out[7][rows[i]], f"cap 16, arena {i}")
    # a cap above the longest episode: every row's tail past its length keeps the sentinel
    cap = int(ref["length"].max()) + 3
    assert cap > ref["length"].max()
    out = _raw(kernel, "config", players, pa, pb, ref["serves"], rows, E, cap)
    _same_finals(out[:4], ref)
    assert out[4][0] == 0
    for i in range(E):
        L, r = int(ref["length"][i]), rows[i]
        _check_ticks(ref, i, L, out[5][r], out[6][r], out[7][r], f"cap {cap}, arena {i}")
        assert _untouched(out[5][r, L:], out[6][r, L:], out[7][r, L:]), f"arena {i}: tail past its length written"
    # nothing recorded: nothing written
    out = _raw(kernel, "config", players, pa, pb, ref["serves"], np.full(E, -1, np.int32), 1, 16)
    _same_finals(out[:4], ref)
    assert out[4][0] == 0 and _untouched(*out[5:8])
    # a row equal to n_rec: counted in status, nothing written, the episodes still played
    bad = np.full(E, -1, np.int32)
    bad[5] = 1
    out = _raw(kernel, "config", players, pa, pb, ref["serves"], bad, 1, 16)
    _same_finals(out[:4], ref)
    assert out[4][0] == 1 and _untouched(*out[5:8])


# ---------------------------------------------------------------- 6: the oracle's tick
@pytest.mark.parametrize("kernel,env", [("qnet", "config"), ("rnn", "config_rnn")])
def test_recorded_actions_replay_through_the_oracle(players, orc, kernel, env):
    """The recorded actions stepped through the oracle env from the serve give every recorded frame,
    bit for bit, and the recorded scores and bounce counts."""
    E = 129
    pa, pb = [PAIR[kernel][0]] * E, [PAIR[kernel][1]] * E
    serves = _serves(E, 100 + E, ENVS[env])
    recs = _fused(kernel, env, players, pa, pb, serves, record=[0, 64, 128])[4]
    P = orc.make_params(orc.env_params_from_kwargs(**ENVS[env]))
    for rec in recs:
        assert not rec.truncated and rec.frames == rec.length > 0
        a = orc.new_arena(*rec.serve)
        st = orc.arena_state(a)
        assert np.array_equal(_bits(st[:7]), _bits(rec.states[0])) and (st[7:] == 0).all()
        for t in range(rec.frames):
            oA, oB, r, done = orc.step(P, a, rec.actions[t, 0], rec.actions[t, 1])
            st = orc.arena_state(a)
            assert np.array_equal(_bits(st[:7]), _bits(rec.states[t + 1])), f"frame {t + 1}"
            assert np.array_equal(st[7:9], rec.scores[t + 1]) and st[9] == rec.bounces[t + 1], f"frame {t + 1}"
            assert np.array_equal(r, rec.rewards[t]) and done == (t == rec.frames - 1)
            gA, gB = rec.obs(t + 1)
            assert np.array_equal(_bits(gA), _bits(oA)) and np.array_equal(_bits(gB), _bits(oB))


# ---------------------------------------------------------------- 7: play_matches end to end
def test_play_matches_records(golden, tmp_path):
    """The five tournament participants of tests/golden, the first episode of every pair recorded:
    the result list is the record=None run's, each record ends with its episode's result and
    carries the participants' names; replay() walks its frames."""
    from pongmi.tournament import load_model_universal, play_matches
    from pongmi.viewer import replay
    models = {}
    for name, (typ, sd) in _golden_state_dicts(golden).items():
        info = {"name": name, "path": "N/A", "type": typ}
        if sd is not None:
            info["path"] = str(tmp_path / f"{name}.pth")
            torch.save({CKPT_KEY[name]: sd, "epsilon": 0.05}, info["path"])
        models[name] = (load_model_universal(info, {}, "cuda"), typ)
    per = 4
    plan = [(a, b, per) for a, b in itertools.combinations(list(models), 2)]
    want = [per * k for k in range(len(plan))][::-1]  # first episode of every pair, asked in reverse
    rng0, rng = random.Random(5), random.Random(5)
    plain = play_matches(ENV_KW, models, plan, "cuda", rng0)
    results, records = play_matches(ENV_KW, models, plan, "cuda", rng, record=want)
    assert results == plain and rng.random() == rng0.random()  # the same episodes, the same draws
    assert list(records) == want
    for k in want:
        a, b, sa, sb = results[k]
        rec = records[k]
        assert rec.players == (a, b) == plan[k // per][:2]
        assert not rec.truncated and rec.length == rec.frames
        assert (int(rec.scores[-1, 0]), int(rec.scores[-1, 1])) == (sa, sb) and max(sa, sb) == 3
        follower = [models[nm][1] == "HardcodedBallFollower" for nm in (a, b)]
        for side in range(2):
            assert np.isnan(rec.q[:, side]).all() == follower[side] and np.isnan(rec.q[:, side]).any() == follower[side]
        assert np.array_equal(rec.q.argmax(2)[:, [s for s in range(2) if not follower[s]]],
                              rec.actions[:, [s for s in range(2) if not follower[s]]])
    views = list(replay(records[want[0]], render_size=64))
    assert len(views) == records[want[0]].frames + 1
    with pytest.raises(ValueError):
        play_matches(ENV_KW, models, plan, "cuda", random.Random(5), rnn="stepped", record=[0])
