"""The match megakernel for QNetRNN players (pm_play_rnn / pongmi.play.play_rnn): whole greedy
episodes in one launch when a side is a QNetRNN.

The yardstick is the stepped loop (`_stepped` below: PongEnv2PBatch + pongmi.rnn.q_step +
pongmi.qnet.q_values + the ball-follower comparison, one launch per player, side and tick), itself
pinned to the reference's tournament in test_gpu_tournament.py. The megakernel runs the same
arithmetic in the same order (rnn_core's MFMA / fmaf chains, the K8 QNet forward, the fp64 tick), so
every comparison is exact equality on every episode: final scores, lengths and the sign of the last
tick's reward. Nets: random-init QNetRNN / QNet and the two trained QNetRNN checkpoints of
tests/golden (long rallies, a hidden state that matters). Shapes: one live column, a second block
of one slot, ragged mixed plans over every pairing of kinds, ranges of several episodes per column
(a stale (h, c) carried into a column's next episode changes lengths), both env configs, the
play_matches switch, and the failure paths.
"""
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


def _serves(E, seed, env_kw=ENV_KW):
    from pongmi.env import draw_serve, env_config
    rng, cfg = random.Random(seed), env_config(**env_kw)
    return np.array([draw_serve(rng, cfg) for _ in range(E)], np.float64).reshape(E, 3)


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
    """Folded eval-mode weights: [("rnn" | "qnet" | "bot", weights)], indices used by the plans below:
    0 trained RNN_Gen1, 1 trained RNN_Soul3, 2 random QNetRNN, 3 random QNet, 4 ball follower."""
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
    torch.manual_seed(7)
    w2 = rnn_weights(None)
    torch.manual_seed(8)
    wq = _qnet.fold(QNet(7, 3).eval().packed().cuda(), _lib.PM_FOLD_EVAL)[0]
    return [("rnn", rnn_weights(sds["RNN_Gen1"][1])), ("rnn", rnn_weights(sds["RNN_Soul3"][1])), ("rnn", w2),
            ("qnet", wq), ("bot", None)]


def _stepped(env_kw, players, pa, pb, serves, max_ticks=1_000_000):
    """The stepped loop: every arena in lockstep, one act per player and side plus one env launch per
    tick. Returns (scoreA, scoreB, length, last) host arrays as play_rnn does."""
    from pongmi import qnet as _qnet, rnn as _rnn
    from pongmi.env import PongEnv2PBatch
    n = len(pa)
    dev = "cuda"
    ta, tb = torch.tensor(pa, device=dev), torch.tensor(pb, device=dev)
    rows = [((ta == k).nonzero().flatten(), (tb == k).nonzero().flatten()) for k in range(len(players))]
    state = [[_rnn.init_state(int(r.numel()), dev) for r in rows[k]] if kind == "rnn" else None
             for k, (kind, _) in enumerate(players)]
    env = PongEnv2PBatch(n, device=dev, serve_table=serves.reshape(n, 1, 3), autoreset=False, **env_kw)
    obsA, obsB = env.reset()
    aA = torch.zeros(n, dtype=torch.int8, device=dev)
    aB = torch.zeros(n, dtype=torch.int8, device=dev)
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    score = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    length = torch.full((n,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(n, dtype=torch.int8, device=dev)
    tol = torch.tensor(0.01, dtype=torch.float32, device=dev)
    for t in range(max_ticks):
        for k, (kind, w) in enumerate(players):
            for side, (obs, out) in enumerate(((obsA, aA), (obsB, aB))):
                r = rows[k][side]
                if r.numel() == 0:
                    continue
                x = obs.index_select(0, r)
                if kind == "rnn":
                    a = _rnn.q_step(w, x, *state[k][side]).argmax(1)
                elif kind == "qnet":
                    a = _qnet.q_values(w, x).argmax(1)
                else:
                    a = torch.where(x[:, 0] < x[:, 4] - tol, 0, torch.where(x[:, 0] > x[:, 4] + tol, 2, 1))
                out.index_copy_(0, r, a.to(out.dtype))
        (obsA, obsB), (rA, rB), done, _ = env.step(aA, aB)
        new = done.bool() & ~finished
        score = torch.where(new.unsqueeze(1), env.i32[0:2].t(), score)
        length = torch.where(new, torch.full_like(length, t + 1), length)
        last = torch.where(new, torch.sign(rB - rA).to(torch.int8), last)
        finished |= new
        if (t + 1) % 16 == 0 and bool(finished.all()):
            break
    assert bool(finished.all())
    s = score.cpu().numpy()
    return s[:, 0], s[:, 1], length.cpu().numpy(), last.cpu().numpy()


def _fused(env_kw, players, pa, pb, serves, **kw):
    """play_rnn on the same players: indices -> play_rnn ids and stacked weights."""
    from pongmi.play import FOLLOWER, play_rnn, rnn_id
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
    return play_rnn(env_kw, torch.stack(wq) if wq else None, torch.stack(wr), [ids[k] for k in pa],
                    [ids[k] for k in pb], serves, **kw)


def _same(got, ref):
    for g, r, what in zip(got, ref, ("scoreA", "scoreB", "length", "last")):
        diff = np.nonzero(np.asarray(g) != np.asarray(r))[0]
        assert diff.size == 0, f"{what}: {diff.size} of {len(r)} episodes differ, first {diff[:5]}"


def _expand(plan):
    pa = [a for a, _, e in plan for _ in range(e)]
    pb = [b for _, b, e in plan for _ in range(e)]
    return pa, pb


@pytest.mark.parametrize("E", [1, 129])
def test_one_pair_sizes(players, E):
    """One live column beside 127 idle ones; a second block holding one slot."""
    pa, pb = [0] * E, [1] * E
    serves = _serves(E, 100 + E)
    ref = _stepped(ENV_KW, players, pa, pb, serves)
    got = _fused(ENV_KW, players, pa, pb, serves)
    _same(got, ref)
    assert (np.maximum(got[0], got[1]) == 3).all() and (got[2] > 0).all()


# every pairing of kinds with a QNetRNN side, ragged counts (player indices: see `players`)
MIXED = [(0, 0, 77), (0, 1, 130), (2, 3, 5), (3, 1, 64), (1, 4, 200), (4, 2, 33), (2, 0, 40)]


@pytest.mark.parametrize("env", ["config", "config_rnn"])
def test_mixed_plan_matches_stepped(players, env):
    """RNN vs itself, vs another RNN, vs QNet, QNet vs RNN, RNN vs follower, follower vs RNN in one
    call, under both env configs."""
    env_kw = ENVS[env]
    pa, pb = _expand(MIXED)
    serves = _serves(len(pa), 31, env_kw)
    ref = _stepped(env_kw, players, pa, pb, serves)
    got = _fused(env_kw, players, pa, pb, serves)
    _same(got, ref)
    assert (np.maximum(got[0], got[1]) == 3).all()


_REFILL = {}


@pytest.mark.parametrize("per_block", [128, 640])
def test_refill_matches_stepped(players, per_block):
    """E = 1300 on one pair: 11 blocks of one slot per column, then blocks of 640 / 640 / 20 slots
    (five episodes per column). Each refilled episode must start from a zero hidden state."""
    E = 1300
    pa, pb = [0] * E, [1] * E
    serves = _serves(E, 77, ENV_RNN_KW)
    if "ref" not in _REFILL:
        _REFILL["ref"] = _stepped(ENV_RNN_KW, players, pa, pb, serves)
    got = _fused(ENV_RNN_KW, players, pa, pb, serves, per_block=per_block)
    _same(got, _REFILL["ref"])


def test_play_matches_fused_equals_stepped(golden, tmp_path):
    """play_matches on the five tournament participants: rnn="fused" and rnn="stepped" return the same
    list and leave the random stream in the same state; the fused path is the default."""
    from pongmi.tournament import load_model_universal, play_matches
    import itertools
    models = {}
    for name, (typ, sd) in _golden_state_dicts(golden).items():
        info = {"name": name, "path": "N/A", "type": typ}
        if sd is not None:
            info["path"] = str(tmp_path / f"{name}.pth")
            torch.save({CKPT_KEY[name]: sd, "epsilon": 0.05}, info["path"])
        models[name] = (load_model_universal(info, {}, "cuda"), typ)
    plan = [(a, b, 4) for a, b in itertools.combinations(list(models), 2)]
    out, after = {}, {}
    for mode in ("fused", "stepped", None):
        rng = random.Random(5)
        kw = {} if mode is None else {"rnn": mode}
        out[mode] = play_matches(ENV_KW, models, plan, "cuda", rng, **kw)
        after[mode] = rng.random()
    assert out["fused"] == out["stepped"] and after["fused"] == after["stepped"]
    assert out[None] == out["fused"] and after[None] == after["fused"]
    assert len(out["fused"]) == 40 and all(max(sa, sb) == 3 for _, _, sa, sb in out["fused"])
    with pytest.raises(ValueError):
        play_matches(ENV_KW, models, plan, "cuda", random.Random(5), rnn="other")


def test_failure_paths(players):
    from pongmi.play import FOLLOWER, play_rnn, rnn_id
    wr = torch.stack([players[0][1], players[1][1]])
    serves = _serves(10, 1)
    with pytest.raises(RuntimeError, match="did not finish"):
        play_rnn(ENV_KW, None, wr, np.full(10, rnn_id(0)), np.full(10, rnn_id(1)), serves, max_steps=3)
    with pytest.raises(ValueError):
        play_rnn(ENV_KW, None, wr, np.full(10, rnn_id(0)), np.full(10, rnn_id(2)), serves)
    with pytest.raises(ValueError):  # a QNet id without QNets
        play_rnn(ENV_KW, None, wr, np.full(10, rnn_id(0)), np.zeros(10), serves)
    with pytest.raises(ValueError):  # a pair without a QNetRNN belongs to play
        play_rnn(ENV_KW, None, wr, np.full(10, FOLLOWER), np.full(10, FOLLOWER), serves)
    out = play_rnn(ENV_KW, None, wr, [], [], np.zeros((0, 3)))
    assert all(o.shape == (0,) for o in out)
    # the calls above left the device usable
    sA, sB, length, _ = play_rnn(ENV_KW, None, wr, np.full(4, rnn_id(1)), np.full(4, FOLLOWER), _serves(4, 2))
    assert (np.maximum(sA, sB) == 3).all() and (length > 0).all()
