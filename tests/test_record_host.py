"""CPU-only checks of match recording: pm_play_rec / pm_play_rnn_rec refuse bad record arguments
before any device work, MatchRecord derives frame 0, rewards and `truncated` correctly and survives
save / load exactly, obs(t) is the oracle's observation, RecordView / replay draw what draw_frame
draws, and play / play_rnn / play_matches refuse a bad `record` before any device call."""
import numpy as np
import pytest

ENV_KW = dict(paddle_width=0.2, paddle_speed=0.03, max_score=3, enable_spin=True, magnus_factor=0.025, restitution=1,
              friction=0.6, ball_mass=1.0, world_ball_radius=0.03, ball_speed_range=[0.03, 0.05], spin_range=[-5, 5],
              ball_angle_intervals=[[-60, -30], [30, 60]], speed_scale_every=1, speed_increment=0.1)
PM_E_ARG, PM_E_SIZE = -1, -2
X = 16  # a non-null pointer value: the checks run before anything is dereferenced


def _args(name, n_blocks=1, n_rec=1, cap=8, row=X, f64=X, q=X, i32=X):
    """Arguments of a recording entry point with every sibling buffer null."""
    if name == "pm_play_rec":
        head = [None, None, 0, None, None, n_blocks, None, None, 0, 0, None, None, None, None, None]
    else:
        head = [None, None, 0, None, 0, None, None, n_blocks, None, None, 0, 0, None, None, None, None, None, None]
    return head + [row, n_rec, cap, f64, q, i32, None]


@pytest.mark.parametrize("name", ["pm_play_rec", "pm_play_rnn_rec"])
def test_recording_entry_points_check_arguments_without_a_gpu(name):
    from pongmi import _lib
    L = _lib.load()
    f = getattr(L, name)

    def refused(code, **kw):
        assert f(*_args(name, **kw)) == code, kw
        assert name.encode() + b":" in L.pm_last_error(), L.pm_last_error()
    refused(PM_E_SIZE, n_rec=-1)
    refused(PM_E_SIZE, n_rec=1, cap=0)
    refused(PM_E_SIZE, n_rec=3, cap=-5)
    for buf in ("row", "f64", "q", "i32"):
        refused(PM_E_ARG, **{buf: None})
    refused(PM_E_SIZE, n_blocks=-1)           # the sibling's own checks, under the new name
    refused(PM_E_ARG)                         # record arguments fine, the sibling's buffers null
    # the record checks come before the n_blocks == 0 early return; a valid empty call is a no-op
    refused(PM_E_SIZE, n_blocks=0, n_rec=-1)
    assert f(*_args(name, n_blocks=0)) == 0
    # n_rec == 0 asks for no buffers and no cap
    assert f(*_args(name, n_blocks=0, n_rec=0, cap=0, row=None, f64=None, q=None, i32=None)) == 0
    assert f(*_args(name, n_rec=0, cap=0, row=None, f64=None, q=None, i32=None)) == PM_E_ARG  # sibling's nulls


def _hand_made(length=None):
    """Five ticks: B scores on tick 2 (A misses), A scores on tick 4."""
    from pongmi.record import MatchRecord
    rng = np.random.default_rng(0)
    cap = 5
    f64 = rng.uniform(0, 1, (cap, 7))
    q = rng.normal(size=(cap, 2, 3)).astype(np.float32)
    q[:, 1] = np.nan  # side B: a ball follower
    i32 = np.zeros((cap, 5), np.int32)
    i32[:, 0] = [0, 1, 2, 1, 0]
    i32[:, 1] = [2, 2, 1, 0, 0]
    i32[:, 2] = [0, 0, 0, 0, 1]   # scoreA
    i32[:, 3] = [0, 0, 1, 1, 1]   # scoreB
    i32[:, 4] = [0, 1, 1, 2, 2]   # bounces
    serve = (0.031, -0.027, 1.5)
    return MatchRecord.from_ticks(ENV_KW, ("net", "bot"), serve, cap if length is None else length, f64, q, i32), \
        f64, q, i32


def test_match_record_frame0_rewards_and_truncated():
    rec, f64, q, i32 = _hand_made()
    assert rec.frames == 5 and rec.length == 5 and not rec.truncated
    assert rec.states.shape == (6, 7) and rec.actions.shape == (5, 2) and rec.q.shape == (5, 2, 3)
    assert rec.scores.shape == (6, 2) and rec.bounces.shape == (6,) and rec.rewards.shape == (5, 2)
    assert rec.states[0].tolist() == [0.5, 0.5, 0.031, -0.027, 1.5, 0.5, 0.5]  # reset(): built from the serve
    assert rec.scores[0].tolist() == [0, 0] and rec.bounces[0] == 0
    assert np.array_equal(rec.states[1:], f64) and np.array_equal(rec.actions, i32[:, :2])
    assert np.array_equal(rec.scores[1:], i32[:, 2:4]) and np.array_equal(rec.bounces[1:], i32[:, 4])
    assert rec.rewards.dtype == np.float32
    assert rec.rewards.tolist() == [[0, 0], [0, 0], [-1, 1], [0, 0], [1, -1]]
    # an episode longer than the recording: only the stored ticks, flagged
    cut, *_ = _hand_made(length=40)
    assert cut.frames == 5 and cut.length == 40 and cut.truncated
    # an episode shorter than the cap: the rows past its length are dropped
    short, *_ = _hand_made(length=3)
    assert short.frames == 3 and not short.truncated and short.states.shape == (4, 7)
    assert short.rewards.tolist() == [[0, 0], [0, 0], [-1, 1]]
    assert rec.players == ("net", "bot") and rec.env_kw == ENV_KW


def test_match_record_save_load_is_exact(tmp_path):
    from pongmi.record import MatchRecord
    rec, *_ = _hand_made(length=40)
    path = tmp_path / "m.npz"
    rec.save(path)
    with np.load(path, allow_pickle=False) as z:  # no pickled objects inside
        assert all(z[k].dtype != object for k in z.files)
    back = MatchRecord.load(path)
    assert back == rec
    for k in ("serve", "states", "actions", "q", "scores", "bounces"):
        a, b = getattr(rec, k), getattr(back, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k  # bit for bit, NaNs included
    assert back.length == 40 and back.truncated and back.players == ("net", "bot") and back.env_kw == ENV_KW
    ids = MatchRecord(ENV_KW, (3, -1), rec.serve, rec.states, rec.actions, rec.q, rec.scores, rec.bounces, 5)
    ids.save(path)
    assert MatchRecord.load(path).players == (3, -1)
    with pytest.raises(ValueError):
        MatchRecord(ENV_KW, (3, -1), rec.serve, rec.states[:-1], rec.actions, rec.q, rec.scores, rec.bounces, 5)


def test_obs_is_the_oracles(orc):
    rec, *_ = _hand_made()
    for t in range(rec.frames + 1):
        a = orc.arena_from_state(np.concatenate([rec.states[t], rec.scores[t], [rec.bounces[t]]]))
        oA, oB = orc.arena_obs(a)
        gA, gB = rec.obs(t)
        assert gA.dtype == np.float32 and gB.dtype == np.float32
        assert gA.tobytes() == oA.tobytes() and gB.tobytes() == oB.tobytes()


def test_record_view_and_replay():
    from pongmi.viewer import ArenaView, RecordView, draw_frame, replay
    rec, *_ = _hand_made()
    views = []
    angle = 0.0
    for t, v in enumerate(replay(rec, render_size=96)):
        views.append(v)
        assert v.t == t
        x, y, vx, vy, sp, top, bot = rec.states[t]
        assert (v.ball_x, v.ball_y, v.ball_vx, v.ball_vy, v.spin, v.top_paddle_x, v.bottom_paddle_x) == \
            (x, y, vx, vy, sp, top, bot)
        assert (v.scoreA, v.scoreB, v.bounce_count) == (rec.scores[t, 0], rec.scores[t, 1], rec.bounces[t])
        assert (v.paddle_width, v.world_ball_radius, v.max_score, v.render_size) == (0.2, 0.03, 3, 96)
        angle += sp
        img = v.frame()
        assert img.shape == (96, 96, 3) and img.dtype == np.uint8
        assert np.array_equal(img, draw_frame(x, y, top, bot, 0.2, angle, 96))
        assert np.array_equal(v.frame(advance_spin=False), img)
        if t == 0:
            assert v.actions is None and v.q is None
        else:
            assert v.actions == tuple(rec.actions[t - 1]) and v.q.tobytes() == rec.q[t - 1].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(v.obs(), rec.obs(t)))
    assert len(views) == rec.frames + 1
    # ArenaView's public attributes and methods
    names = [n for n in dir(ArenaView) if not n.startswith("_") and n != "render"]
    v = RecordView(rec, 2)
    assert all(hasattr(v, n) for n in names), [n for n in names if not hasattr(v, n)]
    for n in ("ball_x", "ball_y", "ball_vx", "ball_vy", "spin", "top_paddle_x", "bottom_paddle_x", "scoreA", "scoreB",
              "bounce_count", "index", "paddle_width", "world_ball_radius", "max_score", "render_size", "spin_angle"):
        assert hasattr(v, n), n
    with pytest.raises(IndexError):
        RecordView(rec, rec.frames + 1)


def _no_device(monkeypatch):
    """Any library load or device allocation from here on fails the test."""
    import torch
    from pongmi import _lib

    def boom(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_lib, "load", boom)
    for fn in ("zeros", "full", "empty", "from_numpy"):
        monkeypatch.setattr(torch, fn, boom)


@pytest.mark.parametrize("record", [[1, 1], [0, 3], [-1], [2, 0, 2], [0.5]])
def test_play_refuses_a_bad_record_before_any_device_call(monkeypatch, record):
    from pongmi.play import FOLLOWER, play, play_rnn, rnn_id
    _no_device(monkeypatch)
    serves = np.zeros((3, 3))
    with pytest.raises(ValueError, match="record"):
        play(ENV_KW, None, [FOLLOWER] * 3, [FOLLOWER] * 3, serves, record=record)
    with pytest.raises(ValueError, match="record"):
        play_rnn(ENV_KW, None, None, [rnn_id(0)] * 3, [FOLLOWER] * 3, serves, record=record)
    with pytest.raises(ValueError, match="record_ticks"):
        play(ENV_KW, None, [FOLLOWER] * 3, [FOLLOWER] * 3, serves, record=[0], record_ticks=0)


def test_play_matches_refuses_record_with_the_stepped_path(monkeypatch):
    from pongmi.tournament import play_matches
    _no_device(monkeypatch)
    models = {"a": ("HardcodedAgent", "HardcodedBallFollower"), "b": ("HardcodedAgent", "HardcodedBallFollower")}
    with pytest.raises(ValueError, match="stepped"):
        play_matches(ENV_KW, models, [("a", "b", 2)], "cuda", rnn="stepped", record=[0])
    for bad in ([0, 0], [2], [-1]):
        with pytest.raises(ValueError, match="record"):
            play_matches(ENV_KW, models, [("a", "b", 2)], "cuda", record=bad)
