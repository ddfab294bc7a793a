"""MatchRecord: one episode of the match megakernels, tick by tick.

pm_play_rec / pm_play_rnn_rec (pongmi.play.play / play_rnn with record=...) store every tick of the
chosen arenas: the fp64 state after the tick, both players' actions and the q values their argmax
consumed, the scores and the bounce count. A MatchRecord is that, with frame 0 (the reset state,
which the kernel never stores: it follows from the serve) put in front, so frame t + 1 is the state
after tick t and what the players saw on tick t is obs(t).

  states  float64 [F + 1, 7]  ball_x, ball_y, ball_vx, ball_vy, spin, top_paddle_x, bottom_paddle_x
  actions int32   [F, 2]      player A (top), player B (bottom): 0 left, 1 stay, 2 right
  q       float32 [F, 2, 3]   the q values behind each action (NaN for the ball follower)
  scores  int32   [F + 1, 2]  scoreA, scoreB
  bounces int32   [F + 1]     paddle hits so far
  length  the episode's full length in ticks; F = min(length, the recording's tick cap)

save() / load() keep all of it in one .npz without pickling.
"""
import json

import numpy as np

STATE_FIELDS = ("ball_x", "ball_y", "ball_vx", "ball_vy", "spin", "top_paddle_x", "bottom_paddle_x")


def _plain(obj):
    """obj as JSON keeps it (tuples become lists, numpy scalars Python numbers), so that a record
    equals its saved copy."""
    return json.loads(json.dumps(obj, default=lambda v: v.tolist()))


class MatchRecord:
    def __init__(self, env_kw, players, serve, states, actions, q, scores, bounces, length):
        self.env_kw = _plain(dict(env_kw))
        self.players = tuple(_plain(list(players)))
        if len(self.players) != 2:
            raise ValueError("players: (player A, player B)")
        self.serve = np.asarray(serve, np.float64).reshape(3)
        self.states = np.ascontiguousarray(states, np.float64)
        self.actions = np.ascontiguousarray(actions, np.int32)
        self.q = np.ascontiguousarray(q, np.float32)
        self.scores = np.ascontiguousarray(scores, np.int32)
        self.bounces = np.ascontiguousarray(bounces, np.int32)
        self.length = int(length)
        F = self.actions.shape[0]
        if (self.states.shape != (F + 1, 7) or self.actions.shape != (F, 2) or self.q.shape != (F, 2, 3)
                or self.scores.shape != (F + 1, 2) or self.bounces.shape != (F + 1,)):
            raise ValueError(f"record arrays do not describe {F} ticks")
        if self.length < F:
            raise ValueError(f"length {self.length} below the {F} recorded ticks")

    @classmethod
    def from_ticks(cls, env_kw, players, serve, length, f64, q, i32):
        """From the kernel's rows of one arena: f64 [cap, 7], q [cap, 2, 3], i32 [cap, 5] (aA, aB,
        scoreA, scoreB, bounces) and the episode's full length. Frame 0 is reset()'s state for the
        serve (envs/my_pong_env_2p.py:83-114): ball at the centre, paddles at 0.5, scores 0."""
        serve = np.asarray(serve, np.float64).reshape(3)
        F = min(int(length), int(f64.shape[0]))
        states = np.empty((F + 1, 7), np.float64)
        states[0] = (0.5, 0.5, serve[0], serve[1], serve[2], 0.5, 0.5)
        states[1:] = f64[:F]
        scores = np.zeros((F + 1, 2), np.int32)
        scores[1:] = i32[:F, 2:4]
        bounces = np.zeros(F + 1, np.int32)
        bounces[1:] = i32[:F, 4]
        return cls(env_kw, players, serve, states, i32[:F, 0:2], q[:F], scores, bounces, length)

    @property
    def frames(self):
        """F: the recorded ticks (the record has F + 1 frames)."""
        return int(self.actions.shape[0])

    @property
    def truncated(self):
        return self.length > self.frames

    @property
    def rewards(self):
        """float32 [F, 2] (rA, rB): +1 for the point's winner and -1 for its loser on the tick a
        score changes, 0 otherwise (envs/my_pong_env_2p.py step())."""
        d = np.diff(self.scores.astype(np.int64), axis=0)
        rA = (d[:, 0] - d[:, 1]).astype(np.float32)
        return np.stack([rA, -rA], 1)

    def obs(self, t):
        """(obsA, obsB) float32 of frame t as _get_obs_for_A / _get_obs_for_B (:235-257) give them:
        what the players act on at tick t."""
        x, y, vx, vy, sp, top, bot = (float(v) for v in self.states[t])
        return (np.array([x, 1.0 - y, vx, -vy, top, bot, sp], np.float32),
                np.array([x, y, vx, vy, bot, top, sp], np.float32))

    def save(self, path):
        """One .npz (numeric arrays, the env kwargs and player names as JSON text)."""
        np.savez(path, states=self.states, actions=self.actions, q=self.q, scores=self.scores, bounces=self.bounces,
                 serve=self.serve, length=np.int64(self.length), env_kw=np.array(json.dumps(self.env_kw)),
                 players=np.array(json.dumps(list(self.players))))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(json.loads(str(z["env_kw"])), json.loads(str(z["players"])), z["serve"], z["states"],
                       z["actions"], z["q"], z["scores"], z["bounces"], int(z["length"]))

    def __eq__(self, other):
        if not isinstance(other, MatchRecord):
            return NotImplemented
        return (self.env_kw == other.env_kw and self.players == other.players and self.length == other.length
                and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                        for a, b in ((getattr(self, k), getattr(other, k))
                                     for k in ("serve", "states", "actions", "q", "scores", "bounces"))))

    __hash__ = None

    def __repr__(self):
        return (f"MatchRecord({self.players[0]!r} v {self.players[1]!r}, {self.frames} of {self.length} ticks, "
                f"final {int(self.scores[-1, 0])}-{int(self.scores[-1, 1])})")
