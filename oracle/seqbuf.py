"""ORACLE — TEST INFRASTRUCTURE ONLY.

A host model of the QNetRNN sequence buffer and its sampler: the part of the self-play loop between
the transition ring and the DRQN update (k_rsp_append's episode table, its two eviction rules, and
k_rsp_sample), restated as the reference's own data structure (SequenceReplayBuffer,
scripts/train_rnn_iterative.py:100-176): a deque(maxlen=capacity) of whole trajectories and one
running trajectory per arena. It is plain Python + numpy and shares nothing with the kernels'
indexing: it holds no ring slot, no table slot and no prefix sum — only copies of the rows it was
fed. A device read of an overwritten or wrong ring / table slot is therefore a data mismatch.

Three layers, kept apart:
  1. the reference class (push_step / the deque / sample's window cut) for n arenas visited in
     ascending order per vector step, which is the push order the batched loop defines;
  2. the ring-safety layer (include/pongmi.h "Ring safety", RNNSelfPlayLearner's docstring), the two
     documented deviations; `depth=None` turns it off and leaves exactly layer 1;
  3. the sampler's Philox draw (`draws`), which replaces np.random.choice / np.random.randint.

A ring row is 16 float32 words: obs_B[0:7], reward_B[7], next_obs_B[8:15], and word 15 holding the
integer bits action | done << 8.
"""
from collections import deque

import numpy as np

from . import oracle as orc

ST_OVERWRITTEN, ST_AGED, ST_TOO_LONG = 1, 2, 4  # pm_rnn_ctrl.status values


class Trajectory(list):
    """A list of copied 16-float rows (what the reference's deque holds), labelled with where it came
    from: the arena, the vector step of its first row and of its last (done) row."""

    def __init__(self, rows, arena, first, finished):
        super().__init__(rows)
        self.arena, self.first, self.finished = int(arena), int(first), int(finished)


class SeqBufferModel:
    def __init__(self, n, T, cap, depth=None):
        self.n, self.T, self.cap = int(n), int(T), int(cap)
        self.depth = None if depth is None else int(depth)  # None: the reference class alone
        self.buffer = deque(maxlen=self.cap)                 # self.buffer of the reference
        self.current = [[] for _ in range(self.n)]           # current_episode_trajectory, per arena
        self.current_first = [0] * self.n
        self.seq_count = 0                                   # trajectories ever appended
        self.status = 0
        self.over_cap_steps = 0                              # vector steps that appended more than cap

    # ------------------------------------------------------------------ layer 1: the reference
    def push_step(self, step, rows):
        """One vector step: rows [n][16], arena i's push_step(obs, act, rew, next, done) in order."""
        rows = np.asarray(rows, np.float32)
        assert rows.shape == (self.n, 16)
        done = (rows[:, 15].copy().view(np.int32) >> 8) & 1  # bit 8 of word 15
        appended = 0
        for i in range(self.n):
            cur = self.current[i]
            if not cur:
                self.current_first[i] = step
            cur.append(rows[i].copy())
            if done[i]:
                if len(cur) >= self.T and self._admits(len(cur)):
                    self.buffer.append(Trajectory(cur, i, self.current_first[i], step))  # a copy
                    self.seq_count += 1
                    appended += 1
                self.current[i] = []
        if appended > self.cap:
            self.over_cap_steps += 1
        self._evict_aged(step)

    def window(self, j, start):
        """episode[start : start + T] of held episode j as the reference's five arrays."""
        tr = self.buffer[int(j)]
        assert 0 <= start and start + self.T <= len(tr)
        rows = np.stack(tr[int(start):int(start) + self.T])
        bits = rows[:, 15].copy().view(np.int32)
        return (rows[:, 0:7].copy(), (bits & 0xFF).astype(np.int32), rows[:, 7].copy(), rows[:, 8:15].copy(),
                ((bits >> 8) & 0xFF).astype(np.uint8))

    def sample_at(self, picks):
        """The batch for given (episode index, start) pairs: obs [B][T][7], act, rew, next, done [B][T]."""
        parts = [self.window(j, s) for j, s in picks]
        return tuple(np.stack([p[k] for p in parts]) for k in range(5))

    # ------------------------------------------------------------------ layer 2: ring safety
    def _admits(self, length):
        """A finished trajectory longer than depth // 2 is not stored (status value 4)."""
        if self.depth is None:
            return True
        if length > self.depth // 2:
            self.status |= ST_TOO_LONG
            return False
        return True

    def _evict_aged(self, now):
        """After the append of step `now`, every episode that finished at or before step
        now - depth // 2 - 1 leaves (status value 2: more left than the capacity rule removed)."""
        if self.depth is None:
            return
        while self.buffer and self.buffer[0].finished <= now - self.depth // 2 - 1:
            self.buffer.popleft()
            self.status |= ST_AGED

    # ------------------------------------------------------------------ read-outs
    @property
    def seq_size(self):
        return len(self.buffer)

    def held(self):
        """The held episodes, oldest first: (arena, first step, length) int64 [seq_size, 3]."""
        return np.array([(t.arena, t.first, len(t)) for t in self.buffer], np.int64).reshape(-1, 3)

    # ------------------------------------------------------------------ layer 3: the sampler's draw
    def draws(self, seed_env, now, u, B):
        """(episode index, start) [B][2] of update u's batch drawn after `now` vector steps: Philox
        counter now | u << 48 under TAG_SEQ, index = the sequence number b; episode
        j = below(r.x, size) (np.random.choice(len(buffer), B, replace=True), :129) and
        start = below(r.y, L - T + 1) (np.random.randint(0, len(episode) - T + 1), :143)."""
        size = len(self.buffer)
        assert size > 0 and 0 <= u < 1 << 15
        r = orc.philox64(np.arange(B), orc.TAG_SEQ, int(now) | (int(u) << 48), seed_env)
        j = orc.below(r[0], size)
        starts = np.array([int(orc.below(r[1][b], len(self.buffer[int(j[b])]) - self.T + 1)) for b in range(B)],
                          np.int64)
        return np.stack([j, starts], 1)

    def sample(self, seed_env, now, u, B):
        return self.sample_at(self.draws(seed_env, now, u, B))
