"""Host side of K9 (pm_rollout, csrc/pm_rollout.hip): inference-only self-play, K vector steps per launch.

BASELINE configs[1]: the rollout of scripts/train_iterative.py:239-242 with the learner switched off
— modelA greedy on its folded weights, modelB epsilon-greedy with fresh NoisyNet noise every vector
step (select_action_B's reset_noise, :125), PongEnv2P autoreset — for n arenas in lockstep. One
launch runs `steps` vector steps with every arena held in registers; the result is bit-identical to
`steps` repetitions of

    w_B = qnet.fold(paramsB, PM_FOLD_TRAIN_FRESH, seed=seed_net, counter=c)
    aA, aB = qnet.act(wA, None, w_B, env.obsA, env.obsB, epsilon, seed=env.seed, counter=c)
    env.step(aA, aB)                       # autoreset, step-keyed serves: env.counter == c

with c = env.counter (tests/test_gpu_rollout.py). The rollout advances env.counter by `steps`, and
leaves env.obsA / env.obsB holding the observations after the last step; rewards / done / term_obs
of the last step are not produced (no learner consumes them).

With `replay=` (a pongmi.replay.DeviceReplay) the same launch is §8f3's collecting rollout
(pm_rollout_push): every vector step also pushes its n transitions into the ring as the training
loop's memory.push((oB, aB, rB, nB, done)) (:242-243) — the rows go from registers to the ring, and
the launch leaves the PER sum tree current — with ep_reward carried per arena (:245) and the stats
gaining the loop's episode wins (ep_reward > 0, :247) and reward sum.
"""
import math
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import PM_QNET_NP, PM_QNET_NW, PM_ROLL_HEADS, check, ptr, require_device, stream_ptr
from ._pop import TableHandle, per_member
from .env import ctypes_ref

STATS = ("episodes", "wins_B", "points_A", "points_B")
STATS_PUSH = STATS + ("wins_B_episode", "reward_B")


def nstep_fold_host(rows_1step, n, steps, N, gamma):
    """The host model of the n-step collector (pm_rollout_push_n): the rows a launch of `steps` vector steps over n
    arenas writes with a window of N ticks, from the rows the one-step launch writes. rows_1step: float32
    [steps * n, PM_TRANS_F] in launch order (row st * n + i is step st's arena i; unwrap a ring first). Returns
    the same shape: row st * n + i is the transition opened at step st with its n-step reward, the s' and done of
    the tick that closed it, and its horizon k as k - 1 in bits 16..18 of the last word. Everything is float32
    in the device's order: per tick R = R + f * r, then f = f * g, from (0, 1). N = 1 returns the input."""
    rows = np.ascontiguousarray(rows_1step, dtype=np.float32).reshape(int(steps), int(n), _lib.PM_TRANS_F)
    N = int(N)
    if not 1 <= N <= _lib.PM_NSTEP_MAX:
        raise ValueError(f"nstep_fold_host: N {N} (1..{_lib.PM_NSTEP_MAX})")
    out = rows.copy()
    if N == 1:
        return out.reshape(-1, _lib.PM_TRANS_F)
    bits, obits = rows[:, :, 15].view(np.int32), out[:, :, 15].view(np.int32)
    g = np.float32(gamma)
    for i in range(int(n)):
        pending = []  # [opening step, R, f, k]
        for st in range(int(steps)):
            r, done = rows[st, i, 7], int(bits[st, i] >> 8) & 1
            pending.append([st, np.float32(0), np.float32(1), 0])
            for e in pending:
                e[1] = np.float32(e[1] + np.float32(e[2] * r))
                e[2] = np.float32(e[2] * g)
                e[3] += 1
            keep = []
            for e in pending:
                t, R, _, k = e
                if done or st == steps - 1 or k == N:
                    out[t, i, 7] = R
                    out[t, i, 8:15] = rows[st, i, 8:15]
                    obits[t, i] = (int(bits[t, i]) & ~0x70100) | (done << 8) | ((k - 1) << 16)
                else:
                    keep.append(e)
            pending = keep
    return out.reshape(-1, _lib.PM_TRANS_F)


class SelfPlayRollout:
    """configs[1]'s workload on a PongEnv2PBatch: modelA (effective weights wA, PM_QNET_NW) against
    modelB (packed parameters paramsB, PM_QNET_NP; NoisyNet heads refolded per vector step).

    run(steps) -> dict of STATS accumulated over the call (host ints; reading them synchronises),
    or the device tensor with sync=False."""

    def __init__(self, env, wA, paramsB, epsilon=0.02, seed_net=0):
        self.lib = _lib.load()
        if env.inject is not None:
            raise _lib.PongmiError("SelfPlayRollout uses production (Philox) serves: the env has a serve table")
        if not env.autoreset:
            raise _lib.PongmiError("SelfPlayRollout needs an autoreset env (the rollout never stops an arena)")
        self.env = env
        self.wA = _weights(wA, PM_QNET_NW, "wA", env.device)
        self.paramsB = _weights(paramsB, PM_QNET_NP, "paramsB", env.device)
        self.epsilon = float(epsilon)
        self.seed_net = int(seed_net) & 0xFFFFFFFFFFFFFFFF
        from .qnet import fold
        # modelB's feature layers (its heads are refolded inside the launch every vector step)
        self.wB = fold(self.paramsB, _lib.PM_FOLD_EVAL).reshape(-1)
        self.heads = torch.empty(0, dtype=torch.float32, device=env.device)
        self.stats = torch.zeros(len(STATS_PUSH), dtype=torch.int64, device=env.device)
        # collecting: ep_reward of each arena's running episode (zero it if the env is reset elsewhere)
        self.ep_reward = torch.zeros(env.n, dtype=torch.float32, device=env.device)

    def set_paramsB(self, paramsB):
        """New modelB parameters (e.g. after a generation's training)."""
        from .qnet import fold
        self.paramsB = _weights(paramsB, PM_QNET_NP, "paramsB", self.env.device)
        self.wB = fold(self.paramsB, _lib.PM_FOLD_EVAL).reshape(-1)

    def reserve(self, steps):
        """Allocate the heads workspace for launches of up to `steps` vector steps ahead of time."""
        if self.heads.numel() < int(steps) * PM_ROLL_HEADS:
            self.heads = torch.empty(int(steps) * PM_ROLL_HEADS, dtype=torch.float32, device=self.env.device)

    def _push(self, steps, replay, nstep, gamma):
        """The collecting launch: pm_rollout_push, or with an nstep (1 included) pm_rollout_push_n."""
        env = self.env
        rp = _lib.RollReplay(trans=ptr(replay.trans), prios=ptr(replay.prios), per_work=ptr(replay.work),
                             ep_reward=ptr(self.ep_reward), pos=replay.pos, cap=replay.cap,
                             prio=replay.push_prio(), alpha=replay.alpha)
        args = (ctypes_ref(env.params), ctypes_ref(env.state), ptr(self.wA), ptr(self.wB), ptr(self.paramsB),
                self.epsilon, env.seed, self.seed_net, env.counter, steps, ptr(self.heads), ptr(env.obsA),
                ptr(env.obsB), ctypes_ref(rp), ptr(self.stats), env.n)
        more = () if nstep is None else (int(nstep), float(gamma))  # what the _n entry takes behind n
        name = "pm_rollout_push_n" if more else "pm_rollout_push"
        check(getattr(self.lib, name)(*args, *more, stream_ptr()), name)
        if more:
            replay.max_horizon = max(replay.max_horizon, more[0])
        if steps and env.n:
            if replay.size == 0:
                replay.max_prio = 1.0
            replay.advance(steps * env.n)

    def run(self, steps, sync=True, replay=None, nstep=1, gamma=0.99):
        """replay: None (inference only, pm_rollout) or a DeviceReplay the launch pushes every step's
        transitions into (pm_rollout_push; steps * n <= replay.cap). nstep > 1 (up to PM_NSTEP_MAX), with a
        replay: the rows are n-step transitions over a window of nstep ticks discounted by gamma
        (pm_rollout_push_n; nstep_fold_host is the model). The window is per launch: transitions still pending
        after the last step are written with their shorter horizon. The trajectory and the stats do not depend
        on nstep."""
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps must be >= 0")
        self.reserve(steps)
        self.stats.zero_()
        env = self.env
        names = STATS
        if replay is None:
            check(self.lib.pm_rollout(ctypes_ref(env.params), ctypes_ref(env.state), ptr(self.wA), ptr(self.wB),
                                      ptr(self.paramsB), self.epsilon, env.seed, self.seed_net, env.counter, steps,
                                      ptr(self.heads), ptr(env.obsA), ptr(env.obsB), ptr(self.stats), env.n,
                                      stream_ptr()), "pm_rollout")
        else:
            names = STATS_PUSH
            self._push(steps, replay, None if int(nstep) == 1 else nstep, gamma)
        env.counter += steps
        if not sync:
            return self.stats
        return dict(zip(names, (int(v) for v in self.stats[:len(names)].cpu().tolist())))


def _weights(t, size, name, device):
    require_device(t, name)
    t = t.reshape(-1)
    if t.numel() != size or t.dtype != torch.float32:
        raise ValueError(f"{name} must hold {size} float32 values, got {t.numel()} {t.dtype}")
    t = t.to(device).contiguous()  # the env's device (a no-op when already there)
    if t.data_ptr() % 16:
        t = t.clone()
    return t


_per_member = partial(per_member, "PopulationRollout")


class PopulationRollout(TableHandle):
    """The collecting rollout for a population (pm_rollout_pop_*, csrc/pm_rollout_pop.hip): n members of m arenas
    each, member p playing arenas [p * m, (p + 1) * m) of `env` against its own opponent and pushing into its
    own DeviceReplay, in one launch per phase instead of n solo rollouts. Member p's arenas, observations, ring,
    priorities, sum tree and stats are bit for bit what SelfPlayRollout.run(steps, replay=replays[p]) leaves on a
    PongEnv2PBatch(m, seed=seed_env[p]) holding the member's slice (tests/test_gpu_rollout_pop.py).

    env       a PongEnv2PBatch of n * m arenas, autoreset, no serve table. Its counter is every member's Philox
              step counter; its seed is only the default of seed_env.
    wA        the opponents' effective weights: one [PM_QNET_NW] net for all members, [n, PM_QNET_NW], or a list
              of n [PM_QNET_NW] tensors (members given the same tensor read the one copy). A contiguous, 16-byte
              aligned float32 [n, PM_QNET_NW] tensor on the env's device is PLAYED IN PLACE: the member table holds
              pointers to its rows (self.wA[p] is a view of row p), so whoever rewrites a row on the stream, such
              as pongmi.matchmaking.Matchmaker.assign on its `wA`, changes the opponent from the next collect on,
              with no call here (tests/test_gpu_match.py pins the row addresses).
    params    the members' stacked [n, PM_QNET_NP] modelB blocks, USED IN PLACE (contiguous float32 on the env's
              device): pass DQNPopulation.params and every collect plays what the learners hold, with no copy.
    replays   n distinct DeviceReplays, cap >= steps_max * m each; one whose `work` is None keeps no sum tree.
    epsilon, seed_env, seed_net   one value or n values; seed_env None = env.seed + p.
    nstep, gamma   one value or n values: member p collects n-step rows as SelfPlayRollout.run(nstep=nstep[p],
              gamma=gamma[p]) does (pm_rollout_nstep_pop_set); all ones (the default) is the one-step launch.
    steps_max the most vector steps one collect takes (default: min(32, min(cap) // m)).
    Bad values raise ValueError before anything is allocated.

    collect(steps) refolds every member's feature image from params in one launch (so a stale image after
    DQNPopulation.update_from or exploit() cannot be played), runs the launches, advances every replay's pos /
    size and env.counter, and marks every replay max_prio_stale: the pushed priority max(prios) is taken on the
    device (no host read), so the replays' tracked max_prio is not kept. The library's table holds each ring's
    pos / size as of the last bind plus the transitions pushed since; it is rebound, the interface's only host
    synchronisation after the first collect, only when a replay's pos / size is not what this collector left
    (someone else pushed into it) or one of its buffers was replaced."""
    _entry = "pm_rollout_pop"

    def __init__(self, env, wA, params, *, n, replays, epsilon=0.02, seed_env=None, seed_net=0, steps_max=None,
                 nstep=1, gamma=0.99):
        n = int(n)
        if not 1 <= n <= _lib.PM_DQN_POP_MAX:
            raise ValueError(f"PopulationRollout: n {n} (1..{_lib.PM_DQN_POP_MAX})")
        if env.n < n or env.n % n:
            raise ValueError(f"PopulationRollout: the env's {env.n} arenas are not n = {n} equal slices")
        m = env.n // n
        if env.inject is not None:
            raise ValueError("PopulationRollout uses production (Philox) serves: the env has a serve table")
        if env.autoreset != 1:
            raise ValueError("PopulationRollout needs an autoreset=True env (the rollout never stops an arena)")
        replays = list(replays)
        if len(replays) != n:
            raise ValueError(f"PopulationRollout: {len(replays)} replays for {n} members")
        if len({id(r) for r in replays}) != n:
            raise ValueError("PopulationRollout: members cannot share a replay while collecting")
        if steps_max is None:
            steps_max = max(1, min(32, min(r.cap for r in replays) // m))
        steps_max = int(steps_max)
        if steps_max < 1:
            raise ValueError(f"PopulationRollout: steps_max {steps_max} (>= 1)")
        for p, r in enumerate(replays):
            if steps_max * m > r.cap:
                raise ValueError(f"PopulationRollout: member {p}: steps_max * m = {steps_max * m} > cap {r.cap}")
        eps = [float(x) for x in _per_member("epsilon", epsilon, n)]
        for p, x in enumerate(eps):
            if not math.isfinite(x):
                raise ValueError(f"PopulationRollout: member {p}: epsilon {x}")
        nsteps = [int(x) for x in _per_member("nstep", nstep, n)]
        gammas = [float(x) for x in _per_member("gamma", gamma, n)]
        for p in range(n):
            if not 1 <= nsteps[p] <= _lib.PM_NSTEP_MAX:
                raise ValueError(f"PopulationRollout: member {p}: nstep {nsteps[p]} (1..{_lib.PM_NSTEP_MAX})")
            if not math.isfinite(gammas[p]):
                raise ValueError(f"PopulationRollout: member {p}: gamma {gammas[p]}")
        mask = 0xFFFFFFFFFFFFFFFF
        if seed_env is None:
            seed_env = [env.seed + p for p in range(n)]
        self.seed_env = [int(x) & mask for x in _per_member("seed_env", seed_env, n)]
        self.seed_net = [int(x) & mask for x in _per_member("seed_net", seed_net, n)]
        if not isinstance(params, torch.Tensor) or tuple(params.shape) != (n, PM_QNET_NP) or \
                params.dtype != torch.float32 or not params.is_contiguous():
            raise ValueError(f"PopulationRollout: params must be a contiguous float32 [n={n}, {PM_QNET_NP}] tensor "
                             "(it is used in place)")
        if isinstance(wA, (list, tuple)):  # one net per member; members given the same tensor read one copy
            if len(wA) != n or not all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and
                                       t.numel() == PM_QNET_NW for t in wA):
                raise ValueError(f"PopulationRollout: wA as a list must hold n = {n} float32 [{PM_QNET_NW}] tensors")
        elif not isinstance(wA, torch.Tensor) or wA.dtype != torch.float32 or \
                wA.numel() not in (PM_QNET_NW, n * PM_QNET_NW):
            raise ValueError(f"PopulationRollout: wA must hold {PM_QNET_NW} or n x {PM_QNET_NW} float32 values")
        dev = torch.device(env.device)
        if params.device.type != dev.type or (dev.index is not None and params.device.index != dev.index):
            raise ValueError("PopulationRollout: params must be on the env's device")
        # ---- nothing above allocates
        self.lib = _lib.load()
        self.env, self.n, self.m, self.steps_max = env, n, m, steps_max
        self.params, self.replays, self.epsilon = params, replays, eps
        self.nstep, self.gamma = nsteps, gammas
        self._nstep_set = max(nsteps) == 1  # the handle's horizons are what self.nstep says (all ones at create)
        dev = env.device
        if isinstance(wA, (list, tuple)):
            own = {id(t): _weights(t, PM_QNET_NW, "wA", dev) for t in wA}
            self.wA = [own[id(t)] for t in wA]
        else:
            wA = wA.to(dev).reshape(-1, PM_QNET_NW).contiguous()
            wA = wA.clone() if wA.data_ptr() % 16 else wA
            self.wA = [wA[0 if wA.shape[0] == 1 else p] for p in range(n)]
        f32 = dict(dtype=torch.float32, device=dev)
        self.wB = torch.zeros((n, PM_QNET_NW), **f32)  # the fold writes the images; their pads stay 0
        self.heads = torch.empty((n, steps_max * PM_ROLL_HEADS), **f32)
        self.ep_reward = torch.zeros(env.n, **f32)  # [n, m] flat: each arena's running episode
        self.prio = torch.ones(n, **f32)  # the priority each member's last collect pushed
        self.stats = torch.zeros((n, len(STATS_PUSH)), dtype=torch.int64, device=dev)
        self._members = (_lib.RollMember * n)()
        self._advance = 0    # transitions every member pushed since the table was bound
        self._left = None    # (pos, size) of every replay as the last collect left them
        self._bufs = None    # the replays' buffers the table points into

    def _fill_members(self):
        for p, r in enumerate(self.replays):
            mb = self._members[p]
            mb.wA = self.wA[p].data_ptr()
            mb.wB = self.wB[p].data_ptr()
            mb.paramsB = self.params[p].data_ptr()
            mb.heads_ws = self.heads[p].data_ptr()
            mb.rp = _lib.RollReplay(trans=ptr(r.trans), prios=ptr(r.prios), per_work=ptr(r.work),
                                    ep_reward=self.ep_reward[p * self.m:].data_ptr(), pos=r.pos, cap=r.cap, prio=1.0,
                                    alpha=r.alpha)
            mb.size = r.size
            mb.prio_dev = self.prio[p:].data_ptr()
            mb.stats = self.stats[p].data_ptr()
            mb.epsilon = self.epsilon[p]
            mb.seed_env, mb.seed_net = self.seed_env[p], self.seed_net[p]

    def _bind(self, stream):
        left = [(r.pos, r.size) for r in self.replays]
        bufs = [(ptr(r.trans), ptr(r.prios), ptr(r.work), r.cap, r.alpha) for r in self.replays]
        if self._handle is not None and left == self._left and bufs == self._bufs:
            return
        self._fill_members()
        self._table(True, (ctypes_ref(self.env.params), ctypes_ref(self.env.state), self._members, self.n, self.m,
                           self.steps_max), (self._members, stream))
        self._advance, self._left, self._bufs = 0, left, bufs
        if not self._nstep_set:
            check(self.lib.pm_rollout_nstep_pop_set(self._handle, (_lib.c_i32 * self.n)(*self.nstep),
                                                    (_lib.c_double * self.n)(*self.gamma), stream),
                  "pm_rollout_nstep_pop_set")
            self._nstep_set = True

    def collect(self, steps, sync=True):
        """`steps` vector steps of every member (0..steps_max). Returns the call's stats as a dict of STATS_PUSH
        names to int64 arrays of n (reading them synchronises), or with sync=False the [n, 6] device tensor
        (zeroed by the next collect)."""
        steps = int(steps)
        if not 0 <= steps <= self.steps_max:
            raise ValueError(f"PopulationRollout.collect: steps {steps} (0..steps_max={self.steps_max})")
        env, st = self.env, stream_ptr()
        self.stats.zero_()
        if steps:
            self._bind(st)
            check(self.lib.pm_qnet_fold(ptr(self.params), None, _lib.PM_FOLD_EVAL, 0, 0, None, ptr(self.wB), self.n, st),
                  "pm_qnet_fold")
            check(self.lib.pm_rollout_pop_push(self._handle, env.counter, steps, self._advance, ptr(env.obsA),
                                               ptr(env.obsB), st), "pm_rollout_pop_push")
            pushed = steps * self.m
            self._advance += pushed
            for p, r in enumerate(self.replays):
                r.advance(pushed)
                r.max_prio_stale = True
                r.max_horizon = max(r.max_horizon, self.nstep[p])
            self._left = [(r.pos, r.size) for r in self.replays]
            env.counter += steps
        if not sync:
            return self.stats
        host = self.stats.cpu().numpy()
        return {name: host[:, k].copy() for k, name in enumerate(STATS_PUSH)}
