"""The stand-alone double-DQN learner (K10): train_step (scripts/train_iterative.py:141-168) on a batch
the caller supplies.

DQNLearner owns modelB's and targetB's packed QNet blocks (pongmi.qnet layout), the Adam moments and
the batch buffers; update() runs one train_step on (s, a, r, s', done[, isw]) as one pm_dqn_update
call — modelB on s and s', targetB (eval mode) on s', the double-DQN target, the importance-weighted
squared loss (or, with loss="huber", smooth-L1), the backward, Adam (with max_norm, behind a clip on
the gradient's total norm) and the target sync — with no host synchronisation, and returns the
device tensor of |q - t| for pongmi.replay.per_update. It is the update a caller with a replay of
their own runs; the fused self-play step (pongmi.selfplay.SelfPlayLearner) keeps its own.
update_from() runs the same update on batches drawn from a pongmi.replay.DeviceReplay on the device
(pm_dqn_replay_update: draw, gather, update, priority scatter, incremental tree refresh), and
ReplayTrainer alternates it with the collecting rollout. DQNPopulation (pongmi.dqn_pop) trains n such
learners with one launch per phase.

train_features=False trains the 520 NoisyNet head parameters, as the reference does (it freezes
modelB.features, :97); train_features=True trains all 5 192 parameters of the QNet.

For data-parallel training, grads() / apply() split the update around the gradient all-reduce: every
rank computes its gradient into `grad` ([PM_DQN_NPARAM] gradients, then a 1 marking a contributing
rank), the ranks sum `grad`, then apply() divides by that count and takes the identical Adam step.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import PM_DQN_NPARAM, PM_MAX_BATCH, PM_QNET_HEAD_OFF, PM_QNET_NP, check, stream_ptr
from .checkpoint import adam_moments, adam_state_dict
from .qnet import PARAM_LAYOUT, fold, pack_state_dict, unpack_state_dict

ALL_SHAPES = [s for _, s in PARAM_LAYOUT[:12]]   # modelB.parameters() order
HEAD_SHAPES = [s for _, s in PARAM_LAYOUT[4:12]]  # list(fc_V.parameters()) + list(fc_A.parameters()) (:101-104)


def check_nstep(who, v):
    """nstep as a learner keeps it (1..PM_NSTEP_MAX), or ValueError in `who`'s name."""
    if int(v) != v or not 1 <= int(v) <= _lib.PM_NSTEP_MAX:
        raise ValueError(f"{who}: nstep {v!r} (1..{_lib.PM_NSTEP_MAX})")
    return int(v)


def load_horizon(who, buf, nstep, rows, horizon):
    """Fill rows [0, rows) of a learner's horizon buffer: the given horizons, or nstep for every row. A learner
    built with nstep=1 has no buffer and takes no horizons."""
    if buf is None:
        if horizon is not None:
            raise _lib.PongmiError(f"{who}: horizons given to a learner built with nstep=1 (it would discount every "
                                   "row by gamma)")
        return
    if horizon is None:
        buf[:rows].fill_(nstep)
    else:
        buf[:rows].copy_(torch.as_tensor(horizon).reshape(rows))


def check_replay_horizon(who, replay, nstep):
    if replay.max_horizon > 1 and nstep == 1:
        raise _lib.PongmiError(f"{who}: the replay holds rows of horizon up to {replay.max_horizon} and the learner was "
                               "built with nstep=1 (it would discount every row by gamma); build it with nstep > 1")


def check_option(who, name, v):
    """loss, huber_beta or max_norm as a learner keeps it, or ValueError in `who`'s name."""
    if name == "loss":
        if v not in ("mse", "huber"):
            raise ValueError(f"{who}: loss {v!r} ('mse' or 'huber')")
        return v
    if name == "max_norm" and v is None:
        return None
    v = float(v)
    if not (math.isfinite(v) and v > 0):  # huber_beta whichever loss: a bad value never waits for a switch
        raise ValueError(f"{who}: {name} {v} " + ("(> 0, finite)" if name == "huber_beta" else "(None, or > 0 and finite)"))
    return v


BUFFERS = ("params", "target", "adam_m", "adam_v", "grad", "stats_buf", "s", "ns", "act", "rew", "done", "isw", "td", "q",
           "idx")


class DQNLearner:
    def __init__(self, modelB, target=None, *, batch=256, gamma=0.99, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8,
                 target_update_interval=1000, train_features=False, fresh_noise=True, seed=0, device="cuda",
                 loss="mse", huber_beta=1.0, max_norm=None, nstep=1):
        """modelB / target: a QNet module, its state_dict, or a packed [PM_QNET_NP] tensor; target None = a
        copy of modelB (copy.deepcopy(modelB), :100). batch: the most rows an update takes (1..256).
        loss: "mse" (the reference's importance-weighted squared loss) or "huber"
        ((isw * F.smooth_l1_loss(q, t, reduction='none', beta=huber_beta)).mean()). max_norm: None, or
        clip_grad_norm_(the trained parameters, max_norm) between the gradient and Adam; stats() then
        also reports the total norm before the clip. With both at their defaults every call goes to the
        plain entry points. nstep: 1, or up to PM_NSTEP_MAX for n-step targets: the learner then owns a horizon
        byte per batch row (`horizon`) and row j's target discounts by gamma^horizon[j] (the float32 product
        chain; pm_dqn_*_n). update_from fills the bytes from the replay's rows; update() takes them as
        horizon=, or sets every row to nstep."""
        lib = _lib.load()
        batch = int(batch)
        if not 1 <= batch <= PM_MAX_BATCH:
            raise ValueError(f"DQNLearner: batch {batch} (1..{PM_MAX_BATCH})")
        loss, huber_beta, max_norm = (check_option("DQNLearner", k, v) for k, v in
                                      (("loss", loss), ("huber_beta", huber_beta), ("max_norm", max_norm)))
        nstep = check_nstep("DQNLearner", nstep)
        self.device = torch.device(device)
        params = self._block(modelB)
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=self.device)  # noqa: E731
        buffers = dict(
            params=params, target=self._block(target) if target is not None else params.clone(),
            adam_m=z(PM_DQN_NPARAM), adam_v=z(PM_DQN_NPARAM), grad=z(PM_DQN_NPARAM + 8),
            stats_buf=z(ctypes.sizeof(_lib.DqnStats), dtype=torch.uint8), s=z(batch, 7), ns=z(batch, 7),
            act=z(batch, dtype=torch.int32), rew=z(batch), done=z(batch, dtype=torch.uint8),
            isw=torch.ones(batch, dtype=torch.float32, device=self.device), td=z(batch), q=z(batch, 3),
            idx=z(batch, dtype=torch.int64))  # idx: update_from's sampled slots
        norm = z(1) if max_norm is not None else None  # total norm before the clip of the last apply
        self._attach(lib, self.device, buffers, norm, batch=batch, gamma=gamma, lr=lr, betas=betas, eps=eps,
                     target_update_interval=target_update_interval, train_features=train_features,
                     fresh_noise=fresh_noise, seed=seed, loss=loss, huber_beta=huber_beta, max_norm=max_norm, nstep=nstep,
                     horizon=torch.ones(batch, dtype=torch.uint8, device=self.device) if nstep > 1 else None)

    @classmethod
    def over(cls, lib, device, buffers, norm, **hyper):
        """A learner over existing tensors (one per name in BUFFERS; norm: [1], given exactly when max_norm is) with
        checked hyper-parameters: nothing is validated, allocated or copied. DQNPopulation.member() uses it."""
        self = cls.__new__(cls)
        self._attach(lib, device, buffers, norm, **hyper)
        return self

    def _attach(self, lib, device, buffers, norm, *, batch, gamma, lr, betas, eps, target_update_interval, train_features,
                fresh_noise, seed, loss, huber_beta, max_norm, nstep=1, horizon=None):
        """Everything a learner is, given its buffers: the attributes, the descriptor and the options.
        horizon: the uint8 [batch] horizon buffer, given exactly when nstep > 1."""
        self.lib, self.device, self.batch = lib, device, batch
        self.nstep, self.horizon = nstep, horizon
        self.ns_desc = _lib.DqnNstep(horizon=horizon.data_ptr()) if horizon is not None else None
        self.loss, self.huber_beta, self.max_norm, self.train_features = loss, huber_beta, max_norm, bool(train_features)
        for name in BUFFERS:
            setattr(self, name, buffers[name])
        d = _lib.Dqn()
        for name in ("params", "target", "adam_m", "adam_v", "grad", "s", "ns", "act", "rew", "done", "td", "q"):
            setattr(d, name, getattr(self, name).data_ptr())
        d.stats = self.stats_buf.data_ptr()
        d.isw = None
        d.batch = self.batch
        d.train_features = int(self.train_features)
        d.noise = _lib.PM_FOLD_TRAIN_FRESH if fresh_noise else _lib.PM_FOLD_TRAIN
        d.target_update_interval = int(target_update_interval)
        d.gamma, d.lr, d.beta1, d.beta2, d.adam_eps = float(gamma), float(lr), float(betas[0]), float(betas[1]), \
            float(eps)
        d.seed_net = int(seed)
        self.desc = d
        # the options: None routes every call to the plain entry points, a pm_dqn_opt to the _opt ones
        self.opt, self.norm = None, norm
        if loss != "mse" or max_norm is not None:
            self.opt = _lib.DqnOpt(loss=_lib.PM_DQN_LOSS_HUBER if loss == "huber" else _lib.PM_DQN_LOSS_SQUARED,
                                   huber_beta=huber_beta, max_norm=max_norm if max_norm is not None else 0.0,
                                   norm=norm.data_ptr() if norm is not None else None)

    def _block(self, m):
        if isinstance(m, torch.Tensor):
            if m.numel() != PM_QNET_NP:
                raise ValueError(f"packed QNet block must have {PM_QNET_NP} floats")
            return m.detach().to(self.device, torch.float32).reshape(-1).clone()
        sd = m.state_dict() if hasattr(m, "state_dict") else m
        return pack_state_dict(sd, self.device)

    def load_batch(self, s, a, r, ns, done, isw=None, horizon=None):
        """Copy a batch of n <= batch rows (any device / dtype) into the learner's input buffers. horizon: the
        rows' horizons (1..PM_NSTEP_MAX) for a learner built with nstep > 1; None sets every row to nstep."""
        s = torch.as_tensor(s)
        n = int(s.reshape(-1, 7).shape[0])
        if not 1 <= n <= self.batch:
            raise ValueError(f"DQNLearner: {n} rows (1..{self.batch})")
        self.s[:n].copy_(s.reshape(n, 7))
        self.ns[:n].copy_(torch.as_tensor(ns).reshape(n, 7))
        self.act[:n].copy_(torch.as_tensor(a).reshape(n))
        self.rew[:n].copy_(torch.as_tensor(r).reshape(n))
        self.done[:n].copy_(torch.as_tensor(done).reshape(n))
        if isw is not None:
            self.isw[:n].copy_(torch.as_tensor(isw).reshape(n))
        load_horizon("DQNLearner", self.horizon, self.nstep, n, horizon)
        self.desc.isw = self.isw.data_ptr() if isw is not None else None
        self.desc.batch = n

    def _tier(self, base):
        """The one place this learner's entry points are chosen: base's name and leading arguments with a horizon
        buffer (_n), with options (_opt), or plain."""
        d, o = ctypes.byref(self.desc), ctypes.byref(self.opt) if self.opt else None
        if self.ns_desc is not None and base != "pm_dqn_apply":  # the apply step has no horizon
            return base + "_n", (d, o, ctypes.byref(self.ns_desc))
        return (base, (d,)) if o is None else (base + "_opt", (d, o))

    def _call(self, base, stream=None, *tail):
        name, args = self._tier(base)
        check(getattr(self.lib, name)(*args, *tail, stream_ptr(stream)), name)

    def update(self, *batch, isw=None, horizon=None, stream=None):
        """One train_step; batch = (s, a, r, ns, done[, isw]) or nothing (buffers already filled).
        Returns |q - t| per row (a view of the device buffer `td`): update_priorities' errors (:163)."""
        if batch:
            self.load_batch(*batch, **({"isw": isw} if isw is not None else {}), horizon=horizon)
        self._call("pm_dqn_update", stream)
        return self.td[:self.desc.batch]

    def update_from(self, replay, updates=1, *, beta_start=0.4, beta_frames=100000, seed=0, uniforms=None, stream=None):
        """`updates` train_steps drawn from a pongmi.replay.DeviceReplay in one pm_dqn_replay_update call:
        per update the PER draw of `batch` slots (beta from stats.steps + 1, read on the device), the
        gather of their rows into this learner's batch buffers, the update, and the priorities written
        back with the sum tree refreshed where they changed — no host synchronisation, and the replay's
        tree stays current (no refresh() needed). uniforms: float64 [updates, batch] to replay given
        draws; None draws u53(Philox(j, TAG_PER, frame, seed)). Returns (idx, td) of the last update as
        device tensors (views of `idx` / `td`; idx is -1 where that update was void, see stats()["status"]).
        A learner built with nstep > 1 reads every drawn row's own horizon (pm_dqn_replay_update_n); one built with
        nstep=1 raises PongmiError on a replay that holds longer horizons."""
        check_replay_horizon("DQNLearner.update_from", replay, self.nstep)
        n = self.batch
        updates = int(updates)
        u = None
        if uniforms is not None:
            u = torch.as_tensor(uniforms, dtype=torch.float64).to(self.device).contiguous()
            if u.numel() != max(updates, 0) * n:
                raise ValueError(f"DQNLearner.update_from: uniforms must hold updates x batch = {updates} x {n} values")
        self.desc.isw = self.isw.data_ptr()
        self.desc.batch = n
        rp = _lib.DqnReplay(trans=replay.trans.data_ptr(), prios=replay.prios.data_ptr(), per_work=replay.work.data_ptr(),
                            idx=self.idx.data_ptr(), u=u.data_ptr() if u is not None else None, cap=replay.cap,
                            size=replay.size, alpha=replay.alpha, beta_start=float(beta_start),
                            beta_frames=int(beta_frames), seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._call("pm_dqn_replay_update", stream, ctypes.byref(rp), updates)
        replay.max_prio_stale = True
        return self.idx[:n], self.td[:n]

    def grads(self, *batch, isw=None, horizon=None, stream=None):
        if batch:
            self.load_batch(*batch, **({"isw": isw} if isw is not None else {}), horizon=horizon)
        self._call("pm_dqn_grads", stream)
        return self.td[:self.desc.batch]

    def apply(self, stream=None):
        self._call("pm_dqn_apply", stream)

    # ------------------------------------------------------------------ state
    def _stats(self):
        return _lib.DqnStats.from_buffer_copy(bytes(self.stats_buf.cpu().numpy()))

    def _set_stats(self, **kw):
        s = self._stats()
        for k, v in kw.items():
            setattr(s, k, v)
        self.stats_buf.copy_(torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8))

    def stats(self):
        """(steps, adam_t, loss, mean q) of the last update (host sync); on a learner built with max_norm
        also `norm`, the total gradient norm before the clip of the last apply."""
        s = self._stats()
        out = dict(steps=s.steps, adam_t=s.adam_t, loss=s.loss, q_mean=s.q_mean, status=s.status)
        if self.norm is not None:
            out["norm"] = float(self.norm.cpu()[0])
        return out

    def state_dict(self):
        """modelB's state_dict (reference key names; the epsilon buffers hold the last update's noise)."""
        return unpack_state_dict(self.params)

    def target_state_dict(self):
        return unpack_state_dict(self.target)

    def acting_weights(self, mode=_lib.PM_FOLD_EVAL, seed=0, counter=0):
        """pongmi.qnet.fold of the current modelB block ([PM_QNET_NW]), for pongmi.qnet.act / q_values."""
        return fold(self.params, mode, seed=seed, counter=counter)[0]

    def load_params(self, modelB, target=None):
        """modelB <- state; targetB <- target (default: a copy of the new modelB)."""
        self.params.copy_(self._block(modelB))
        self.target.copy_(self._block(target) if target is not None else self.params)

    # ------------------------------------------------------------------ optimizer / counters
    def _opt_layout(self):
        return (ALL_SHAPES, 0) if self.train_features else (HEAD_SHAPES, PM_QNET_HEAD_OFF)

    def optimizer_state_dict(self):
        """torch.optim.Adam(...).state_dict() over modelB.parameters() (train_features) or over the
        reference's list(fc_V.parameters()) + list(fc_A.parameters()) (:101-104)."""
        shapes, off = self._opt_layout()
        return adam_state_dict(shapes, self.adam_m[off:], self.adam_v[off:], self._stats().adam_t, self.desc.lr,
                               (self.desc.beta1, self.desc.beta2), self.desc.adam_eps)

    def load_optimizer_state_dict(self, sd):
        shapes, off = self._opt_layout()
        m, v, step = adam_moments(sd, shapes)
        self.adam_m[off:].copy_(m)
        self.adam_v[off:].copy_(v)
        self._set_stats(adam_t=step)

    def new_optimizer(self):
        """optim.Adam(..., lr=lr): zero moments, step 0."""
        self.adam_m.zero_()
        self.adam_v.zero_()
        self._set_stats(adam_t=0)

    def set_train_steps(self, steps):
        self._set_stats(steps=int(steps))


class ReplayTrainer:
    """Collect-and-train over the whole QNet (or its heads) at device speed: run(iterations) alternates

        rollout.run(collect_steps, replay=replay, sync=False)   # pm_rollout_push: n * collect_steps transitions
        learner.update_from(replay, updates)                    # pm_dqn_replay_update
        rollout.set_paramsB(learner.params)                     # the next rollout plays the trained modelB

    and returns the accumulated rollout stats (pongmi.rollout.STATS_PUSH) as host ints. Per iteration the
    host reads 4 bytes (DeviceReplay.push_prio's max(prios), the priority memory.push stores, :57) and
    nothing else; the stats are summed on the device and read once at the end."""

    def __init__(self, env, wA, learner, replay, *, collect_steps, updates, epsilon=0.02, seed_net=0, beta_start=0.4,
                 beta_frames=100000, seed=0, nstep=None):
        """nstep: the collector's window (None: the learner's nstep). The collector discounts by the learner's gamma;
        a window above 1 needs a learner built with nstep > 1."""
        from .rollout import SelfPlayRollout
        self.nstep = learner.nstep if nstep is None else check_nstep("ReplayTrainer", nstep)
        if self.nstep > 1 and learner.nstep == 1:
            raise ValueError(f"ReplayTrainer: nstep {self.nstep} with a learner built with nstep=1")
        self.learner, self.replay = learner, replay
        self.collect_steps, self.updates = int(collect_steps), int(updates)
        if self.collect_steps < 1 or self.updates < 1:
            raise ValueError("ReplayTrainer: collect_steps and updates must be >= 1")
        if self.collect_steps * env.n > replay.cap:
            raise ValueError(f"ReplayTrainer: collect_steps * arenas = {self.collect_steps * env.n} > cap {replay.cap}")
        self.beta_start, self.beta_frames, self.seed = float(beta_start), int(beta_frames), int(seed)
        self.rollout = SelfPlayRollout(env, wA, learner.params, epsilon=epsilon, seed_net=seed_net)

    def run(self, iterations):
        from .rollout import STATS_PUSH
        total = torch.zeros_like(self.rollout.stats)
        for _ in range(int(iterations)):
            total += self.rollout.run(self.collect_steps, replay=self.replay, sync=False, nstep=self.nstep,
                                      gamma=self.learner.desc.gamma)
            self.learner.update_from(self.replay, self.updates, beta_start=self.beta_start,
                                     beta_frames=self.beta_frames, seed=self.seed)
            self.rollout.set_paramsB(self.learner.params)
        return dict(zip(STATS_PUSH, (int(v) for v in total.cpu().tolist())))


class PopulationTrainer:
    """ReplayTrainer for a population: run(iterations) alternates

        rollout.collect(collect_steps, sync=False)       # pm_rollout_pop_push: m * collect_steps transitions per member
        population.update_from(replays, updates)         # pm_dqn_pop_replay_update

    with `rollout` a pongmi.rollout.PopulationRollout over population.params in place (every collect refolds the
    members' feature images first, so it plays what the learners hold), and returns the accumulated rollout
    stats (pongmi.rollout.STATS_PUSH) as int64 arrays of n. Member p's rings, learner state and stats are bit for
    bit those of a ReplayTrainer on a PongEnv2PBatch(m, seed=seed_env[p]) holding the member's slice.

    Host synchronisation: the stats are summed on the device and read once at the end, and the pushed priority
    max(prios) is taken on the device. While the rings are still filling, DQNPopulation rebinds its table once
    per iteration (the table holds each ring's fill `size`), which waits for the stream; once every ring is full
    a run() performs no host synchronisation until that final read."""

    def __init__(self, env, wA, population, replays, *, collect_steps, updates, epsilon=0.02, seed_env=None, seed_net=0,
                 beta_start=0.4, beta_frames=100000, seed=0, nstep=None):
        """nstep: the collectors' windows, one value or n (None: the members' own nstep). Member p's collector
        discounts by member p's gamma; a window above 1 needs a member built with nstep > 1."""
        from ._pop import per_member
        from .rollout import PopulationRollout
        own = list(getattr(population, "nstep", [1] * population.n))  # a population without the attribute: one step
        self.nstep = own if nstep is None else \
            [check_nstep("PopulationTrainer", x) for x in per_member("PopulationTrainer", "nstep", nstep, population.n)]
        for p, k in enumerate(self.nstep):
            if k > 1 and own[p] == 1:
                raise ValueError(f"PopulationTrainer: member {p}: nstep {k} with a member built with nstep=1")
        self.population, self.replays = population, list(replays)
        self.collect_steps, self.updates = int(collect_steps), int(updates)
        if self.collect_steps < 1 or self.updates < 1:
            raise ValueError("PopulationTrainer: collect_steps and updates must be >= 1")
        self.beta_start, self.beta_frames, self.seed = float(beta_start), int(beta_frames), seed
        self.rollout = PopulationRollout(env, wA, population.params, n=population.n, replays=self.replays,
                                         epsilon=epsilon, seed_env=seed_env, seed_net=seed_net,
                                         steps_max=self.collect_steps, nstep=self.nstep,
                                         gamma=population.hyper["gamma"] if max(self.nstep) > 1 else 0.99)

    def run(self, iterations):
        from .rollout import STATS_PUSH
        total = torch.zeros_like(self.rollout.stats)
        for _ in range(int(iterations)):
            total += self.rollout.collect(self.collect_steps, sync=False)
            self.population.update_from(self.replays, self.updates, beta_start=self.beta_start,
                                        beta_frames=self.beta_frames, seed=self.seed)
        host = total.cpu().numpy()
        return {name: host[:, k].copy() for k, name in enumerate(STATS_PUSH)}


from .dqn_pop import DQNPopulation  # noqa: E402,F401  (pongmi.dqn.DQNPopulation; dqn_pop imports DQNLearner from here)
