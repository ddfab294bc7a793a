"""A population of stand-alone double-DQN learners trained together (K12: pm_dqn_pop_*).

DQNPopulation holds n independent members in stacked tensors (params [n, PM_QNET_NP], target, adam_m /
adam_v [n, PM_DQN_NPARAM], grad, stats_buf, td, q, idx, norm, and the batch buffers [n, batch, ...]) and
trains all of them with one launch per phase, a grid of n workgroups, workgroup p running member p. Each
member has its own hyper-parameters, loss and clip options, and is bit for bit what a DQNLearner built with
that member's arguments computes: learning-rate, loss or gamma sweeps, seed replicates, a league of agents
and population-based training (exploit(), set_hyper()) cost one call per step instead of n.

update() is DQNLearner.update for every member (pm_dqn_pop_update); update_from() is
DQNLearner.update_from with one pongmi.replay.DeviceReplay per member (pm_dqn_pop_replay_update); members
may share a ring's `trans` tensor and keep priorities of their own. With shared_batch=True there is one
set of batch buffers that every member reads (a hyper-parameter sweep on one batch); update_from needs
batch buffers per member.

The library keeps the members' descriptors in a device table. The class remembers what the bound table
holds (rows, isw, hyper-parameters, and for update_from the replays' buffers and fill sizes, the uniforms
and the draw's arguments) and rebinds, the interface's only host synchronisation, when one of them changed:
a loop over a fixed batch shape, or over full replays, never synchronises.
"""
import ctypes
from functools import partial

import numpy as np
import torch

from . import _lib
from ._lib import PM_DQN_NPARAM, PM_DQN_POP_MAX, PM_MAX_BATCH, PM_QNET_NP, check, stream_ptr
from ._pop import TableHandle, per_member
from .dqn import BUFFERS, DQNLearner, check_nstep, check_option, check_replay_horizon, load_horizon
from .qnet import fold, unpack_state_dict

PER_MEMBER = ("gamma", "lr", "betas", "eps", "target_update_interval", "train_features", "fresh_noise", "seed", "loss",
              "huber_beta", "max_norm")
_STATS_DTYPE = np.dtype([("steps", "<i8"), ("adam_t", "<i8"), ("loss", "<f4"), ("q_mean", "<f4"), ("status", "<i4"),
                         ("_pad", "<i4")])
_per_member = partial(per_member, "DQNPopulation")


def _validate(name, v):
    """One member's value of one hyper-parameter, as the descriptor stores it."""
    if name in ("loss", "huber_beta", "max_norm"):
        return check_option("DQNPopulation", name, v)
    if name == "betas":
        if len(v) != 2:
            raise ValueError(f"DQNPopulation: betas {v!r} (a pair)")
        return float(v[0]), float(v[1])
    if name == "target_update_interval":
        if int(v) < 1:
            raise ValueError(f"DQNPopulation: target_update_interval {v} (>= 1)")
        return int(v)
    if name in ("train_features", "fresh_noise"):
        return bool(v)
    if name == "seed":
        return int(v) & 0xFFFFFFFFFFFFFFFF
    return float(v)  # gamma, lr, eps


class DQNPopulation(TableHandle):
    _entry = "pm_dqn_pop"

    def __init__(self, models, targets=None, *, n=None, batch=256, device="cuda", shared_batch=False, gamma=0.99,
                 lr=2.5e-4, betas=(0.9, 0.999), eps=1e-8, target_update_interval=1000, train_features=False,
                 fresh_noise=True, seed=0, loss="mse", huber_beta=1.0, max_norm=None, nstep=1):
        """models / targets: a sequence of n QNet modules, state_dicts or packed [PM_QNET_NP] tensors, a stacked
        [n, PM_QNET_NP] tensor, or ONE of them with n given (every member starts from a copy); targets None =
        copies of models. batch: the most rows an update takes (1..256). It and every other keyword of
        DQNLearner's are given as one value for all members or as a sequence of n (the stacked batch buffers
        have max(batch) rows; update_from draws batch[p] rows for member p). nstep: one value or n, as
        DQNLearner's: members with nstep > 1 get a row of the stacked `horizon` bytes [n, batch]
        (pm_dqn_nstep_pop_set), the others keep the one-step target. Bad values raise ValueError before anything
        is allocated."""
        many = isinstance(models, (list, tuple)) or (isinstance(models, torch.Tensor) and models.dim() == 2)
        if n is None:
            if not many:
                raise ValueError("DQNPopulation: give n, or a sequence of models")
            n = len(models)
        n = int(n)
        if not 1 <= n <= PM_DQN_POP_MAX:
            raise ValueError(f"DQNPopulation: n {n} (1..{PM_DQN_POP_MAX})")
        if many and len(models) != n:
            raise ValueError(f"DQNPopulation: {len(models)} models for {n} members")
        t_many = isinstance(targets, (list, tuple)) or (isinstance(targets, torch.Tensor) and targets.dim() == 2)
        if t_many and len(targets) != n:
            raise ValueError(f"DQNPopulation: {len(targets)} targets for {n} members")
        self.batches = [int(b) for b in _per_member("batch", batch, n)]  # the most rows each member's update takes
        for b in self.batches:
            if not 1 <= b <= PM_MAX_BATCH:
                raise ValueError(f"DQNPopulation: batch {b} (1..{PM_MAX_BATCH})")
        self.batch = max(self.batches)  # the stacked buffers' row count
        if shared_batch and min(self.batches) != self.batch:
            raise ValueError("DQNPopulation: shared_batch needs one batch size for every member")
        given = dict(gamma=gamma, lr=lr, betas=betas, eps=eps, target_update_interval=target_update_interval,
                     train_features=train_features, fresh_noise=fresh_noise, seed=seed, loss=loss, huber_beta=huber_beta,
                     max_norm=max_norm)
        self.hyper = {k: [_validate(k, v) for v in _per_member(k, given[k], n, k == "betas")] for k in PER_MEMBER}
        self.nstep = [check_nstep("DQNPopulation", v) for v in _per_member("nstep", nstep, n)]
        # ---- nothing above allocates
        self.lib = _lib.load()
        self.n, self.shared_batch = n, bool(shared_batch)
        self.device = torch.device(device)
        self.params = self._blocks(models, many)
        self.target = self._blocks(targets, t_many) if targets is not None else self.params.clone()
        f32 = dict(dtype=torch.float32, device=self.device)
        B = self.batch
        self.adam_m = torch.zeros((n, PM_DQN_NPARAM), **f32)
        self.adam_v = torch.zeros((n, PM_DQN_NPARAM), **f32)
        self.grad = torch.zeros((n, PM_DQN_NPARAM + 8), **f32)
        self.stats_buf = torch.zeros((n, ctypes.sizeof(_lib.DqnStats)), dtype=torch.uint8, device=self.device)
        lead = () if self.shared_batch else (n,)
        self.s = torch.zeros(lead + (B, 7), **f32)
        self.ns = torch.zeros(lead + (B, 7), **f32)
        self.act = torch.zeros(lead + (B,), dtype=torch.int32, device=self.device)
        self.rew = torch.zeros(lead + (B,), **f32)
        self.done = torch.zeros(lead + (B,), dtype=torch.uint8, device=self.device)
        self.isw = torch.ones(lead + (B,), **f32)
        self.td = torch.zeros((n, B), **f32)
        self.q = torch.zeros((n, B, 3), **f32)
        self.idx = torch.zeros((n, B), dtype=torch.int64, device=self.device)  # update_from's sampled slots
        self.norm = torch.zeros(n, **f32)  # every member's total gradient norm before the clip of its last apply
        # the members' horizon bytes (rows of their own even with shared_batch: the replay gather writes them)
        self.horizon = torch.ones((n, B), dtype=torch.uint8, device=self.device) if max(self.nstep) > 1 else None
        self._ns = (_lib.DqnNstep * n)()
        for p in range(n):
            self._ns[p].horizon = self.horizon[p].data_ptr() if self.nstep[p] > 1 else None
        self._ns_set = self.horizon is None  # the handle's horizon buffers are _ns (none at create)
        self._d = (_lib.Dqn * n)()
        self._o = (_lib.DqnOpt * n)()
        for p in range(n):
            d = self._d[p]
            for name in ("params", "target", "adam_m", "adam_v", "grad", "td", "q"):
                setattr(d, name, getattr(self, name)[p].data_ptr())
            d.stats = self.stats_buf[p].data_ptr()
            for name in ("s", "ns", "act", "rew", "done"):
                t = getattr(self, name)
                setattr(d, name, (t if self.shared_batch else t[p]).data_ptr())
            d.isw = None
            d.batch = self.batches[p]
            self._o[p].norm = self.norm[p:p + 1].data_ptr()
        self._write_hyper()
        self._bound = None    # (bytes of _d, bytes of _o, bytes of the replay descriptors or None) the table holds
        self._rp = None       # the bound replay descriptors, kept across update() rebinds
        self._rp_key = None   # what _rp was built from
        self._keep = None     # the replays and the uniforms the table points into

    def _blocks(self, m, many):
        if isinstance(m, torch.Tensor) and m.dim() == 2:
            if m.shape[1] != PM_QNET_NP:
                raise ValueError(f"stacked QNet blocks must be [n, {PM_QNET_NP}]")
            return m.detach().to(self.device, torch.float32).contiguous().clone()
        one = lambda x: DQNLearner._block(self, x).reshape(1, -1)  # noqa: E731
        if many:
            return torch.cat([one(x) for x in m]).contiguous()
        return one(m).repeat(self.n, 1).contiguous()

    def _write_hyper(self):
        h = self.hyper
        for p in range(self.n):
            d, o = self._d[p], self._o[p]
            d.train_features = int(h["train_features"][p])
            d.noise = _lib.PM_FOLD_TRAIN_FRESH if h["fresh_noise"][p] else _lib.PM_FOLD_TRAIN
            d.target_update_interval = h["target_update_interval"][p]
            d.gamma, d.lr, d.adam_eps = h["gamma"][p], h["lr"][p], h["eps"][p]
            d.beta1, d.beta2 = h["betas"][p]
            d.seed_net = h["seed"][p]
            o.loss = _lib.PM_DQN_LOSS_HUBER if h["loss"][p] == "huber" else _lib.PM_DQN_LOSS_SQUARED
            o.huber_beta = h["huber_beta"][p]
            o.max_norm = h["max_norm"][p] if h["max_norm"][p] is not None else 0.0

    def set_hyper(self, **kw):
        """Change per-member hyper-parameters (any of PER_MEMBER: one value, or a sequence of n). The next update
        rebinds the table, which waits for the stream once."""
        new = {}
        for k, v in kw.items():
            if k not in PER_MEMBER:
                raise ValueError(f"DQNPopulation: unknown hyper-parameter {k!r}")
            new[k] = [_validate(k, x) for x in _per_member(k, v, self.n, k == "betas")]
        self.hyper.update(new)
        self._write_hyper()

    # ------------------------------------------------------------------ batches
    def _load(self, p, s, a, r, ns, done, isw, horizon=None):
        s = torch.as_tensor(s)
        rows = int(s.reshape(-1, 7).shape[0])
        cap = self.batch if p is None else self.batches[p]
        if not 1 <= rows <= cap:
            raise ValueError(f"DQNPopulation: {rows} rows (1..{cap})")
        pick = (lambda t: t) if self.shared_batch else (lambda t: t[p])
        pick(self.s)[:rows].copy_(s.reshape(rows, 7))
        pick(self.ns)[:rows].copy_(torch.as_tensor(ns).reshape(rows, 7))
        pick(self.act)[:rows].copy_(torch.as_tensor(a).reshape(rows))
        pick(self.rew)[:rows].copy_(torch.as_tensor(r).reshape(rows))
        pick(self.done)[:rows].copy_(torch.as_tensor(done).reshape(rows))
        if isw is not None:
            pick(self.isw)[:rows].copy_(torch.as_tensor(isw).reshape(rows))
        for q in (range(self.n) if self.shared_batch else (p,)):
            self._d[q].isw = pick(self.isw).data_ptr() if isw is not None else None
            self._d[q].batch = rows
            load_horizon("DQNPopulation", self.horizon[q] if self.nstep[q] > 1 else None, self.nstep[q], rows,
                         horizon if self.nstep[q] > 1 or not self.shared_batch else None)

    def load_batch(self, member, s, a, r, ns, done, isw=None, horizon=None):
        """Copy rows <= batch rows (any device / dtype) into one member's input buffers; with shared_batch into
        the one set every member reads (`member` is then ignored). horizon: the rows' horizons for members built
        with nstep > 1 (None: the member's nstep for every row)."""
        if not self.shared_batch and not 0 <= int(member) < self.n:
            raise ValueError(f"DQNPopulation: member {member} (0..{self.n - 1})")
        self._load(None if self.shared_batch else int(member), s, a, r, ns, done, isw, horizon)

    def load_batches(self, s, a, r, ns, done, isw=None, horizon=None):
        """Stacked inputs, [n, rows, ...] (the same row count for every member); with shared_batch [rows, ...]."""
        if self.shared_batch:
            return self._load(None, s, a, r, ns, done, isw, horizon)
        s, a, r, ns, done = (torch.as_tensor(x) for x in (s, a, r, ns, done))
        if s.shape[0] != self.n:
            raise ValueError(f"DQNPopulation: {s.shape[0]} stacked batches for {self.n} members")
        for p in range(self.n):
            self._load(p, s[p], a[p], r[p], ns[p], done[p], None if isw is None else torch.as_tensor(isw)[p],
                       None if horizon is None else torch.as_tensor(horizon)[p])

    def rows(self):
        """The row count each member's next update() takes."""
        return [self._d[p].batch for p in range(self.n)]

    # ------------------------------------------------------------------ the table
    def _bind(self, rp, stream):
        """Make the device table hold (_d, _o, rp): create it, or rebind it if it holds something else."""
        want = (bytes(self._d), bytes(self._o), bytes(rp) if rp is not None else None)
        self._table(want != self._bound, (self._d, self._o, rp, self.n), (self._d, self._o, rp, stream_ptr(stream)))
        self._bound = want
        if not self._ns_set:
            check(self.lib.pm_dqn_nstep_pop_set(self._handle, self._ns, stream_ptr(stream)), "pm_dqn_nstep_pop_set")
            self._ns_set = True

    def update(self, stream=None):
        """One train_step of every member on the batch its buffers hold, as one launch. Returns td [n, batch]
        (member p's |q - t| in td[p, :rows]), the device buffer itself."""
        if self._bound is not None and self._bound[:2] == (bytes(self._d), bytes(self._o)):
            rp = self._rp  # nothing update() reads changed: a table with replay descriptors serves as it is
        else:
            rp = self._rp if self._rp is not None and all(d.isw for d in self._d) else None
            if rp is None:
                self._rp = self._rp_key = None
        self._bind(rp, stream)
        check(self.lib.pm_dqn_pop_update(self._handle, stream_ptr(stream)), "pm_dqn_pop_update")
        return self.td

    def update_from(self, replays, updates=1, *, beta_start=0.4, beta_frames=100000, seed=0, uniforms=None, stream=None):
        """`updates` train_steps of every member, member p drawing from replays[p] (a pongmi.replay.DeviceReplay):
        DQNLearner.update_from for all members in `updates` x three launches. Members may share a ring:
        DeviceReplays whose `trans` is the same tensor, each with its own prios / work. seed: one value or n;
        uniforms: float64 [n, updates, batch] to replay given draws (a sequence of n [updates, batch[p]] arrays
        where the members' batch sizes differ). Marks every replay max_prio_stale.
        Returns (idx, td) of the last update, [n, batch] device buffers (idx[p] is -1 where member p's last
        update was void, see stats()["status"])."""
        n = self.n
        if self.shared_batch:
            raise ValueError("DQNPopulation.update_from: needs batch buffers per member (shared_batch=False)")
        replays = list(replays)
        if len(replays) != n:
            raise ValueError(f"DQNPopulation.update_from: {len(replays)} replays for {n} members")
        for p, r in enumerate(replays):
            check_replay_horizon(f"DQNPopulation.update_from: member {p}", r, self.nstep[p])
        updates = int(updates)
        seeds = [int(x) & 0xFFFFFFFFFFFFFFFF for x in _per_member("seed", seed, n)]
        u = None
        u_off = np.concatenate([[0], np.cumsum([max(updates, 0) * b for b in self.batches])]).tolist()  # in values
        if uniforms is not None:
            if isinstance(uniforms, (list, tuple)):
                uniforms = torch.cat([torch.as_tensor(x, dtype=torch.float64).reshape(-1) for x in uniforms])
            u = uniforms if isinstance(uniforms, torch.Tensor) and uniforms.dtype == torch.float64 and \
                uniforms.device == self.device and uniforms.is_contiguous() else \
                torch.as_tensor(uniforms, dtype=torch.float64).to(self.device).contiguous()
            if u.numel() != u_off[-1]:
                raise ValueError(f"DQNPopulation.update_from: uniforms must hold updates x batch = {updates} x "
                                 f"{self.batches} values per member")
        for p in range(n):
            self._d[p].isw = self.isw[p].data_ptr()
            self._d[p].batch = self.batches[p]
        key = (tuple((id(r), r.trans.data_ptr(), r.prios.data_ptr(), r.work.data_ptr(), r.cap, r.size, r.alpha)
                     for r in replays), u.data_ptr() if u is not None else None, max(updates, 0) if u is not None else 0,
               float(beta_start), int(beta_frames), tuple(seeds))
        if key != self._rp_key:
            rp = (_lib.DqnReplay * n)()
            for p, r in enumerate(replays):
                rp[p] = _lib.DqnReplay(trans=r.trans.data_ptr(), prios=r.prios.data_ptr(), per_work=r.work.data_ptr(),
                                       idx=self.idx[p].data_ptr(),
                                       u=u.data_ptr() + 8 * u_off[p] if u is not None else None, cap=r.cap,
                                       size=r.size, alpha=r.alpha, beta_start=float(beta_start),
                                       beta_frames=int(beta_frames), seed=seeds[p])
            self._rp, self._rp_key, self._keep = rp, key, (replays, u)
        self._bind(self._rp, stream)
        check(self.lib.pm_dqn_pop_replay_update(self._handle, updates, stream_ptr(stream)), "pm_dqn_pop_replay_update")
        for r in replays:
            r.max_prio_stale = True
        return self.idx, self.td

    # ------------------------------------------------------------------ state
    def stats(self):
        """Every member's counters and last-update figures as arrays of n (one read of the stacked stats, one of
        norm): steps, adam_t, loss, q_mean, status, norm (a member's total gradient norm before the clip of
        its last apply; 0 until it took one)."""
        st = np.frombuffer(bytes(self.stats_buf.cpu().numpy()), dtype=_STATS_DTYPE)
        out = {k: st[k].copy() for k in ("steps", "adam_t", "loss", "q_mean", "status")}
        out["norm"] = self.norm.cpu().numpy()
        return out

    def state_dict(self, member):
        """Member's modelB state_dict (reference key names)."""
        return unpack_state_dict(self.params[member])

    def target_state_dict(self, member):
        return unpack_state_dict(self.target[member])

    def acting_weights(self, mode=_lib.PM_FOLD_EVAL, seed=0, counter=0):
        """pongmi.qnet.fold of every member's modelB block, [n, PM_QNET_NW]: the nets play_matches takes."""
        return torch.stack([fold(self.params[p], mode, seed=seed, counter=counter)[0].reshape(-1) for p in range(self.n)])

    def member(self, i):
        """A DQNLearner over member i's slices of the stacked tensors (views, not copies): state_dict(),
        target_state_dict(), optimizer_state_dict(), load_optimizer_state_dict(), stats(), so checkpoints go
        through the existing code. It carries the member's hyper-parameters as they are now."""
        i = int(i)
        if not 0 <= i < self.n:
            raise ValueError(f"DQNPopulation: member {i} (0..{self.n - 1})")
        h = {k: v[i] for k, v in self.hyper.items()}
        batch, buffers = self.batches[i], {}
        for name in BUFFERS:
            t = getattr(self, name)
            t = t if self.shared_batch and name in ("s", "ns", "act", "rew", "done", "isw") else t[i]
            buffers[name] = t if name in ("params", "target", "adam_m", "adam_v", "grad", "stats_buf") else t[:batch]
        L = DQNLearner.over(self.lib, self.device, buffers, self.norm[i:i + 1] if h["max_norm"] is not None else None,
                            batch=batch, nstep=self.nstep[i],
                            horizon=self.horizon[i][:batch] if self.nstep[i] > 1 else None, **h)
        L.desc.isw, L.desc.batch = self._d[i].isw, self._d[i].batch  # as the table has them now
        return L

    # ------------------------------------------------------------------ population-based training
    def exploit(self, src_of):
        """Member p takes params, target, both Adam moments and the steps / adam_t counters of member src_of[p],
        gathered from the state before the call. src_of: n indices, a host sequence or a device tensor (so a
        ranking computed on the device drives it with no host read). Hyper-parameters stay the members' own."""
        src = torch.as_tensor(src_of).to(device=self.device, dtype=torch.long).reshape(-1)
        if src.numel() != self.n:
            raise ValueError(f"DQNPopulation.exploit: {src.numel()} sources for {self.n} members")
        for t in (self.params, self.target, self.adam_m, self.adam_v):
            t.copy_(t[src])
        counters = self.stats_buf.view(torch.int64)  # [n, 4]: steps, adam_t, (loss | q_mean), (status | pad)
        counters[:, :2] = counters[src, :2]
