"""Prioritized replay on the device (K4: pm_per_sample / pm_per_update).

Mirrors PrioritizedReplay (scripts/train_iterative.py:49-76): proportional sampling of
prios[0:size]^alpha with replacement, IS weights (size * P(i))^-beta / max, priority update
|err| + 1e-6 with the last duplicate winning.
"""
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

_work = {}


def _workspace(cap, device):
    key = (int(cap), str(device))
    if key not in _work:
        nbytes = _lib.load().pm_per_work_bytes(int(cap))
        _work[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    return _work[key]


def per_sample(prios, size, bs, beta, alpha=0.6, uniforms=None, seed=0, counter=0, stream=None):
    """Returns (idx int64 [bs], weights f32 [bs]). `uniforms` (float64 [bs]) replays
    np.random.choice's own draws; None draws them from Philox(seed, counter)."""
    lib = _lib.load()
    _lib.require_device(prios, "prios")
    dev = prios.device
    idx = torch.empty(bs, dtype=torch.int64, device=dev)
    w = torch.empty(bs, dtype=torch.float32, device=dev)
    if uniforms is not None:
        uniforms = torch.as_tensor(uniforms, dtype=torch.float64).to(dev).contiguous()
    work = _workspace(prios.numel(), dev)
    check(lib.pm_per_sample(ptr(prios), int(size), float(alpha), float(beta), ptr(uniforms), int(seed), int(counter),
                            ptr(idx), ptr(w), int(bs), ptr(work), stream_ptr(stream)), "pm_per_sample")
    return idx, w


def per_update(prios, idx, errors, stream=None):
    lib = _lib.load()
    idx = idx.to(device=prios.device, dtype=torch.int64).contiguous()
    errors = errors.to(device=prios.device, dtype=torch.float32).contiguous()
    check(lib.pm_per_update(ptr(prios), ptr(idx), ptr(errors), idx.numel(), stream_ptr(stream)), "pm_per_update")


class DeviceReplay:
    """The replay ring of PrioritizedReplay (train_iterative.py:49-63) as device buffers, filled by the
    collecting rollout (pongmi.rollout.SelfPlayRollout.run(..., replay=...), pm_rollout_push):
    trans [cap][PM_TRANS_F] rows (s[7], r, s'[7], bits(a | done << 8)), prios [cap], and the PER sum
    tree of pm_per_sample (`work`), which every collecting launch leaves current. pos / size mirror
    memory.pos / len(memory.buffer); max_prio is the priority the next push stores (max(prios), 1.0
    while empty, :57) — pushes never change it, so it is tracked here; call refresh() after
    changing prios by other means (it also rebuilds the sum tree). push() adds the caller's own
    transitions (pm_replay_push); DQNLearner.update_from trains from the ring and keeps the tree
    current itself (it marks max_prio stale, and the next push_prio() re-reads it).
    A row carries its own n-step horizon (1..PM_NSTEP_MAX, as k - 1 in bits 16..18 of its last word; rows
    pushed without one are one step). max_horizon is the largest ever pushed into this ring, by push(horizon=)
    or by an n-step collector: a learner built with nstep=1 refuses a ring where it is above 1."""

    def __init__(self, cap, device, alpha=0.6):
        self.cap = int(cap)
        if self.cap <= 0:
            raise ValueError("cap must be > 0")
        self.alpha = float(alpha)
        self.trans = torch.zeros((self.cap, _lib.PM_TRANS_F), dtype=torch.float32, device=device)
        self.prios = torch.zeros(self.cap, dtype=torch.float32, device=device)
        nbytes = _lib.load().pm_per_work_bytes(self.cap)
        self.work = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=device)
        self.pos = 0
        self.size = 0
        self.max_prio = 1.0
        self.max_prio_stale = False  # set by DQNLearner.update_from: prios changed on the device
        self.max_horizon = 1

    def push_prio(self):
        """The priority the next push stores. After DQNLearner.update_from changed prios on the device the
        tracked maximum is stale: it is read back once here (self.prios.max(), :57 — a 4-byte host sync)."""
        if self.max_prio_stale and self.size > 0:
            self.max_prio = float(self.prios[:self.size].max())
        self.max_prio_stale = False
        return self.max_prio if self.size > 0 else 1.0

    def advance(self, pushed):
        self.pos = (self.pos + pushed) % self.cap
        self.size = min(self.cap, self.size + pushed)

    def push(self, s, a, r, ns, done, stream=None, horizon=None):
        """memory.push (:56-63) of n <= cap transitions of the caller's (tensors or arrays of any device /
        dtype: s, ns [n, 7]; a in 0..2, r, done [n]) at pos with push_prio() as their priority
        (pm_replay_push); the sum tree stays current. Actions are checked where the host sees them (inputs
        not on the device). horizon: None (one-step rows), or [n] values in 1..PM_NSTEP_MAX for the caller's own
        n-step rows (r then the n-step reward, ns the state after the last of the row's ticks; pm_replay_push_n).
        Its maximum is read on the host (a sync where it is a device tensor)."""
        dev = self.trans.device
        s = torch.as_tensor(s)
        n = int(s.reshape(-1, 7).shape[0])
        if not 1 <= n <= self.cap:
            raise ValueError(f"DeviceReplay.push: {n} transitions (1..cap={self.cap})")
        a = torch.as_tensor(a).reshape(n)
        if not a.is_cuda and n and (int(a.min()) < 0 or int(a.max()) > 2):
            raise ValueError("DeviceReplay.push: actions must be 0, 1 or 2")
        f32 = dict(device=dev, dtype=torch.float32)
        s = s.reshape(n, 7).to(**f32).contiguous()
        ns = torch.as_tensor(ns).reshape(n, 7).to(**f32).contiguous()
        r = torch.as_tensor(r).reshape(n).to(**f32).contiguous()
        a = a.to(device=dev, dtype=torch.int32).contiguous()
        done = torch.as_tensor(done).reshape(n).to(device=dev, dtype=torch.uint8).contiguous()
        if horizon is not None:
            horizon = torch.as_tensor(horizon).reshape(n)
            lo, hi = int(horizon.min()), int(horizon.max())
            if lo < 1 or hi > _lib.PM_NSTEP_MAX:
                raise ValueError(f"DeviceReplay.push: horizons must be 1..{_lib.PM_NSTEP_MAX}")
            horizon = horizon.to(device=dev, dtype=torch.uint8).contiguous()
        name = "pm_replay_push"
        args = [ptr(self.trans), ptr(self.prios), ptr(self.work), self.cap, self.pos, self.alpha, self.push_prio(), ptr(s),
                ptr(a), ptr(r), ptr(ns), ptr(done)]
        if horizon is not None:  # the _n entry takes the horizons behind done
            name += "_n"
            args.append(ptr(horizon))
        check(getattr(_lib.load(), name)(*args, n, stream_ptr(stream)), name)
        if horizon is not None:
            self.max_horizon = max(self.max_horizon, hi)
        if self.size == 0:
            self.max_prio = 1.0
        self.advance(n)

    def refresh(self):
        """After the host changed prios: rebuild the sum tree (pm_per_build) and the tracked max."""
        check(_lib.load().pm_per_build(ptr(self.prios), self.cap, self.alpha, ptr(self.work), stream_ptr()),
              "pm_per_build")
        self.max_prio = float(self.prios[:self.size].max()) if self.size else 1.0
        self.max_prio_stale = False

    def leaves(self):
        """The PER leaves (prio^alpha, f32 [cap]) inside the tree workspace."""
        off = _pad(-(-self.cap // 1024)) + _pad(-(-self.cap // 64))
        return self.work[off:off + 4 * self.cap].view(torch.float32)

    def sample(self, bs, beta, seed=0, counter=0, uniforms=None):
        return per_sample(self.prios, self.size, bs, beta, alpha=self.alpha, uniforms=uniforms, seed=seed,
                          counter=counter)


def _pad(n_doubles):
    return ((n_doubles * 8 + 255) // 256) * 256
