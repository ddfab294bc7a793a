"""CPU-only checks of the replay-driven DQN update's boundary (pm_dqn_replay_update, pm_replay_push,
pongmi.replay.DeviceReplay.push / push_prio): the struct layout, header / EXPORTED / library agreement,
every argument rejection before any launch, and the ring bookkeeping with the library call stubbed. No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_dqn_replay_sizeof", "pm_dqn_replay_update", "pm_replay_push")
DQN_BUFS = ("params", "target", "adam_m", "adam_v", "grad", "stats", "s", "ns", "act", "rew", "done", "td")


def _desc(_lib, **kw):
    d = _lib.Dqn()
    for name in DQN_BUFS + ("isw",):
        setattr(d, name, 4096)  # never dereferenced: every check below fails on the host
    d.batch, d.noise, d.target_update_interval = 256, _lib.PM_FOLD_TRAIN_FRESH, 1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rp(_lib, **kw):
    rp = _lib.DqnReplay(trans=4096, prios=4096, per_work=4096, idx=4096, u=None, cap=1024, size=1024, alpha=0.6,
                        beta_start=0.4, beta_frames=100000, seed=0)
    for k, v in kw.items():
        setattr(rp, k, v)
    return rp


def test_struct_size_and_exports_agree():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_dqn_replay_sizeof() == ctypes.sizeof(_lib.DqnReplay) == 88
    assert L.pm_abi_version() == 27 and L.pm_sizeof(11) == -1  # additive: no ABI bump, pm_sizeof as it was
    hdr = open(os.path.join(ROOT, "include", "pongmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.EXPORTED and hasattr(L, name), name
        assert re.search(rf" T {name}\b", nm), name
    # the struct's fields, in the header's order, are the mirror's
    body = re.search(r"typedef struct pm_dqn_replay \{(.*?)\} pm_dqn_replay;", code, re.S).group(1)
    types = {"const", "float", "void", "double", "int64_t", "uint64_t"}
    names = [w for w in re.findall(r"\w+", body) if w not in types]
    assert names == [f for f, _ in _lib.DqnReplay._fields_], names
    assert "bit 0" in hdr and "bit 1" in hdr  # pm_dqn_stats.status is documented


def test_update_rejects_bad_arguments_without_a_gpu():
    from pongmi import _lib
    L = _lib.load()
    fn = L.pm_dqn_replay_update

    def call(d, rp, updates=1):
        return fn(ctypes.byref(d) if d is not None else None, ctypes.byref(rp) if rp is not None else None, updates, None)

    assert call(None, _rp(_lib)) == -1
    assert call(_desc(_lib), None) == -1 and b"null" in L.pm_last_error()
    # everything pm_dqn_update rejects
    for name in DQN_BUFS:
        assert call(_desc(_lib, **{name: None}), _rp(_lib)) == -1, name
        assert b"null" in L.pm_last_error()
    for batch in (0, -1, 257, 1 << 20):
        assert call(_desc(_lib, batch=batch), _rp(_lib)) == -2, batch
        assert b"batch" in L.pm_last_error()
    assert call(_desc(_lib, noise=_lib.PM_FOLD_EVAL), _rp(_lib)) == -1
    assert call(_desc(_lib, target_update_interval=0), _rp(_lib)) == -1
    # its own
    assert call(_desc(_lib, isw=None), _rp(_lib)) == -1 and b"isw" in L.pm_last_error()
    for name in ("trans", "prios", "per_work", "idx"):
        assert call(_desc(_lib), _rp(_lib, **{name: None})) == -1, name
        assert b"null" in L.pm_last_error()
    for name in ("trans", "per_work"):
        assert call(_desc(_lib), _rp(_lib, **{name: 4096 + 8})) == -1, name
        assert b"aligned" in L.pm_last_error()
    for size, cap in ((0, 1024), (-1, 1024), (1025, 1024), (1, 0)):
        assert call(_desc(_lib), _rp(_lib, size=size, cap=cap)) == -2, (size, cap)
        assert b"size" in L.pm_last_error()
    for updates in (0, -1):
        assert call(_desc(_lib), _rp(_lib), updates) == -2 and b"updates" in L.pm_last_error()
    for bf in (0, -5):
        assert call(_desc(_lib), _rp(_lib, beta_frames=bf)) == -2 and b"beta_frames" in L.pm_last_error()


def test_push_rejects_bad_arguments_without_a_gpu():
    from pongmi import _lib
    L = _lib.load()
    good = dict(trans=4096, prios=4096, per_work=4096, cap=1024, pos=0, alpha=0.6, prio=1.0, s=4096, act=4096, rew=4096,
                ns=4096, done=4096, n=64, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return L.pm_replay_push(*(a[k] for k in good))

    for name in ("trans", "prios", "per_work", "s", "act", "rew", "ns", "done"):
        assert call(**{name: None}) == -1, name
        assert b"null" in L.pm_last_error()
    for name in ("trans", "per_work"):
        assert call(**{name: 4096 + 4}) == -1 and b"aligned" in L.pm_last_error()
    for n in (0, -1, 1025, 1 << 30):
        assert call(n=n) == -2 and b"n=" in L.pm_last_error(), n
    for pos in (-1, 1024, 1 << 40):
        assert call(pos=pos) == -2 and b"pos" in L.pm_last_error(), pos
    for cap in (0, -7):
        assert call(cap=cap) == -2, cap


class _Stub:
    """libpongmi with pm_replay_push recorded instead of launched."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def pm_per_work_bytes(self, cap):
        return self.real.pm_per_work_bytes(cap)

    def pm_replay_push(self, trans, prios, work, cap, pos, alpha, prio, s, a, r, ns, done, n, stream):
        self.calls.append(dict(cap=cap, pos=pos, prio=prio, n=n, alpha=alpha))
        return 0


def test_device_replay_push_bookkeeping(monkeypatch):
    """pos / size / wrap, the priority a push stores, and the stale mark that DQNLearner.update_from sets:
    push_prio() re-reads prios[:size].max() once and clears it; an untouched replay never reads prios."""
    from pongmi import _lib, replay
    stub = _Stub(_lib.load())
    monkeypatch.setattr(replay._lib, "load", lambda: stub)
    monkeypatch.setattr(replay, "stream_ptr", lambda stream=None: 0)
    R = replay.DeviceReplay(10, "cpu", alpha=0.6)
    assert (R.pos, R.size, R.max_prio_stale) == (0, 0, False) and R.push_prio() == 1.0

    def push(n, a=None):
        R.push(torch.rand(n, 7), torch.zeros(n, dtype=torch.int64) if a is None else a, torch.zeros(n), torch.rand(n, 7),
               torch.zeros(n, dtype=torch.bool))

    push(4)
    assert stub.calls[-1] == dict(cap=10, pos=0, prio=1.0, n=4, alpha=0.6) and (R.pos, R.size) == (4, 4)
    R.max_prio = 2.5  # as after refresh()
    push(7)  # wraps
    assert stub.calls[-1]["pos"] == 4 and stub.calls[-1]["prio"] == 2.5 and (R.pos, R.size) == (1, 10)
    push(10)  # a whole ring
    assert stub.calls[-1]["pos"] == 1 and (R.pos, R.size) == (1, 10)
    for n in (0, 11):
        with pytest.raises(ValueError):
            push(n) if n else R.push(torch.zeros(0, 7), [], [], torch.zeros(0, 7), [])
    for bad in (torch.tensor([0, 3]), torch.tensor([-1, 2])):
        with pytest.raises(ValueError, match="actions"):
            push(2, bad)
    assert len(stub.calls) == 3 and (R.pos, R.size) == (1, 10)
    # the stale mark: set by update_from, resolved by the next push_prio() from prios[:size]
    R.prios[:] = torch.arange(10, dtype=torch.float32)
    assert R.push_prio() == 2.5  # not stale: the tracked value, prios not read
    R.max_prio_stale = True
    assert R.push_prio() == 9.0 and R.max_prio_stale is False and R.max_prio == 9.0
    R.prios[9] = 0.5
    assert R.push_prio() == 9.0  # read once only
    R.max_prio_stale = True
    push(1)
    assert stub.calls[-1]["prio"] == 8.0 and R.max_prio_stale is False
    # an empty replay pushes 1.0 whatever the mark says
    E = replay.DeviceReplay(4, "cpu")
    E.max_prio_stale = True
    assert E.push_prio() == 1.0 and E.max_prio_stale is False


def test_update_from_marks_the_replay_stale(monkeypatch):
    from pongmi import _lib, dqn, replay
    from models.qnet import QNet
    seen = {}

    def fake(d, rp, updates, stream):
        r = ctypes.cast(rp, ctypes.POINTER(_lib.DqnReplay)).contents
        seen.update(updates=updates, cap=r.cap, size=r.size, beta_frames=r.beta_frames, u=r.u, seed=r.seed,
                    isw=ctypes.cast(d, ctypes.POINTER(_lib.Dqn)).contents.isw)
        return 0

    L = dqn.DQNLearner(QNet(7, 3), batch=8, device="cpu")
    monkeypatch.setattr(dqn, "stream_ptr", lambda stream=None: 0)
    L.lib = type("S", (), {"pm_dqn_replay_update": staticmethod(fake)})()
    R = replay.DeviceReplay(32, "cpu")
    R.size = 20
    idx, td = L.update_from(R, 3, beta_frames=50, seed=-1, uniforms=torch.rand(3, 8))
    assert R.max_prio_stale is True
    assert seen["updates"] == 3 and (seen["cap"], seen["size"], seen["beta_frames"]) == (32, 20, 50)
    assert seen["u"] and seen["isw"] == L.isw.data_ptr() and seen["seed"] == 0xFFFFFFFFFFFFFFFF
    assert idx.data_ptr() == L.idx.data_ptr() and td.data_ptr() == L.td.data_ptr() and idx.dtype == torch.int64
    with pytest.raises(ValueError, match="uniforms"):
        L.update_from(R, 2, uniforms=torch.rand(3, 8))
