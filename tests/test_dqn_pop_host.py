"""CPU-only checks of the population learner (pm_dqn_pop_*, pongmi.dqn.DQNPopulation): the additive ABI,
header / EXPORTED / library agreement, every rejection of pm_dqn_pop_create with its code and the offending
member's index in the message (fake, well-separated pointers; every check comes before the first HIP
call), the aliasing rule for each writable buffer kind, the update calls' handle checks, the constructor's
ValueErrors before anything is allocated, and which entry points a population calls and when it rebinds.
No GPU. What needs a live handle (a population without replay descriptors refused by
pm_dqn_pop_replay_update, updates <= 0, shared read-only buffers accepted) is in test_gpu_dqn_pop.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP_ENTRIES = ("pm_dqn_pop_create", "pm_dqn_pop_rebind", "pm_dqn_pop_update", "pm_dqn_pop_replay_update",
               "pm_dqn_pop_info", "pm_dqn_pop_destroy")
ALWAYS_WRITABLE = ("params", "target", "adam_m", "adam_v", "grad", "stats", "td", "q", "norm")
REPLAY_WRITABLE = ("s", "ns", "act", "rew", "done", "isw", "idx", "prios", "per_work")
DQN_FIELDS = ("params", "target", "adam_m", "adam_v", "grad", "stats", "s", "ns", "act", "rew", "done", "isw", "td", "q")
RP_FIELDS = ("trans", "prios", "per_work", "idx")
MIB = 1 << 20
NAN, INF = float("nan"), float("inf")


def _members(_lib, n, replay=False, shared=()):
    """n valid members whose every buffer lies 1 MiB from every other one (the largest, per_work of cap 1024,
    is under 8 KiB); the kinds in `shared` are member 0's for everyone."""
    d, o = (_lib.Dqn * n)(), (_lib.DqnOpt * n)()
    rp = (_lib.DqnReplay * n)() if replay else None
    names = DQN_FIELDS + ("norm",) + RP_FIELDS
    for p in range(n):
        addr = {k: (1 + (0 if k in shared else p) * 32 + i) * MIB for i, k in enumerate(names)}
        for k in DQN_FIELDS:
            setattr(d[p], k, addr[k])
        d[p].batch, d[p].noise, d[p].target_update_interval = 256, _lib.PM_FOLD_TRAIN_FRESH, 1000
        o[p].norm = addr["norm"]
        if replay:
            for k in RP_FIELDS:
                setattr(rp[p], k, addr[k])
            rp[p].cap, rp[p].size, rp[p].alpha, rp[p].beta_start, rp[p].beta_frames = 1024, 1024, 0.6, 0.4, 100000
    return d, o, rp


def _create(L, d, o, rp, n, want_out=True):
    h = ctypes.c_void_p()
    rc = L.pm_dqn_pop_create(d, o, rp, n, ctypes.byref(h) if want_out else None)
    if rc == 0:  # a machine with a GPU: the table of fake pointers was uploaded and is never launched
        assert L.pm_dqn_pop_destroy(h) == 0
    return rc, L.pm_last_error()


def _get(d, o, rp, p, kind):
    if kind == "norm":
        return o[p].norm
    return getattr(rp[p], kind) if kind in ("idx", "prios", "per_work", "trans") else getattr(d[p], kind)


def _set(d, o, rp, p, kind, v):
    if kind == "norm":
        o[p].norm = v
    elif kind in ("idx", "prios", "per_work", "trans"):
        setattr(rp[p], kind, v)
    else:
        setattr(d[p], kind, v)


def test_abi_is_additive_and_the_six_entry_points_agree():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_abi_version() == _lib.ABI_VERSION == 27
    assert L.pm_sizeof(11) == -1
    assert L.pm_sizeof(9) == ctypes.sizeof(_lib.Dqn) and L.pm_dqn_opt_sizeof() == 32 and L.pm_dqn_replay_sizeof() == 88
    hdr = open(os.path.join(ROOT, "include", "pongmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in POP_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.EXPORTED and hasattr(L, name), name
        assert re.search(rf" T {name}\b", nm), name
    assert sorted(n for n in _lib.EXPORTED if n.startswith("pm_dqn_pop_")) == sorted(POP_ENTRIES)
    assert int(re.search(r"#define PM_DQN_POP_MAX\s+(\d+)", hdr).group(1)) == _lib.PM_DQN_POP_MAX == 1024
    assert "typedef struct pm_dqn_pop pm_dqn_pop;" in code  # opaque
    assert "ONLY host synchronisations" in hdr  # the header says where the interface synchronises


def test_create_rejects_bad_counts_and_null_arrays():
    from pongmi import _lib
    L = _lib.load()
    d, o, rp = _members(_lib, 3)
    for n in (0, -1, 1025):
        rc, msg = _create(L, d, o, None, n)
        assert rc == -2 and b"n=" in msg, (n, rc, msg)
    rc, msg = _create(L, None, o, None, 3)
    assert rc == -1 and b"null" in msg
    rc, msg = _create(L, d, o, None, 3, want_out=False)
    assert rc == -1 and b"out" in msg
    rc, msg = _create(L, d, None, None, 3)  # a null opt is the defaults: no argument error
    assert rc not in (-1, -2), (rc, msg)


def test_create_names_the_member_a_check_fails_on():
    from pongmi import _lib
    L = _lib.load()

    def bad(code, word, member, replay=False, **kw):
        d, o, rp = _members(_lib, 3, replay)
        for k, v in kw.items():
            if k in ("loss", "huber_beta", "max_norm"):
                setattr(o[member], k, v)
            elif k in ("size", "cap", "trans", "beta_frames"):
                setattr(rp[member], k, v)
            else:
                setattr(d[member], k, v)
        rc, msg = _create(L, d, o, rp, 3)
        assert rc == code and word in msg and b"member %d" % member in msg, (kw, rc, msg)

    for batch in (0, -1, 257):
        bad(-2, b"batch", 2, batch=batch)
    bad(-1, b"noise", 2, noise=_lib.PM_FOLD_EVAL)
    bad(-1, b"target_update_interval", 2, target_update_interval=0)
    bad(-1, b"null", 1, grad=None)
    bad(-1, b"loss", 1, loss=2)
    bad(-1, b"huber_beta", 0, loss=_lib.PM_DQN_LOSS_HUBER, huber_beta=0.0)
    bad(-1, b"huber_beta", 2, loss=_lib.PM_DQN_LOSS_HUBER, huber_beta=NAN)
    for mn in (-1.0, NAN, INF):
        bad(-1, b"max_norm", 1, max_norm=mn)
    # with replay descriptors: what pm_dqn_replay_update_opt rejects
    bad(-1, b"isw", 2, replay=True, isw=None)
    bad(-2, b"size", 1, replay=True, size=0)
    bad(-2, b"size", 0, replay=True, size=1025)
    bad(-1, b"aligned", 2, replay=True, trans=5 * MIB + 4)
    bad(-2, b"beta_frames", 1, replay=True, beta_frames=0)
    # without them a null isw is fine (all ones) and the replay fields are not read
    d, o, _ = _members(_lib, 3)
    d[1].isw = None
    rc, msg = _create(L, d, o, None, 3)
    assert rc not in (-1, -2), (rc, msg)


@pytest.mark.parametrize("kind", ALWAYS_WRITABLE + REPLAY_WRITABLE)
def test_writable_buffers_must_not_overlap_between_members(kind):
    """Equal base pointers, for each writable kind in turn; the kinds that are writable only with replay
    descriptors are checked with them, and shared without them is no error."""
    from pongmi import _lib
    L = _lib.load()
    replay = kind in REPLAY_WRITABLE
    d, o, rp = _members(_lib, 3, replay)
    _set(d, o, rp, 2, kind, _get(d, o, rp, 0, kind))
    rc, msg = _create(L, d, o, rp, 3)
    assert rc == -1 and b"member 2" in msg and b"member 0" in msg and kind.encode() in msg and b"overlap" in msg, (rc, msg)
    if kind in ("s", "ns", "act", "rew", "done", "isw"):
        d, o, _ = _members(_lib, 3, False, shared=("s", "ns", "act", "rew", "done", "isw"))
        rc, msg = _create(L, d, o, None, 3)
        assert rc not in (-1, -2), (rc, msg)


def test_overlap_compares_byte_ranges_not_base_pointers():
    from pongmi import _lib
    L = _lib.load()
    nbytes = 4 * _lib.PM_QNET_NP
    for off, clash in ((16, True), (nbytes - 16, True), (nbytes, False), (-nbytes + 16, True), (-nbytes, False)):
        d, o, rp = _members(_lib, 2)
        d[1].params = d[0].params + off  # member 1's params start inside member 0's (or just past their end)
        rc, msg = _create(L, d, o, None, 2)
        if clash:
            assert rc == -1 and b"member 1" in msg and b"params" in msg, (off, rc, msg)
        else:
            assert rc not in (-1, -2), (off, rc, msg)
    # two different kinds: member 1's td inside member 0's grad
    d, o, rp = _members(_lib, 2)
    d[1].td = d[0].grad + 4 * 5000
    rc, msg = _create(L, d, o, None, 2)
    assert rc == -1 and b"td" in msg and b"grad" in msg, (rc, msg)
    # a small buffer between two of another member's, and the ranges of ONE member may touch each other
    d, o, rp = _members(_lib, 2)
    d[0].td = d[0].grad  # the same member's: not this rule's business
    rc, msg = _create(L, d, o, None, 2)
    assert rc not in (-1, -2), (rc, msg)
    # the size of td follows the member's row count
    d, o, rp = _members(_lib, 2)
    d[0].batch = 8
    d[1].td = d[0].td + 32  # just past 8 floats
    rc, msg = _create(L, d, o, None, 2)
    assert rc not in (-1, -2), (rc, msg)
    d[1].td = d[0].td + 28
    rc, msg = _create(L, d, o, None, 2)
    assert rc == -1 and b"td" in msg


def test_shared_read_only_buffers_are_not_aliasing():
    """One ring for every member (trans), each with priorities of its own: no argument error."""
    from pongmi import _lib
    L = _lib.load()
    d, o, rp = _members(_lib, 4, True, shared=("trans",))
    assert len({rp[p].trans for p in range(4)}) == 1
    rc, msg = _create(L, d, o, rp, 4)
    assert rc not in (-1, -2), (rc, msg)


def test_update_calls_and_rebind_reject_a_null_handle():
    from pongmi import _lib
    L = _lib.load()
    d, o, rp = _members(_lib, 2, True)
    assert L.pm_dqn_pop_update(None, None) == -1 and b"null handle" in L.pm_last_error()
    for updates in (1, 0, -3):
        assert L.pm_dqn_pop_replay_update(None, updates, None) == -1 and b"null handle" in L.pm_last_error()
    assert L.pm_dqn_pop_rebind(None, d, o, rp, None) == -1 and b"null handle" in L.pm_last_error()
    assert L.pm_dqn_pop_info(None, None, None) == -1 and L.pm_dqn_pop_destroy(None) == -1


# ----------------------------------------------------------------------------- DQNPopulation
@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(n=1025), dict(n=3, lr=[1e-3, 2e-3]), dict(n=3, seed=[1, 2, 3, 4]),
                                dict(n=2, loss="l1"), dict(n=2, loss=["mse", "MSE"]), dict(n=2, huber_beta=[1.0, 0.0]),
                                dict(n=2, max_norm=[None, -1.0]), dict(n=2, max_norm=NAN), dict(n=2, batch=0),
                                dict(n=2, batch=257), dict(n=2, betas=(0.9,)), dict(n=3, betas=[(0.9, 0.99)] * 2),
                                dict(n=2, target_update_interval=[10, 0]), dict()])
def test_constructor_rejects_bad_values_before_touching_a_device(kw):
    """device stays "cuda": the ValueError comes before any allocation, so it comes without a GPU too."""
    from models.qnet import QNet
    from pongmi.dqn import DQNPopulation
    with pytest.raises(ValueError, match="DQNPopulation"):
        DQNPopulation(QNet(7, 3), **kw)


def test_constructor_counts_models():
    from models.qnet import QNet
    from pongmi.dqn import DQNPopulation
    with pytest.raises(ValueError, match="DQNPopulation"):
        DQNPopulation([QNet(7, 3), QNet(7, 3)], n=3)
    with pytest.raises(ValueError, match="DQNPopulation"):
        DQNPopulation([QNet(7, 3)] * 2, [QNet(7, 3)] * 3)


class _Rec:
    """libpongmi with the population's entry points recorded instead of run."""

    def __init__(self, _lib):
        self._lib, self.calls, self.tables = _lib, [], []

    def _table(self, d, o, rp, n):
        L = self._lib
        self.tables.append(([L.Dqn.from_buffer_copy(d[p]) for p in range(n)], [L.DqnOpt.from_buffer_copy(o[p]) for p in range(n)],
                            None if rp is None else [L.DqnReplay.from_buffer_copy(rp[p]) for p in range(n)]))

    def pm_dqn_pop_create(self, d, o, rp, n, out):
        self.n = n
        self._table(d, o, rp, n)
        out._obj.value = 0x1234
        self.calls.append("create")
        return 0

    def pm_dqn_pop_rebind(self, h, d, o, rp, stream):
        assert h.value == 0x1234
        self._table(d, o, rp, self.n)
        self.calls.append("rebind")
        return 0

    def pm_dqn_pop_update(self, h, stream):
        self.calls.append("update")
        return 0

    def pm_dqn_pop_replay_update(self, h, updates, stream):
        self.calls.append(f"replay_update {updates}")
        return 0

    def pm_dqn_pop_destroy(self, h):
        self.calls.append("destroy")
        return 0

    def take(self):
        c, self.calls = self.calls, []
        return c


def _batch(rng, rows):
    return (rng.random((rows, 7), dtype=np.float32), rng.integers(0, 3, rows), rng.random(rows, dtype=np.float32),
            rng.random((rows, 7), dtype=np.float32), rng.random(rows) < 0.1)


def test_population_calls_and_rebinds_only_when_the_table_changed(monkeypatch):
    from models.qnet import QNet
    from pongmi import _lib, dqn_pop, replay
    from pongmi.dqn import DQNPopulation
    assert DQNPopulation is dqn_pop.DQNPopulation
    monkeypatch.setattr(dqn_pop, "stream_ptr", lambda stream=None: 0)
    P = DQNPopulation(QNet(7, 3), n=3, batch=8, device="cpu", lr=[1e-3, 2e-3, 3e-3], loss=["mse", "huber", "mse"],
                      max_norm=[None, 0.5, None], seed=[4, 5, 6], train_features=[False, True, False])
    rec = P.lib = _Rec(_lib)
    rng = np.random.default_rng(0)
    assert P.params.shape == (3, _lib.PM_QNET_NP) and P.td.shape == (3, 8) and P.s.shape == (3, 8, 7)
    assert torch.equal(P.params[0], P.params[2]) and torch.equal(P.target, P.params)
    td = P.update()
    assert rec.take() == ["create", "update"] and td.data_ptr() == P.td.data_ptr()
    d, o, rp = rec.tables[-1]
    assert rp is None
    assert [x.lr for x in d] == [1e-3, 2e-3, 3e-3] and [x.seed_net for x in d] == [4, 5, 6]
    assert [x.train_features for x in d] == [0, 1, 0] and [x.batch for x in d] == [8, 8, 8]
    assert [(x.loss, x.max_norm) for x in o] == [(0, 0.0), (1, 0.5), (0, 0.0)]
    assert [x.params for x in d] == [P.params[p].data_ptr() for p in range(3)]
    assert [x.norm for x in o] == [P.norm[p:p + 1].data_ptr() for p in range(3)] and all(x.isw is None for x in d)
    P.update()
    assert rec.take() == ["update"]  # a fixed batch never rebinds
    P.load_batch(1, *_batch(rng, 5))
    P.update()
    assert rec.take() == ["rebind", "update"] and [x.batch for x in rec.tables[-1][0]] == [8, 5, 8]  # rows changed
    P.load_batch(1, *_batch(rng, 5))
    P.update()
    assert rec.take() == ["update"]  # new data, same rows
    P.load_batch(2, *_batch(rng, 8), isw=np.ones(8, np.float32))
    P.update()
    assert rec.take() == ["rebind", "update"] and rec.tables[-1][0][2].isw == P.isw[2].data_ptr()
    P.set_hyper(lr=[1e-3, 2e-3, 3e-3])
    P.update()
    assert rec.take() == ["update"]  # the same values
    P.set_hyper(lr=5e-4, gamma=[0.9, 0.95, 0.99])
    P.update()
    assert rec.take() == ["rebind", "update"]
    assert [(x.lr, x.gamma) for x in rec.tables[-1][0]] == [(5e-4, 0.9), (5e-4, 0.95), (5e-4, 0.99)]
    with pytest.raises(ValueError, match="DQNPopulation"):
        P.set_hyper(lr=[1.0, 2.0])
    with pytest.raises(ValueError, match="DQNPopulation"):
        P.set_hyper(momentum=0.9)
    # the replay path
    R = [replay.DeviceReplay(32, "cpu") for _ in range(3)]
    R[1].trans = R[0].trans  # one ring, two learners
    for r in R:
        r.size = 20
    idx, td = P.update_from(R, 2, seed=[1, 2, 3])
    assert rec.take() == ["rebind", "replay_update 2"] and idx.data_ptr() == P.idx.data_ptr() and td.data_ptr() == P.td.data_ptr()
    d, o, rp = rec.tables[-1]
    assert [x.batch for x in d] == [8, 8, 8] and [x.isw for x in d] == [P.isw[p].data_ptr() for p in range(3)]
    assert [x.size for x in rp] == [20, 20, 20] and [x.seed for x in rp] == [1, 2, 3] and rp[0].trans == rp[1].trans != rp[2].trans
    assert [x.idx for x in rp] == [P.idx[p].data_ptr() for p in range(3)] and all(x.u is None for x in rp)
    assert all(r.max_prio_stale for r in R)
    P.update_from(R, 4, seed=[1, 2, 3])
    assert rec.take() == ["replay_update 4"]  # full or unchanged replays never rebind
    R[2].size = 21
    P.update_from(R, 1, seed=[1, 2, 3])
    assert rec.take() == ["rebind", "replay_update 1"] and [x.size for x in rec.tables[-1][2]] == [20, 20, 21]
    u = torch.rand(3, 2, 8, dtype=torch.float64)
    P.update_from(R, 2, seed=[1, 2, 3], uniforms=u)
    assert rec.take() == ["rebind", "replay_update 2"]
    assert [x.u for x in rec.tables[-1][2]] == [u.data_ptr() + 8 * 16 * p for p in range(3)]
    P.update_from(R, 2, seed=[1, 2, 3], uniforms=u)
    assert rec.take() == ["replay_update 2"]
    P.update()
    assert rec.take() == ["update"]  # the table update_from bound serves update() as it is
    with pytest.raises(ValueError, match="DQNPopulation"):
        P.update_from(R[:2])
    with pytest.raises(ValueError, match="uniforms"):
        P.update_from(R, 3, uniforms=u)
    # stats, members and exploit on the host tensors
    st = P.stats()
    assert set(st) == {"steps", "adam_t", "loss", "q_mean", "status", "norm"} and all(len(v) == 3 for v in st.values())
    M = P.member(1)
    assert M.params.data_ptr() == P.params[1].data_ptr() and M.train_features and M.opt.max_norm == 0.5
    assert set(M.state_dict()) == set(QNet(7, 3).state_dict()) and set(P.target_state_dict(2)) == set(M.state_dict())
    M._set_stats(steps=7, adam_t=7)
    M.adam_m.fill_(0.5)
    sd = M.optimizer_state_dict()
    assert sd["state"][0]["step"] == 7 or float(sd["state"][0]["step"]) == 7.0
    P.member(0).load_optimizer_state_dict(P.member(0).optimizer_state_dict())
    P.params[0].fill_(1.0)
    P.params[2].fill_(3.0)
    P.exploit(torch.tensor([1, 1, 0]))
    st = P.stats()
    assert st["steps"].tolist() == [7, 7, 0] and st["adam_t"].tolist() == [7, 7, 0]
    assert torch.all(P.params[2] == 1.0) and torch.equal(P.params[0], P.params[1]) and torch.all(P.adam_m[0] == 0.5)
    with pytest.raises(ValueError, match="DQNPopulation"):
        P.exploit([0, 1])


def test_shared_batch_points_every_member_at_one_set(monkeypatch):
    from models.qnet import QNet
    from pongmi import _lib, dqn_pop, replay
    monkeypatch.setattr(dqn_pop, "stream_ptr", lambda stream=None: 0)
    P = dqn_pop.DQNPopulation([QNet(7, 3) for _ in range(4)], batch=16, device="cpu", shared_batch=True, gamma=[0.9, 0.95, 0.99, 0.999])
    rec = P.lib = _Rec(_lib)
    assert P.n == 4 and P.s.shape == (16, 7) and not torch.equal(P.params[0], P.params[1])
    P.load_batch(None, *_batch(np.random.default_rng(1), 9))
    P.update()
    assert rec.take() == ["create", "update"]
    d = rec.tables[-1][0]
    assert len({x.s for x in d}) == 1 and d[0].s == P.s.data_ptr() and [x.batch for x in d] == [9] * 4
    assert len({x.td for x in d}) == 4
    with pytest.raises(ValueError, match="shared_batch"):
        P.update_from([replay.DeviceReplay(32, "cpu") for _ in range(4)])
