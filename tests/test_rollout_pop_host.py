"""CPU-only checks of the population's collecting rollout (pm_rollout_pop_*, pongmi.rollout.PopulationRollout,
pongmi.dqn.PopulationTrainer): the additive ABI, header / _lib / library agreement, every rejection of
pm_rollout_pop_create with its code and the offending member's index in the message (fake, well-separated
pointers; every check comes before the first HIP call), the aliasing rule for each writable buffer kind, the
null-handle errors, the constructor's ValueErrors before anything is allocated, and which entry points a
collect calls, with what `advance`, and when it rebinds. No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pm_rollout_pop_create", "pm_rollout_pop_rebind", "pm_rollout_pop_push", "pm_rollout_pop_info",
           "pm_rollout_pop_destroy")
WRITABLE = ("trans", "prios", "per_work", "ep_reward", "heads_ws", "stats", "prio_dev", "wB")
READ_ONLY = ("wA", "paramsB")
RP_KINDS = ("trans", "prios", "per_work", "ep_reward")
MIB = 1 << 20
M, STEPS_MAX, CAP = 8, 4, 1024


def _members(_lib, n, shared=()):
    """n valid members whose every buffer lies 1 MiB from every other one (the largest, trans of cap 1024, is
    64 KiB); the kinds in `shared` are member 0's for everyone."""
    mb = (_lib.RollMember * n)()
    for p in range(n):
        for i, k in enumerate(WRITABLE + READ_ONLY):
            _set(mb, p, k, (1 + (0 if k in shared else p) * 32 + i) * MIB)
        mb[p].rp.pos, mb[p].rp.cap, mb[p].rp.prio, mb[p].rp.alpha = 0, CAP, 1.0, 0.6
        mb[p].size, mb[p].epsilon, mb[p].seed_env, mb[p].seed_net = 0, 0.02, p, 0
    return mb


def _get(mb, p, kind):
    return getattr(mb[p].rp if kind in RP_KINDS else mb[p], kind)


def _set(mb, p, kind, v):
    setattr(mb[p].rp if kind in RP_KINDS else mb[p], kind, v)


def _env(_lib):
    from pongmi.env import env_params
    return env_params(), _lib.EnvState(*[(200 + k) * MIB for k in range(11)])


def _create(L, _lib, mb, n, m=M, steps_max=STEPS_MAX, want_out=True, params=True, state=None, members=True):
    p, s = _env(_lib)
    if state is not None:
        s = state
    h = ctypes.c_void_p()
    rc = L.pm_rollout_pop_create(ctypes.byref(p) if params is True else params, ctypes.byref(s),
                                 mb if members else None, n, m, steps_max, ctypes.byref(h) if want_out else None)
    if rc == 0:  # a machine with a GPU: the table of fake pointers was uploaded and is never launched
        n_, m_, s_ = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert L.pm_rollout_pop_info(h, ctypes.byref(n_), ctypes.byref(m_), ctypes.byref(s_)) == 0
        assert (n_.value, m_.value, s_.value) == (n, m, steps_max)
        assert L.pm_rollout_pop_destroy(h) == 0
    return rc, L.pm_last_error()


def test_abi_is_additive_and_header_lib_and_ctypes_agree():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_abi_version() == _lib.ABI_VERSION == 27
    assert L.pm_sizeof(11) == -1 and L.pm_sizeof(8) == ctypes.sizeof(_lib.RollReplay) == 56
    assert L.pm_roll_member_sizeof() == ctypes.sizeof(_lib.RollMember) == 136
    hdr = open(os.path.join(ROOT, "include", "pongmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert int(re.search(r"#define PM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 27
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in ENTRIES + ("pm_roll_member_sizeof",):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.EXPORTED and hasattr(L, name), name
        assert re.search(rf" T {name}\b", nm), name
    assert sorted(n for n in _lib.EXPORTED if n.startswith("pm_rollout_pop_")) == sorted(ENTRIES)
    assert "typedef struct pm_rollout_pop pm_rollout_pop;" in code  # opaque
    # the record's fields, in the header's order
    body = re.search(r"typedef struct pm_roll_member \{(.*?)\} pm_roll_member;", code, flags=re.S).group(1)
    names = [n for n in re.findall(r"\*?\s*(\w+)\s*[,;]", body)]
    assert names == [f[0] for f in _lib.RollMember._fields_], names
    assert _lib.RollMember.rp.offset == 32 and _lib.RollMember.size.offset == 88 and _lib.RollMember.seed_net.offset == 128


def test_create_rejects_bad_counts_and_null_arguments():
    from pongmi import _lib
    L = _lib.load()
    mb = _members(_lib, 3)
    for n in (0, -1, 1025):
        rc, msg = _create(L, _lib, mb, n)
        assert rc == -2 and b"n=" in msg, (n, rc, msg)
    for m in (0, -5):
        rc, msg = _create(L, _lib, mb, 3, m=m)
        assert rc == -2 and b"m=" in msg, (m, rc, msg)
    rc, msg = _create(L, _lib, _members(_lib, 2), 2, m=1 << 30)  # n * m past int32
    assert rc == -2 and b"n * m" in msg, (rc, msg)
    for sm in (0, -1):
        rc, msg = _create(L, _lib, mb, 3, steps_max=sm)
        assert rc == -2 and b"steps_max" in msg, (sm, rc, msg)
    rc, msg = _create(L, _lib, mb, 3, members=False)
    assert rc == -1 and b"null" in msg
    rc, msg = _create(L, _lib, mb, 3, want_out=False)
    assert rc == -1 and b"out" in msg
    rc, msg = _create(L, _lib, mb, 3, params=None)
    assert rc == -1 and b"null" in msg
    _, s = _env(_lib)
    s.spin = None
    rc, msg = _create(L, _lib, mb, 3, state=s)
    assert rc == -1 and b"null" in msg
    p, _ = _env(_lib)
    p.speed_scale_every = 0
    rc, msg = _create(L, _lib, mb, 3, params=ctypes.byref(p))
    assert rc == -1 and b"speed_scale_every" in msg
    rc, msg = _create(L, _lib, mb, 3)  # and the valid table is no argument error
    assert rc not in (-1, -2), (rc, msg)


def test_create_names_the_member_a_check_fails_on():
    from pongmi import _lib
    L = _lib.load()

    def bad(code, word, member, **kw):
        mb = _members(_lib, 3)
        for k, v in kw.items():
            if k in RP_KINDS + ("pos", "cap"):
                setattr(mb[member].rp, k, v)
            else:
                setattr(mb[member], k, v)
        rc, msg = _create(L, _lib, mb, 3)
        assert rc == code and word in msg and b"member %d" % member in msg, (kw, rc, msg)

    for k in ("wA", "wB", "paramsB", "heads_ws", "trans", "prios", "ep_reward"):
        bad(-1, b"null", 2, **{k: None})
    for k in ("wA", "wB", "heads_ws", "trans", "per_work"):
        bad(-1, b"aligned", 1, **{k: 150 * MIB + 4})
    bad(-2, b"cap", 0, cap=0)
    bad(-2, b"pos", 2, pos=-1)
    bad(-2, b"pos", 2, pos=CAP)
    bad(-2, b"size", 1, size=-1)
    bad(-2, b"size", 1, size=CAP + 1)
    bad(-2, b"steps_max * m", 1, cap=M * STEPS_MAX - 1)  # a slot would be written twice in one launch
    bad(-1, b"epsilon", 2, epsilon=float("nan"))
    bad(-1, b"epsilon", 0, epsilon=float("inf"))
    # the nullable ones, and a ring exactly steps_max * m long
    mb = _members(_lib, 3)
    mb[1].rp.per_work = mb[1].prio_dev = mb[1].stats = None
    mb[2].rp.cap = M * STEPS_MAX
    mb[2].size = M * STEPS_MAX
    rc, msg = _create(L, _lib, mb, 3)
    assert rc not in (-1, -2), (rc, msg)


@pytest.mark.parametrize("kind", WRITABLE)
def test_writable_buffers_must_not_overlap_between_members(kind):
    from pongmi import _lib
    L = _lib.load()
    mb = _members(_lib, 3)
    _set(mb, 2, kind, _get(mb, 0, kind))
    rc, msg = _create(L, _lib, mb, 3)
    assert rc == -1 and b"member 2" in msg and b"member 0" in msg and kind.encode() in msg and b"overlap" in msg, (rc, msg)


def test_overlap_compares_byte_ranges_and_read_only_buffers_may_be_shared():
    from pongmi import _lib
    L = _lib.load()
    sizes = dict(trans=64 * CAP, prios=4 * CAP, ep_reward=4 * M, heads_ws=4 * _lib.PM_ROLL_HEADS * STEPS_MAX, stats=48,
                 prio_dev=4, wB=4 * _lib.PM_QNET_NW, per_work=L.pm_per_work_bytes(CAP))
    for kind, nbytes in sizes.items():
        step = 16 if kind in ("trans", "per_work", "heads_ws", "wB") else 4  # keep the aligned ones aligned
        for off, clash in ((nbytes - step, True), (nbytes, False), (-nbytes + step, True), (-nbytes, False)):
            mb = _members(_lib, 2)
            _set(mb, 1, kind, _get(mb, 0, kind) + off)
            rc, msg = _create(L, _lib, mb, 2)
            if clash:
                assert rc == -1 and b"member 1" in msg and kind.encode() in msg, (kind, off, rc, msg)
            else:
                assert rc not in (-1, -2), (kind, off, rc, msg)
    # two different kinds: member 1's stats inside member 0's trans
    mb = _members(_lib, 2)
    mb[1].stats = mb[0].rp.trans + 4096
    rc, msg = _create(L, _lib, mb, 2)
    assert rc == -1 and b"stats" in msg and b"trans" in msg, (rc, msg)
    # wA and paramsB are only read: one opponent, one parameter block for everyone
    mb = _members(_lib, 4, shared=READ_ONLY)
    assert len({mb[p].wA for p in range(4)}) == 1 and len({mb[p].paramsB for p in range(4)}) == 1
    rc, msg = _create(L, _lib, mb, 4)
    assert rc not in (-1, -2), (rc, msg)


def test_calls_reject_a_null_handle():
    from pongmi import _lib
    L = _lib.load()
    mb = _members(_lib, 2)
    for steps in (1, 0, -1):
        assert L.pm_rollout_pop_push(None, 0, steps, 0, 1 * MIB, 2 * MIB, None) == -1 and b"null handle" in L.pm_last_error()
    assert L.pm_rollout_pop_rebind(None, mb, None) == -1 and b"null handle" in L.pm_last_error()
    assert L.pm_rollout_pop_info(None, None, None, None) == -1 and b"null handle" in L.pm_last_error()
    assert L.pm_rollout_pop_destroy(None) == -1 and b"null handle" in L.pm_last_error()


# ----------------------------------------------------------------------------- PopulationRollout
def _fake_env(n_arenas, device="cuda", seed=5, inject=None, autoreset=1):
    from pongmi import _lib
    from pongmi.env import env_params
    return types.SimpleNamespace(n=n_arenas, device=torch.device(device), seed=seed, inject=inject, autoreset=autoreset,
                                 counter=0, params=env_params(), state=_lib.EnvState(),
                                 obsA=torch.zeros((n_arenas, 7)), obsB=torch.zeros((n_arenas, 7)))


def _fake_replays(n, cap=64):
    return [types.SimpleNamespace(cap=cap) for _ in range(n)]


def _ctor_cases():
    from pongmi import _lib
    NP, NW = _lib.PM_QNET_NP, _lib.PM_QNET_NW
    ok = dict(env=_fake_env(12), wA=torch.zeros(NW), params=torch.zeros((3, NP)), n=3, replays=_fake_replays(3))
    shared = _fake_replays(1) * 3
    return [dict(ok, n=0), dict(ok, n=1025), dict(ok, n=5), dict(ok, env=_fake_env(2)),
            dict(ok, env=_fake_env(12, inject=object())), dict(ok, env=_fake_env(12, autoreset=0)),
            dict(ok, env=_fake_env(12, autoreset=2)), dict(ok, replays=_fake_replays(2)), dict(ok, replays=shared),
            dict(ok, steps_max=0), dict(ok, steps_max=17), dict(ok, replays=_fake_replays(3, cap=3)),
            dict(ok, epsilon=[0.1, 0.2]), dict(ok, epsilon=float("nan")), dict(ok, seed_env=[1, 2]), dict(ok, seed_net=[1] * 4),
            dict(ok, params=torch.zeros((2, NP))), dict(ok, params=torch.zeros((3, NP), dtype=torch.float64)),
            dict(ok, params=torch.zeros((NP, 3)).t()), dict(ok, params=np.zeros((3, NP), np.float32)),
            dict(ok, wA=torch.zeros(2 * NW)), dict(ok, wA=torch.zeros(NW, dtype=torch.float64)),
            dict(ok)]  # the last: valid but for params on the host while the env is on "cuda"


@pytest.mark.parametrize("case", range(23))
def test_constructor_rejects_bad_values_before_touching_a_device(case):
    """The env's device stays "cuda": the ValueError comes before any allocation, so it comes without a GPU too."""
    from pongmi.rollout import PopulationRollout
    kw = _ctor_cases()[case]
    env, wA, params = kw.pop("env"), kw.pop("wA"), kw.pop("params")
    with pytest.raises(ValueError, match="PopulationRollout"):
        PopulationRollout(env, wA, params, **kw)


def test_trainer_rejects_bad_counts():
    from pongmi.dqn import PopulationTrainer
    pop = types.SimpleNamespace(n=3, params=torch.zeros((3, 5452)))
    for kw in (dict(collect_steps=0, updates=1), dict(collect_steps=2, updates=0)):
        with pytest.raises(ValueError, match="PopulationTrainer"):
            PopulationTrainer(_fake_env(12), torch.zeros(9944), pop, _fake_replays(3), **kw)
    with pytest.raises(ValueError, match="PopulationRollout"):  # collect_steps * m > cap, from the collector
        PopulationTrainer(_fake_env(12), torch.zeros(9944), pop, _fake_replays(3, cap=7), collect_steps=2, updates=1)


class _Rec:
    """libpongmi with the collector's entry points recorded instead of run."""

    def __init__(self, _lib):
        self._lib, self.calls, self.tables = _lib, [], []

    def pm_rollout_pop_create(self, p, s, mb, n, m, steps_max, out):
        self.n = n
        self.tables.append([self._lib.RollMember.from_buffer_copy(mb[k]) for k in range(n)])
        out._obj.value = 0x4321
        self.calls.append(f"create {n} {m} {steps_max}")
        return 0

    def pm_rollout_pop_rebind(self, h, mb, stream):
        assert h.value == 0x4321
        self.tables.append([self._lib.RollMember.from_buffer_copy(mb[k]) for k in range(self.n)])
        self.calls.append("rebind")
        return 0

    def pm_qnet_fold(self, blocks, params_out, mode, seed, counter, counter_dev, w, k, stream):
        self.calls.append(f"fold {k} {mode}")
        self.fold_args = (blocks, w)
        return 0

    def pm_rollout_pop_push(self, h, counter0, steps, advance, obsA, obsB, stream):
        self.calls.append(f"push c={counter0} steps={steps} advance={advance}")
        return 0

    def pm_rollout_pop_destroy(self, h):
        self.calls.append("destroy")
        return 0

    def take(self):
        c, self.calls = self.calls, []
        return c


def test_collect_calls_and_rebinds_only_when_someone_else_pushed(monkeypatch):
    from pongmi import _lib, replay, rollout
    monkeypatch.setattr(rollout, "stream_ptr", lambda stream=None: 0)
    n, m, NP, NW = 3, 4, _lib.PM_QNET_NP, _lib.PM_QNET_NW
    env = _fake_env(n * m, device="cpu", seed=7)
    R = [replay.DeviceReplay(cap, "cpu") for cap in (32, 40, 64)]
    R[2].work = None  # a member without a sum tree
    R[1].pos, R[1].size = 30, 35
    params = torch.zeros((n, NP))
    wA = torch.zeros((n, NW))
    C = rollout.PopulationRollout(env, wA, params, n=n, replays=R, epsilon=[0.0, 0.02, 1.0], seed_net=[1, 2, 3], steps_max=8)
    rec = C.lib = _Rec(_lib)
    assert C.m == m and C.wB.shape == (n, NW) and C.heads.shape == (n, 8 * _lib.PM_ROLL_HEADS) and C.stats.shape == (n, 6)
    out = C.collect(2)
    assert rec.take() == ["create 3 4 8", f"fold 3 {_lib.PM_FOLD_EVAL}", "push c=0 steps=2 advance=0"]
    assert rec.fold_args == (params.data_ptr(), C.wB.data_ptr())  # params in place, the images into the table's wB
    assert set(out) == set(rollout.STATS_PUSH) and all(v.shape == (n,) and v.dtype == np.int64 for v in out.values())
    t = rec.tables[-1]
    assert [x.paramsB for x in t] == [params[p].data_ptr() for p in range(n)]
    assert [x.wA for x in t] == [C.wA[p].data_ptr() for p in range(n)] and [x.wB for x in t] == [C.wB[p].data_ptr() for p in range(n)]
    assert [x.rp.ep_reward for x in t] == [C.ep_reward.data_ptr() + 4 * m * p for p in range(n)]
    assert [x.prio_dev for x in t] == [C.prio.data_ptr() + 4 * p for p in range(n)]
    assert [x.stats for x in t] == [C.stats[p].data_ptr() for p in range(n)]
    assert [(x.rp.pos, x.size, x.rp.cap) for x in t] == [(0, 0, 32), (30, 35, 40), (0, 0, 64)]
    assert [x.rp.per_work for x in t] == [R[0].work.data_ptr(), R[1].work.data_ptr(), None]
    assert [x.seed_env for x in t] == [7, 8, 9] and [x.seed_net for x in t] == [1, 2, 3]
    assert [round(x.epsilon, 6) for x in t] == [0.0, 0.02, 1.0]
    assert [(r.pos, r.size) for r in R] == [(8, 8), (38, 40), (8, 8)] and all(r.max_prio_stale for r in R) and env.counter == 2
    st = C.collect(3, sync=False)  # a loop of collects never rebinds: advance carries the rings' progress
    assert rec.take() == [f"fold 3 {_lib.PM_FOLD_EVAL}", "push c=2 steps=3 advance=8"] and st.data_ptr() == C.stats.data_ptr()
    assert [(r.pos, r.size) for r in R] == [(20, 20), (10, 40), (20, 20)] and env.counter == 5
    C.collect(0)
    assert rec.take() == [] and env.counter == 5
    for r in R:  # what update_from does to a replay leaves the table as it is
        r.max_prio_stale = True
    C.collect(1)
    assert rec.take() == [f"fold 3 {_lib.PM_FOLD_EVAL}", "push c=5 steps=1 advance=20"]
    R[0].advance(5)  # someone else pushed into member 0's ring
    C.collect(1)
    assert rec.take() == ["rebind", f"fold 3 {_lib.PM_FOLD_EVAL}", "push c=6 steps=1 advance=0"]
    assert [(x.rp.pos, x.size) for x in rec.tables[-1]] == [(29, 29), (14, 40), (24, 24)]
    with pytest.raises(ValueError, match="PopulationRollout"):
        C.collect(9)
    with pytest.raises(ValueError, match="PopulationRollout"):
        C.collect(-1)
    one = rollout.PopulationRollout(env, torch.zeros(NW), params, n=n, replays=R)  # one opponent for everyone
    assert one.steps_max == 8  # min(32, min(cap) // m)
    one.lib = _Rec(_lib)
    one.collect(1)
    assert len({x.wA for x in one.lib.tables[-1]}) == 1


# ----------------------------------------------------------------------------- the ring tables of the GPU tests
# Mirrored from csrc/pm_rollout_pop.hip: k_rpp_prios runs kPriosBlock = 1024 threads per member, each with four
# float4 loads per round (element e + k * kPriosBlock, clamped to e past the end) and a scalar tail; k_rpp_nodes
# gives a block 64 level-1 nodes of PER_SUB = 64 leaves (csrc/pm_per.h).
PRIOS_BLOCK, PRIOS_LOADS, BLOCK_NODES, NODE_LEAVES = 1024, 4, 64, 64


def _prios_visits(fill, aligned):
    """What k_rpp_prios does for one member: ({(round, k, clamped)} over all threads, entries left to the scalar loop)."""
    n4 = fill // 4 if aligned else 0
    loads = set()
    for rnd, e0 in enumerate(range(0, n4, PRIOS_LOADS * PRIOS_BLOCK)):
        for t in range(min(PRIOS_BLOCK, n4 - e0)):
            loads |= {(rnd, k, e0 + t + k * PRIOS_BLOCK >= n4) for k in range(PRIOS_LOADS)}
    return loads, fill - 4 * n4


def _prios_reader(entry, fill, aligned):
    """The load that reads `entry`: (round, k), or "tail" for the scalar loop."""
    n4 = fill // 4 if aligned else 0
    if entry >= 4 * n4:
        return "tail"
    per_round = PRIOS_LOADS * PRIOS_BLOCK
    return entry // 4 // per_round, entry // 4 % per_round // PRIOS_BLOCK


def _node_blocks(cap):
    nsub = -(-cap // NODE_LEAVES)
    return -(-nsub // BLOCK_NODES), nsub


def test_ring_tables_reach_the_paths_they_claim():
    """tests/test_gpu_rollout_pop_rings.py's member tables against a model of which loads k_rpp_prios issues and how
    many blocks k_rpp_nodes gives a ring: fails when someone shrinks the rings back into the one-round, one-block
    configuration."""
    import test_gpu_rollout_pop_rings as rings
    src = open(os.path.join(ROOT, "pingpong-selfplay-ai_amd", "csrc", "pm_rollout_pop.hip")).read()
    for text in ("constexpr int kPriosBlock = 1024;", "e += 4 * kPriosBlock", "for (int k = 0; k < 4; ++k)",
                 "e + k * kPriosBlock", "blockIdx.x * 64 >= tr.nsub"):
        assert text in src, text  # the constants above are still the source's
    tab = rings.PRIO_MEMBERS
    where, tails, every = set(), set(), set()
    for c in tab:
        assert 0 < c["fill"] <= c["cap"] and all(0 <= e < c["fill"] for e, _ in c["marks"]), c
        top = [e for e, v in c["marks"] if v != v] or [e for e, v in c["marks"] if v == rings.MARK]
        assert len(top) == 1, c  # one entry decides the member's maximum: its NaN, else its one marker
        loads, tail = _prios_visits(c["fill"], c["aligned"])
        reader = _prios_reader(top[0], c["fill"], c["aligned"])
        every |= loads
        if reader == "tail":
            assert top[0] == c["fill"] - 1  # the tail's last entry
            tails.add((tail, c["aligned"]))
        else:
            assert (*reader, False) in loads
            where.add(reader + (any(rnd == reader[0] and clamped for rnd, _, clamped in loads),))
    # a maximum behind a real load at each k of the first round, and in each of four rounds
    assert {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 2), (3, 3)} <= {w[:2] for w in where}
    # ... behind a real k = 1 load of a round whose other k = 1 loads are clamped, and in a second round that has
    # clamped loads at every k >= 1
    assert (0, 1, True) in where and (1, 0, True) in where
    assert {(1, k, True) for k in (1, 2, 3)} <= every and {(0, k, True) for k in (1, 2, 3)} <= every
    # ... in tails of 1, 2 and 3 entries behind float4 rounds, and at the end of a many-pass unaligned loop
    assert {(1, True), (2, True), (3, True)} <= tails
    assert any(not a and t > 4 * PRIOS_BLOCK for t, a in tails)
    assert any(v != v for c in tab for _, v in c["marks"])  # a NaN
    assert all(2 * 32 <= c["cap"] for c in tab)

    blocks = [_node_blocks(c["cap"]) for c in rings.NODE_MEMBERS if c["tree"]]
    grid = max(b for b, _ in blocks)
    assert grid == 16 and len({b for b, _ in blocks}) >= 3  # unequal across the launch's members
    assert any(1 < b < grid for b, _ in blocks) and any(b == 1 for b, _ in blocks)  # members that leave blocks
    assert any(b > 1 and nsub - BLOCK_NODES * (b - 1) == 1 and c["cap"] % NODE_LEAVES == 1
               for (b, nsub), c in zip(blocks, (c for c in rings.NODE_MEMBERS if c["tree"])))  # one node, one leaf
    assert (1, BLOCK_NODES) in blocks and any(b == 1 and nsub < BLOCK_NODES for b, nsub in blocks)
    assert any(not c["tree"] for c in rings.NODE_MEMBERS)
    assert all(30 * 33 <= c["cap"] for c in rings.NODE_MEMBERS)

    chain = rings.CHAIN_MEMBERS
    assert len({_node_blocks(c["cap"])[0] for c in chain}) == 3 and len({c["size"] / c["cap"] for c in chain}) == 3
    assert 6 * 20 * 33 >= 3 * min(c["cap"] for c in chain) and all(20 * 33 <= c["cap"] for c in chain)
