"""The population learner (pm_dqn_pop_*, pongmi.dqn.DQNPopulation) on the MI355X.

Every member is compared with a solo pongmi.dqn.DQNLearner given the same initial blocks, seeds, options and
inputs, bit for bit (torch.equal on the raw bits / oracle.bits_equal): params, target, adam_m, adam_v, grad,
td[:rows], q[:rows], steps, adam_t, loss, q_mean, status and, where the solo learner has one, norm; on the
replay path also idx, isw, the gathered batch, prios and the whole tree workspace, which in turn equals a
fresh pm_per_build. The update is a pure function of its inputs, so there is no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_dqn_replay as tr
from test_gpu_dqn import _batch

pytestmark = pytest.mark.gpu

MN = 0.02  # test_gpu_dqn_opt.py's max_norm that bites under the Huber loss too
STATE = ("params", "target", "adam_m", "adam_v", "grad")
STAT_KEYS = ("steps", "adam_t", "loss", "q_mean", "status")


@pytest.fixture(scope="module")
def nets():
    """Two unrelated QNets: targetB's feature layers differ from modelB's until a sync."""
    from models.qnet import QNet
    torch.manual_seed(11)
    return QNet(7, 3).state_dict(), QNet(7, 3).state_dict()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _solo(nets, batch, **kw):
    from pongmi.dqn import DQNLearner
    return DQNLearner(nets[0], nets[1], batch=batch, **kw)


def _pop(nets, cfgs, batch, **kw):
    """A population whose member p is DQNLearner(nets, batch=batch[p], **cfgs[p])."""
    from pongmi.dqn import DQNPopulation
    keys = sorted({k for c in cfgs for k in c})
    defaults = dict(gamma=0.99, lr=2.5e-4, target_update_interval=1000, train_features=False, fresh_noise=True, seed=0,
                    loss="mse", huber_beta=1.0, max_norm=None)
    per = {k: [c.get(k, defaults[k]) for c in cfgs] for k in keys}
    return DQNPopulation(nets[0], nets[1], n=len(cfgs), batch=batch, **per, **kw)


def _assert_member(P, st, p, L, rows, what):
    """Member p of the population against the solo learner L (st = P.stats(), read once by the caller)."""
    for name in STATE:
        assert _same_bits(getattr(P, name)[p], getattr(L, name)), f"{what}: member {p}: {name}"
    assert _same_bits(P.td[p, :rows], L.td[:rows]), f"{what}: member {p}: td"
    assert _same_bits(P.q[p, :rows], L.q[:rows]), f"{what}: member {p}: q"
    sl = L.stats()
    for k in STAT_KEYS:
        a, b = np.asarray(st[k][p]), np.asarray(sl[k], dtype=st[k].dtype)
        assert a.tobytes() == b.tobytes(), f"{what}: member {p}: stats.{k}: {a} vs {b}"
    if L.norm is not None:
        assert _same_bits(P.norm[p:p + 1], L.norm), f"{what}: member {p}: norm {float(P.norm[p])} vs {float(L.norm)}"


# ----------------------------------------------------------------------------- 1. members that differ in everything
CFGS = [
    dict(rows=1, train_features=False, fresh_noise=True, seed=10),
    dict(rows=33, train_features=True, fresh_noise=True, seed=11, loss="huber", huber_beta=0.5, max_norm=MN),
    dict(rows=256, train_features=True, fresh_noise=False, seed=12, target_update_interval=2),
    dict(rows=32, train_features=False, seed=13, max_norm=1e9),
    dict(rows=255, train_features=False, seed=14, lr=1e-3, gamma=0.9, isw=True),
]


@pytest.mark.parametrize("members", [(1,), (0, 1, 2, 3, 4)], ids=["n1", "n5"])
def test_members_equal_their_solo_learners(nets, members):
    """n = 1 (the Huber + clip + whole-net member) and n = 5, three updates with a fresh batch each: rows 1, 33
    (one past a 32-row tile), 256, 32 and 255; heads and whole net; fresh and as-is noise; squared and Huber
    loss; a clip that bites, one that does not and none; a target sync inside (interval 2); isw given; an
    lr and gamma of a member's own."""
    cfgs = [dict(CFGS[m]) for m in members]
    rows = [c.pop("rows") for c in cfgs]
    use_isw = [c.pop("isw", False) for c in cfgs]
    P = _pop(nets, cfgs, 256)
    solo = [_solo(nets, 256, **c) for c in cfgs]
    for k in range(3):
        for p, L in enumerate(solo):
            batch, iw = _batch(np.random.RandomState(100 * k + members[p]), rows[p])
            iw = iw if use_isw[p] else None
            P.load_batch(p, *batch, isw=iw)
            L.update(*batch, isw=iw)
        td = P.update()
        torch.cuda.synchronize()
        assert td.data_ptr() == P.td.data_ptr() and P.rows() == rows
        st = P.stats()
        for p, L in enumerate(solo):
            _assert_member(P, st, p, L, rows[p], f"update {k}")
            assert st["steps"][p] == k + 1 and st["status"][p] == 0
            if cfgs[p].get("max_norm") == MN:
                assert MN / (L.stats()["norm"] + 1e-6) < 1.0, "the clip bites: coef < 1"
            if cfgs[p].get("max_norm") == 1e9:
                assert 0 < L.stats()["norm"] < 1e9, "the clip does not bite"
            if cfgs[p].get("target_update_interval") == 2 and k == 1:
                assert torch.equal(P.target[p], P.params[p]), "the sync fell inside"
    for p, c in enumerate(cfgs):
        if not c["train_features"]:  # heads only: the frozen part keeps every bit
            assert _same_bits(P.params[p, :4672], solo[p].params[:4672]) and not P.adam_m[p, :4672].any()
    M = P.member(0)  # a DQNLearner over the member's slices: the existing checkpoint code reads it
    assert _same_bits(M.params, solo[0].params) and M.stats()["steps"] == 3
    for a, b in zip(M.optimizer_state_dict()["state"].values(), solo[0].optimizer_state_dict()["state"].values()):
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert P.acting_weights().shape == (len(members), 9944)


# ----------------------------------------------------------------------------- 2. more workgroups than compute units
def test_a_grid_larger_than_the_cu_count(nets):
    """n = 257 on 256 CUs, rows 32, heads only, ONE shared read-only batch (accepted, not aliasing), two
    updates. Members 0, 128 and 256 carry an lr and a seed of their own and equal their solo learners; all
    others are identical to each other and to one solo learner."""
    from pongmi.dqn import DQNPopulation
    n, rows, own = 257, 32, {0: (1e-3, 21), 128: (5e-4, 22), 256: (2e-3, 23)}
    lr = [own.get(p, (2.5e-4, 5))[0] for p in range(n)]
    seed = [own.get(p, (2.5e-4, 5))[1] for p in range(n)]
    P = DQNPopulation(nets[0], nets[1], n=n, batch=rows, shared_batch=True, lr=lr, seed=seed)
    solo = {p: _solo(nets, rows, lr=v[0], seed=v[1]) for p, v in own.items()}
    common = _solo(nets, rows, lr=2.5e-4, seed=5)
    others = torch.tensor([p for p in range(n) if p not in own], device="cuda")
    for k in range(2):
        batch, _ = _batch(np.random.RandomState(200 + k), rows)
        P.load_batch(None, *batch)
        for L in list(solo.values()) + [common]:
            L.update(*batch)
        P.update()
        torch.cuda.synchronize()
        st = P.stats()
        for p, L in solo.items():
            _assert_member(P, st, p, L, rows, f"update {k}")
        _assert_member(P, st, 1, common, rows, f"update {k}")
        for name in STATE + ("td", "q"):
            got = _bits(getattr(P, name)[others])
            assert torch.equal(got, got[:1].expand_as(got)), f"update {k}: {name}: the common members differ"
        assert (st["steps"] == k + 1).all() and (st["status"] == 0).all()
        assert len(set(st["loss"][others.cpu().numpy()].tolist())) == 1
    assert not _same_bits(P.params[0], P.params[1]) and not _same_bits(P.params[128], P.params[256])


# ----------------------------------------------------------------------------- 3. from the replays
REPLAY_CASES = [
    dict(cap=1025, size=1025, batch=256, cfg=dict(train_features=True, seed=5)),
    dict(cap=17409, size=5000, batch=255, cfg=dict(train_features=False, seed=6, loss="huber", max_norm=MN)),
    dict(cap=64, size=5, batch=64, cfg=dict(train_features=True, seed=7)),  # duplicates: the last one wins
]


def _rings(cases, seed, void=()):
    rng = np.random.default_rng(seed)
    out = []
    for p, c in enumerate(cases):
        trans = tr._rows(rng, c["cap"])
        prios = np.zeros(c["cap"], np.float32) if p in void else tr._prios(rng, c["cap"], c["size"])
        out.append((trans, prios))
    return out


def _assert_replay_member(orc, P, st, p, L, Rp, Rl, batch, what):
    _assert_member(P, st, p, L, batch, what)
    for name in ("idx", "isw", "s", "ns", "act", "rew", "done"):
        assert _same_bits(getattr(P, name)[p, :batch], getattr(L, name)), f"{what}: member {p}: {name}"
    assert _same_bits(Rp.prios, Rl.prios), f"{what}: member {p}: prios"
    assert torch.equal(Rp.work, Rl.work), f"{what}: member {p}: the tree workspace"
    tr._assert_tree_is_rebuild(orc, Rp, f"{what}: member {p}")


@pytest.mark.parametrize("philox", [False, True], ids=["injected", "philox"])
def test_replay_updates_equal_the_solo_calls(orc, nets, philox):
    """n = 3, U = 3 in one call: (cap 1025, full, batch 256, whole net), (cap 17409, size 5000, batch 255,
    heads, Huber + clip) and (cap 64, size 5, batch 64: duplicates), with injected uniforms and with Philox."""
    U = 3
    rings = _rings(REPLAY_CASES, 31 + philox)
    kw = dict(target_update_interval=2, fresh_noise=True)
    cfgs = [dict(c["cfg"], **kw) for c in REPLAY_CASES]
    batches = [c["batch"] for c in REPLAY_CASES]
    P = _pop(nets, cfgs, batches)
    Rp = [tr._replay(t, pr, c["size"]) for (t, pr), c in zip(rings, REPLAY_CASES)]
    Rl = [tr._replay(t, pr, c["size"]) for (t, pr), c in zip(rings, REPLAY_CASES)]
    rng = np.random.default_rng(9)
    u = None if philox else [rng.random((U, b)) for b in batches]
    seeds = [41, 42, 43]
    solo = [_solo(nets, b, **c) for b, c in zip(batches, cfgs)]
    for p, L in enumerate(solo):
        tr._from(L, Rl[p], U, seed=seeds[p], uniforms=None if philox else u[p])
    idx, td = P.update_from(Rp, U, beta_start=tr.BETA_START, beta_frames=tr.BETA_FRAMES, seed=seeds, uniforms=u)
    torch.cuda.synchronize()
    assert idx.data_ptr() == P.idx.data_ptr() and td.data_ptr() == P.td.data_ptr() and all(r.max_prio_stale for r in Rp)
    st = P.stats()
    for p, L in enumerate(solo):
        _assert_replay_member(orc, P, st, p, L, Rp[p], Rl[p], batches[p], "U = 3")
        assert st["steps"][p] == U and st["status"][p] == 0
    assert len(set(P.idx[2, :64].tolist())) < 64  # 64 draws of 5 slots
    assert MN / (solo[1].stats()["norm"] + 1e-6) < 1.0  # the clip was active: coef < 1
    # a second call draws from the trees the first one left, without a rebind (full or unchanged replays)
    bound = P._bound
    if philox:
        for p, L in enumerate(solo):
            tr._from(L, Rl[p], 1, seed=seeds[p])
        P.update_from(Rp, 1, beta_start=tr.BETA_START, beta_frames=tr.BETA_FRAMES, seed=seeds)
        torch.cuda.synchronize()
        assert P._bound is bound or P._bound == bound
        st = P.stats()
        for p, L in enumerate(solo):
            _assert_replay_member(orc, P, st, p, L, Rp[p], Rl[p], batches[p], "the next call")


# ----------------------------------------------------------------------------- 4. a void member among live ones
def test_a_void_member_does_not_disturb_the_others(orc, nets):
    """Member 1's priorities are all zero: status bit 0, idx -1, no step, nothing gathered, its norm untouched;
    members 0 and 2 equal their solo runs."""
    cases = [dict(cap=1025, size=700, batch=64, cfg=dict(train_features=True, seed=p, max_norm=1.0)) for p in range(3)]
    rings = _rings(cases, 44, void=(1,))
    cfgs = [c["cfg"] for c in cases]
    P = _pop(nets, cfgs, 64)
    Rp = [tr._replay(t, pr, 700) for t, pr in rings]
    Rl = [tr._replay(t, pr, 700) for t, pr in rings]
    P.member(1).set_train_steps(4)
    P.norm[1] = 123.0
    before = {n: getattr(P, n)[1].clone() for n in STATE[:4] + ("s", "ns", "isw", "act", "rew", "done")}
    work1 = Rp[1].work.clone()
    solo = {p: _solo(nets, 64, **cfgs[p]) for p in (0, 2)}
    for p, L in solo.items():
        tr._from(L, Rl[p], 3, seed=3)
    P.update_from(Rp, 3, beta_start=tr.BETA_START, beta_frames=tr.BETA_FRAMES, seed=3)
    torch.cuda.synchronize()
    st = P.stats()
    assert st["status"][1] & 1 and st["steps"][1] == 4 and st["adam_t"][1] == 0 and st["norm"][1] == 123.0
    assert (P.idx[1] == -1).all()
    for n, v in before.items():
        assert _same_bits(getattr(P, n)[1], v), f"the void member's {n}"
    assert not Rp[1].prios.any() and torch.equal(Rp[1].work, work1)
    for p, L in solo.items():
        _assert_replay_member(orc, P, st, p, L, Rp[p], Rl[p], 64, "beside a void member")
        assert st["status"][p] == 0 and st["steps"][p] == 3


# ----------------------------------------------------------------------------- 5. one ring, two learners
def test_two_members_share_one_ring(orc, nets):
    """Two DeviceReplays whose `trans` is the same tensor, each with its own prios / work (accepted, not
    aliasing). Each member equals a solo run on a private copy of the ring; the ring's bits are unchanged."""
    cap, size, batch = 1025, 900, 128
    rng = np.random.default_rng(55)
    trans = tr._rows(rng, cap)
    prios = [tr._prios(rng, cap, size) for _ in range(2)]
    cfgs = [dict(train_features=True, seed=1), dict(train_features=False, seed=2, lr=1e-3)]
    P = _pop(nets, cfgs, batch)
    Rp = [tr._replay(trans, pr, size) for pr in prios]
    Rp[1].trans = Rp[0].trans
    Rl = [tr._replay(trans, pr, size) for pr in prios]
    solo = [_solo(nets, batch, **c) for c in cfgs]
    for p, L in enumerate(solo):
        tr._from(L, Rl[p], 2, seed=8 + p)
    P.update_from(Rp, 2, beta_start=tr.BETA_START, beta_frames=tr.BETA_FRAMES, seed=[8, 9])
    torch.cuda.synchronize()
    st = P.stats()
    for p, L in enumerate(solo):
        _assert_replay_member(orc, P, st, p, L, Rp[p], Rl[p], batch, "shared ring")
        assert st["status"][p] == 0
    assert orc.bits_equal(tr._np(Rp[0].trans), trans)
    assert not _same_bits(Rp[0].prios, Rp[1].prios)


# ----------------------------------------------------------------------------- 6. exploit and set_hyper
def test_exploit_and_set_hyper(nets):
    rows = 33
    cfgs = [dict(train_features=True, seed=3, lr=1e-3), dict(train_features=True, seed=3, lr=2e-3),
            dict(train_features=True, seed=4, lr=3e-3)]
    P = _pop(nets, cfgs, rows)
    for k in range(2):  # the members drift apart
        for p in range(3):
            batch, _ = _batch(np.random.RandomState(300 + 10 * k + p), rows)
            P.load_batch(p, *batch)
        P.update()
    torch.cuda.synchronize()
    assert not _same_bits(P.params[0], P.params[1])
    before = {n: getattr(P, n).clone() for n in STATE[:4]}
    P.exploit(torch.tensor([0, 0, 2], device="cuda"))  # a device tensor: no host read
    P.set_hyper(lr=[1e-3, 1e-3, 3e-3])
    for n, v in before.items():
        assert _same_bits(getattr(P, n)[1], v[0]) and _same_bits(getattr(P, n)[0], v[0]) and _same_bits(getattr(P, n)[2], v[2]), n
    batch, _ = _batch(np.random.RandomState(333), rows)
    for p in range(3):
        P.load_batch(p, *batch)
    P.update()
    torch.cuda.synchronize()
    st = P.stats()
    for n in STATE + ("td", "q"):
        assert _same_bits(getattr(P, n)[0], getattr(P, n)[1]), f"after exploit: {n}"
    assert st["steps"].tolist() == [3, 3, 3] and st["loss"][0] == st["loss"][1]
    # set_hyper: the next update equals a solo learner started from the same state with that lr
    L = _solo(nets, rows, train_features=True, seed=4, lr=7e-4)
    for n in STATE[:4]:
        getattr(L, n).copy_(getattr(P, n)[2])
    L.set_train_steps(3)
    L._set_stats(adam_t=3)
    P.set_hyper(lr=[1e-3, 1e-3, 7e-4])
    batch, _ = _batch(np.random.RandomState(334), rows)
    for p in range(3):
        P.load_batch(p, *batch)
    L.update(*batch)
    P.update()
    torch.cuda.synchronize()
    _assert_member(P, P.stats(), 2, L, rows, "after set_hyper")


# ----------------------------------------------------------------------------- 7. what needs a live handle
def test_update_calls_check_the_handle_they_get(nets):
    from pongmi import _lib
    from pongmi.dqn import DQNPopulation
    L = _lib.load()
    P = DQNPopulation(nets[0], n=2, batch=32)
    P.update()
    n, has = ctypes.c_int32(), ctypes.c_int32(7)
    assert L.pm_dqn_pop_info(P._handle, ctypes.byref(n), ctypes.byref(has)) == 0 and (n.value, has.value) == (2, 0)
    assert L.pm_dqn_pop_replay_update(P._handle, 1, _lib.stream_ptr()) == -1 and b"without replay" in L.pm_last_error()
    R = [tr._replay(*_rings([dict(cap=64, size=64)], 70 + p)[0], 64) for p in range(2)]
    P.update_from(R, 1)
    assert L.pm_dqn_pop_info(P._handle, ctypes.byref(n), ctypes.byref(has)) == 0 and (n.value, has.value) == (2, 1)
    for updates in (0, -1):
        assert L.pm_dqn_pop_replay_update(P._handle, updates, _lib.stream_ptr()) == -2 and b"updates" in L.pm_last_error()
    torch.cuda.synchronize()
    assert (P.stats()["steps"] == 2).all() and (P.stats()["status"] == 0).all()
