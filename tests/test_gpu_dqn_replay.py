"""The stand-alone learner trained straight from a device replay (pm_dqn_replay_update /
DQNLearner.update_from), pm_replay_push / DeviceReplay.push and pongmi.dqn.ReplayTrainer on the MI355X.

Every comparison is bit for bit (oracle.bits_equal): the draw against oracle.per_sample_tree (the device's
own summation order restated), the weights against its float32 weights divided in float32 by their float32
maximum, the gathered batch against the ring's rows, the update against pm_dqn_update on that batch, the
priorities against oracle.per_update, and all three levels of the sum tree against a fresh pm_per_build of
the resulting priorities. The update is a pure function of its inputs and a recomputed tree node has the
bits of a rebuilt one, so there is no tolerance anywhere (but the 2e-5 of the QNet module comparison that
test_gpu_dqn.py::test_toy_loop_trains_the_whole_net uses for the same check)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA, TAG_PER = 0.6, 5
BETA_START, BETA_FRAMES = 0.4, 1000
STAT_KEYS = ("steps", "adam_t", "loss", "q_mean")


@pytest.fixture(scope="module")
def nets():
    from models.qnet import QNet
    torch.manual_seed(11)
    return QNet(7, 3).state_dict(), QNet(7, 3).state_dict()


def _np(t):
    return t.detach().cpu().numpy()


def _rows(rng, cap):
    """[cap][16] ring rows: s[7] | r | s'[7] | bits(a | done << 8)."""
    t = rng.random((cap, 16), dtype=np.float32) * 2 - 1
    t[:, 7] = rng.integers(-1, 2, cap).astype(np.float32)
    bits = (rng.integers(0, 3, cap) | ((rng.random(cap) < 0.1).astype(np.int64) << 8)).astype(np.int32)
    t[:, 15] = bits.view(np.float32)
    return t


def _prios(rng, cap, size):
    p = np.zeros(cap, np.float32)
    p[:size] = rng.uniform(0.01, 3.0, size).astype(np.float32)
    return p


def _replay(trans, prios, size):
    from pongmi.replay import DeviceReplay
    cap = len(prios)
    R = DeviceReplay(cap, "cuda", alpha=ALPHA)
    R.trans.copy_(torch.from_numpy(trans))
    R.prios.copy_(torch.from_numpy(prios))
    R.size, R.pos = size, size % cap
    R.refresh()
    return R


def _levels(work, cap):
    from pongmi.replay import _pad
    b = _np(work)
    nch, nsub = -(-cap // 1024), -(-cap // 64)
    o1 = _pad(nch)
    o2 = o1 + _pad(nsub)
    return b[:8 * nch].view(np.float64), b[o1:o1 + 8 * nsub].view(np.float64), b[o2:o2 + 4 * cap].view(np.float32)


def _assert_tree_is_rebuild(orc, R, what=""):
    """All three levels of R's workspace against a fresh pm_per_build of R.prios (padding excluded)."""
    from pongmi import _lib
    fresh = torch.zeros_like(R.work)
    _lib.check(_lib.load().pm_per_build(R.prios.data_ptr(), R.cap, R.alpha, fresh.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for name, got, ref in zip(("chunk", "sub", "leaf"), _levels(R.work, R.cap), _levels(fresh, R.cap)):
        assert orc.bits_equal(got, ref), f"{what}: tree level {name}: {(got != ref).sum()} nodes differ"


def _beta(steps):
    frame = steps + 1
    b = BETA_START + frame * (1.0 - BETA_START) / BETA_FRAMES
    return b if b < 1.0 else 1.0


def _philox_u(orc, batch, frame, seed):
    r = orc.philox64(np.arange(batch), TAG_PER, frame, seed)
    return orc.u53(r[0], r[1])


def _oracle_draw(orc, prios, size, cap, steps, u):
    idx, w = orc.per_sample_tree(prios, size, cap, _beta(steps), u, alpha=ALPHA)
    return idx, (w / w.max()).astype(np.float32)  # float32 / float32


def _learner(nets, batch, tf, **kw):
    from pongmi.dqn import DQNLearner
    kw.setdefault("target_update_interval", 1000)
    return DQNLearner(nets[0], nets[1], batch=batch, train_features=tf, seed=5, **kw)


def _from(L, R, updates=1, **kw):
    out = L.update_from(R, updates, beta_start=BETA_START, beta_frames=BETA_FRAMES, **kw)
    torch.cuda.synchronize()
    return out


def _assert_batch_is_rows(orc, L, trans, idx, w, what):
    rows = trans[idx]
    bits = rows[:, 15].copy().view(np.int32)
    assert np.array_equal(_np(L.idx), idx), f"{what}: {(_np(L.idx) != idx).sum()} slots differ from the oracle's"
    assert orc.bits_equal(_np(L.isw), w), f"{what}: isw"
    assert orc.bits_equal(_np(L.s), rows[:, 0:7]) and orc.bits_equal(_np(L.ns), rows[:, 8:15]), f"{what}: s / ns"
    assert orc.bits_equal(_np(L.rew), rows[:, 7]), f"{what}: rew"
    assert np.array_equal(_np(L.act), bits & 0xFF) and np.array_equal(_np(L.done), (bits >> 8) & 1), f"{what}: act / done"


def _same_learner(orc, A, B, what):
    for name in ("params", "target", "adam_m", "adam_v", "grad", "td", "q"):
        assert orc.bits_equal(_np(getattr(A, name)), _np(getattr(B, name))), f"{what}: {name}"
    sa, sb = A.stats(), B.stats()
    for k in STAT_KEYS:
        assert orc.bits_equal(np.float64(sa[k]), np.float64(sb[k])), f"{what}: stats.{k}: {sa[k]} vs {sb[k]}"


def _compose(orc, C, trans, prios, size, steps, u):
    """One update as the parent's pieces compose it, on the host copy `prios` (updated in place): the
    oracle's draw, pm_dqn_update on those rows with its weights, update_priorities."""
    idx, w = _oracle_draw(orc, prios, size, len(prios), steps, u)
    rows = trans[idx]
    bits = rows[:, 15].copy().view(np.int32)
    td = C.update(rows[:, 0:7], bits & 0xFF, rows[:, 7], rows[:, 8:15], (bits >> 8) & 1, isw=w)
    torch.cuda.synchronize()
    orc.per_update(prios, idx, _np(td))
    return idx, w


CASES = [(1, 1, 1), (63, 63, 64), (64, 21, 65), (65, 65, 63), (1023, 341, 256), (1024, 1024, 256), (1025, 1025, 256),
         (17409, 5000, 255)]


# ----------------------------------------------------------------------------- 1. draw and gather
@pytest.mark.parametrize("cap,size,batch", CASES)
def test_draw_and_gather(orc, nets, cap, size, batch):
    """The slots, the normalised weights and every batch buffer, with injected uniforms and with the Philox
    draw, at beta's three regimes (steps 0, beta_frames / 2, past beta_frames); the tree each call leaves
    is the next one's input."""
    rng = np.random.default_rng(1000 * cap + batch)
    trans = _rows(rng, cap)
    R = _replay(trans, _prios(rng, cap, size), size)
    L = _learner(nets, batch, False)
    for steps in (0, BETA_FRAMES // 2, BETA_FRAMES + 10):
        for philox in (False, True):
            what = f"cap {cap} size {size} batch {batch} steps {steps} {'philox' if philox else 'injected'}"
            L.set_train_steps(steps)
            prios = _np(R.prios)
            u = _philox_u(orc, batch, steps + 1, 77) if philox else rng.random(batch)
            idx, w = _oracle_draw(orc, prios, size, cap, steps, u)
            assert idx.min() >= 0 and idx.max() < size
            got_idx, got_td = _from(L, R, seed=77, uniforms=None if philox else u)
            assert got_idx.data_ptr() == L.idx.data_ptr() and got_td.data_ptr() == L.td.data_ptr()
            _assert_batch_is_rows(orc, L, trans, idx, w, what)
            st = L.stats()
            assert st["steps"] == steps + 1 and st["status"] == 0, what
            assert R.max_prio_stale
    _assert_tree_is_rebuild(orc, R, f"cap {cap}")


# ----------------------------------------------------------------------------- 2. one call = the composition
@pytest.mark.parametrize("tf", [False, True])
@pytest.mark.parametrize("cap,size,batch", [(1025, 1025, 256), (17409, 5000, 255)])
def test_one_call_equals_the_composition(orc, nets, cap, size, batch, tf):
    rng = np.random.default_rng(cap + tf)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, size)
    R = _replay(trans, prios, size)
    A, C = _learner(nets, batch, tf), _learner(nets, batch, tf)
    for steps, philox in ((0, False), (1, True)):
        u = _philox_u(orc, batch, steps + 1, 3) if philox else rng.random(batch)
        _from(A, R, seed=3, uniforms=None if philox else u)
        idx, w = _compose(orc, C, trans, prios, size, steps, u)
        what = f"cap {cap} tf {tf} update {steps}"
        _assert_batch_is_rows(orc, A, trans, idx, w, what)
        _same_learner(orc, A, C, what)
        assert A.stats()["status"] == 0
        assert orc.bits_equal(_np(R.prios), prios), f"{what}: {(_np(R.prios) != prios).sum()} priorities differ"
        _assert_tree_is_rebuild(orc, R, what)


# ----------------------------------------------------------------------------- 3. duplicates
def test_duplicates_last_wins(orc, nets):
    cap, size, batch = 64, 5, 64
    rng = np.random.default_rng(3)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, size)
    R = _replay(trans, prios, size)
    A, C = _learner(nets, batch, True), _learner(nets, batch, True)
    u = rng.random(batch)
    _from(A, R, uniforms=u)
    idx, _ = _compose(orc, C, trans, prios, size, 0, u)
    assert len(set(idx.tolist())) < batch  # 64 draws of 5 slots
    assert np.array_equal(_np(A.idx), idx)
    assert orc.bits_equal(_np(R.prios), prios)
    for i in set(idx.tolist()):  # the last occurrence's error, not an earlier one's
        assert prios[i] == np.float32(abs(_np(C.td)[np.nonzero(idx == i)[0][-1]])) + np.float32(1e-6)
    _assert_tree_is_rebuild(orc, R, "duplicates")


# ----------------------------------------------------------------------------- 4. U updates in one call
@pytest.mark.parametrize("tf", [False, True])
def test_updates_in_one_call_equal_separate_calls(orc, nets, tf):
    cap, size, batch, U = 1025, 1025, 256, 3
    rng = np.random.default_rng(40 + tf)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, size)
    Ra, Rb = _replay(trans, prios, size), _replay(trans, prios, size)
    kw = dict(target_update_interval=2, fresh_noise=True)
    A, B, C = _learner(nets, batch, tf, **kw), _learner(nets, batch, tf, **kw), _learner(nets, batch, tf, **kw)
    _from(A, Ra, U, seed=9)
    for _ in range(U):
        _from(B, Rb, 1, seed=9)
    for k in range(U):
        idx, w = _compose(orc, C, trans, prios, size, k, _philox_u(orc, batch, k + 1, 9))
    assert A.stats()["steps"] == U and A.stats()["status"] == 0
    assert torch.equal(A.target, A.params) is False  # the sync was inside (after update 2), not at the end
    _assert_batch_is_rows(orc, A, trans, idx, w, "last update")
    _same_learner(orc, A, B, "one call of 3 vs 3 calls")
    _same_learner(orc, A, C, "one call of 3 vs the composition")
    assert orc.bits_equal(_np(Ra.prios), prios) and orc.bits_equal(_np(Rb.prios), prios)
    _assert_tree_is_rebuild(orc, Ra, "one call")
    _assert_tree_is_rebuild(orc, Rb, "three calls")
    # injected uniforms advance per update inside a call
    Rc = _replay(trans, _np(Ra.prios), size)
    D, E = _learner(nets, batch, tf, **kw), _learner(nets, batch, tf, **kw)
    uu = rng.random((2, batch))
    _from(D, Rc, 2, uniforms=uu)
    p = _np(Ra.prios).copy()
    for k in range(2):
        _compose(orc, E, trans, p, size, k, uu[k])
    _same_learner(orc, D, E, "two injected draws")
    assert orc.bits_equal(_np(Rc.prios), p)


# ----------------------------------------------------------------------------- 5. more than one prefix round
def test_multi_round_tree(orc, nets):
    tail = 1025
    cap = 1048576 + tail  # 1026 chunks: the second prefix round holds two
    batch = 64
    rng = np.random.default_rng(5)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, cap)
    leaf = orc.det_pow_f32(prios, ALPHA).astype(np.float64)
    f = (leaf[:-tail].sum() / 9.0) / leaf[-tail:].sum()  # a tenth of the mass in the last 1025 entries
    prios[-tail:] *= np.float32(f ** (1.0 / ALPHA))
    R = _replay(trans, prios, cap)
    A, C = _learner(nets, batch, True), _learner(nets, batch, True)
    u = rng.random(batch)
    _from(A, R, uniforms=u)
    idx, w = _compose(orc, C, trans, prios, cap, 0, u)
    assert (idx >= 1048576).any() and (idx < 1048576).any()  # draws in both rounds
    _assert_batch_is_rows(orc, A, trans, idx, w, "multi-round")
    _same_learner(orc, A, C, "multi-round")
    assert orc.bits_equal(_np(R.prios), prios)
    _assert_tree_is_rebuild(orc, R, "multi-round")


# ----------------------------------------------------------------------------- 6. void and NaN
def test_void_update_without_mass(orc, nets):
    cap, size, batch = 1025, 700, 64
    rng = np.random.default_rng(6)
    R = _replay(_rows(rng, cap), np.zeros(cap, np.float32), size)
    A = _learner(nets, batch, True)
    A.set_train_steps(4)
    before = {n: _np(getattr(A, n)).copy() for n in ("params", "target", "adam_m", "adam_v", "s", "ns", "isw")}
    work = _np(R.work).copy()
    idx, _ = _from(A, R, 3)
    st = A.stats()
    assert st["status"] & 1 and st["steps"] == 4 and st["adam_t"] == 0
    assert (_np(idx) == -1).all()
    for n, v in before.items():
        assert orc.bits_equal(_np(getattr(A, n)), v), n
    assert not _np(R.prios).any() and np.array_equal(_np(R.work), work)


def test_nan_priority_is_stored_and_latched(orc, nets):
    cap, size, batch = 130, 130, 64
    rng = np.random.default_rng(7)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, size)
    bad = 77
    trans[bad, 7] = np.nan
    prios[bad] = 400.0  # most of the mass: drawn for certain
    R = _replay(trans, prios, size)
    A = _learner(nets, batch, False)
    u = rng.random(batch)
    idx = orc.per_sample_tree(prios, size, cap, _beta(0), u, alpha=ALPHA)[0]
    assert (idx == bad).any() and (idx != bad).any()
    _from(A, R, uniforms=u)
    assert np.array_equal(_np(A.idx), idx)
    st = A.stats()
    assert st["status"] == 2 and st["steps"] == 1
    p = _np(R.prios)
    assert np.isnan(p[bad]) and np.isfinite(np.delete(p, bad)).all()
    assert _levels(R.work, cap)[2][bad] == 0.0
    _assert_tree_is_rebuild(orc, R, "NaN priority")
    torch.cuda.synchronize()  # the run ends clean


# ----------------------------------------------------------------------------- 7. pm_replay_push
@pytest.mark.parametrize("cap", [65, 1025, 4099])
def test_push_equals_host_ring(orc, cap):
    from pongmi import _lib
    rng = np.random.default_rng(cap)
    trans = _rows(rng, cap)
    prios = _prios(rng, cap, cap)
    R = _replay(trans, prios, cap)
    for n in (1, 63, 64, 65, 1025):
        new = _rows(rng, n)
        bits = new[:, 15].copy().view(np.int32)
        args = (torch.from_numpy(new[:, 0:7].copy()).cuda(), bits & 0xFF, new[:, 7], new[:, 8:15], (bits >> 8) & 1)
        if n > cap:  # rejected by the host class and by the entry point itself
            with pytest.raises(ValueError):
                R.push(*args)
            p = args[0].data_ptr()  # rejected before anything is read
            rc = _lib.load().pm_replay_push(R.trans.data_ptr(), R.prios.data_ptr(), R.work.data_ptr(), cap, 0, ALPHA, 1.0,
                                            p, p, p, p, p, n, _lib.stream_ptr())
            assert rc == -2 and orc.bits_equal(_np(R.trans), trans)
            continue
        for pos in (0, cap - 1, (cap - n // 2) % cap):
            prio = float(np.float32(rng.uniform(0.5, 4.0)))
            R.pos, R.max_prio = pos, prio
            R.push(*args)
            torch.cuda.synchronize()
            slots = (pos + np.arange(n)) % cap
            trans[slots] = new
            prios[slots] = np.float32(prio)
            what = f"cap {cap} n {n} pos {pos}"
            assert R.pos == (pos + n) % cap and R.size == cap, what
            assert orc.bits_equal(_np(R.trans), trans), what
            assert orc.bits_equal(_np(R.prios), prios), what
            _assert_tree_is_rebuild(orc, R, what)
            leaf = orc.per_tree(prios, cap, ALPHA)[2]
            assert orc.bits_equal(_levels(R.work, cap)[2], leaf), what


def test_push_then_collect_then_train_keeps_the_tree(orc, nets):
    """A DeviceReplay filled by push (from empty: priority 1), then by a collecting rollout, then trained
    from, then pushed into again (push_prio re-reads max(prios) after the training changed them)."""
    from pongmi import _lib
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import fold, pack_state_dict
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import SelfPlayRollout
    cap, n = 3000, 256
    rng = np.random.default_rng(8)
    R = DeviceReplay(cap, "cuda", alpha=ALPHA)
    first = _rows(rng, 700)
    bits = first[:, 15].copy().view(np.int32)
    R.push(first[:, 0:7], bits & 0xFF, first[:, 7], first[:, 8:15], (bits >> 8) & 1)
    assert (R.pos, R.size) == (700, 700) and (_np(R.prios)[:700] == 1.0).all() and not _np(R.prios)[700:].any()
    assert orc.bits_equal(_np(R.trans)[:700], first)
    _assert_tree_is_rebuild(orc, R, "push")
    env = PongEnv2PBatch(n, seed=3, autoreset=True)
    env.reset()
    L = _learner(nets, 256, True)
    wA = fold(pack_state_dict(nets[1]), _lib.PM_FOLD_EVAL).reshape(-1)
    roll = SelfPlayRollout(env, wA, L.params, epsilon=0.1, seed_net=2)
    roll.run(10, replay=R)  # wraps: 700 + 2560 > 3000
    assert (R.pos, R.size) == (260, cap)
    _assert_tree_is_rebuild(orc, R, "collect")
    _from(L, R, 4, seed=1)
    assert L.stats()["steps"] == 4 and L.stats()["status"] == 0 and R.max_prio_stale
    _assert_tree_is_rebuild(orc, R, "train")
    mx = float(R.prios.max())
    R.push(first[:5, 0:7], bits[:5] & 0xFF, first[:5, 7], first[:5, 8:15], (bits[:5] >> 8) & 1)
    assert not R.max_prio_stale and R.max_prio == mx and (_np(R.prios)[260:265] == np.float32(mx)).all()
    _assert_tree_is_rebuild(orc, R, "push after training")


# ----------------------------------------------------------------------------- 8. ReplayTrainer
def test_replay_trainer_trains_the_whole_net(orc, nets):
    from models.qnet import QNet
    from pongmi import _lib
    from pongmi.dqn import ReplayTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import fold, pack_state_dict, q_values
    from pongmi.replay import DeviceReplay

    def run():
        env = PongEnv2PBatch(512, autoreset=True, seed=4)
        env.reset()
        L = _learner(nets, 256, True, target_update_interval=8)
        R = DeviceReplay(8192, "cuda", alpha=ALPHA)
        wA = fold(pack_state_dict(nets[1]), _lib.PM_FOLD_EVAL).reshape(-1)
        T = ReplayTrainer(env, wA, L, R, collect_steps=4, updates=4, epsilon=0.1, seed_net=1, seed=3)
        stats = T.run(5)
        torch.cuda.synchronize()
        return L, R, stats

    w2_before = nets[0]["features.2.weight"].clone()
    L, R, stats = run()
    st = L.stats()
    assert np.isfinite(st["loss"]) and st["steps"] == 20 and st["adam_t"] == 20 and st["status"] == 0
    assert (R.pos, R.size) == (512 * 20 % 8192, 8192) and set(stats) >= {"episodes", "wins_B"}
    assert not torch.equal(L.state_dict()["features.2.weight"].cpu(), w2_before)
    assert torch.isfinite(L.params).all()
    _assert_tree_is_rebuild(orc, R, "after ReplayTrainer")
    L2, R2, stats2 = run()
    assert orc.bits_equal(_np(L.params), _np(L2.params)) and orc.bits_equal(_np(R.prios), _np(R2.prios))
    assert stats == stats2
    x = R.trans[:256, 0:7].contiguous()
    net = QNet(7, 3)
    net.load_state_dict(L.state_dict())
    net.eval()
    with torch.no_grad():
        ref = net(x.cpu())
    got = q_values(L.acting_weights(_lib.PM_FOLD_EVAL), x).cpu()
    assert (got - ref).abs().max() < 2e-5
