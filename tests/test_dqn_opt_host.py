"""CPU-only checks of the stand-alone DQN learner's loss / clip options (pm_dqn_opt, pm_dqn_*_opt,
DQNLearner(loss=, huber_beta=, max_norm=)): the additive ABI (version and pm_sizeof as they were, a size
function of its own), header / EXPORTED / library agreement, every rejection before any launch, the
constructor's ValueErrors before anything is allocated, and which entry points a learner calls. No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_ENTRIES = ("pm_dqn_grads_opt", "pm_dqn_apply_opt", "pm_dqn_update_opt", "pm_dqn_replay_update_opt")
DQN_BUFS = ("params", "target", "adam_m", "adam_v", "grad", "stats", "s", "ns", "act", "rew", "done", "td")
NAN, INF = float("nan"), float("inf")


def _desc(_lib, **kw):
    d = _lib.Dqn()
    for name in DQN_BUFS + ("isw",):
        setattr(d, name, 4096)  # never dereferenced: every check below fails on the host
    d.batch, d.noise, d.target_update_interval = 256, _lib.PM_FOLD_TRAIN_FRESH, 1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _rp(_lib):
    return _lib.DqnReplay(trans=4096, prios=4096, per_work=4096, idx=4096, u=None, cap=1024, size=1024, alpha=0.6,
                          beta_start=0.4, beta_frames=100000, seed=0)


def _opt(_lib, **kw):
    o = _lib.DqnOpt(loss=_lib.PM_DQN_LOSS_SQUARED, huber_beta=1.0, max_norm=0.0, norm=None)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _call(L, _lib, entry, d, o, rp="default", updates=1):
    fn = getattr(L, entry)
    dp = ctypes.byref(d) if d is not None else None
    op = ctypes.byref(o) if o is not None else None
    if entry == "pm_dqn_replay_update_opt":
        rp = _rp(_lib) if rp == "default" else rp
        return fn(dp, op, ctypes.byref(rp) if rp is not None else None, updates, None)
    return fn(dp, op, None)


def test_abi_is_additive_and_the_struct_matches_the_header():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_abi_version() == _lib.ABI_VERSION == 27
    assert L.pm_dqn_opt_sizeof() == ctypes.sizeof(_lib.DqnOpt) == 32
    assert L.pm_sizeof(11) == -1
    assert L.pm_sizeof(9) == ctypes.sizeof(_lib.Dqn) and L.pm_sizeof(10) == ctypes.sizeof(_lib.DqnStats) == 32
    assert L.pm_dqn_replay_sizeof() == ctypes.sizeof(_lib.DqnReplay) == 88
    hdr = open(os.path.join(ROOT, "include", "pongmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in OPT_ENTRIES + ("pm_dqn_opt_sizeof",):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.EXPORTED and hasattr(L, name), name
        assert re.search(rf" T {name}\b", nm), name
    body = re.search(r"typedef struct pm_dqn_opt \{(.*?)\} pm_dqn_opt;", code, re.S).group(1)
    names = [w for w in re.findall(r"\w+", body) if w not in {"int32_t", "double", "float"}]
    assert names == [f for f, _ in _lib.DqnOpt._fields_], names
    for k in ("PM_DQN_LOSS_SQUARED", "PM_DQN_LOSS_HUBER"):
        assert int(re.search(rf"#define {k}\s+(\d+)", hdr).group(1)) == getattr(_lib, k), k
    assert "HALF the squared loss" in hdr  # the beta = 1 quadratic zone is documented


@pytest.mark.parametrize("entry", OPT_ENTRIES)
def test_opt_entry_points_reject_bad_arguments_without_a_gpu(entry):
    from pongmi import _lib
    L = _lib.load()
    H = _lib.PM_DQN_LOSS_HUBER

    def bad(o, word):
        assert _call(L, _lib, entry, _desc(_lib), o) == -1, (entry, word)
        msg = L.pm_last_error()
        assert msg and word in msg, (entry, word, msg)

    # an unknown loss
    for loss in (2, -1, 1 << 20):
        bad(_opt(_lib, loss=loss), b"loss")
    # huber_beta <= 0 or not finite, with Huber selected
    for beta in (0.0, -1.0, -0.0, NAN, INF, -INF):
        bad(_opt(_lib, loss=H, huber_beta=beta), b"huber_beta")
    # max_norm < 0 or not finite, under either loss
    for mn in (-1.0, -1e-300, NAN, INF, -INF):
        bad(_opt(_lib, max_norm=mn), b"max_norm")
        bad(_opt(_lib, loss=H, max_norm=mn), b"max_norm")
    # a null pm_dqn, with a null and with a good opt
    assert _call(L, _lib, entry, None, None) == -1 and b"null" in L.pm_last_error()
    assert _call(L, _lib, entry, None, _opt(_lib, loss=H, max_norm=1.0)) == -1 and b"null" in L.pm_last_error()
    # whatever the plain entry points reject, with a good opt and with a null one
    for o in (_opt(_lib, loss=H, huber_beta=2.0, max_norm=1.0), None):
        for name in DQN_BUFS:
            assert _call(L, _lib, entry, _desc(_lib, **{name: None}), o) == -1, name
            assert b"null" in L.pm_last_error()
        for batch in (0, -1, 257, 1 << 20):
            assert _call(L, _lib, entry, _desc(_lib, batch=batch), o) == -2, batch
            assert b"batch" in L.pm_last_error()
        assert _call(L, _lib, entry, _desc(_lib, noise=_lib.PM_FOLD_EVAL), o) == -1
        assert _call(L, _lib, entry, _desc(_lib, target_update_interval=0), o) == -1


def test_replay_update_opt_keeps_the_replay_checks():
    from pongmi import _lib
    L = _lib.load()
    e, o = "pm_dqn_replay_update_opt", _opt(_lib, loss=_lib.PM_DQN_LOSS_HUBER, max_norm=1.0)
    assert _call(L, _lib, e, _desc(_lib), o, rp=None) == -1 and b"null" in L.pm_last_error()
    assert _call(L, _lib, e, _desc(_lib, isw=None), o) == -1 and b"isw" in L.pm_last_error()
    rp = _rp(_lib)
    rp.size = 0
    assert _call(L, _lib, e, _desc(_lib), o, rp=rp) == -2 and b"size" in L.pm_last_error()
    assert _call(L, _lib, e, _desc(_lib), o, updates=0) == -2 and b"updates" in L.pm_last_error()
    # a bad opt is an argument error even where the replay is bad too
    assert _call(L, _lib, e, _desc(_lib), _opt(_lib, loss=7), rp=rp) == -1 and b"loss" in L.pm_last_error()


@pytest.mark.parametrize("kw", [dict(loss="l1"), dict(loss="MSE"), dict(loss=None), dict(huber_beta=0), dict(huber_beta=-1.0),
                                dict(loss="huber", huber_beta=NAN), dict(loss="huber", huber_beta=INF),
                                dict(max_norm=-1), dict(max_norm=0), dict(max_norm=NAN), dict(max_norm=INF)])
def test_constructor_rejects_bad_options_before_touching_a_device(kw):
    """device stays at its default "cuda": the ValueError comes before any allocation, so it comes on a
    machine without a GPU too (there an allocation would raise something else)."""
    from models.qnet import QNet
    from pongmi.dqn import DQNLearner
    with pytest.raises(ValueError, match="DQNLearner"):
        DQNLearner(QNet(7, 3), batch=32, **kw)


class _Rec:
    """libpongmi with the learner's entry points recorded instead of launched."""

    def __init__(self, _lib):
        self._lib, self.calls = _lib, []
        for name in ("pm_dqn_grads", "pm_dqn_apply", "pm_dqn_update"):
            setattr(self, name, self._plain(name))
            setattr(self, name + "_opt", self._with_opt(name + "_opt"))

    def _plain(self, name):
        def f(d, stream):
            self.calls.append((name, None))
            return 0
        return f

    def _with_opt(self, name):
        def f(d, o, stream):
            c = ctypes.cast(o, ctypes.POINTER(self._lib.DqnOpt)).contents
            self.calls.append((name, (c.loss, c.huber_beta, c.max_norm, c.norm)))
            return 0
        return f

    def pm_dqn_replay_update(self, d, rp, updates, stream):
        self.calls.append(("pm_dqn_replay_update", None))
        return 0

    def pm_dqn_replay_update_opt(self, d, o, rp, updates, stream):
        c = ctypes.cast(o, ctypes.POINTER(self._lib.DqnOpt)).contents
        self.calls.append(("pm_dqn_replay_update_opt", (c.loss, c.huber_beta, c.max_norm, c.norm)))
        return 0


@pytest.mark.parametrize("kw,opt", [(dict(), None), (dict(loss="mse", huber_beta=3.0), None),
                                    (dict(loss="huber"), (1, 1.0, 0.0, False)),
                                    (dict(loss="huber", huber_beta=2.0, max_norm=0.5), (1, 2.0, 0.5, True)),
                                    (dict(max_norm=10), (0, 1.0, 10.0, True))])
def test_learner_routes_to_the_plain_or_the_opt_entry_points(monkeypatch, kw, opt):
    """Both options at their defaults: the four plain entry points, as before. Otherwise the _opt ones with the
    learner's pm_dqn_opt; stats() has `norm` exactly on a learner built with max_norm; ReplayTrainer's
    update_from call carries the options because the learner does."""
    from models.qnet import QNet
    from pongmi import _lib, dqn, replay
    L = dqn.DQNLearner(QNet(7, 3), batch=8, device="cpu", **kw)
    monkeypatch.setattr(dqn, "stream_ptr", lambda stream=None: 0)
    rec = L.lib = _Rec(_lib)
    R = replay.DeviceReplay(32, "cpu")
    R.size = 20
    L.update()
    L.grads()
    L.apply()
    L.update_from(R, 2)
    suffix = "" if opt is None else "_opt"
    assert [n for n, _ in rec.calls] == [n + suffix for n in ("pm_dqn_update", "pm_dqn_grads", "pm_dqn_apply",
                                                              "pm_dqn_replay_update")]
    for _, got in rec.calls:
        if opt is None:
            assert got is None
        else:
            assert got[:3] == opt[:3] and bool(got[3]) == opt[3]
            assert not opt[3] or got[3] == L.norm.data_ptr()
    keys = {"steps", "adam_t", "loss", "q_mean", "status"}
    assert set(L.stats()) == (keys | {"norm"} if "max_norm" in kw else keys)
    assert R.max_prio_stale is True
