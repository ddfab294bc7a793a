"""Host-only checks of the n-step additions: the ABI stays 27 with every pinned size, the new entry points exist and
reject bad windows before any HIP call, the numpy model of the collector's window (pongmi.rollout.nstep_fold_host)
against a per-transition forward sum, and the guard that keeps a one-step learner off a ring of longer horizons.
No GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

NEW = ("pm_dqn_nstep_sizeof", "pm_dqn_grads_n", "pm_dqn_update_n", "pm_dqn_replay_update_n", "pm_dqn_nstep_pop_set",
       "pm_rollout_push_n", "pm_rollout_nstep_pop_set", "pm_replay_push_n")


def test_abi_is_additive():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_abi_version() == _lib.ABI_VERSION == 27
    for which, cls in ((0, _lib.EnvParams), (1, _lib.EnvState), (2, _lib.Ctrl), (3, _lib.SelfPlay), (4, _lib.Drqn),
                       (5, _lib.DrqnStats), (6, _lib.RnnCtrl), (7, _lib.RnnSelfPlay), (8, _lib.RollReplay), (9, _lib.Dqn),
                       (10, _lib.DqnStats)):
        assert L.pm_sizeof(which) == ctypes.sizeof(cls), cls.__name__
    assert L.pm_sizeof(11) == -1
    assert L.pm_dqn_opt_sizeof() == 32 and L.pm_dqn_replay_sizeof() == 88
    assert L.pm_sizeof(8) == 56 and L.pm_roll_member_sizeof() == 136
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert L.pm_dqn_nstep_sizeof() == ctypes.sizeof(_lib.DqnNstep) == 8
    assert _lib.PM_NSTEP_MAX == 8


def _err(L):
    return L.pm_last_error().decode()


def test_bad_windows_are_rejected_on_the_host():
    from pongmi import _lib
    L = _lib.load()
    none16 = [None] * 5 + [0.0, 0, 0, 0, 4] + [None] * 5 + [8]
    for nstep in (0, -1, 9, 1 << 20):
        assert L.pm_rollout_push_n(*none16, nstep, 0.99, None) == -2  # PM_E_SIZE
        assert f"pm_rollout_push_n: nstep={nstep} (1..8)" in _err(L)
    for gamma in (float("nan"), float("inf"), -float("inf")):
        assert L.pm_rollout_push_n(*none16, 3, gamma, None) == -1  # PM_E_ARG
        assert "pm_rollout_push_n: gamma is not finite" in _err(L)
    # a good window reaches pm_rollout_push's own checks
    assert L.pm_rollout_push_n(*none16, 8, 0.99, None) == -1 and "pm_rollout_push: null replay buffer" in _err(L)
    assert L.pm_rollout_push_n(*none16, 1, 0.99, None) == -1 and "pm_rollout_push: null replay buffer" in _err(L)
    # the population calls need a handle
    assert L.pm_rollout_nstep_pop_set(None, None, None, None) == -1 and "pm_rollout_nstep_pop_set: null handle" in _err(L)
    assert L.pm_dqn_nstep_pop_set(None, None, None) == -1 and "pm_dqn_nstep_pop_set: null handle" in _err(L)
    # the learner entries: a null struct or horizon is the _opt entry, with its checks; the replay entry needs one
    assert L.pm_dqn_update_n(None, None, None, None) == -1 and "pm_dqn: null descriptor" in _err(L)
    assert L.pm_dqn_grads_n(None, None, ctypes.byref(_lib.DqnNstep()), None) == -1 and "null descriptor" in _err(L)
    d, rp = _lib.Dqn(), _lib.DqnReplay()
    assert L.pm_dqn_replay_update_n(ctypes.byref(d), None, None, ctypes.byref(rp), 1, None) == -1
    assert "pm_dqn_replay_update_n: null horizon" in _err(L)
    assert L.pm_dqn_replay_update_n(ctypes.byref(d), None, ctypes.byref(_lib.DqnNstep()), ctypes.byref(rp), 1, None) == -1
    assert "pm_dqn_replay_update_n: null horizon" in _err(L)
    assert L.pm_replay_push_n(*[None] * 3, 8, 0, 0.6, 1.0, *[None] * 6, 1, None) == -1 and "null replay buffer" in _err(L)


def test_python_classes_name_the_offending_member():
    from pongmi.dqn import DQNLearner, DQNPopulation
    from pongmi.rollout import PopulationRollout
    env = types.SimpleNamespace(n=12, inject=None, autoreset=1, seed=1, device="cpu")
    replays = [types.SimpleNamespace(cap=64) for _ in range(3)]
    for kw, word in ((dict(nstep=[1, 9, 2]), "member 1: nstep 9"), (dict(nstep=0), "member 0: nstep 0"),
                     (dict(nstep=2, gamma=[0.9, 0.9, float("nan")]), "member 2: gamma")):
        with pytest.raises(ValueError, match=word):
            PopulationRollout(env, torch.zeros(9944), torch.zeros((3, 5452)), n=3, replays=replays, **kw)
    with pytest.raises(ValueError, match="nstep 9"):
        DQNPopulation(torch.zeros((2, 5452)), nstep=[1, 9], device="cpu")
    with pytest.raises(ValueError, match="nstep 0"):
        DQNLearner(torch.zeros(5452), nstep=0, device="cpu")


# ----------------------------------------------------------------------------- the host model
def _rows(rewards, dones, seed=0):
    """[steps * n][16] one-step rows in launch order from [steps][n] rewards and dones."""
    steps, n = np.shape(rewards)
    rng = np.random.default_rng(seed)
    rows = rng.random((steps, n, 16), dtype=np.float32)
    rows[:, :, 7] = np.asarray(rewards, np.float32)
    bits = rng.integers(0, 3, (steps, n)).astype(np.int32) | (np.asarray(dones, np.int32) << 8)
    rows[:, :, 15] = bits.view(np.float32)
    return rows.reshape(-1, 16)


def _forward(rows, n, steps, N, gamma):
    """The same rows transition by transition: the one opened at step t of an arena ends at e = the first of (a done
    at or after t, t + N - 1, the last step) and sums its rewards forward."""
    r = rows.reshape(steps, n, 16)
    bits = r[:, :, 15].view(np.int32)
    out = r.copy()
    g = np.float32(gamma)
    for i in range(n):
        for t in range(steps):
            R, f, e = np.float32(0), np.float32(1), t
            while True:
                R = np.float32(R + np.float32(f * r[e, i, 7]))
                f = np.float32(f * g)
                if (bits[e, i] >> 8) & 1 or e == steps - 1 or e - t + 1 == N:
                    break
                e += 1
            out[t, i, 7] = R
            out[t, i, 8:15] = r[e, i, 8:15]
            out[t, i, 15] = np.int32((bits[t, i] & 0xFF) | (bits[e, i] & 0x100) | ((e - t) << 16)).view(np.float32)
    return out.reshape(-1, 16)


def _case(name):
    z = np.zeros((12, 3))
    r, d = z.copy(), z.copy().astype(int)
    if name == "done on the first step":
        d[0, 0], r[0, 0] = 1, -1
    elif name == "done on the last step":
        d[11, 1], r[11, 1] = 1, 1
    elif name == "two dones fewer than N apart":  # one step, then two steps apart, in one arena
        d[3, 2] = d[4, 2] = d[6, 2] = 1
        r[3, 2], r[4, 2], r[6, 2] = 1, -1, 1
    elif name == "steps < N":
        r, d = r[:2], d[:2]
        r[1, 0] = 1
    elif name == "everything":
        rng = np.random.default_rng(1)
        d = (rng.random((12, 3)) < 0.3).astype(int)
        r = np.where(d, rng.choice([-1.0, 1.0], (12, 3)), 0.0)
    return r, d


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["done on the first step", "done on the last step", "two dones fewer than N apart",
                                  "no done", "steps < N", "everything"])
def test_fold_model(name, N):
    from pongmi.rollout import nstep_fold_host
    r, d = _case(name)
    steps, n = r.shape
    rows = _rows(r + 0.25 * (name == "no done"), d)  # a reward on every tick where nothing ends
    got = nstep_fold_host(rows, n, steps, N, 0.97)
    assert got.dtype == np.float32 and got.shape == rows.shape
    assert np.array_equal(got.view(np.int32), _forward(rows, n, steps, N, 0.97).view(np.int32))
    assert np.array_equal(got[:, :7], rows[:, :7])  # s stays
    k = ((got[:, 15].view(np.int32) >> 16) & 7) + 1
    assert k.max() <= min(N, steps)
    if N == 1:
        assert np.array_equal(got.view(np.int32), rows.view(np.int32))
    elif name == "no done":
        assert k.reshape(steps, n)[:steps - N + 1].min() == N and k.reshape(steps, n)[-1].max() == 1


def test_fold_model_by_hand():
    from pongmi.rollout import nstep_fold_host
    rows = _rows([[0], [1], [0], [-1]], [[0], [1], [0], [0]])
    got = nstep_fold_host(rows, 1, 4, 3, 0.5)
    assert got[:, 7].tolist() == [0.5, 1.0, -0.5, -1.0]
    bits = got[:, 15].view(np.int32)
    assert ((bits >> 16) & 7).tolist() == [1, 0, 1, 0] and ((bits >> 8) & 1).tolist() == [1, 1, 0, 0]
    assert np.array_equal(got[0, 8:15], rows[1, 8:15]) and np.array_equal(got[2, 8:15], rows[3, 8:15])
    with pytest.raises(ValueError, match="N 9"):
        nstep_fold_host(rows, 1, 4, 9, 0.5)


# ----------------------------------------------------------------------------- the guard
def _cpu_learner(nstep):
    from pongmi import _lib
    from pongmi.dqn import BUFFERS, DQNLearner
    buffers = {name: torch.zeros((4, 7) if name in ("s", "ns") else 64) for name in BUFFERS}
    return DQNLearner.over(_lib.load(), torch.device("cpu"), buffers, None, batch=4, gamma=0.99, lr=1e-3, betas=(0.9, 0.999),
                           eps=1e-8, target_update_interval=10, train_features=False, fresh_noise=True, seed=0, loss="mse",
                           huber_beta=1.0, max_norm=None, nstep=nstep,
                           horizon=torch.ones(4, dtype=torch.uint8) if nstep > 1 else None)


def test_one_step_learner_refuses_a_ring_of_longer_horizons():
    from pongmi import _lib
    from pongmi.dqn_pop import check_replay_horizon
    ring = types.SimpleNamespace(max_horizon=3)
    with pytest.raises(_lib.PongmiError, match="horizon up to 3 .* nstep=1"):
        _cpu_learner(1).update_from(ring)
    with pytest.raises(_lib.PongmiError, match="member 2"):
        check_replay_horizon("DQNPopulation.update_from: member 2", ring, 1)
    check_replay_horizon("x", ring, 2)  # a learner built for horizons takes any ring
    check_replay_horizon("x", types.SimpleNamespace(max_horizon=1), 1)
    L = _cpu_learner(3)
    assert L.nstep == 3 and L.ns_desc.horizon == L.horizon.data_ptr()
    with pytest.raises(_lib.PongmiError, match="nstep=1"):
        _cpu_learner(1).load_batch(np.zeros((2, 7)), [0, 1], [0, 0], np.zeros((2, 7)), [0, 0], horizon=[1, 2])
