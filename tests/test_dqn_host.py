"""CPU-only checks of the stand-alone DQN learner's boundary (pm_dqn_*, pongmi.dqn.DQNLearner): struct
layouts, argument rejection before any launch, and the optimizer state_dict of both modes against a
real torch.optim.Adam. No GPU."""
import ctypes

import numpy as np
import pytest
import torch


def _desc(_lib, **kw):
    d = _lib.Dqn()
    for name in ("params", "target", "adam_m", "adam_v", "grad", "stats", "s", "ns", "act", "rew", "done", "td"):
        setattr(d, name, 4096)  # never dereferenced: every check below fails on the host
    d.batch, d.noise, d.target_update_interval = 256, _lib.PM_FOLD_TRAIN_FRESH, 1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_struct_sizes_and_constants_match_header():
    import os
    import re
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_abi_version() == _lib.ABI_VERSION == 27
    assert L.pm_sizeof(9) == ctypes.sizeof(_lib.Dqn)
    assert L.pm_sizeof(10) == ctypes.sizeof(_lib.DqnStats) == 32
    assert L.pm_sizeof(11) == -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pongmi.h")).read()
    assert int(re.search(r"#define PM_DQN_NPARAM (\d+)", hdr).group(1)) == _lib.PM_DQN_NPARAM == _lib.PM_QNET_EPS_OFF
    for name in ("pm_dqn_grads", "pm_dqn_apply", "pm_dqn_update"):
        assert name in _lib.EXPORTED and hasattr(L, name)


@pytest.mark.parametrize("entry", ["pm_dqn_grads", "pm_dqn_apply", "pm_dqn_update"])
def test_entry_points_reject_bad_arguments_without_a_gpu(entry):
    from pongmi import _lib
    L = _lib.load()
    fn = getattr(L, entry)
    assert fn(None, None) == -1
    for name in ("params", "target", "adam_m", "adam_v", "grad", "stats", "s", "ns", "act", "rew", "done", "td"):
        assert fn(ctypes.byref(_desc(_lib, **{name: None})), None) == -1, name
        assert b"null" in L.pm_last_error()
    for batch in (0, -1, 257, 1 << 20):
        assert fn(ctypes.byref(_desc(_lib, batch=batch)), None) == -2, batch
        assert b"batch" in L.pm_last_error()
    assert fn(ctypes.byref(_desc(_lib, noise=_lib.PM_FOLD_EVAL)), None) == -1
    assert fn(ctypes.byref(_desc(_lib, target_update_interval=0)), None) == -1


@pytest.mark.parametrize("train_features", [False, True])
def test_optimizer_state_dict_loads_into_torch_adam_and_round_trips(train_features):
    from models.qnet import QNet
    from pongmi._lib import PM_DQN_NPARAM, PM_QNET_HEAD_OFF
    from pongmi.dqn import DQNLearner
    torch.manual_seed(3)
    net = QNet(7, 3)
    L = DQNLearner(net, batch=32, lr=3e-4, betas=(0.8, 0.99), eps=1e-7, train_features=train_features, device="cpu")
    off = 0 if train_features else PM_QNET_HEAD_OFF
    assert L.optimizer_state_dict()["state"] == {}  # a fresh optimizer has no per-parameter state
    L.adam_m[off:] = torch.randn(PM_DQN_NPARAM - off)
    L.adam_v[off:] = torch.rand(PM_DQN_NPARAM - off)
    L._set_stats(adam_t=17, steps=40)
    sd = L.optimizer_state_dict()
    params = list(net.parameters()) if train_features else list(net.fc_V.parameters()) + list(net.fc_A.parameters())
    assert sum(p.numel() for p in params) == PM_DQN_NPARAM - off
    opt = torch.optim.Adam(params, lr=1.0)
    opt.load_state_dict(sd)  # a real Adam over the same parameters takes it
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"]) == (3e-4, (0.8, 0.99), 1e-7)
    o = off
    for p in params:
        st = opt.state[p]
        assert float(st["step"]) == 17.0 and st["exp_avg"].shape == p.shape
        assert torch.equal(st["exp_avg"].reshape(-1), L.adam_m[o:o + p.numel()])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), L.adam_v[o:o + p.numel()])
        o += p.numel()
    assert o == PM_DQN_NPARAM
    M = DQNLearner(net, batch=32, train_features=train_features, device="cpu")
    M.load_optimizer_state_dict(opt.state_dict())
    assert torch.equal(M.adam_m, L.adam_m) and torch.equal(M.adam_v, L.adam_v)
    assert M.stats()["adam_t"] == 17 and M.stats()["steps"] == 0
    assert np.all(M.adam_m[:off].numpy() == 0)  # heads only: the feature slots are not the optimizer's
    M.new_optimizer()
    assert M.stats()["adam_t"] == 0 and not M.adam_m.any() and not M.adam_v.any()
    M.set_train_steps(9)
    assert M.stats()["steps"] == 9
    assert list(L.state_dict().keys()) == list(net.state_dict().keys())
    for k, v in net.state_dict().items():
        assert torch.equal(L.state_dict()[k], v) and torch.equal(L.target_state_dict()[k], v), k
