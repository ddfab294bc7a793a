#!/usr/bin/env python3
"""Golden fixture for whole-net double-DQN training (pm_dqn_update with train_features = 1), produced
with the REFERENCE's QNet module and torch autograd.

Run only in the build container (the reference does not exist on the GPU box):

    python -B tests/golden/make_golden_dqn_full.py

make_golden.py's make_dqn with nothing frozen: modelB = the reference's QNet with model5-5_fault.pth's
modelB weights, every parameter trainable, Adam(modelB.parameters(), lr 2.5e-4); targetB = a deep copy
in eval mode; three consecutive train_step bodies (scripts/train_iterative.py:141-168) at batch 256
with target_update_interval 2, gamma 0.99.

Condition on the inputs: the smallest top-2 gap of Q_B(s') is > 1e-4 on all three steps (so no a* hangs
on float32 rounding); the generator asserts it and moves to the next seed otherwise.

Writes dqn_full_steps.npz: dqn_steps.npz's keys (init.<state_dict key>, param_names, and per step k
s{k}.s / ns / a / r / d / iw, s{k}.noiseB.<epsilon key>, s{k}.grads, s{k}.loss, s{k}.q, s{k}.targets,
s{k}.na, s{k}.errors, s{k}.params_after, s{k}.target_heads_after), where grads / params_after cover all
5 192 parameters in modelB.parameters() order, plus
  s{k}.grads64         the float64-autograd gradient of the same step on a .double() copy
  s{k}.target_after    targetB's 5 192 parameters after the step
  s{k}.gap             the smallest top-2 gap of Q_B(s')
  seed                 the RandomState seed used
"""
import copy
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("PONG_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
GAMMA, LR, INTERVAL, BATCH, MIN_GAP = 0.99, 2.5e-4, 2, 256, 1e-4


def obs_batch(rng, n):
    lo = np.array([0, 0, -0.08, -0.08, 0, 0, -5], np.float32)
    hi = np.array([1, 1, 0.08, 0.08, 1, 1, 5], np.float32)
    return (lo + (hi - lo) * rng.random_sample((n, 7))).astype(np.float32)


def flat(tensors):
    return np.concatenate([t.detach().numpy().ravel() for t in tensors])


def loss_of(modelB, targetB, s, a, r, ns, d, iw):
    q_vals = modelB(s).gather(1, a.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        qn = modelB(ns)
        na = qn.argmax(1, keepdim=True)
        nq = targetB(ns).gather(1, na).squeeze(1)
    targets = r + GAMMA * nq * (~d)
    return (iw * (q_vals - targets).pow(2)).mean(), q_vals, targets, na, qn


def run(QNet, cp, seed):
    modelB = QNet(7, 3)
    modelB.load_state_dict(cp["modelB"], strict=True)
    targetB = copy.deepcopy(modelB)
    targetB.eval()
    params = list(modelB.parameters())
    opt = torch.optim.Adam(params, lr=LR)
    out = {f"init.{k}": v.detach().numpy().astype(np.float32) for k, v in modelB.state_dict().items()}
    out["param_names"] = np.array([n for n, _ in modelB.named_parameters()])
    out["seed"] = np.int64(seed)
    rng = np.random.RandomState(seed)
    train_steps = 0
    for step in range(3):
        s, ns = obs_batch(rng, BATCH), obs_batch(rng, BATCH)
        a = rng.randint(0, 3, BATCH).astype(np.int64)
        r = rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0], BATCH).astype(np.float32)
        d = rng.rand(BATCH) < 0.1
        iw = rng.uniform(0.2, 1.0, BATCH).astype(np.float32)
        iw /= iw.max()
        torch.manual_seed(1000 + step)
        modelB.reset_noise()
        targetB.reset_noise()
        out[f"s{step}.s"], out[f"s{step}.ns"], out[f"s{step}.a"] = s, ns, a
        out[f"s{step}.r"], out[f"s{step}.d"], out[f"s{step}.iw"] = r, d, iw
        for k, v in modelB.state_dict().items():
            if "epsilon" in k:
                out[f"s{step}.noiseB.{k}"] = v.numpy().copy()
        t = [torch.from_numpy(x) for x in (s, a, r, ns, d, iw)]
        # the same step in float64 (parameters, noise and inputs widened exactly)
        mB64, mT64 = copy.deepcopy(modelB).double(), copy.deepcopy(targetB).double()
        t64 = [x.double() if x.dtype == torch.float32 else x for x in t]
        loss64 = loss_of(mB64, mT64, *t64)[0]
        loss64.backward()
        out[f"s{step}.grads64"] = flat([p.grad for p in mB64.parameters()])
        loss, q_vals, targets, na, qn = loss_of(modelB, targetB, *t)
        top2 = torch.sort(qn, dim=1, descending=True).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        if not gap > MIN_GAP:
            return None
        opt.zero_grad()
        loss.backward()
        out[f"s{step}.grads"] = flat([p.grad for p in params])
        opt.step()
        out[f"s{step}.gap"] = np.float64(gap)
        out[f"s{step}.loss"] = np.float32(loss.item())
        out[f"s{step}.q"] = q_vals.detach().numpy()
        out[f"s{step}.targets"] = targets.detach().numpy()
        out[f"s{step}.na"] = na.squeeze(1).numpy()
        out[f"s{step}.errors"] = (q_vals - targets).detach().abs().numpy()
        out[f"s{step}.params_after"] = flat(params)
        train_steps += 1
        if train_steps % INTERVAL == 0:
            targetB.load_state_dict(modelB.state_dict())
        out[f"s{step}.target_after"] = flat(list(targetB.parameters()))
        out[f"s{step}.target_heads_after"] = flat(list(targetB.fc_V.parameters()) + list(targetB.fc_A.parameters()))
    return out


def main():
    sys.path.insert(0, REF)
    from models.qnet import QNet  # the reference module
    cp = torch.load(os.path.join(REF, "checkpoints", "model5-5_fault.pth"), map_location="cpu", weights_only=True)
    seed = 11
    while (out := run(QNet, cp, seed)) is None:
        seed += 1
    path = os.path.join(OUT, "dqn_full_steps.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, seed", seed, "losses",
          [float(out[f"s{i}.loss"]) for i in range(3)], "gaps", [float(out[f"s{i}.gap"]) for i in range(3)])


if __name__ == "__main__":
    main()
