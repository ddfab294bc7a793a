"""Time the stand-alone double-DQN update (pm_dqn_update: k_dqn_grads + k_dqn_apply) at batch 256, heads
only and whole net, and the same two updates through torch on the device (models.qnet.QNet +
torch.optim.Adam + the loss of scripts/train_iterative.py:152-161): after 50 warm-up updates, 500
back-to-back updates on one stream between two events. Prints one JSON line; --out also writes it,
with the device's identity, as a text file. --loss huber / --max-norm N time the same update with the
learner's options (pm_dqn_update_opt) and give the torch side F.smooth_l1_loss / clip_grad_norm_ too; the
result line then also names them. Without them the invocation and its keys are as they were."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from models.qnet import QNet  # noqa: E402
from pongmi.dqn import DQNLearner  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--loss", choices=("mse", "huber"), default="mse")
ap.add_argument("--huber-beta", type=float, default=1.0)
ap.add_argument("--max-norm", type=float, default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, dev = args.batch, torch.device("cuda")
g = torch.Generator().manual_seed(0)
s, ns = torch.rand(B, 7, generator=g).to(dev), torch.rand(B, 7, generator=g).to(dev)
a = torch.randint(0, 3, (B,), generator=g).to(dev)
r = torch.randint(-1, 2, (B,), generator=g).float().to(dev)
d = (torch.rand(B, generator=g) < 0.1).to(dev)
iw = (0.2 + 0.8 * torch.rand(B, generator=g)).to(dev)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.n


def torch_update(train_features):
    """What a caller has without pm_dqn_update: the reference's train_step body on device tensors."""
    torch.manual_seed(1)
    modelB = QNet(7, 3).to(dev)
    targetB = QNet(7, 3).to(dev)
    targetB.load_state_dict(modelB.state_dict())
    targetB.eval()
    if not train_features:
        for p in modelB.features.parameters():
            p.requires_grad = False
    params = list(modelB.parameters()) if train_features else \
        list(modelB.fc_V.parameters()) + list(modelB.fc_A.parameters())
    opt = torch.optim.Adam(params, lr=2.5e-4)
    steps = [0]

    def step():
        modelB.reset_noise()
        q = modelB(s).gather(1, a.unsqueeze(1)).squeeze(1)
        with torch.no_grad():  # the drop-in QNet routes these two forwards to pm_qnet_fold + pm_qnet_q
            na = modelB(ns).argmax(1, keepdim=True)
            nq = targetB(ns).gather(1, na).squeeze(1)
        t = r + 0.99 * nq * (~d)
        if args.loss == "huber":
            loss = (iw * torch.nn.functional.smooth_l1_loss(q, t, reduction="none", beta=args.huber_beta)).mean()
        else:
            loss = (iw * (q - t).pow(2)).mean()
        opt.zero_grad()
        loss.backward()
        if args.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        opt.step()
        steps[0] += 1
        if steps[0] % 1000 == 0:
            targetB.load_state_dict(modelB.state_dict())

    return step


res = {"batch": B, "warmup": args.warmup, "updates": args.n}
options = args.loss != "mse" or args.max_norm is not None
kw = dict(loss=args.loss, huber_beta=args.huber_beta, max_norm=args.max_norm) if options else {}
if options:
    res.update(loss_fn=args.loss, huber_beta=args.huber_beta, max_norm=args.max_norm)
for tf, name in ((False, "heads"), (True, "whole_net")):
    torch.manual_seed(1)
    L = DQNLearner(QNet(7, 3), batch=B, train_features=tf, seed=1, **kw)
    L.load_batch(s, a, r, ns, d, isw=iw)
    res[f"pm_dqn_update_{name}_us"] = round(timed(L.update), 2)
    res[f"loss_{name}"] = L.stats()["loss"]
    if args.max_norm is not None:
        res[f"norm_{name}"] = L.stats()["norm"]
    res[f"torch_{name}_us"] = round(timed(torch_update(tf)), 2)
p = torch.cuda.get_device_properties(0)
res["device"] = f"{p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, " \
                f"HIP {torch.version.hip}"
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        opts = (f" --loss {args.loss}" if args.loss != "mse" else "") + \
            (f" --huber-beta {args.huber_beta}" if args.loss == "huber" and args.huber_beta != 1.0 else "") + \
            (f" --max-norm {args.max_norm}" if args.max_norm is not None else "")
        fh.write(f"# python tools/dqn_update_time.py --batch {B} --warmup {args.warmup} --n {args.n}{opts}\n")
        fh.write(f"# {res['device']}\n")
        for k, v in res.items():
            if k != "device":
                fh.write(f"{k}: {v}\n")
