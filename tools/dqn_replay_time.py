"""Time the stand-alone DQN update drawn from a device replay (pm_dqn_replay_update, DQNLearner.update_from)
at batch 256, heads only and whole net, over a full replay of each capacity in --caps, per update and by
stream events, after --warmup updates:

  a  the loop of INTEGRATION.md's "your own loop" on a DeviceReplay: per_sample (a full tree rebuild inside)
     + five torch gathers + DQNLearner.update + per_update + DeviceReplay.refresh() (a second rebuild and a
     host read of max(prios))
  b  update_from(replay, 1), --n times
  c  update_from(replay, 64), ceil(n / 64) times
  d  pm_dqn_update on a resident batch: the floor

--runs rounds of a, b, c, d in turn (interleaved). Prints one raw line per measurement and a JSON summary
line; --out also writes all of it as a text file."""
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
from pongmi.replay import DeviceReplay, per_sample, per_update  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--caps", default="1048576,8192")
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--multi", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, dev = args.batch, torch.device("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, per_call):
    """us per update of `fn` (per_call updates a call): warm-up, then ceil(n / per_call) calls between two events."""
    for _ in range(-(-args.warmup // per_call)):
        fn()
    torch.cuda.synchronize()
    calls = -(-args.n // per_call)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * per_call)


def setup(cap, tf):
    g = torch.Generator().manual_seed(cap + tf)
    R = DeviceReplay(cap, dev)
    R.trans.copy_(torch.rand(cap, 16, generator=g) * 2 - 1)
    R.trans[:, 7] = torch.randint(-1, 2, (cap,), generator=g).float().to(dev)
    bits = torch.randint(0, 3, (cap,), generator=g, dtype=torch.int32) | \
        ((torch.rand(cap, generator=g) < 0.1).to(torch.int32) << 8)
    R.trans[:, 15] = bits.view(torch.float32).to(dev)
    R.prios.copy_(0.01 + 2.99 * torch.rand(cap, generator=g))
    R.size, R.pos = cap, 0
    R.refresh()
    torch.manual_seed(1)
    L = DQNLearner(QNet(7, 3), batch=B, train_features=tf, seed=1)
    # the separate arrays of INTEGRATION.md's loop
    S, NS, Rw = R.trans[:, 0:7].contiguous(), R.trans[:, 8:15].contiguous(), R.trans[:, 7].contiguous()
    A, D = (bits & 0xFF).to(dev), ((bits >> 8) & 1).to(torch.uint8).to(dev)
    step = [0]

    def a():
        bi, w = per_sample(R.prios, R.size, B, beta=0.4, seed=3, counter=step[0])
        td = L.update(S[bi], A[bi], Rw[bi], NS[bi], D[bi], isw=w)
        per_update(R.prios, bi, td)
        R.refresh()
        step[0] += 1

    def b():
        L.update_from(R, 1, seed=3)

    def c():
        L.update_from(R, args.multi, seed=3)

    def d():
        L.update()

    return {"a": (a, 1), "b": (b, 1), "c": (c, args.multi), "d": (d, 1)}, L


p = torch.cuda.get_device_properties(0)
say(f"# python tools/dqn_replay_time.py --batch {B} --caps {args.caps} --warmup {args.warmup} --n {args.n} "
    f"--runs {args.runs} --multi {args.multi}")
say(f"# {p.name} ({getattr(p, 'gcnArchName', '?')}, {p.multi_processor_count} CUs), torch {torch.__version__}, "
    f"HIP {torch.version.hip}")
say("# us per update; a = per_sample + gathers + update + per_update + refresh, b = update_from(1), "
    f"c = update_from({args.multi}), d = pm_dqn_update on a resident batch")
res = {}
for cap in (int(c) for c in args.caps.split(",")):
    for tf, name in ((False, "heads"), (True, "whole_net")):
        fns, L = setup(cap, tf)
        t = {k: [] for k in fns}
        for run in range(args.runs):
            for k, (fn, per_call) in fns.items():
                us = timed(fn, per_call)
                t[k].append(us)
                say(f"cap {cap} {name} run {run} {k} {us:.2f}")
        st = L.stats()
        assert st["status"] == 0, st
        key = f"{cap}_{name}"
        res[key] = {k: [round(v, 2) for v in vs] for k, vs in t.items()}
        med = {k: sorted(vs)[len(vs) // 2] for k, vs in t.items()}
        res[key]["c_below_every_a"] = max(t["c"]) < min(t["a"])
        res[key]["b_minus_d_us"] = round(med["b"] - med["d"], 2)
        res[key]["c_minus_d_us"] = round(med["c"] - med["d"], 2)
        say(f"cap {cap} {name}: median a {med['a']:.2f} b {med['b']:.2f} c {med['c']:.2f} d {med['d']:.2f} us; "
            f"b - d {med['b'] - med['d']:.2f}, c - d {med['c'] - med['d']:.2f}; every c below every a: "
            f"{res[key]['c_below_every_a']}")
say(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
