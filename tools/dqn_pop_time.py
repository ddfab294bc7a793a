"""Time the population learner (pm_dqn_pop_update / pm_dqn_pop_replay_update, DQNPopulation.update /
update_from) against the loop of n solo DQNLearner calls it replaces, at batch 256, heads only and whole net,
for every n in --sizes, by stream events, after a warm-up:

  pu  DQNPopulation.update(): one launch of n workgroups                       us per call (n updates)
  su  n solo DQNLearner.update() calls in a Python loop                        us per loop (n updates)
  pr  DQNPopulation.update_from(replays, --multi): --multi x three launches    us per update step (n updates)
  sr  n solo DQNLearner.update_from(replay, --multi) calls in a Python loop    us per update step (n updates)

Every member has a full replay of --cap entries of its own; the population and the solo learners draw from
the same replays (each keeps the trees current). For n = 1 the solo loop is the solo call itself. --runs
rounds of pu, su, pr, sr in turn (interleaved). Prints one raw line per measurement, one line of ranges per
(n, mode) and a JSON summary line; --out also writes all of it as a text file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from models.qnet import QNet  # noqa: E402
from pongmi.dqn import DQNLearner, DQNPopulation  # noqa: E402
from pongmi.replay import DeviceReplay  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--sizes", default="1,8,64,256")
ap.add_argument("--cap", type=int, default=8192)
ap.add_argument("--warmup", type=int, default=20, help="population steps of update() before timing")
ap.add_argument("--n", type=int, default=100, help="population steps of update() per measurement")
ap.add_argument("--multi", type=int, default=64)
ap.add_argument("--calls", type=int, default=2, help="update_from(.., multi) calls per measurement (one more warms up)")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, dev = args.batch, torch.device("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm, calls, per_call):
    """us per unit of `fn` (per_call units a call): `warm` calls, then `calls` calls between two events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (calls * per_call)


def replay(seed):
    cap = args.cap
    g = torch.Generator().manual_seed(seed)
    R = DeviceReplay(cap, dev)
    R.trans.copy_(torch.rand(cap, 16, generator=g) * 2 - 1)
    R.trans[:, 7] = torch.randint(-1, 2, (cap,), generator=g).float().to(dev)
    bits = torch.randint(0, 3, (cap,), generator=g, dtype=torch.int32) | \
        ((torch.rand(cap, generator=g) < 0.1).to(torch.int32) << 8)
    R.trans[:, 15] = bits.view(torch.float32).to(dev)
    R.prios.copy_(0.01 + 2.99 * torch.rand(cap, generator=g))
    R.size, R.pos = cap, 0
    R.refresh()
    return R


def setup(n, tf):
    torch.manual_seed(1)
    net = QNet(7, 3)
    P = DQNPopulation(net, n=n, batch=B, train_features=tf, seed=list(range(n)))
    solo = [DQNLearner(net, batch=B, train_features=tf, seed=p) for p in range(n)]
    Rs = [replay(p) for p in range(n)]
    P.update_from(Rs, 1, seed=3)  # fills every member's batch buffers; the solo learners' likewise
    for L, R in zip(solo, Rs):
        L.update_from(R, 1, seed=3)

    def su():
        for L in solo:
            L.update()

    def sr():
        for L, R in zip(solo, Rs):
            L.update_from(R, args.multi, seed=3)

    return {"pu": (P.update, args.warmup, args.n, 1), "su": (su, args.warmup, args.n, 1),
            "pr": (lambda: P.update_from(Rs, args.multi, seed=3), 1, args.calls, args.multi),
            "sr": (sr, 1, args.calls, args.multi)}, P, solo


prop = torch.cuda.get_device_properties(0)
say(f"# python tools/dqn_pop_time.py --batch {B} --sizes {args.sizes} --cap {args.cap} --warmup {args.warmup} --n {args.n} "
    f"--multi {args.multi} --calls {args.calls} --runs {args.runs}")
say(f"# {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
    f"HIP {torch.version.hip}")
say("# us per population step (n updates): pu = DQNPopulation.update(), su = n solo update() calls, "
    f"pr = DQNPopulation.update_from(.., {args.multi}) per update step, sr = n solo update_from(.., {args.multi}) per update step")
res = {}
for n in (int(x) for x in args.sizes.split(",")):
    for tf, name in ((False, "heads"), (True, "whole_net")):
        fns, P, solo = setup(n, tf)
        t = {k: [] for k in fns}
        for run in range(args.runs):
            for k, (fn, warm, calls, per_call) in fns.items():
                us = timed(fn, warm, calls, per_call)
                t[k].append(us)
                say(f"n {n} {name} run {run} {k} {us:.2f}")
        st = P.stats()
        assert (st["status"] == 0).all() and all(L.stats()["status"] == 0 for L in solo), st
        key = f"{n}_{name}"
        res[key] = {k: [round(v, 2) for v in vs] for k, vs in t.items()}
        rng = {k: (min(vs), max(vs)) for k, vs in t.items()}
        res[key]["pu_below_every_su"] = rng["pu"][1] < rng["su"][0]
        res[key]["pr_below_every_sr"] = rng["pr"][1] < rng["sr"][0]
        say(f"n {n} {name}: update pop {rng['pu'][0]:.2f}..{rng['pu'][1]:.2f} vs solo loop {rng['su'][0]:.2f}..{rng['su'][1]:.2f} us; "
            f"update_from pop {rng['pr'][0]:.2f}..{rng['pr'][1]:.2f} vs solo loop {rng['sr'][0]:.2f}..{rng['sr'][1]:.2f} us "
            "per update step")
        del fns, P, solo
say(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
