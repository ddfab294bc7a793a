"""Time one collect step of a population (pm_rollout_pop_push, PopulationRollout.collect) against the loop of n solo
collecting rollouts it replaces and against one solo launch over all n * m arenas, for every n in --sizes and m in
--arenas, by stream events, after a warm-up:

  pc  PopulationRollout.collect(steps, sync=False): one fold + the population's launches      us per collect step
  sl  the solo loop, as a trainer runs it after an update: for every member replay.max_prio_stale (update_from
      sets it), SelfPlayRollout.run(steps, replay=.., sync=False), whose push_prio() reads max(prios) back, and
      set_paramsB(params[p])                                                                    us per collect step
  fl  the floor: ONE solo SelfPlayRollout.run(steps, replay=.., sync=False) over n * m arenas into one ring (one
      opponent, one modelB, no host read): the same arena-steps, none of the population's structure   us per call

A collect step is `--steps` vector steps of all n * m arenas. Every member's ring holds --fill collect steps
(steps * m * fill entries) and is full, so neither side rebinds or grows. --runs rounds of pc, sl, fl in turn
(interleaved); --only restricts the modes (an A/B of two library builds times pc alone, one process per build,
alternating). Prints one raw line per measurement, one line of ranges per (n, m) and a JSON summary line; --out
also writes all of it as a text file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from models.qnet import QNet  # noqa: E402
from pongmi import _lib  # noqa: E402
from pongmi.env import PongEnv2PBatch  # noqa: E402
from pongmi.qnet import fold, pack_state_dict  # noqa: E402
from pongmi.replay import DeviceReplay  # noqa: E402
from pongmi.rollout import PopulationRollout, SelfPlayRollout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,16,256")
ap.add_argument("--arenas", default="256,2048")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--fill", type=int, default=4, help="collect steps a member's ring holds")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=10, help="collect steps per measurement")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--only", default="pc,sl,fl")
ap.add_argument("--label", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm, calls):
    """us per call of `fn`: `warm` calls, then `calls` calls between two events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def full_ring(cap, seed):
    g = torch.Generator().manual_seed(seed)
    R = DeviceReplay(cap, dev)
    R.prios.copy_(0.01 + 2.99 * torch.rand(cap, generator=g))
    R.size, R.pos = cap, 0
    R.refresh()
    return R


def env_of(n, seed):
    e = PongEnv2PBatch(n, seed=seed, autoreset=True)
    e.reset()
    return e


def setup(n, m):
    torch.manual_seed(1)
    wA = fold(pack_state_dict(QNet(7, 3).state_dict()), _lib.PM_FOLD_TRAIN).reshape(-1)
    base = pack_state_dict(QNet(7, 3).state_dict()).reshape(1, -1)
    params = (base + 0.01 * torch.randn((n, base.shape[1]), device=base.device)).contiguous()
    cap, steps = args.steps * m * args.fill, args.steps
    fns = {}
    if "pc" in only:
        pop = PopulationRollout(env_of(n * m, 1), wA, params, n=n, replays=[full_ring(cap, p) for p in range(n)],
                                seed_net=list(range(n)), steps_max=steps)
        fns["pc"] = lambda: pop.collect(steps, sync=False)
    if "sl" in only:
        Rs = [full_ring(cap, p) for p in range(n)]
        solo = [SelfPlayRollout(env_of(m, 1 + p), wA, params[p], seed_net=p) for p in range(n)]

        def sl():
            for p in range(n):
                Rs[p].max_prio_stale = True
                solo[p].run(steps, replay=Rs[p], sync=False)
                solo[p].set_paramsB(params[p])
        fns["sl"] = sl
    if "fl" in only:
        R = full_ring(cap * n, 0)
        one = SelfPlayRollout(env_of(n * m, 1), wA, params[0], seed_net=0)
        fns["fl"] = lambda: one.run(steps, replay=R, sync=False)
    return fns


only = args.only.split(",")
prop = torch.cuda.get_device_properties(0)
say(f"# python tools/rollout_pop_time.py --sizes {args.sizes} --arenas {args.arenas} --steps {args.steps} --fill {args.fill} "
    f"--warmup {args.warmup} --calls {args.calls} --runs {args.runs} --only {args.only}" + (f" --label {args.label}" if args.label else ""))
say(f"# {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
    f"HIP {torch.version.hip}")
say(f"# us per collect step ({args.steps} vector steps of n x m arenas): pc = PopulationRollout.collect, sl = the loop of n solo "
    "run + push_prio + set_paramsB, fl = one solo launch over n * m arenas")
res = {}
for n in (int(x) for x in args.sizes.split(",")):
    for m in (int(x) for x in args.arenas.split(",")):
        fns = setup(n, m)
        t = {k: [] for k in fns}
        for run in range(args.runs):
            for k, fn in fns.items():
                us = timed(fn, args.warmup, args.calls)
                t[k].append(us)
                say(f"n {n} m {m} run {run} {k} {us:.2f}")
        key = f"{n}x{m}"
        res[key] = {k: [round(v, 2) for v in vs] for k, vs in t.items()}
        say(f"n {n} m {m}{' ' + args.label if args.label else ''}: " +
            "; ".join(f"{k} {min(vs):.2f}..{max(vs):.2f}" for k, vs in t.items()) + " us per collect step")
        del fns
say(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
