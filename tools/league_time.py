"""Time one fitness evaluation + selection of a population by matches, the device path (pongmi.league) against what a
user of the parent commit does with pongmi.play.play, by stream events around the calls and one final synchronise:

  A  the host path: fold every member (DQNPopulation.acting_weights' loop of n folds), draw every serve on the
     host with CPython's `random` (pongmi.env.draw_serve), pongmi.play.play (numpy block plan, three uploads, four
     result arrays and status read back), win rates per member in numpy, argsort
  B  League.evaluate + League.select + one synchronise

Shapes: `versus` (every member as B against one fixed opponent, --versus members x --versus-episodes episodes) and
`round_robin` (--rr members, every ordered pair, --rr-episodes episodes). The League is built once, outside the
timing: that is the point of it. Both sides play the same block schedule of the same kernel; the serves differ (A's
come from `random`, B's from Philox), so the episodes are not the same ones. --runs rounds of A, B in turn
(interleaved) on one device. Per shape also the share of k_play's columns that start with a slot,
sum(episodes) / (128 * blocks). Prints one raw line per measurement, one line of ranges per shape and a JSON summary
line; --out also writes all of it as a text file."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.qnet import QNet  # noqa: E402
from pongmi import _lib  # noqa: E402
from pongmi.env import draw_serve, env_config  # noqa: E402
from pongmi.league import League  # noqa: E402
from pongmi.play import play  # noqa: E402
from pongmi.qnet import fold, pack_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--versus", default="64,256")
ap.add_argument("--versus-episodes", type=int, default=128)
ap.add_argument("--rr", default="16,64")
ap.add_argument("--rr-episodes", type=int, default=16)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--calls", type=int, default=3, help="evaluations per measurement")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ENV_KW = dict(max_score=3)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm, calls):
    """(ms per call between two stream events, ms per call on the host clock) of `fn`, after `warm` calls; the
    second event is waited for once, at the end."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, (time.perf_counter() - t0) * 1e3 / calls


def setup(kind, n):
    torch.manual_seed(1)
    base = pack_state_dict(QNet(7, 3).state_dict()).reshape(1, -1)
    params = (base + 0.05 * torch.randn((n, base.shape[1]), device=base.device)).contiguous()
    opp = fold(pack_state_dict(QNet(7, 3).state_dict()), _lib.PM_FOLD_EVAL).reshape(-1)
    if kind == "versus":
        L = League.versus(ENV_KW, n, [opp], args.versus_episodes)
    else:
        L = League.round_robin(ENV_KW, n, args.rr_episodes)
    pa = np.array([a for a, _, _ in L.pairs])
    pb = np.array([b for _, b, _ in L.pairs])
    ep = np.array([e for _, _, e in L.pairs])
    who_a, who_b = np.repeat(pa, ep), np.repeat(pb, ep)
    cfg, rng = env_config(**ENV_KW), random.Random(0)
    state = dict(round=0)

    def host_path():
        w = torch.stack([fold(params[p], _lib.PM_FOLD_EVAL)[0].reshape(-1) for p in range(n)])
        if kind == "versus":
            w = torch.cat([w, opp.reshape(1, -1)])
        serves = np.array([draw_serve(rng, cfg) for _ in range(L.E)], np.float64)
        sA, sB, _, _ = play(ENV_KW, w, L.net_A, L.net_B, serves)
        wins = np.bincount(who_a, (sA > sB).astype(np.float64), n + 1) + np.bincount(who_b, (sB > sA).astype(np.float64), n + 1)
        games = np.bincount(who_a, minlength=n + 1) + np.bincount(who_b, minlength=n + 1)
        fitness = wins[:n] / np.maximum(games[:n], 1)
        return np.argsort(-fitness, kind="stable")

    def device_path():
        fitness = L.evaluate(params, state["round"])
        state["round"] += 1
        return L.select(fitness, state["round"])

    return L, {"A": host_path, "B": device_path}


prop = torch.cuda.get_device_properties(0)
say(f"# python tools/league_time.py --versus {args.versus} --versus-episodes {args.versus_episodes} --rr {args.rr} "
    f"--rr-episodes {args.rr_episodes} --warmup {args.warmup} --calls {args.calls} --runs {args.runs}")
say(f"# {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
    f"HIP {torch.version.hip}")
say("# ms per evaluation + selection: A = fold loop + host serves + pongmi.play.play + numpy win rates + argsort, "
    "B = League.evaluate + League.select; `ev` between two stream events, `host` on the host clock, both ended by "
    "one synchronise after the last call")
res = {}
shapes = [("versus", int(x)) for x in args.versus.split(",") if x] + [("round_robin", int(x)) for x in args.rr.split(",") if x]
for kind, n in shapes:
    L, fns = setup(kind, n)
    share = L.column_share()
    t = {k: [] for k in fns}
    for run in range(args.runs):
        for k, fn in fns.items():
            ev, host = timed(fn, args.warmup, args.calls)
            t[k].append((ev, host))
            say(f"{kind} n {n} run {run} {k} ev {ev:.3f} host {host:.3f}")
    L.results()  # raises if an episode of the last evaluation did not finish
    key = f"{kind}_{n}"
    res[key] = dict(episodes=L.E, blocks=L.n_blocks, column_share=round(share, 4),
                    **{k: dict(ev=[round(v[0], 3) for v in vs], host=[round(v[1], 3) for v in vs]) for k, vs in t.items()})
    say(f"{kind} n {n}: {L.n_pairs} pairs, {L.E} episodes, {L.n_blocks} blocks, column share {share:.4f}; " +
        "; ".join(f"{k} ev {min(v[0] for v in vs):.3f}..{max(v[0] for v in vs):.3f} host "
                  f"{min(v[1] for v in vs):.3f}..{max(v[1] for v in vs):.3f}" for k, vs in t.items()) + " ms")
    del fns, L
say(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
