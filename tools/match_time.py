"""Time one opponent assignment and one rating of a population, the device path (pongmi.matchmaking.Matchmaker) against
what a user of the parent commit has to do, by stream events around the calls and one final synchronise:

  A  the host path: read pair_stats back, pongmi.matchmaking.match_host (numpy weights, prefix sums and Philox draws),
     upload the chosen rows' indices, index_select the rows of the weight table into the collector's table
  B  Matchmaker.assign: one launch of pm_league_match
  R  Matchmaker.rate(32): one launch of pm_league_rate (no host counterpart is timed: the parent has no rating)

Shapes: n members, member p meeting members p + 1 .. p + k (mod n) as A, so every list holds 2 k entries: n = 64 with
2, n = 256 with 126 and n = 1 024 with 2 046 (every ordered pair). pair_stats are synthetic (random results of 1..40
games per pair): no match is played, both sides read the same table and, the draws being the same Philox stream, pick
the same opponents, which the tool checks once per shape. --runs rounds of A, B, R in turn (interleaved) on one
device. Prints one raw line per measurement, one line of ranges per shape and a JSON summary line; --out also writes
all of it as a text file."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pongmi._lib import PM_QNET_NW  # noqa: E402
from pongmi.matchmaking import Matchmaker, match_host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64:1,256:63,1024:1023", help="n:k, member p meets the next k members as A")
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--calls", type=int, default=3, help="calls per measurement of A (the host path)")
ap.add_argument("--calls-assign", type=int, default=200, help="calls per measurement of B: microseconds each, so many")
ap.add_argument("--calls-rate", type=int, default=5, help="calls per measurement of R")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--iterations", type=int, default=32)
ap.add_argument("--out", default=None)
args = ap.parse_args()
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


def setup(n, k):
    rng = np.random.default_rng(n)
    a = np.repeat(np.arange(n), k)
    b = (a + np.tile(np.arange(1, k + 1), n)) % n
    n_pairs = n * k
    g = rng.integers(1, 41, n_pairs)
    wa = rng.integers(0, g + 1)
    wb = rng.integers(0, g - wa + 1)
    ps = np.zeros((n_pairs, 8), np.int64)
    ps[:, 0], ps[:, 1], ps[:, 2], ps[:, 3] = g, wa, wb, g - wa - wb
    owner = np.stack([a, b], 1).reshape(-1)
    by = np.argsort(owner, kind="stable")
    player_pairs = np.arange(2 * n_pairs)[by].astype(np.int32)
    player_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int32)
    dev = torch.device("cuda")
    # what a Matchmaker reads of a League (pongmi.league.League builds the same fields from played matches)
    league = SimpleNamespace(n=n, n_players=n, n_pairs=n_pairs, n_nets=n, members_first=True, device=dev,
                             pairs=list(zip(a.tolist(), b.tolist(), [1] * n_pairs)), kinds=[("member", p) for p in range(n)],
                             player_off=player_off, player_pairs=player_pairs,
                             d_player_off=torch.from_numpy(player_off).to(dev),
                             d_player_pairs=torch.from_numpy(player_pairs).to(dev),
                             pair_stats=torch.from_numpy(ps).to(dev),
                             w=torch.randn((n, PM_QNET_NW), device=dev))
    mm = Matchmaker(league, mode="hard", power=2, seed=1)
    wA_host = torch.zeros_like(mm.wA)
    state = dict(round=0)

    def host_path():
        stats = league.pair_stats.cpu().numpy()
        opp, _ = match_host(stats, mm.pair_players, player_off, player_pairs, n, mm.net_of, n, n, "hard", 2, 1,
                            state["round"])
        rows = torch.from_numpy(mm.net_of[np.maximum(opp, 0)].astype(np.int64)).to(dev)
        wA_host.copy_(league.w.index_select(0, rows))  # every member has somebody to draw here
        state["round"] += 1
        return opp

    def device_path():
        out = mm.assign(state["round"])
        state["round"] += 1
        return out

    def rate():
        return mm.rate(args.iterations)

    # the two paths agree: same opponents, same rows
    state["round"] = 12345
    o_host = host_path()
    state["round"] = 12345
    o_dev = device_path()[0].cpu().numpy()
    assert np.array_equal(o_host, o_dev) and torch.equal(wA_host, mm.wA), "the host path and the device path differ"
    assert np.isfinite(rate().cpu().numpy()).all()
    state["round"] = 0
    return league, {"A": host_path, "B": device_path, "R": rate}


prop = torch.cuda.get_device_properties(0)
say(f"# python tools/match_time.py --shapes {args.shapes} --warmup {args.warmup} --calls {args.calls} --calls-assign "
    f"{args.calls_assign} --calls-rate {args.calls_rate} --runs {args.runs} --iterations {args.iterations}")
say(f"# {prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
    f"HIP {torch.version.hip}")
say("# ms per call: A = read pair_stats + match_host + index_select of the chosen rows, B = Matchmaker.assign, "
    f"R = Matchmaker.rate({args.iterations}); `ev` between two stream events, `host` on the host clock, both ended by one "
    "synchronise after the last call")
res = {}
for shape in args.shapes.split(","):
    n, k = (int(x) for x in shape.split(":"))
    league, fns = setup(n, k)
    t = {key: [] for key in fns}
    for run in range(args.runs):
        for key, fn in fns.items():
            ev, host = timed(fn, args.warmup, {"A": args.calls, "B": args.calls_assign, "R": args.calls_rate}[key])
            t[key].append((ev, host))
            say(f"n {n} list {2 * k} run {run} {key} ev {ev:.3f} host {host:.3f}")
    res[f"n{n}_list{2 * k}"] = dict(pairs=league.n_pairs,
                                    **{key: dict(ev=[round(v[0], 3) for v in vs], host=[round(v[1], 3) for v in vs])
                                       for key, vs in t.items()})
    say(f"n {n}, lists of {2 * k}: {league.n_pairs} pairs; " +
        "; ".join(f"{key} ev {min(v[0] for v in vs):.3f}..{max(v[0] for v in vs):.3f} host "
                  f"{min(v[1] for v in vs):.3f}..{max(v[1] for v in vs):.3f}" for key, vs in t.items()) + " ms")
    del fns, league
say(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
