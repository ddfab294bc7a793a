"""What recording costs: wall time of play_matches with no episode recorded, with one episode per
pair recorded, and with every episode recorded, on the two plans of tools/play_rnn_bench.py plus a
QNet-only plan.

  evaluate  one trained QNetRNN pair, config_rnn.yaml's eval_episodes (pm_play_rnn);
  arena     10 participants, 45 pairs x 100 episodes (pm_play_rnn, and pm_play for the pairs without
            a QNetRNN);
  qnet      4 random QNets and the ball follower, 10 pairs x 1000 episodes (pm_play only).

Each plan runs in a child process of its own under a time limit: a warm-up of each of the three
modes, then three timed repeats of each, interleaved (none, per pair, all, none, ...) so that a
drift of the box falls on all three alike. record=None is the plain kernels' launch (the REC = false
instantiations, the same code as before recording existed); the other two launch the recording
instantiations and copy the stored ticks to the host and into MatchRecords, which is part of the
time. The parent starts nothing more after a child fails.

    python tools/play_record_bench.py [--json profiles/play_record_bench.json] [--limit 300]
"""
import argparse
import itertools
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd"), os.path.join(ROOT, "tools")]

REPEATS = 3
MODES = ("none", "per_pair", "all")


def build(plan_name, tmp):
    import torch
    import play_rnn_bench as prb
    if plan_name != "qnet":
        return prb.build(plan_name, tmp)
    from models.qnet import QNet
    env, _ = prb.env_of("config.yaml")
    models = {}
    for k in range(4):
        torch.manual_seed(400 + k)
        models[f"QNet_init{k}"] = (QNet(7, 3).eval().cuda(), "QNet")
    models["Follower"] = ("HardcodedAgent", "HardcodedBallFollower")
    return env, models, [(a, b, 1000) for a, b in itertools.combinations(list(models), 2)]


def child(plan_name):
    import torch
    from pongmi.tournament import play_matches
    with tempfile.TemporaryDirectory() as tmp:
        env, models, plan = build(plan_name, tmp)
    seed = 1234
    n = sum(e for _, _, e in plan)
    firsts = list(itertools.accumulate([0] + [e for _, _, e in plan[:-1]]))
    record = {"none": None, "per_pair": firsts, "all": list(range(n))}

    def run(mode):
        out = play_matches(env, models, plan, "cuda", random.Random(seed), record=record[mode])
        torch.cuda.synchronize()
        return out
    ref = run("none")
    ticks = {}
    for mode in MODES[1:]:  # warm-up; the recorded runs return the same results
        res, recs = run(mode)
        assert res == ref and len(recs) == len(record[mode])
        ticks[mode] = sum(r.frames for r in recs.values())
        assert not any(r.truncated for r in recs.values())
    secs = {m: [] for m in MODES}
    for _ in range(REPEATS):
        for mode in MODES:
            t0 = time.perf_counter()
            run(mode)
            secs[mode].append(round(time.perf_counter() - t0, 5))
    row = dict(plan=plan_name, episodes=n, pairs=len(plan), env_steps=ticks["all"],
               recorded_ticks=dict(per_pair=ticks["per_pair"], all=ticks["all"]))
    for m in MODES:
        row[m] = dict(seconds=secs[m], best=min(secs[m]), spread=round(max(secs[m]) - min(secs[m]), 5))
    for m in MODES[1:]:
        row[f"{m}_over_none_best"] = round(row[m]["best"] / row["none"]["best"], 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "play_record_bench.json"))
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per plan's child process")
    ap.add_argument("--one", metavar="PLAN", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return child(args.one)
    rows = []
    for plan_name in ("evaluate", "arena", "qnet"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", plan_name], capture_output=True,
                               text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{plan_name}: no result within {args.limit} s; stopping", flush=True)
            return 1
        if r.returncode != 0:
            print(f"{plan_name}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as fjs:
        json.dump(rows, fjs, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
