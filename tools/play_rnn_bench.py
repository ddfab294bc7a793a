"""QNetRNN match megakernel (pm_play_rnn) vs the stepped loop: wall time of play_matches with
rnn="fused" and rnn="stepped" on the same plans and serves.

  evaluate  one QNetRNN pair (the two trained checkpoints of tests/golden), config_rnn.yaml's
            eval_episodes: the shape of RNNGenerations.evaluate;
  arena     10 participants (6 QNetRNN: 2 trained, 2 perturbed copies, 2 random-init; 3 QNet; the
            ball follower), 45 pairs x 100 episodes: the shape of the reference's results_arena.

Each (plan, path) runs in a child process of its own under a time limit: a warm-up, then three
timed repeats. The parent starts nothing more after a child fails. env_steps / max_len are those of
the episodes with a QNetRNN player (the ones the two paths play differently).

    python tools/play_rnn_bench.py [--json profiles/play_rnn_bench.json] [--limit 300]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd")]

CKPT_KEY = {"RNN_Gen1": "modelB_state", "RNN_Soul3": "modelB_state", "Legacy4_12": "modelB", "Noisy5_5": "modelB"}
REPEATS = 3


def env_of(name):
    import yaml
    with open(os.path.join(ROOT, "pingpong-selfplay-ai_amd", name)) as f:
        cfg = yaml.safe_load(f)
    return cfg["env"], cfg


def golden_models(tmp):
    """name -> (module or "HardcodedAgent", type) of the five participants in tests/golden."""
    import numpy as np
    import torch
    from pongmi.tournament import load_model_universal
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "tournament.npz"), allow_pickle=False))
    gr = dict(np.load(os.path.join(ROOT, "tests", "golden", "rnn.npz"), allow_pickle=False))
    models = {}
    for i, (name, typ) in enumerate(zip(g["names"].tolist(), g["types"].tolist())):
        info = {"name": name, "path": "N/A", "type": typ}
        if typ != "HardcodedBallFollower":
            if name == "RNN_Soul3":
                sd = {k[7:]: torch.from_numpy(v) for k, v in gr.items() if k.startswith("params.")}
            else:
                sd = {k[len(f"sd{i}."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"sd{i}.")}
            info["path"] = os.path.join(tmp, f"{name}.pth")
            torch.save({CKPT_KEY[name]: sd, "epsilon": 0.05}, info["path"])
        models[name] = (load_model_universal(info, {}, "cuda"), typ)
    return models


def build(plan_name, tmp):
    """(env params, models, plan) of a named plan."""
    import copy
    import torch
    from models.qnet import QNet
    from models.qnet_rnn import QNetRNN
    models = golden_models(tmp)
    if plan_name == "evaluate":
        env, cfg = env_of("config_rnn.yaml")
        E = int(cfg["training"]["eval_episodes"])
        return env, {k: models[k] for k in ("RNN_Gen1", "RNN_Soul3")}, [("RNN_Gen1", "RNN_Soul3", E)]
    env, _ = env_of("config.yaml")
    for k, src in enumerate(("RNN_Gen1", "RNN_Soul3")):  # perturbed copies: distinct nets that still rally
        m = copy.deepcopy(models[src][0])
        gen = torch.Generator(device="cpu").manual_seed(100 + k)
        with torch.no_grad():
            for prm in m.parameters():
                prm.add_((0.02 * prm.std().item() if prm.numel() > 1 else 0.0) *
                         torch.randn(prm.shape, generator=gen).to(prm.device))
        models[f"RNN_var{k}"] = (m.eval(), "QNetRNN")
    for k in range(2):
        torch.manual_seed(200 + k)
        m = QNetRNN(input_dim=7, output_dim=3, feature_dim=128, lstm_hidden_dim=128, lstm_layers=1, head_hidden_dim=128)
        models[f"RNN_init{k}"] = (m.eval().cuda(), "QNetRNN")
    torch.manual_seed(300)
    models["QNet_init"] = (QNet(7, 3).eval().cuda(), "QNet")
    assert len(models) == 10
    return env, models, [(a, b, 100) for a, b in itertools.combinations(list(models), 2)]


def rnn_episode_lengths(env, models, plan, seed):
    """Lengths of the plan's episodes with a QNetRNN player (same serves as play_matches draws)."""
    import numpy as np
    import torch
    from pongmi import _lib, qnet as _qnet, rnn as _rnn
    from pongmi.env import draw_serve, env_config
    from pongmi.play import FOLLOWER, play_rnn, rnn_id
    env_kw = {k: v for k, v in dict(env).items() if k not in ("render_size", "enable_render")}
    cfg, rng = env_config(**env_kw), random.Random(seed)
    eps = [(a, b) for a, b, e in plan for _ in range(int(e))]
    serves = np.array([draw_serve(rng, cfg) for _ in eps], np.float64).reshape(len(eps), 3)
    ids, wq, wr = {}, [], []
    for nm, (module, typ) in models.items():
        if typ == "QNetRNN":
            ids[nm] = rnn_id(len(wr))
            wr.append(_rnn.fold(module.packed().cuda(), _lib.PM_FOLD_EVAL)[0])
        elif typ == "QNet":
            ids[nm] = len(wq)
            wq.append(_qnet.fold(module.packed().cuda(), _lib.PM_FOLD_EVAL)[0])
        else:
            ids[nm] = FOLLOWER
    keep = [k for k, (a, b) in enumerate(eps) if ids[a] <= rnn_id(0) or ids[b] <= rnn_id(0)]
    _, _, length, _ = play_rnn(env_kw, torch.stack(wq) if wq else None, torch.stack(wr),
                               [ids[eps[k][0]] for k in keep], [ids[eps[k][1]] for k in keep], serves[keep])
    return length


def child(plan_name, mode):
    import torch
    from pongmi.tournament import play_matches
    with tempfile.TemporaryDirectory() as tmp:
        env, models, plan = build(plan_name, tmp)
    seed = 1234
    ref = play_matches(env, models, plan, "cuda", random.Random(seed), rnn=mode)  # warm-up
    torch.cuda.synchronize()
    secs = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = play_matches(env, models, plan, "cuda", random.Random(seed), rnn=mode)
        torch.cuda.synchronize()
        secs.append(round(time.perf_counter() - t0, 5))
        assert out == ref
    length = rnn_episode_lengths(env, models, plan, seed)
    print(json.dumps(dict(plan=plan_name, rnn=mode, episodes=len(ref), rnn_episodes=int(length.size),
                          seconds=secs, env_steps=int(length.sum()), max_len=int(length.max()),
                          scores=[sum(r[2] for r in ref), sum(r[3] for r in ref)])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "play_rnn_bench.json"))
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per (plan, path) child process")
    ap.add_argument("--one", nargs=2, metavar=("PLAN", "PATH"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return child(*args.one)
    rows = []
    for plan_name in ("evaluate", "arena"):
        row = {"plan": plan_name}
        for mode in ("fused", "stepped"):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", plan_name, mode],
                                   capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print(f"{plan_name}/{mode}: no result within {args.limit} s; stopping", flush=True)
                return 1
            if r.returncode != 0:
                print(f"{plan_name}/{mode}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
                return 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
            for k in ("episodes", "rnn_episodes", "env_steps", "max_len", "scores"):
                assert row.setdefault(k, res[k]) == res[k], (k, row[k], res[k])  # both paths: the same episodes
            row[mode] = dict(seconds=res["seconds"], best=min(res["seconds"]),
                             spread=round(max(res["seconds"]) - min(res["seconds"]), 5))
        f, s = row["fused"], row["stepped"]
        row["speedup_best"] = round(s["best"] / f["best"], 2)
        # the fused path counts as faster only beyond the spread of the repeats
        row["fused_faster"] = max(f["seconds"]) + max(f["spread"], s["spread"]) < min(s["seconds"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as fjs:
        json.dump(rows, fjs, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
