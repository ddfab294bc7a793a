"""Record matches between two players tick by tick, for watching model X play model Y.

Loads the two players as the tournament does (pongmi.tournament.load_model_universal: QNet or
QNetRNN checkpoints, or the HardcodedBallFollower), plays `--episodes` greedy episodes in the match
megakernel with every episode recorded (pongmi.tournament.play_matches(record=...)), and writes one
MatchRecord per episode:

    <out>/match_<A>_vs_<B>_ep<k>.npz           states, actions, q values, scores, bounces per tick
    <out>/match_<A>_vs_<B>_ep<k>_frames.npy    with --frames: uint8 [F + 1, size, size, 3] RGB frames

    python tools/record_match.py --a ckpt/gen5.pth --a-type QNet --b follower --env config.yaml \\
        --episodes 3 --out records [--frames] [--ticks 4096] [--seed 0] [--render-size 400]

A record is read back with pongmi.record.MatchRecord.load(path) and walked with
pongmi.viewer.replay(record) (one RecordView per frame: a PongEnv2P viewer's attributes, frame()).
"""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd")]

FOLLOWER = "HardcodedBallFollower"


def player(path, typ, fallback):
    """(name, model_info) of one side; `follower` (or --x-type HardcodedBallFollower) needs no file."""
    if path.lower() == "follower" or typ == FOLLOWER:
        return fallback, {"name": fallback, "path": "N/A", "type": FOLLOWER}
    name = os.path.splitext(os.path.basename(path))[0]
    return name, {"name": name, "path": path, "type": typ}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", required=True, help="player A (top): checkpoint path, or 'follower'")
    ap.add_argument("--b", required=True, help="player B (bottom): checkpoint path, or 'follower'")
    ap.add_argument("--a-type", default="QNet", choices=["QNet", "QNetRNN", FOLLOWER])
    ap.add_argument("--b-type", default="QNet", choices=["QNet", "QNetRNN", FOLLOWER])
    ap.add_argument("--env", default=os.path.join(ROOT, "pingpong-selfplay-ai_amd", "config.yaml"),
                    help="yaml with an `env` section (and, for a QNetRNN, its architecture under `training`)")
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--ticks", type=int, default=4096, help="ticks kept per episode")
    ap.add_argument("--seed", type=int, default=0, help="seed of the serves' random stream")
    ap.add_argument("--frames", action="store_true", help="also save the RGB frames as .npy")
    ap.add_argument("--render-size", type=int, default=None)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)

    import numpy as np
    import yaml
    from pongmi.tournament import load_model_universal, play_matches
    from pongmi.viewer import replay
    with open(args.env) as f:
        cfg = yaml.safe_load(f)
    env = cfg["env"]
    nameA, infoA = player(args.a, args.a_type, "FollowerA")
    nameB, infoB = player(args.b, args.b_type, "FollowerB")
    if nameA == nameB:
        nameA, nameB = nameA + "_A", nameB + "_B"
        infoA["name"], infoB["name"] = nameA, nameB
    models = {nm: (load_model_universal(info, cfg.get("training"), args.device), info["type"])
              for nm, info in ((nameA, infoA), (nameB, infoB))}
    E = int(args.episodes)
    results, records = play_matches(env, models, [(nameA, nameB, E)], args.device, random.Random(args.seed),
                                    record=list(range(E)), record_ticks=args.ticks)
    os.makedirs(args.out, exist_ok=True)
    size = args.render_size or int(env.get("render_size", 400))
    for k in range(E):
        rec = records[k]
        stem = os.path.join(args.out, f"match_{nameA}_vs_{nameB}_ep{k + 1}")
        rec.save(stem + ".npz")
        if args.frames:
            np.save(stem + "_frames.npy", np.stack([v.frame() for v in replay(rec, render_size=size)]))
        _, _, sA, sB = results[k]
        cut = f" (first {rec.frames} kept)" if rec.truncated else ""
        print(f"episode {k + 1}: {nameA} {sA} - {sB} {nameB}, {rec.length} ticks{cut} -> {stem}.npz")
    return 0


if __name__ == "__main__":
    sys.exit(main())
