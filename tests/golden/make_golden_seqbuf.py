#!/usr/bin/env python3
"""Golden fixture for the sequence buffer model (oracle/seqbuf.py), recorded from the REFERENCE's own
SequenceReplayBuffer (scripts/train_rnn_iterative.py:100-176).

Run only in the build container (the reference does not exist on the GPU box):

    python -B tests/golden/make_golden_seqbuf.py

Importing the reference script starts a training run, so the class is cut out of the script's source
at generation time (ast) and executed on its own with the names it uses (deque, np, torch, device);
no reference text is kept here or in the fixture — only the arrays it produced.

A scripted, seeded stream of pushes is fed to it. Observation words 0 and 1 hold (arena, step), so a
sampled window names its episode and its start; the other words are seeded noise, and next_obs is
noise of its own (never the obs shift), so act / rew / next / done taken from another step cannot
pass. The reference class steps ONE env; for n arenas each arena has its own instance (its own
current_episode_trajectory) and all of them append to one shared deque, visited in ascending arena
order per step — the push order of the batched loop. The n = 1 streams are the reference class with
nothing added.

Streams (n, trace_length, capacity, steps): episodes shorter than, equal to and longer than
trace_length, capacities that wrap several times, trace_length 1 and 8.

Writes seqbuf.npz; for stream k:
  s{k}_meta         [n, T, cap, steps]
  s{k}_rows         [steps][n][16] float32: the push stream as ring rows (obs 0:7, rew 7, next 8:15,
                    word 15 = the integer bits act | done << 8)
  s{k}_pts          the steps after whose pushes the deque was recorded
  s{k}_held         [.][4]: (point index, arena, first step, length) of every held episode, oldest
                    first within a point
  s{k}_spt          [S] point index each sample() was taken at
  s{k}_pick         [S][B][2] recovered (episode index, start)
  s{k}_obs, _act, _rew, _next, _done   the S sample() outputs ([S][B][T][7] / [S][B][T])
The file is written with fixed zip timestamps: a rerun reproduces it byte for byte.
"""
import ast
import io
import os
import sys
import zipfile
from collections import deque

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("PONG_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
BATCH = 16
STREAMS = [  # n, T, cap, steps, episode lengths to cycle through (seeded shuffle per arena)
    (1, 8, 4, 400, (3, 8, 9, 20, 7, 8, 31, 12, 1)),
    (1, 1, 3, 120, (1, 2, 5, 1, 9, 3)),
    (6, 8, 5, 260, (3, 8, 9, 20, 7, 8, 31, 12, 1, 16)),
    (5, 1, 7, 60, (1, 2, 4, 1, 6)),
]


def reference_class():
    src = open(os.path.join(REF, "scripts", "train_rnn_iterative.py"), encoding="utf-8").read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "SequenceReplayBuffer")
    ns = dict(deque=deque, np=np, torch=torch, device=torch.device("cpu"))
    exec(compile(ast.Module(body=[node], type_ignores=[]), "SequenceReplayBuffer", "exec"), ns)
    return ns["SequenceReplayBuffer"]


def stream(rng, n, steps, lengths):
    """rows [steps][n][16]: every arena plays episodes whose lengths cycle through a shuffle of
    `lengths`, so that ends fall on different steps in different arenas (and sometimes the same)."""
    rows = rng.uniform(-1, 1, (steps, n, 16)).astype(np.float32)
    bits = np.zeros((steps, n), np.int32)
    for i in range(n):
        order = rng.permutation(len(lengths))
        t, k = 0, 0
        while t < steps:
            t += lengths[order[k % len(order)]]
            k += 1
            if t - 1 < steps:
                bits[t - 1, i] = 1 << 8
    bits |= rng.integers(0, 3, (steps, n)).astype(np.int32)
    rows[:, :, 0] = np.arange(n)[None, :]
    rows[:, :, 1] = np.arange(steps)[:, None]
    rows[:, :, 15] = bits.view(np.float32)
    return rows


def record(Ref, k, n, T, cap, steps, lengths, out):
    rng = np.random.default_rng(100 + k)
    rows = stream(rng, n, steps, lengths)
    bufs = [Ref(cap, T) for _ in range(n)]
    for b in bufs[1:]:
        b.buffer = bufs[0].buffer  # one memory, n running trajectories
    pts, held, spt, pick, outs = [], [], [], [], [[] for _ in range(5)]
    np.random.seed(7 + k)
    for s in range(steps):
        for i in range(n):
            r = rows[s, i]
            b = int(r[15:16].view(np.int32)[0])
            bufs[i].push_step(r[0:7].copy(), b & 0xFF, float(r[7]), r[8:15].copy(), bool(b >> 8), None, None)
        if s % 7 == 3 or s == steps - 1:
            p = len(pts)
            pts.append(s)
            memory = bufs[0].buffer
            for ep in memory:
                held.append((p, int(ep[0][0][0]), int(ep[0][0][1]), len(ep)))
            if len(memory):
                got = bufs[0].sample(BATCH)
                arrs = [x.numpy() for x in got[:5]]
                assert arrs[0].shape == (BATCH, T, 7)
                pk = []
                for o in arrs[0]:  # the window's first obs names (arena, step)
                    j = [q for q, ep in enumerate(memory) if ep[0][0][0] == o[0, 0] and ep[0][0][1] <= o[0, 1] <= ep[-1][0][1]]
                    assert len(j) == 1
                    pk.append((j[0], int(o[0, 1]) - int(memory[j[0]][0][0][1])))
                spt.append(p)
                pick.append(pk)
                for dst, a in zip(outs, arrs):
                    dst.append(a)
    out[f"s{k}_meta"] = np.array([n, T, cap, steps], np.int64)
    out[f"s{k}_rows"] = rows
    out[f"s{k}_pts"] = np.array(pts, np.int64)
    out[f"s{k}_held"] = np.array(held, np.int64).reshape(-1, 4)
    out[f"s{k}_spt"] = np.array(spt, np.int64)
    out[f"s{k}_pick"] = np.array(pick, np.int64)
    for name, v in zip(("obs", "act", "rew", "next", "done"), outs):
        out[f"s{k}_{name}"] = np.stack(v)
    h = out[f"s{k}_held"]
    lens = h[:, 3]
    stored = len({(a, f) for _, a, f, _ in h.tolist()})
    print(f"stream {k}: n={n} T={T} cap={cap}: {len(pts)} points, {stored} distinct episodes seen held (cap {cap}), "
          f"{len(spt)} samples; held lengths == T: {(lens == T).sum()}, > T: {(lens > T).sum()}")
    assert stored > 3 * cap  # wrapped several times


def write_npz(path, arrays):
    """An .npz with fixed member timestamps (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    Ref = reference_class()
    out = {"n_streams": np.array(len(STREAMS), np.int64)}
    for k, (n, T, cap, steps, lengths) in enumerate(STREAMS):
        record(Ref, k, n, T, cap, steps, lengths, out)
    path = os.path.join(OUT, "seqbuf.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
