"""k_actenv's two ends, per block: the env blocks' phase table (tools/env_blocks.py's) and, for the 32
sampler blocks, every stamp of every block with the CU / XCC it ran on, from the diagnostic library.

    make -C pingpong-selfplay-ai_amd/csrc diag && python tools/actenv_ends.py

A sampler block "shares" when an env block of the same launch ran on its CU (288 blocks on 256 CUs).
The launch ends with its latest block, so the table that matters is the last one: per launch, the
latest sampler block's phases against the launch's median block, and whether it shared its CU.

Diagnostic only (libpongmi_diag.so, or PONGMI_DIAG_LIB, never the product library).
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["PONGMI_LIB"] = os.environ.get("PONGMI_DIAG_LIB") or os.path.join(
    ROOT, "pingpong-selfplay-ai_amd", "pongmi", "libpongmi_diag.so")
sys.path.insert(0, os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.env_blocks import PHASES  # noqa: E402

# pm_diag_blk slots of a sampler block, in time order
SLOTS = [(0, "begin"), (4, "level2"), (5, "level1"), (6, "leaves"), (1, "sampled"), (2, "end")]
STEPS = ["begin", "-> level2", "-> level1", "-> leaves", "-> sampled", "-> end"]


def main():
    import bench
    from pongmi import _lib
    from pongmi.selfplay import SelfPlayLearner
    lib = _lib.load()
    for f in (lib.pm_diag_read_env, lib.pm_diag_read_env_place, lib.pm_diag_read_blk):
        f.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    n, launches = 65536, 20
    sdB, sdA = bench.synthetic_qnet(1), bench.synthetic_qnet(2)
    pool = [bench.synthetic_qnet(100 + k) for k in range(8)]
    L = SelfPlayLearner(bench.ENV_KW, n, sdB, sdA, pool, batch=256, memory_size=1_000_000, epsilon=0.08, seed=7)
    assert L.overlap, "the fused step's launch"
    for _ in range(40):
        L.step()
    torch.cuda.synchronize()
    nb, nsb = (n + 255) // 256, (256 + 7) // 8
    ebuf = (ctypes.c_uint64 * (8 * 1024))()
    pbuf = (ctypes.c_uint64 * 1024)()
    bbuf = (ctypes.c_uint64 * (8 * 4096))()
    env, eplace, samp, splace = [], [], [], []
    for _ in range(launches):
        L.actenv()
        torch.cuda.synchronize()
        lib.pm_diag_read_env(ebuf)
        lib.pm_diag_read_env_place(pbuf)
        lib.pm_diag_read_blk(bbuf)
        e = np.array(ebuf[:], dtype=np.int64).reshape(8, 1024)[:7, :nb]
        b = np.array(bbuf[:], dtype=np.int64).reshape(8, 4096)[:, :nsb]
        env.append(e)
        eplace.append(np.array(pbuf[:nb], dtype=np.int64))
        samp.append(np.stack([(b[s] - e[0].min()) * 0.01 for s, _ in SLOTS]))  # [slot][block], us
        splace.append(b[3].copy())
        L.learn(act_next=True)
        L.apply()

    spans, deltas = [], [[] for _ in PHASES]
    for a in env:
        t0 = a[0].min()
        spans.append((a[6].max() - t0) * 0.01)
        deltas[0].extend((a[0] - t0) * 0.01)
        for k in range(1, 7):
            deltas[k].extend((a[k] - a[k - 1]) * 0.01)
    print(f"env blocks: {nb}; span first begin -> last end: median {np.median(spans):.2f} us")
    for k, name in enumerate(PHASES):
        v = np.array(deltas[k])
        label = "begin offset" if k == 0 else name
        print(f"  {label:54s} p50 {np.percentile(v, 50):5.2f}  p90 {np.percentile(v, 90):5.2f}  max {v.max():5.2f} us")

    s = np.stack(samp)  # [launch][slot][block]
    shared = np.stack([np.isin(sp, ep) for sp, ep in zip(splace, eplace)])  # [launch][block]
    # the env blocks that share a CU with another env block or a sampler block
    esh = [len(ep) - len(np.unique(ep)) for ep in eplace]
    print(f"sampler blocks: {nsb}; sharing a CU with an env block: {shared.sum(1).min()}-{shared.sum(1).max()} per launch; "
          f"env blocks on a CU that holds another env block: {min(esh)}-{max(esh)} per launch")
    q = lambda v: " ".join(f"{x:5.2f}" for x in np.percentile(v, [0, 50, 90, 100]))  # noqa: E731
    print("times from the first env block's begin (min p50 p90 max), all blocks / sharing / alone:")
    for k, (_, name) in enumerate(SLOTS):
        v = s[:, k]
        a = q(v[shared]) if shared.any() else "-"
        c = q(v[~shared]) if (~shared).any() else "-"
        print(f"  {name:8s} {q(v)} | {a} | {c}")
    d = np.concatenate([s[:, :1], np.diff(s, axis=1)], axis=1)  # per-phase durations
    print("phase durations (p50 max), sharing / alone:")
    for k, name in enumerate(STEPS):
        v = d[:, k]
        a = f"{np.median(v[shared]):5.2f} {v[shared].max():5.2f}" if shared.any() else "-"
        c = f"{np.median(v[~shared]):5.2f} {v[~shared].max():5.2f}" if (~shared).any() else "-"
        print(f"  {name:11s} {a} | {c}")

    print("per launch: the latest sampler block against the launch's median block (us; phase durations)")
    print("  launch blk xcc  cu shares |" + "".join(f"{x:>11s}" for x in STEPS) + " |   end (median end)")
    for r in range(launches):
        b = int(np.argmax(s[r, -1]))
        med = np.median(d[r], axis=1)
        cells = "".join(f" {d[r, k, b]:4.2f}/{med[k]:4.2f} " for k in range(len(STEPS)))
        print(f"  {r:6d} {b:3d} {splace[r][b] >> 16:3d} {splace[r][b] & 0xffff:3d} {'yes' if shared[r, b] else ' no':>6s} |"
              f"{cells}| {s[r, -1, b]:5.2f} ({np.median(s[r, -1]):5.2f})")

    r = launches - 1
    print(f"launch {r}, every sampler block (us from the first env block's begin):")
    print("  blk xcc  cu shares " + "".join(f"{name:>8s}" for _, name in SLOTS))
    for b in range(nsb):
        print(f"  {b:3d} {splace[r][b] >> 16:3d} {splace[r][b] & 0xffff:3d} {'yes' if shared[r, b] else ' no':>6s} " +
              "".join(f"{s[r, k, b]:8.2f}" for k in range(len(SLOTS))))


if __name__ == "__main__":
    main()
