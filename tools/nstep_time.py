"""Time the n-step entry points against the one-step ones (profiles/nstep_ab.txt).

    python tools/nstep_time.py [--pkg DIR] [--label NAME] [--runs 5] [--calls 10] [--warmup 3]

Stream events around `calls` back-to-back calls after `warmup` calls, `runs` times per case, microseconds per
call. --pkg DIR puts another build of the package (a directory holding pongmi/ with its libpongmi.so) in front of
this tree's, so the parent commit is measured by the same script in a process of its own: there only the cases
that exist in it run (the one-step entries).

Cases: one collect step of 8 vector steps, a population of 256 members x 256 arenas (PopulationRollout.collect) and
the solo collector at 65 536 arenas (SelfPlayRollout.run(replay=)), with the window N = 1 through the n-step
entry, N = 3 and N = 8; one update() at batch 256 with and without a horizon buffer, a solo DQNLearner and a
256-member DQNPopulation."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "pingpong-selfplay-ai_amd"))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    sys.path[:0] = [a.pkg, ROOT, os.path.join(ROOT, "pingpong-selfplay-ai_amd")]
    import torch
    from models.qnet import QNet
    from pongmi import _lib
    from pongmi.dqn import DQNLearner, DQNPopulation
    from pongmi.env import PongEnv2PBatch
    from pongmi.qnet import fold, pack_state_dict
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import PopulationRollout, SelfPlayRollout
    has_n = hasattr(SelfPlayRollout, "_push")
    props = torch.cuda.get_device_properties(0)
    print(f"## process: {a.label}\n# {props.name} ({props.gcnArchName}, {props.multi_processor_count} CUs), "
          f"torch {torch.__version__}, n-step entries: {has_n}; {a.runs} runs x {a.calls} calls after {a.warmup}")

    def timed(name, call):
        out = []
        for _ in range(a.runs):
            for _ in range(a.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                call()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        print(f"{name:44s} us/call  " + " ".join(f"{v:8.1f}" for v in out) + f"   range {min(out):.1f}..{max(out):.1f}")

    torch.manual_seed(1)
    sdA, sdB = QNet(7, 3).state_dict(), QNet(7, 3).state_dict()
    wA = fold(pack_state_dict(sdA), _lib.PM_FOLD_TRAIN).reshape(-1)
    steps = 8

    # ---- the population's collect step, 256 x 256
    n, m = 256, 256
    for N in ((None, 1, 3, 8) if has_n else (None,)):
        env = PongEnv2PBatch(n * m, seed=5, autoreset=True)
        env.reset()
        params = pack_state_dict(sdB).reshape(1, -1).repeat(n, 1).contiguous()
        replays = [DeviceReplay(steps * m * 4, "cuda") for _ in range(n)]
        kw = {} if N is None else dict(nstep=N, gamma=0.99)
        pop = PopulationRollout(env, wA, params, n=n, replays=replays, steps_max=steps, **kw)
        if N == 1:  # through the new entry: all ones dispatches the one-step kernel
            pop._nstep_set = False
        timed(f"collect 256 x 256, {'one-step entry' if N is None else f'N = {N}'}", lambda: pop.collect(steps, sync=False))
        del pop, replays, env

    # ---- the solo collector, 65 536 arenas
    n = 65536
    for N in ((None, 1, 3, 8) if has_n else (None,)):
        env = PongEnv2PBatch(n, seed=5, autoreset=True)
        env.reset()
        R = DeviceReplay(n * steps * 2, "cuda")
        roll = SelfPlayRollout(env, wA, pack_state_dict(sdB).reshape(-1))
        roll.reserve(steps)
        if N is None:
            call = lambda: roll.run(steps, sync=False, replay=R)  # noqa: E731
        else:
            def call():
                roll.stats.zero_()
                roll._push(steps, R, N, 0.99)
                env.counter += steps
        timed(f"collect solo 65536, {'one-step entry' if N is None else f'N = {N}'}", call)
        del roll, R, env

    # ---- one update() at batch 256
    B = 256
    g = torch.Generator().manual_seed(3)
    batch = (torch.rand((B, 7), generator=g), torch.randint(0, 3, (B,), generator=g), torch.zeros(B),
             torch.rand((B, 7), generator=g), torch.zeros(B, dtype=torch.uint8))
    for nstep in ((1, 3) if has_n else (1,)):
        kw = {} if not has_n else dict(nstep=nstep)
        L = DQNLearner(sdB, batch=B, train_features=True, **kw)
        L.load_batch(*batch)
        timed(f"update solo, {'horizon buffer' if nstep > 1 else 'no horizon'}", lambda: L.update())
        P = DQNPopulation(sdB, n=256, batch=B, train_features=True, **kw)
        for p in range(256):
            P.load_batch(p, *batch)
        timed(f"update 256 members, {'horizon buffer' if nstep > 1 else 'no horizon'}", lambda: P.update())
        del L, P


if __name__ == "__main__":
    main()
