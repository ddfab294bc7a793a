"""The QNetRNN sequence buffer and its sampler (k_rsp_append's episode table, its eviction by capacity
and by age, k_rsp_sample) against the host model oracle/seqbuf.py, every vector step, exactly.

The model is the reference's SequenceReplayBuffer held literally (a deque(maxlen=capacity) of copied
trajectories, pinned to the reference class by tests/test_seqbuf_host.py) plus the two documented
ring-safety rules; it is fed the ring rows each step writes (pinned to the oracle by
tests/test_gpu_rnn_selfplay.py) and keeps no ring or table index. After every rollout the device's
episode table, seq_count, seq_size, status and enable flag equal the model's, and the sampled batch
(obs, act, rew, next, done) equals the model's own cut of its own trajectories at the restated Philox
draw, bit for bit: a duplicated, skipped, misordered or wrongly evicted entry, a biased or shifted
draw, a field taken from another step, or a read of an overwritten ring slot all fail here. No
tolerance appears in this file.

Case c runs a capacity below one step's output of storable episodes (the reference's deque then
keeps the last `cap` of that step in arena order): k_rsp_append writes only a step's newest seq_cap
entries, one thread per table slot. Before that, entries e and e + seq_cap of one step were written
to the same slot by two threads with no order between them.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_rnn_selfplay import _learner

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _batch(L):
    t = L.learner
    return tuple(x.cpu().numpy() for x in (t.obs, t.act, t.rew, t.next, t.done))


def _assert_batch(got, want, what):
    for name, g, w in zip(("obs", "act", "rew", "next", "done"), got, want):
        assert g.shape == w.shape, f"{what}: {name} shape"
        same = np.array_equal(_bits(g), _bits(w)) if g.dtype == np.float32 else np.array_equal(g, w)
        assert same, f"{what}: sampled {name} differs from the model's window"


def _run(golden, n, cap, T, batch, steps, seed, depth=None, max_episode_steps=1000, extra_updates=0):
    """`steps` rollouts of a learner (random play: epsilon 1, sampling on as soon as one episode is
    held, no update) with the model fed each step's ring rows; every comparison of the module
    docstring after every step. Returns the model's coverage counts."""
    from oracle.seqbuf import SeqBufferModel
    L = _learner(golden, n=n, n_pool=2, batch=batch, trace_length=T, memory_size=cap, depth=depth, epsilon=1.0,
                 min_epsilon=1.0, min_episodes_for_training_start=0, seed=seed, max_episode_steps=max_episode_steps,
                 overlap=False)
    assert L.batch == batch and L.T == T and L.sp.min_episodes == 0
    m = SeqBufferModel(n, T, cap, L.depth)
    seed_env = L.sp.seed_env
    cov = dict(steps=steps, sampled_steps=0, draws=0, len_eq_T=0, last_window=0, first_episode=0, last_episode=0,
               cut_windows=0, alike_pairs=0, first_status={}, max_held=0)
    for k in range(steps):
        L.rollout()
        c = L.counters()
        rows = L.trans[k % L.depth].cpu().numpy()
        m.push_step(k, rows)
        now = k + 1
        assert c["step"] == now
        held = m.held()
        assert np.array_equal(L.episodes().numpy(), held), f"step {k}: episode table"
        assert c["seq_count"] == m.seq_count and c["seq_size"] == m.seq_size, f"step {k}: table counters"
        assert c["status"] == m.status and c["status"] & 1 == 0, f"step {k}: status {c['status']} vs {m.status}"
        for bit in (2, 4):
            if m.status & bit and bit not in cov["first_status"]:
                cov["first_status"][bit] = k
        en = int(m.seq_size > L.sp.min_episodes)
        assert c["train"] == en and int(L.enable.item()) == en, f"step {k}: enable"
        cov["max_held"] = max(cov["max_held"], m.seq_size)
        if not en:
            continue
        batches = []
        for u in range(1 + extra_updates):
            if u:
                L.sample(u)
            picks = m.draws(seed_env, now, u, batch)
            want = m.sample_at(picks)
            got = _batch(L)
            _assert_batch(got, want, f"step {k} u={u}")
            batches.append(got)
            lens = held[picks[:, 0], 2]
            cov["draws"] += batch
            cov["len_eq_T"] += int((lens == T).sum())
            cov["last_window"] += int(((lens > T) & (picks[:, 1] == lens - T)).sum())
            cov["first_episode"] += int((picks[:, 0] == 0).sum())
            cov["last_episode"] += int((picks[:, 0] == m.seq_size - 1).sum())
            obs, nxt = want[0], want[3]
            cov["cut_windows"] += int(np.any(_bits(obs[:, 1:]) != _bits(nxt[:, :-1]), axis=(1, 2)).sum())
        for a in range(len(batches)):
            for b in range(a):
                cov["alike_pairs"] += int(np.array_equal(batches[a][0], batches[b][0]))
        cov["sampled_steps"] += 1
    cov["stored"], cov["over_cap_steps"], cov["status"] = m.seq_count, m.over_cap_steps, m.status
    print(f"\nseqbuf n={n} cap={cap} T={T} B={batch} depth={L.depth}: {cov}")
    assert cov["sampled_steps"] > 0 and L.counters()["train_steps"] == 0
    return cov


def test_seqbuf_ragged_wrap(golden):
    """a: n = 300 (a partial last env block), a table of 400 before and after it wraps."""
    cov = _run(golden, n=300, cap=400, T=8, batch=64, steps=140, seed=11)
    assert cov["stored"] > 2 * 400 and cov["max_held"] == 400 and cov["status"] == 0
    assert cov["first_episode"] > 0 and cov["last_episode"] > 0 and cov["last_window"] > 0


def test_seqbuf_one_arena_tiny_capacity(golden):
    """b: one arena, capacity 3, T = 1: every episode is stored and has L windows."""
    cov = _run(golden, n=1, cap=3, T=1, batch=32, steps=400, seed=12)
    assert cov["stored"] > 3 and cov["max_held"] == 3
    assert cov["first_episode"] > 0 and cov["last_episode"] > 0 and cov["last_window"] > 0


def test_seqbuf_capacity_below_one_step(golden):
    """c: more storable episodes finish in one step than the table holds (n = 2048, capacity 16): the
    table is the last 16 of them in arena order, as deque(maxlen=16) leaves it."""
    cov = _run(golden, n=2048, cap=16, T=8, batch=96, steps=70, seed=13)
    assert cov["over_cap_steps"] >= 1 and cov["max_held"] == 16


def test_seqbuf_age_eviction_and_long_trajectories(golden):
    """d: depth 64 — trajectories longer than 32 steps are dropped (status value 4) and episodes leave
    32 steps after they finished (status value 2); each value appears on the step the model sets it
    (the per-step status equality), and both do appear."""
    cov = _run(golden, n=512, cap=100_000, T=8, batch=64, steps=150, seed=14, depth=64)
    assert cov["status"] == 6 and set(cov["first_status"]) == {2, 4} and cov["max_held"] < cov["stored"]


def test_seqbuf_windows_across_step_cuts(golden):
    """e: max_episode_steps = 24 — stored trajectories span episode cuts, where obs[t + 1] != next[t]
    (the re-serve); at least one sampled window contains one, so `next` is pinned on its own."""
    cov = _run(golden, n=257, cap=400, T=8, batch=64, steps=120, seed=15, max_episode_steps=24)
    assert cov["cut_windows"] >= 1


def test_seqbuf_long_traces_large_batch(golden):
    """f: T = 33, batch 256: B * T = 8448 items over the sampler's 512 threads; episodes of exactly T
    steps are drawn (a single window). depth 256 holds trajectories up to 128 steps."""
    cov = _run(golden, n=1024, cap=500, T=33, batch=256, steps=140, seed=16, depth=256)
    assert cov["stored"] > 500 and cov["max_held"] == 500 and cov["len_eq_T"] > 0 and cov["last_window"] > 0 and cov["first_episode"] > 0 and cov["last_episode"] > 0


def test_seqbuf_further_updates_of_a_step(golden):
    """g: pm_rnn_selfplay_sample for updates 1 and 2 of every step, each exact against the model's
    draw for that u; the three batches of a step differ pairwise."""
    cov = _run(golden, n=1024, cap=2000, T=8, batch=64, steps=80, seed=17, extra_updates=2)
    assert cov["stored"] > 2000 and cov["draws"] == 3 * 64 * cov["sampled_steps"] and cov["alike_pairs"] == 0


def test_seqbuf_sample_rejects_bad_arguments(golden):
    """pm_rnn_selfplay_sample refuses a learner whose T is not the buffer's and u outside [0, 2^15)
    (PM_E_ARG, nothing launched), and takes the ends of that range."""
    from pongmi import _lib
    from pongmi.drqn import DRQNLearner
    from test_gpu_rnn_selfplay import _golden_sd
    PM_OK, PM_E_ARG = 0, -1
    L = _learner(golden, n=64, n_pool=0, trace_length=8, memory_size=64, overlap=False)
    other = DRQNLearner(_golden_sd(golden("rnn")), batch=64, T=4, enable=L.enable, device=L.device)
    stream = _lib.stream_ptr()
    call = lambda d, u: L.lib.pm_rnn_selfplay_sample(ctypes.byref(L.sp), ctypes.byref(d.desc), u, stream)  # noqa: E731
    assert call(L.learner, 0) == PM_OK and call(L.learner, (1 << 15) - 1) == PM_OK
    assert call(other, 1) == PM_E_ARG
    for u in (-1, 1 << 15, 1 << 20):
        assert call(L.learner, u) == PM_E_ARG
        with pytest.raises(_lib.PongmiError):
            L.sample(u)
    torch.cuda.synchronize()
    assert L.counters()["train"] == 0 and not L.learner.obs.any()  # an empty buffer: nothing sampled
