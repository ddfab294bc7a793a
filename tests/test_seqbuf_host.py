"""The host model of the QNetRNN sequence buffer (oracle/seqbuf.py) pinned to the reference's own
SequenceReplayBuffer (tests/golden/seqbuf.npz, recorded by tests/golden/make_golden_seqbuf.py), and
the uniformity of its restated sampler draw. CPU-only; tests/test_gpu_rnn_seqbuf.py then holds the
device to this model step by step."""
import math

import numpy as np
import pytest

from oracle.seqbuf import SeqBufferModel


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_model_is_the_reference_buffer(golden, k):
    """Ring-safety layer off: at every recorded point the model holds exactly the reference deque's
    episodes in its order, and for the recorded (episode index, start) of every reference sample()
    the model's window cut returns the reference's five arrays bit for bit."""
    g = golden("seqbuf")
    assert k < int(g["n_streams"])
    n, T, cap, steps = (int(v) for v in g[f"s{k}_meta"])
    rows, pts, held, spt = g[f"s{k}_rows"], g[f"s{k}_pts"], g[f"s{k}_held"], g[f"s{k}_spt"]
    m = SeqBufferModel(n, T, cap, depth=None)
    p = checked = 0
    for s in range(steps):
        m.push_step(s, rows[s])
        if p < len(pts) and pts[p] == s:
            want = held[held[:, 0] == p][:, 1:]
            assert np.array_equal(m.held(), want), f"stream {k} step {s}"
            assert m.seq_size == len(want) <= cap and m.status == 0
            for q in np.nonzero(spt == p)[0]:
                obs, act, rew, nxt, done = m.sample_at(g[f"s{k}_pick"][q])
                assert np.array_equal(_bits(obs), _bits(g[f"s{k}_obs"][q]))
                assert np.array_equal(_bits(nxt), _bits(g[f"s{k}_next"][q]))
                assert np.array_equal(_bits(rew), _bits(g[f"s{k}_rew"][q]))
                assert np.array_equal(act.astype(np.int64), g[f"s{k}_act"][q])
                assert np.array_equal(done.astype(bool), g[f"s{k}_done"][q])
                checked += 1
            p += 1
    assert p == len(pts) and checked == len(spt) > 5
    assert m.seq_count > 3 * cap  # the capacity wrapped several times


def test_fixture_covers_lengths_and_wraps(golden):
    """Episodes shorter than (never held), equal to and longer than trace_length, trace_length 1 and
    8, more than one arena finishing on one step, every window position of some episode sampled."""
    g = golden("seqbuf")
    Ts = set()
    for k in range(int(g["n_streams"])):
        n, T, cap, steps = (int(v) for v in g[f"s{k}_meta"])
        Ts.add(T)
        held, rows = g[f"s{k}_held"], g[f"s{k}_rows"]
        assert held[:, 3].min() >= T and (held[:, 3] == T).any() and (held[:, 3] > T).any()
        done = (rows[:, :, 15].copy().view(np.int32) >> 8) & 1
        ends = np.nonzero(done)
        # lengths pushed, from the stream itself: some are too short to store when T > 1
        lens = []
        for i in range(n):
            e = ends[0][ends[1] == i]
            lens += list(np.diff(np.concatenate([[-1], e])))
        assert (np.array(lens) < T).any() == (T > 1)
        if n > 1:
            assert done.sum(1).max() >= 2
        pick = g[f"s{k}_pick"]
        assert pick[..., 1].min() == 0 and pick[..., 0].min() == 0 and pick[..., 0].max() == cap - 1
    assert Ts == {1, 8}


def _chi2_sf_even(x, df):
    """P(chi-square_df > x) for even df: exp(-x/2) * sum_{k < df/2} (x/2)^k / k! (closed form)."""
    assert df % 2 == 0
    h, term, tot = x / 2.0, 1.0, 0.0
    for k in range(df // 2):
        tot += term
        term *= h / (k + 1)
    return math.exp(-h) * tot


def test_restated_draw_is_uniform():
    """The sampler's draw (SeqBufferModel.draws: Philox under TAG_SEQ, j = below(r.x, size),
    start = below(r.y, L - T + 1)) is uniform over (episode, window), as np.random.choice(len, B,
    replace=True) and np.random.randint(0, L - T + 1) are: 3 held episodes of T + 6 steps (7 windows
    each, 21 cells), 64 vector steps x 64 sequences = 4096 draws for each of u = 0 and u = 3, fixed
    seed. Pearson's chi-square against the uniform law has 20 degrees of freedom; the bound is that
    distribution's upper quantile for a false-alarm probability of 1e-6, 65.421 (the closed-form
    survival function for even degrees of freedom, bisected below; not tuned to the observed value)."""
    T, L, size, B, seed = 8, 14, 3, 64, 0x5EED1234ABCD
    m = SeqBufferModel(size, T, size, depth=None)
    for s in range(L):
        rows = np.zeros((size, 16), np.float32)
        rows[:, 15] = np.full(size, 256 if s == L - 1 else 0, np.int32).view(np.float32)
        m.push_step(s, rows)
    assert m.seq_size == size
    lo, hi = 0.0, 500.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf_even(mid, 20) > 1e-6 else (lo, mid)
    bound = hi
    assert abs(bound - 65.421) < 1e-3
    cells = size * (L - T + 1)
    for u in (0, 3):
        d = np.concatenate([m.draws(seed, now, u, B) for now in range(1, 65)])
        assert d[:, 0].min() == 0 and d[:, 0].max() == size - 1 and d[:, 1].min() == 0 and d[:, 1].max() == L - T
        cnt = np.bincount(d[:, 0] * (L - T + 1) + d[:, 1], minlength=cells)
        exp = len(d) / cells
        chi2 = float(((cnt - exp) ** 2 / exp).sum())
        print(f"u={u}: chi-square {chi2:.2f} over {cells} cells, bound {bound:.3f}")
        assert chi2 <= bound
    # the update index changes the draw
    assert not np.array_equal(m.draws(seed, 5, 0, B), m.draws(seed, 5, 1, B))
