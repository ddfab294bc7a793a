"""CPU-only checks of the QNetRNN match megakernel's boundary: pm_play_rnn rejects bad arguments
before any device work, the scratch size is what the kernel indexes, and the host planner groups
arenas by pair for player ids below the ball follower's (play_rnn's QNetRNN ids)."""
import numpy as np
import pytest


def test_pm_play_rnn_rejects_null_buffers_without_a_gpu():
    from pongmi import _lib
    L = _lib.load()
    args = [None, None, 0, None, 0, None, None, 1, None, None, 0, 0, None, None, None, None, None, None, None]
    assert L.pm_play_rnn(*args) == -1
    assert b"pm_play_rnn" in L.pm_last_error()
    args[7] = 0  # n_blocks = 0 is a no-op
    assert L.pm_play_rnn(*args) == 0
    args[7] = -1
    assert L.pm_play_rnn(*args) == -2


def test_scratch_bytes():
    from pongmi import _lib
    L = _lib.load()
    assert L.pm_play_rnn_scratch_bytes(3) == 3 * 2 * 128 * 256 * 4
    assert L.pm_play_rnn_scratch_bytes(0) == 0
    assert L.pm_play_rnn_scratch_bytes(4096) == 4096 * 2 * 128 * 256 * 4  # past 2^31 bytes


def test_rnn_ids_round_trip():
    from pongmi.play import FOLLOWER, RNN_BASE, rnn_id
    assert [rnn_id(k) for k in range(3)] == [-2, -3, -4] and RNN_BASE < FOLLOWER
    assert all(rnn_id(rnn_id(k)) == k for k in range(5))


def test_planner_groups_pairs_with_ids_below_the_follower():
    """Pairs in first-appearance order, arenas ascending within a pair, blk_nets the ids as given."""
    from pongmi.play import plan_blocks
    idA = np.array([-2, -3, 5, -2, -1, -3, -2, 5, -7])
    idB = np.array([-3, -2, -2, -3, -4, -2, -3, -2, -7])
    nets, rng, order = plan_blocks(idA, idB, per_block=2)
    assert nets.tolist() == [[-2, -3], [-2, -3], [-3, -2], [5, -2], [-1, -4], [-7, -7]]
    assert rng.tolist() == [[0, 2], [2, 1], [3, 2], [5, 2], [7, 1], [8, 1]]
    assert order.tolist() == [0, 3, 6, 1, 5, 2, 7, 4, 8]
    assert nets.dtype == np.int32 and rng.dtype == np.int32 and order.dtype == np.int32
    # (-2, -3) and (-3, -2) are different pairs; every slot's arena has its block's ids
    for (a, b), (lo, cnt) in zip(nets.tolist(), rng.tolist()):
        assert (idA[order[lo:lo + cnt]] == a).all() and (idB[order[lo:lo + cnt]] == b).all()


def test_planner_unchanged_for_qnet_and_follower_ids():
    """Ids >= -1 plan as before the generalisation (same key, same grouping)."""
    from pongmi.play import plan_blocks
    rng = np.random.default_rng(0)
    idA, idB = rng.integers(-1, 4, 700), rng.integers(-1, 4, 700)
    nets, ranges, order = plan_blocks(idA, idB)
    seen = list(dict.fromkeys(zip(idA.tolist(), idB.tolist())))
    got = list(dict.fromkeys(map(tuple, nets.tolist())))
    assert got == seen
    assert sorted(order.tolist()) == list(range(700)) and int(ranges[:, 1].sum()) == 700
    for (a, b), (lo, cnt) in zip(nets.tolist(), ranges.tolist()):
        sl = order[lo:lo + cnt]
        assert (idA[sl] == a).all() and (idB[sl] == b).all() and (np.diff(sl) > 0).all() and cnt <= 128
    with pytest.raises(ValueError):
        plan_blocks([0, 1], [0])
