"""Level 2 of the PER descent (pm_per.h per_round_prefix + per_lds_search: the chunk sums' prefix on
the DPP wave scan and the five-round base-4 search of it) through pm_per_sample, against
oracle.per_sample_tree, at chunk counts on both sides of every width the level has: one thread's 4
chunks, a wave's 256, the search's strides 4, 64 and 256, and one round's 1024 (1025 chunks are two
rounds, and the tie in front of chunk 1024 is the first round's 'no value above x').
Indices are exact and the oracle alone says what they are."""
import numpy as np
import pytest

from test_gpu_per import U_LAST, check_sample

pytestmark = pytest.mark.gpu

CH = 1024  # entries per chunk
CHUNKS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MASS = (3, 200, 517, 1023)  # the four entries of a chunk that hold priority 1: every chunk sums to 4


def _prios(nb, live):
    """nb chunks; chunk c holds four ones if live[c], else nothing (alpha = 1: a leaf is its priority)."""
    pr = np.zeros(nb * CH, np.float32)
    for c in np.nonzero(live)[0]:
        pr[c * CH + np.array(MASS)] = 1.0
    return pr


def _chunk_prefix(orc, pr, size):
    """The level-2 prefix values the oracle's own tree gives (exact here: small integers)."""
    chunk = orc.per_tree(pr, size, 1.0)[0]
    return chunk, np.cumsum(chunk)


@pytest.mark.parametrize("nb", CHUNKS)
def test_every_chunk_boundary_is_a_tie_once(orc, nb):
    """Every chunk sum is 4, u = j / nb for every j: u * total is the prefix value in front of chunk j
    exactly, and 'the first prefix value above x' is chunk j, whatever positions the search probes.
    Preconditions from the oracle's numbers: the products are exact ties, and every chunk is drawn."""
    size = nb * CH
    pr = _prios(nb, np.ones(nb, bool))
    chunk, pre = _chunk_prefix(orc, pr, size)
    assert (chunk == 4.0).all()
    u = np.arange(nb) / nb
    x = u * pre[-1]
    assert np.array_equal(x, np.concatenate([[0.0], pre[:-1]]))  # each x is a prefix value: a tie
    idx = check_sample(orc, pr, size, nb, 1.0, 0.4, u, choice=False)
    tidx = orc.per_sample_tree(pr, size, size, 0.4, u, alpha=1.0)[0]
    assert np.array_equal(tidx // CH, np.arange(nb))  # the oracle: sample j lands in chunk j
    assert np.array_equal(tidx % CH, np.full(nb, MASS[0])) and np.array_equal(idx, tidx)


def _zero_runs(nb):
    """Chunks without mass at the front, in the middle and at the end (as far as nb chunks allow)."""
    live = np.ones(nb, bool)
    if nb >= 3:
        live[:max(1, nb // 5)] = False
        live[nb - max(1, nb // 7):] = False
    if nb >= 5:
        live[nb // 2 - max(1, nb // 9) // 2:nb // 2 + (max(1, nb // 9) + 1) // 2] = False
    if not live.any():
        live[nb // 2] = True
    # a power-of-two count of chunks with mass (the trailing run grows), so that j / count is exact
    nz = np.nonzero(live)[0]
    live[nz[1 << (len(nz).bit_length() - 1):]] = False
    return live


@pytest.mark.parametrize("nb", CHUNKS)
def test_plateaus_of_zero_chunks(orc, nb):
    """Runs of zero chunks are plateaus of the prefix. u = j / nnz ties with the plateau's value: the
    draw must skip the whole run to the next chunk with mass (never a zero-priority entry), and
    u = 1 - 2^-53 must take the last chunk with mass in front of the trailing run."""
    size = nb * CH
    live = _zero_runs(nb)
    pr = _prios(nb, live)
    nz = np.nonzero(live)[0]
    chunk, pre = _chunk_prefix(orc, pr, size)
    ties = np.arange(len(nz)) / len(nz)
    assert np.array_equal(ties * pre[-1], 4.0 * np.arange(len(nz)))
    u = np.concatenate([ties, [U_LAST, 1.0 - 2.0 ** -52, 0.0, 2.0 ** -1074]])
    idx = check_sample(orc, pr, size, len(u), 1.0, 0.4, u, choice=False)
    tidx = orc.per_sample_tree(pr, size, size, 0.4, u, alpha=1.0)[0]
    assert np.array_equal(tidx[:len(nz)] // CH, nz)  # the oracle: tie j is the j-th chunk with mass
    assert tidx[len(nz)] // CH == nz[-1] and tidx[len(nz) + 2] // CH == nz[0]
    assert np.array_equal(idx, tidx)
    if nb >= 5:
        assert not live[0] and not live[-1] and not live[nb // 2]


@pytest.mark.parametrize("nb", (1023, 1024, 1025))
def test_last_nonzero_chunk_fallback(orc, nb):
    """No prefix value exceeds u * total (test_gpu_per.py's 'one_round' / 'carried' layouts: a 2^53 leaf
    in chunk 0 absorbs the ones of two chunks of the first round's last two threads when the prefix adds
    them one by one, while the round's end value takes the wave's 1 + 1 whole): the search returns
    'none' and the first chunk to reach the round's end value is taken; at 1025 chunks the second round
    has no mass and the choice is carried. The oracle reports that the chunk level's fallback decided."""
    size = nb * CH
    last = min(nb, 1024) - 1
    pr = np.zeros(size, np.float32)
    pr[5], pr[(last - 4) * CH + 3], pr[last * CH + 9] = 2.0 ** 53, 1, 1
    u = np.array([U_LAST, 0.5, 0.0, 1.0 - 2.0 ** -52, 0.25])
    idx = check_sample(orc, pr, size, len(u), 1.0, 0.4, u, choice=False)
    fell = orc.per_sample_tree(pr, size, size, 0.4, u, alpha=1.0, want_fallback=True)[2]
    assert fell[0] & 4 and fell[3] & 4 and not fell[1] and not fell[2] and not fell[4]
    assert idx[1] == idx[2] == idx[4] == 5


@pytest.mark.parametrize("nb", CHUNKS)
def test_random_priorities(orc, nb):
    """Random priorities (10 % zeros) and uniforms, a size that ends inside the last chunk."""
    rng = np.random.RandomState(1000 + nb)
    size = nb * CH - int(rng.randint(0, CH - 1)) if nb > 1 else 700
    pr = rng.uniform(0, 3, size).astype(np.float32)
    pr[rng.rand(size) < 0.1] = 0.0
    pr[0] = 0.5
    u = np.concatenate([[0.0, U_LAST], rng.random_sample(254)])
    assert (size + CH - 1) // CH == nb
    check_sample(orc, pr, size, 256, 0.6, 0.4, u, choice=False)
