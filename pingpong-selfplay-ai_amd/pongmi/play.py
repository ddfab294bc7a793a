"""Host side of K8 (pm_play, csrc/pm_play.hip): whole greedy matches in one launch.

The kernel plays every arena from its serve to the end of the episode with both players' nets
staged once per block; a block works through a range of slots (arenas of one (net A, net B) pair)
128 columns at a time, a column taking the next slot when its episode ends. The host groups the
arenas by pair (first-appearance order, arenas ascending within a pair), splits each group into
block ranges, and hands the serves over in slot order. Net id FOLLOWER (-1) is the
HardcodedBallFollower. Used by pongmi.evaluate (eval_vs_model / eval_vs_pool) and
pongmi.tournament (QNet / ball-follower pairs).

play_rnn is the same for pairs with a QNetRNN player (pm_play_rnn, csrc/pm_playrnn.hip): the
block's RNN sides take one block-wide K5 step per tick, their (h, c) per column in a device scratch.

Both take record=[arena, ...]: those arenas' episodes come back tick by tick as
pongmi.record.MatchRecord (pm_play_rec / pm_play_rnn_rec, the kernels' recording instantiations);
without it the launch is the plain kernel's.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PM_QNET_NW, check, ptr, stream_ptr
from .env import env_params
from .record import MatchRecord

FOLLOWER = -1
RNN_BASE = -2        # play_rnn: QNetRNN net k has id RNN_BASE - k
COLUMNS = 128        # arenas a block plays at once
MAX_SLOTS = 1024     # slots per block range (the kernel stages them in LDS)
TARGET_BLOCKS = 512  # 2 blocks (8 waves) per CU on 256 CUs before ranges grow past one slot per column
TARGET_BLOCKS_RNN = 256  # play_rnn: one block per CU (its LDS ring and register file fill the CU)


def plan_blocks(netA, netB, per_block=None):
    """(blk_nets int32 [nb, 2], blk_range int32 [nb, 2] = (start, count), order int32 [E]: arena of
    each slot) for per-arena net ids (any integers: play_rnn's QNetRNN ids lie below FOLLOWER).
    per_block: slots per block (default: COLUMNS, or more once the arenas would need more than
    TARGET_BLOCKS blocks, so columns refill instead of adding waves)."""
    netA = np.asarray(netA, np.int64).reshape(-1)
    netB = np.asarray(netB, np.int64).reshape(-1)
    if netA.shape != netB.shape:
        raise ValueError("netA / netB must have one id per arena")
    E = netA.shape[0]
    if per_block is None:
        per_block = min(MAX_SLOTS, COLUMNS * max(1, -(-E // (COLUMNS * TARGET_BLOCKS))))
    if not 0 < per_block <= MAX_SLOTS:
        raise ValueError(f"per_block must be in [1, {MAX_SLOTS}]")
    if E == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    shift = max(1, -int(min(netA.min(), netB.min())))  # ids start at FOLLOWER, or at the lowest QNetRNN id
    ka, kb = netA + shift, netB + shift
    width = int(kb.max()) + 1
    key = ka * width + kb
    span = int(key.max()) + 1
    if span <= (1 << 22):  # dense pair ids: first appearance by a scatter-min, no sort
        first_of = np.full(span, E, np.int64)
        np.minimum.at(first_of, key, np.arange(E))
        present = np.nonzero(first_of < E)[0]
        first = first_of[present]
        lut = np.empty(span, np.int64)
        lut[present] = np.arange(len(present))
        inv = lut[key]
    else:
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))  # pairs in first-appearance order
    grp = rank[inv.reshape(-1)]
    # stable sort by pair (radix sort for < 65536 pairs): ascending arena index within a pair
    order = np.argsort(grp.astype(np.uint16) if len(first) < (1 << 16) else grp, kind="stable").astype(np.int32)
    sizes = np.bincount(grp, minlength=len(first))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    nblk = -(-sizes // per_block)
    g = np.repeat(np.arange(len(first)), nblk)                      # group of each block
    j = np.arange(len(g)) - np.repeat(np.cumsum(nblk) - nblk, nblk)  # block index within its group
    lo = starts[g] + j * per_block
    cnt = np.minimum(per_block, sizes[g] - j * per_block)
    head = order[starts[g]]
    blk_nets = np.stack([netA[head], netB[head]], 1).astype(np.int32)
    return blk_nets, np.stack([lo, cnt], 1).astype(np.int32), order


class _Recording:
    """The record buffers of one launch: rows in the order asked, record_ticks ticks each."""

    def __init__(self, record, E, record_ticks):
        """Checks `record` (arena indices, any order) on the host: before any device call."""
        idx = np.asarray(list(record), dtype=object)
        if any(not isinstance(k, (int, np.integer)) or isinstance(k, bool) for k in idx):
            raise ValueError("record: arena indices (integers)")
        self.arenas = idx.astype(np.int64)
        if self.arenas.size and (self.arenas.min() < 0 or self.arenas.max() >= E):
            raise ValueError(f"record: arena index outside [0, {E})")
        if np.unique(self.arenas).size != self.arenas.size:
            raise ValueError("record: an arena is listed twice")
        self.cap = int(record_ticks)
        if self.cap <= 0:
            raise ValueError("record_ticks must be positive")
        self.rows = np.full(E, -1, np.int32)
        self.rows[self.arenas] = np.arange(self.arenas.size, dtype=np.int32)

    def alloc(self, dev):
        n = self.arenas.size
        self.d_rows = torch.from_numpy(self.rows).to(dev)
        self.f64 = torch.empty((n, self.cap, 7), dtype=torch.float64, device=dev)
        self.q = torch.empty((n, self.cap, 2, 3), dtype=torch.float32, device=dev)
        self.i32 = torch.empty((n, self.cap, 5), dtype=torch.int32, device=dev)

    def args(self):
        return (ptr(self.d_rows), int(self.arenas.size), self.cap, ptr(self.f64), ptr(self.q), ptr(self.i32))

    def records(self, env_kw, idA, idB, serves, length):
        """One MatchRecord per asked arena. Only the ticks an episode has are copied back."""
        idA, idB = np.asarray(idA).reshape(-1), np.asarray(idB).reshape(-1)
        F = np.minimum(length[self.arenas], self.cap).astype(np.int64)
        dev = self.f64.device
        stored = torch.arange(self.cap, device=dev)[None, :] < torch.from_numpy(F).to(dev)[:, None]
        f64, q, i32 = (t[stored].cpu().numpy() for t in (self.f64, self.q, self.i32))  # rows back to back
        lo = np.concatenate([[0], np.cumsum(F)])
        return [MatchRecord.from_ticks(env_kw, (int(idA[i]), int(idB[i])), serves[i], int(length[i]),
                                       f64[lo[r]:lo[r + 1]], q[lo[r]:lo[r + 1]], i32[lo[r]:lo[r + 1]])
                for r, i in enumerate(self.arenas.tolist())]


def play(env_kw, w_nets, netA, netB, serves, device="cuda", max_steps=1_000_000, per_block=None, record=None,
         record_ticks=4096):
    """Play one greedy episode per arena. w_nets: effective weights [nets, PM_QNET_NW] (or None when
    every id is FOLLOWER); netA / netB: per-arena net ids; serves [E, 3] (vx, vy, spin).
    Returns host arrays (scoreA int32 [E], scoreB int32 [E], length int32 [E], last int8 [E]:
    sign(rB - rA) of the final tick).
    record: arena indices (any order, no duplicates) whose episodes are also returned tick by tick, as
    a fifth value: a list of MatchRecord in that order, each holding at most record_ticks ticks (the
    players named by their net ids)."""
    serves = np.ascontiguousarray(np.asarray(serves, np.float64).reshape(-1, 3))
    E = serves.shape[0]
    rec = None if record is None else _Recording(record, E, record_ticks)
    lib = _lib.load()
    dev = torch.device(device)
    sA = torch.zeros(E, dtype=torch.int32, device=dev)
    sB = torch.zeros(E, dtype=torch.int32, device=dev)
    length = torch.full((E,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(E, dtype=torch.int8, device=dev)
    if E == 0:
        out = (sA.cpu().numpy(), sB.cpu().numpy(), length.cpu().numpy(), last.cpu().numpy())
        return out if rec is None else out + ([],)
    blk_nets, blk_range, order = plan_blocks(netA, netB, per_block)
    if w_nets is None:
        w = torch.zeros((1, PM_QNET_NW), dtype=torch.float32, device=dev)
        n_nets = 0
    else:
        w = w_nets.to(dev, torch.float32).reshape(-1, PM_QNET_NW).contiguous()
        n_nets = int(w.shape[0])
    if int(blk_nets.max(initial=-1)) >= n_nets:
        raise ValueError(f"net id {int(blk_nets.max())} but only {n_nets} nets given")
    host = np.concatenate([blk_nets.reshape(-1), blk_range.reshape(-1), order]).astype(np.int32)
    d_int = torch.from_numpy(host).to(dev)  # one copy: nets | ranges | order
    nb = blk_nets.shape[0]
    d_serves = torch.from_numpy(np.ascontiguousarray(serves[order])).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    prm = env_params(**env_kw)
    # the kernel bounds a wave's ticks over all its slots: max_steps per episode x slots per column
    per_col = -(-int(blk_range[:, 1].max()) // COLUMNS)
    wave_steps = min(int(max_steps) * per_col + per_col, 2**31 - 1)
    if rec is None:
        check(lib.pm_play(ctypes.byref(prm), ptr(w), n_nets, ptr(d_int), ptr(d_int[2 * nb:]), nb, ptr(d_int[4 * nb:]),
                          ptr(d_serves), E, wave_steps, ptr(sA), ptr(sB), ptr(length), ptr(last), ptr(status),
                          stream_ptr()), "pm_play")
    else:
        rec.alloc(dev)
        check(lib.pm_play_rec(ctypes.byref(prm), ptr(w), n_nets, ptr(d_int), ptr(d_int[2 * nb:]), nb,
                              ptr(d_int[4 * nb:]), ptr(d_serves), E, wave_steps, ptr(sA), ptr(sB), ptr(length),
                              ptr(last), ptr(status), *rec.args(), stream_ptr()), "pm_play_rec")
    out = (sA.cpu().numpy(), sB.cpu().numpy(), length.cpu().numpy(), last.cpu().numpy())
    st = int(status.item())
    if st or (out[2] < 0).any():
        raise RuntimeError(f"pm_play: {int((out[2] < 0).sum())} arenas did not finish within {max_steps} steps "
                           f"({st} invalid ids or cut episodes)")
    return out if rec is None else out + (rec.records(env_kw, netA, netB, serves, out[2]),)


def rnn_id(k):
    """play_rnn's player id of QNetRNN net k (and back: rnn_id(rnn_id(k)) == k)."""
    return RNN_BASE - k


def play_rnn(env_kw, w_qnet, w_rnn, idA, idB, serves, device="cuda", max_steps=1_000_000, per_block=None, record=None,
             record_ticks=4096):
    """Play one greedy episode per arena, at least one QNetRNN on each pair. w_qnet: effective QNet
    weights [nets, PM_QNET_NW] or None; w_rnn: effective QNetRNN weights [nets, PM_RNN_NW]
    (pongmi.rnn.fold); idA / idB: per-arena player ids (>= 0 QNet, FOLLOWER, rnn_id(k) QNetRNN k);
    serves [E, 3] (vx, vy, spin). Every episode starts from a zero hidden state. Returns host arrays
    (scoreA int32 [E], scoreB int32 [E], length int32 [E], last int8 [E]) as play does, and with
    record=[arena, ...] the list of MatchRecord as play does (players named by their ids)."""
    serves = np.ascontiguousarray(np.asarray(serves, np.float64).reshape(-1, 3))
    E = serves.shape[0]
    rec = None if record is None else _Recording(record, E, record_ticks)
    lib = _lib.load()
    dev = torch.device(device)
    sA = torch.zeros(E, dtype=torch.int32, device=dev)
    sB = torch.zeros(E, dtype=torch.int32, device=dev)
    length = torch.full((E,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(E, dtype=torch.int8, device=dev)
    if E == 0:
        out = (sA.cpu().numpy(), sB.cpu().numpy(), length.cpu().numpy(), last.cpu().numpy())
        return out if rec is None else out + ([],)
    if per_block is None:
        per_block = min(MAX_SLOTS, COLUMNS * max(1, -(-E // (COLUMNS * TARGET_BLOCKS_RNN))))
    blk_nets, blk_range, order = plan_blocks(idA, idB, per_block)
    if (blk_nets.min(1) > RNN_BASE).any():
        raise ValueError("play_rnn: every pair needs a QNetRNN player (use play for the others)")

    def weights(w, width):
        if w is None:
            return torch.zeros((1, width), dtype=torch.float32, device=dev), 0
        w = w.to(dev, torch.float32).reshape(-1, width).contiguous()
        return w, int(w.shape[0])
    wq, n_qnet = weights(w_qnet, PM_QNET_NW)
    wr, n_rnn = weights(w_rnn, _lib.PM_RNN_NW)
    if int(blk_nets.max()) >= n_qnet:
        raise ValueError(f"QNet id {int(blk_nets.max())} but only {n_qnet} QNets given")
    if RNN_BASE - int(blk_nets.min()) >= n_rnn:
        raise ValueError(f"QNetRNN id {RNN_BASE - int(blk_nets.min())} but only {n_rnn} QNetRNNs given")
    host = np.concatenate([blk_nets.reshape(-1), blk_range.reshape(-1), order]).astype(np.int32)
    d_int = torch.from_numpy(host).to(dev)  # one copy: nets | ranges | order
    nb = blk_nets.shape[0]
    d_serves = torch.from_numpy(np.ascontiguousarray(serves[order])).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.pm_play_rnn_scratch_bytes(nb)) // 4, dtype=torch.float32, device=dev)
    prm = env_params(**env_kw)
    # the kernel bounds a block's ticks over all its slots: max_steps per episode x slots per column
    per_col = -(-int(blk_range[:, 1].max()) // COLUMNS)
    block_steps = min(int(max_steps) * per_col + per_col, 2**31 - 1)
    if rec is None:
        check(lib.pm_play_rnn(ctypes.byref(prm), ptr(wq), n_qnet, ptr(wr), n_rnn, ptr(d_int), ptr(d_int[2 * nb:]), nb,
                              ptr(d_int[4 * nb:]), ptr(d_serves), E, block_steps, ptr(scratch), ptr(sA), ptr(sB),
                              ptr(length), ptr(last), ptr(status), stream_ptr()), "pm_play_rnn")
    else:
        rec.alloc(dev)
        check(lib.pm_play_rnn_rec(ctypes.byref(prm), ptr(wq), n_qnet, ptr(wr), n_rnn, ptr(d_int), ptr(d_int[2 * nb:]),
                                  nb, ptr(d_int[4 * nb:]), ptr(d_serves), E, block_steps, ptr(scratch), ptr(sA),
                                  ptr(sB), ptr(length), ptr(last), ptr(status), *rec.args(), stream_ptr()),
              "pm_play_rnn_rec")
    out = (sA.cpu().numpy(), sB.cpu().numpy(), length.cpu().numpy(), last.cpu().numpy())
    st = int(status.item())
    if st or (out[2] < 0).any():
        raise RuntimeError(f"pm_play_rnn: {int((out[2] < 0).sum())} arenas did not finish within {max_steps} steps "
                           f"({st} invalid ids or cut episodes)")
    return out if rec is None else out + (rec.records(env_kw, idA, idB, serves, out[2]),)
