"""The population's collecting rollout (pm_rollout_pop_push, csrc/pm_rollout_pop.hip) on rings of 4096 to 65 536
entries, where the two kernels whose work grows with the ring take the paths that rings of 4000 entries
(tests/test_gpu_rollout_pop.py) never reach:

  k_rpp_prios   max(prios[0:fill]): four float4 loads per thread and round (element e + k * 1024), loads past the
                end clamped, one round per 16 384 entries, a scalar tail, a scalar loop for unaligned priorities, a
                NaN priority, fill = min(size + advance, cap);
  k_rpp_nodes   a (node blocks, n) grid: one block per 64 level-1 nodes (4096 entries), members with shorter trees
                than the longest leaving their surplus blocks.

Everything goes through test_gpu_rollout_pop's Pair, so every member is compared bit for bit with a solo
SelfPlayRollout.run(steps, replay=...), pm_per_build and oracle.per_tree; the pushed priority is also compared
with a float32 maximum taken in numpy over a host copy of prios[:fill]. The member tables are module data:
tests/test_rollout_pop_host.py checks without a GPU that they reach the paths named above. m stays 32 or 33 and the
step counts small: the ring's length is under test, not the workload."""
import numpy as np
import pytest
import torch

from test_gpu_rollout_pop import Pair, _nets, _tree_is_oracle

pytestmark = pytest.mark.gpu

MARK = 50.0  # above every seeded priority (0.01 .. 3.01)
NAN = float("nan")
FULL = 65536  # four rounds of k_rpp_prios, sixteen node blocks


def _full(entry, value=MARK):
    return dict(cap=FULL, fill=FULL, aligned=True, marks=((entry, value),))


# Part 1: one launch, one member per row. fill < cap: pos = size = fill. marks: (entry, priority) written over the
# seeded priorities; the last column of the comment is the load of k_rpp_prios that reads the maximum.
PRIO_MEMBERS = (
    _full(0),                              # round 0, k = 0, thread 0
    _full(4 * (1024 + 4)),                 # round 0, k = 1
    _full(4 * (2048 + 7) + 1),             # round 0, k = 2
    _full(4 * (3072 + 1023) + 3),          # round 0, k = 3, thread 1023
    _full(4 * (4096 + 5)),                 # round 1
    _full(4 * (8192 + 2048 + 9) + 2),      # round 2, k = 2
    _full(FULL - 1),                       # round 3, k = 3, thread 1023
    # n4 = 1029: k = 1 is real for threads 0..4 and clamped for the rest; a 3-entry tail
    dict(cap=8192, fill=4119, aligned=True, marks=((4 * 1028, MARK),)),
    dict(cap=8192, fill=4119, aligned=True, marks=((4118, MARK),)),
    # n4 = 4098: a second round of two threads whose k >= 1 loads are clamped; no tail
    dict(cap=20000, fill=16392, aligned=True, marks=((16391, MARK),)),
    # priorities 4 bytes past a 16-byte boundary: the scalar loop alone, 20 passes
    dict(cap=20000, fill=20000, aligned=False, marks=((19999, MARK),)),
    # a NaN among finite markers: the pushed priority is the quiet NaN
    dict(cap=FULL, fill=FULL, aligned=True, marks=((0, MARK), (4 * (2048 + 7) + 1, NAN), (FULL - 1, MARK))),
    # tails of one and of two entries
    dict(cap=8192, fill=4117, aligned=True, marks=((4116, MARK),)),
    dict(cap=8192, fill=4118, aligned=True, marks=((4117, MARK),)),
)

# Part 3: one launch, rings that start full. cap -> node blocks: 16; 2 (the second holds one node over one leaf);
# 1 (exactly); 1 (partial); none (the member keeps no sum tree).
NODE_MEMBERS = (dict(cap=FULL, tree=True), dict(cap=4097, tree=True), dict(cap=4096, tree=True),
                dict(cap=1320, tree=True), dict(cap=2000, tree=False))

# Part 4: the chain's rings and what they hold at the start.
CHAIN_MEMBERS = (dict(cap=1320, pos=700, size=700), dict(cap=4097, pos=4000, size=4097),
                 dict(cap=FULL, pos=30000, size=30000))


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _pushed_slots_hold(R, pos, count, want):
    slots = (pos + np.arange(count)) % R.cap
    got = R.prios.cpu().numpy().view(np.int32)[slots]
    assert (got == _bits(want)).all(), (pos, count, want)


def test_pushed_priority_at_every_load_of_k_rpp_prios():
    """Every member's maximum sits where one particular load of k_rpp_prios reads it (PRIO_MEMBERS): a kernel with a
    wrong stride, clamp, round start, tail or unaligned loop pushes a seeded priority (below 3.02) instead of 50."""
    tab, m, steps = PRIO_MEMBERS, 32, 2
    n = len(tab)

    def prepare(p, R):
        for e, v in tab[p]["marks"]:
            R.prios[e] = v

    P = Pair(n, m, [c["cap"] for c in tab], pos=[c["fill"] if c["fill"] < c["cap"] else 100 for c in tab],
             size=[c["fill"] for c in tab], steps_max=steps, unaligned=[p for p in range(n) if not tab[p]["aligned"]],
             prepare=prepare)
    before = [R.prios.cpu().numpy().copy() for R in P.Rp]
    pos = [R.pos for R in P.Rp]
    for p, c in enumerate(tab):
        assert P.Rp[p].prios.data_ptr() % 16 == (0 if c["aligned"] else 4), p
        assert (P.Rp[p].size, P.Rp[p].work is not None) == (c["fill"], True), p
    P.collect(steps)
    assert P.pop._advance == steps * m
    got = P.pop.prio.cpu().numpy()
    for p, c in enumerate(tab):
        want = before[p][:c["fill"]].max()  # numpy's maximum: float32, carries a NaN
        assert want.dtype == np.float32
        if any(v != v for _, v in c["marks"]):
            assert _bits(want) == 0x7FC00000, p
        else:
            assert want == MARK, p
        assert _bits(got[p]) == _bits(want), (p, c, got[p], want)
        _pushed_slots_hold(P.Rp[p], pos[p], steps * m, want)
        assert P.Rp[p].size == min(c["cap"], c["fill"] + steps * m), p
    P.check(vacuous_ok=True)


def test_fill_is_honoured_past_size():
    """max(prios[0:fill]) is k_rpp_prios' stated contract, and `size` in pm_roll_member comes from the ABI's
    caller: a ring of 65 536 bound at size 20 000 whose entries past 20 000 hold 1000.0 pushes the maximum of
    its first 20 000 entries, and after `advance` = steps * m more the maximum of 20 000 + steps * m, never 1000.
    PopulationRollout itself cannot produce this state (what lies past `size` in a DeviceReplay is zero); the
    member keeps no sum tree, so no sampler is asked about the entries past size."""
    m, steps, size = 32, 2, 20000

    def prepare(p, R):
        R.prios[size:] = 1000.0

    P = Pair(1, m, FULL, pos=size, size=size, steps_max=steps, trees=[False], prepare=prepare)
    for k in range(2):
        fill = size + k * steps * m
        host = P.Rp[0].prios.cpu().numpy()
        want = host[:fill].max()
        assert want < 3.02 and (host[fill:] == 1000.0).all()
        P.collect(steps)
        assert P.pop._advance == (k + 1) * steps * m  # the second launch ran on the first one's table
        assert _bits(P.pop.prio.cpu().numpy()[0]) == _bits(want), (k, float(P.pop.prio[0]), want)
        _pushed_slots_hold(P.Rp[0], fill, steps * m, want)
    P.check(vacuous_ok=True)
    assert (P.Rp[0].pos, P.Rp[0].size) == (size + 2 * steps * m,) * 2


def test_fill_saturates_at_cap_under_an_advance():
    """Rings bound ten entries short of full. The first collect fills them and wraps; a marker then goes into one
    of the last ten entries (on the device, as a learner's scatter would put it). The second collect runs on the
    same table with size + advance > cap: its fill is cap, so it pushes the marker. A fill that ignored
    `advance` would stop ten entries short of the end and miss it."""
    n, m, steps, caps = 2, 32, 2, [FULL, 5000]
    P = Pair(n, m, caps, pos=[c - 10 for c in caps], size=[c - 10 for c in caps], steps_max=steps)
    P.collect(steps)
    for p in range(n):
        assert (P.Rp[p].pos, P.Rp[p].size) == (steps * m - 10, caps[p])
        for R in (P.Rp[p], P.Rs[p]):
            R.prios[caps[p] - 3] = MARK
            R.max_prio_stale = True
            R.refresh()
    assert P.pop._advance == steps * m
    pos = [R.pos for R in P.Rp]
    P.collect(steps)
    assert P.pop._advance == 2 * steps * m  # no rebind: size + advance = cap + 54 in the second launch
    for p in range(n):
        assert _bits(P.pop.prio.cpu().numpy()[p]) == _bits(MARK), (p, float(P.pop.prio[p]))
        _pushed_slots_hold(P.Rp[p], pos[p], steps * m, MARK)
    P.check(vacuous_ok=True)


def test_node_grids_of_several_and_of_unequal_block_counts():
    """One launch over NODE_MEMBERS: k_rpp_nodes' grid is 16 blocks wide, the shorter trees' members leave 14 or
    15 of them, a second block holds a single node over a single leaf, and one member has no tree. The rings
    start full with their write slots 7 * m + p entries before the end, so every ring wraps and the leaf that the
    one-node block sums is rewritten. check(): every tree equals the solo run's, pm_per_build and oracle.per_tree."""
    tab, m, steps = NODE_MEMBERS, 33, 30
    n = len(tab)
    caps = [c["cap"] for c in tab]
    P = Pair(n, m, caps, pos=[caps[p] - 7 * m - p for p in range(n)], size=caps, steps_max=steps,
             trees=[c["tree"] for c in tab])
    assert [R.work is not None for R in P.Rp] == [c["tree"] for c in tab]
    P.collect(steps)
    assert [R.pos for R in P.Rp] == [(steps - 7) * m - p for p in range(n)]  # every ring wrapped
    P.check()


def test_long_chain_without_a_rebind_then_a_rebind_on_the_device():
    """Six collects of 20 steps on one table: `advance` grows to 3960, three times the shortest ring, which wraps
    three times while the longest never does, and the rings fill from different sizes. Then someone else pushes
    five transitions into member 1's ring (the population's and the solo's alike): the next collect rebinds, its
    `advance` restarts, and every member still equals its solo run."""
    tab, m, steps = CHAIN_MEMBERS, 33, 20
    n = len(tab)
    caps = [c["cap"] for c in tab]
    P = Pair(n, m, caps, pos=[c["pos"] for c in tab], size=[c["size"] for c in tab], steps_max=steps)
    for k in range(6):
        P.collect(steps)
        done = (k + 1) * steps * m
        assert P.pop._advance == done  # never rebound
        for p, c in enumerate(tab):
            want = ((c["pos"] + done) % c["cap"], min(c["cap"], c["size"] + done))
            assert (P.Rp[p].pos, P.Rp[p].size) == (P.Rs[p].pos, P.Rs[p].size) == want, (k, p)
        P.check(vacuous_ok=True)
    assert P.pop._advance == 3960 == 3 * caps[0] and P.episodes > 0 and P.wrapped  # launches 4 to 6: advance > cap
    g = torch.Generator().manual_seed(8)
    s, ns, r = torch.randn((5, 7), generator=g), torch.randn((5, 7), generator=g), torch.randn(5, generator=g)
    a, done = torch.tensor([0, 2, 1, 1, 0]), torch.tensor([0, 1, 0, 0, 1])
    for R in (P.Rp[1], P.Rs[1]):
        R.push(s, a, r, ns, done)
    P.collect(steps)
    assert P.pop._advance == steps * m  # rebound: the table holds the rings as the push left them
    P.check()
    assert (P.Rp[1].pos, P.Rp[1].size) == ((4000 + 3960 + 5 + steps * m) % 4097, 4097)


def test_trainer_on_rings_past_4096():
    """test_trainer_equals_two_replay_trainers on rings of 5000 and 9000 entries: ring 0 fills, wraps and has two
    node blocks; ring 1 ends at 6144 of 9000, and the last k_rpp_prios pass over it (fill 5120, n4 = 1280) has real
    k = 1 loads. The priorities k_rpp_prios reads are the ones the learners' scatter wrote."""
    from models.qnet import QNet
    from pongmi.dqn import DQNLearner, DQNPopulation, PopulationTrainer, ReplayTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import STATS_PUSH
    n, m, caps, k, cs = 2, 64, [5000, 9000], 6, 16
    torch.manual_seed(21)
    nets = [QNet(7, 3) for _ in range(n)]
    wA = _nets(1, 6)[0]
    kw = dict(batch=64, lr=1e-3, train_features=True, target_update_interval=3)
    env = PongEnv2PBatch(n * m, seed=31, autoreset=True)
    env.reset()
    solo_envs = []
    for p in range(n):
        e = PongEnv2PBatch(m, seed=31 + p, autoreset=True)
        e.f64.copy_(env.f64[:, p * m:(p + 1) * m])
        e.i32.copy_(env.i32[:, p * m:(p + 1) * m])
        solo_envs.append(e)
    Pop = DQNPopulation(nets, seed=[7, 8], **kw)
    Rp = [DeviceReplay(caps[p], "cuda") for p in range(n)]
    got = PopulationTrainer(env, wA, Pop, Rp, collect_steps=cs, updates=1, epsilon=[0.1, 0.3], seed_net=[1, 2],
                            seed=[3, 4]).run(k)
    episodes = 0
    for p in range(n):
        L = DQNLearner(nets[p], seed=7 + p, **kw)
        R = DeviceReplay(caps[p], "cuda")
        ref = ReplayTrainer(solo_envs[p], wA, L, R, collect_steps=cs, updates=1, epsilon=[0.1, 0.3][p], seed_net=1 + p,
                            seed=3 + p).run(k)
        assert [int(got[s][p]) for s in STATS_PUSH] == [ref[s] for s in STATS_PUSH], p
        episodes += ref["episodes"]
        assert (Rp[p].pos, Rp[p].size) == (R.pos, R.size) == [(k * cs * m - caps[0], caps[0]), (k * cs * m,) * 2][p]
        assert torch.equal(Rp[p].trans.view(torch.int32), R.trans.view(torch.int32))
        assert torch.equal(Rp[p].prios.view(torch.int32), R.prios.view(torch.int32))
        assert torch.equal(Rp[p].work, R.work)
        _tree_is_oracle(Rp[p])
        for name in ("params", "target", "adam_m", "adam_v", "stats_buf"):
            assert torch.equal(getattr(Pop, name)[p], getattr(L, name)), (p, name)
        assert torch.equal(env.f64[:, p * m:(p + 1) * m], solo_envs[p].f64)
    # played to the end of episodes; ring 0 wrapped, ring 1 is still filling past 4096 entries
    assert episodes > 0 and k * cs * m > caps[0] and 4096 + cs * m < k * cs * m < caps[1]
