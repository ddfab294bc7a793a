"""The population's collecting rollout (pm_rollout_pop_*, pongmi.rollout.PopulationRollout,
pongmi.dqn.PopulationTrainer) on the MI355X: every member against a solo SelfPlayRollout.run(steps, replay=...) on
its own PongEnv2PBatch(m, seed=seed_env[p]) whose state the member's slice was copied from. Everything is compared
bit for bit, with no tolerance (the kernels are pure functions of their inputs): the ten state fields, obsA /
obsB, ep_reward, the ring rows and prios as int32, the whole tree workspace (which in turn equals a fresh
pm_per_build and the numpy model oracle.per_tree), pos / size and all six stats.

Ring sizes: the rings bound here have at most 4000 entries, so k_rpp_prios runs one round with one real load
per thread and k_rpp_nodes one block per member. Rings of 4096 to 65 536 entries (every load of every round of
k_rpp_prios, its tail, unaligned and NaN paths, fill honoured and saturating, node grids of several and of
unequal block counts, long chains of collects and a rebind on the device) are tests/test_gpu_rollout_pop_rings.py,
on this file's Pair.

Step counts: with random nets the CPU port (oracle/cpu_selfplay.py CpuRollout, seeds 0..5) ends its first
episode after 14-19 vector steps at 32, 33 and 100 arenas, whatever epsilon, and after 16-101 steps at one arena.
So every case with m >= 32 plays at least 30 steps and asserts that its solo references finished episodes and
that a ring wrapped; the cases with m = 1 assert neither."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "vx", "vy", "spin", "top", "bot", "scoreA", "scoreB", "bounces")


def _nets(k, seed):
    """k opponents' effective weights."""
    from models.qnet import QNet
    from pongmi import _lib
    from pongmi.qnet import fold, pack_state_dict
    torch.manual_seed(seed)
    return [fold(pack_state_dict(QNet(7, 3).state_dict()), _lib.PM_FOLD_TRAIN).reshape(-1) for _ in range(k)]


def _params(n, seed):
    """n different modelB blocks, stacked: one random QNet, every member a perturbation of it."""
    from models.qnet import QNet
    from pongmi.qnet import pack_state_dict
    torch.manual_seed(seed)
    base = pack_state_dict(QNet(7, 3).state_dict()).reshape(1, -1)
    g = torch.Generator().manual_seed(seed)
    return (base.cpu() + 0.05 * torch.randn((n, base.shape[1]), generator=g)).cuda().contiguous()


def _seed_ring(R, pos, size, seed, tree=True, prepare=None):
    """A ring as a learner left it: `size` filled slots with priorities of its own, write slot `pos`. prepare(R)
    runs on the seeded ring before its tree and tracked maximum are taken (markers in prios)."""
    if not tree:
        R.work = None
    R.pos, R.size = pos, size
    if size:
        g = torch.Generator().manual_seed(seed)
        R.prios[:size] = (torch.rand(size, generator=g) * 3 + 0.01).cuda()
        R.trans[:size] = torch.randn((size, 16), generator=g).cuda()
    if prepare is not None:
        prepare(R)
    _refresh(R)


def _refresh(R):
    if R.work is not None:
        R.refresh()
    else:  # refresh() without the tree
        R.max_prio = float(R.prios[:R.size].max()) if R.size else 1.0
        R.max_prio_stale = False


def _tree_is_rebuild(R):
    from pongmi import _lib
    from pongmi._lib import check, ptr, stream_ptr
    w = torch.zeros_like(R.work)
    check(_lib.load().pm_per_build(ptr(R.prios), R.cap, R.alpha, ptr(w), stream_ptr()), "pm_per_build")
    assert torch.equal(R.work, w)


def _tree_is_oracle(R):
    """The workspace's chunk, sub and leaf sections against the numpy model of the tree (oracle.per_tree), which
    shares no code with the library."""
    import numpy as np
    from oracle import oracle
    from pongmi import replay as rp
    cap = R.cap
    chunk, sub, leaf = oracle.per_tree(R.prios.cpu().numpy(), cap, R.alpha)
    work = R.work.cpu().numpy()
    nchunk, nsub = -(-cap // 1024), -(-cap // 64)
    o1 = rp._pad(nchunk)
    o2 = o1 + rp._pad(nsub)
    assert np.array_equal(work[:8 * nchunk].view(np.float64), chunk)
    assert np.array_equal(work[o1:o1 + 8 * nsub].view(np.float64), sub)
    assert np.array_equal(work[o2:o2 + 4 * cap].view(np.int32), leaf.view(np.int32))


class Pair:
    """A population collector and its n solo references on copies of the same state. prepare(p, R) is called on
    both of member p's rings once they are seeded, before their trees and tracked maxima are taken."""

    def __init__(self, n, m, caps, *, pos=0, size=0, eps=0.02, seed_env=None, seed_net=0, wA=None, steps_max, trees=None,
                 unaligned=(), pop_seed=77, prepare=None):
        from pongmi.env import PongEnv2PBatch
        from pongmi.replay import DeviceReplay
        from pongmi.rollout import PopulationRollout, SelfPlayRollout, _per_member
        self.n, self.m = n, m
        caps, pos, size = (_per_member("x", v, n) for v in (caps, pos, size))
        self.eps, seed_net = _per_member("x", eps, n), _per_member("x", seed_net, n)
        self.env = PongEnv2PBatch(n * m, seed=pop_seed, autoreset=True)
        self.env.reset()
        if seed_env is None:
            seed_env = [pop_seed + p for p in range(n)]
        self.params = _params(n, 11 * n + m)
        wA = wA if wA is not None else _nets(1, 5)[0]
        trees = trees or [True] * n
        self.Rp, self.Rs, self.solo_env, self.solo = [], [], [], []
        for p in range(n):
            for R in (self.Rp, self.Rs):
                R.append(DeviceReplay(caps[p], "cuda"))
                if p in unaligned:  # prios 4 bytes past a 16-byte boundary
                    R[-1].prios = torch.zeros(caps[p] + 1, device="cuda")[1:]
                _seed_ring(R[-1], pos[p], size[p], 1000 + p, trees[p],
                           prepare=None if prepare is None else (lambda ring, p=p: prepare(p, ring)))
            e = PongEnv2PBatch(m, seed=seed_env[p], autoreset=True)
            e.f64.copy_(self.env.f64[:, p * m:(p + 1) * m])
            e.i32.copy_(self.env.i32[:, p * m:(p + 1) * m])
            e.obsA.copy_(self.env.obsA[p * m:(p + 1) * m])
            e.obsB.copy_(self.env.obsB[p * m:(p + 1) * m])
            self.solo_env.append(e)
            wa = wA[p] if isinstance(wA, (list, tuple)) else (wA if wA.dim() == 1 else wA[p])
            self.solo.append(SelfPlayRollout(e, wa, self.params[p].clone(), epsilon=self.eps[p], seed_net=seed_net[p]))
        self.pop = PopulationRollout(self.env, wA, self.params, n=n, replays=self.Rp, epsilon=eps,
                                     seed_env=None if seed_env == [pop_seed + p for p in range(n)] else seed_env,
                                     seed_net=seed_net, steps_max=steps_max)
        self.episodes, self.wrapped = 0, False

    def collect(self, steps):
        from pongmi.rollout import STATS_PUSH
        got = self.pop.collect(steps)
        for p in range(self.n):
            before = self.Rs[p].pos
            ref = self.solo[p].run(steps, replay=self.Rs[p])
            self.wrapped |= before + steps * self.m >= self.Rs[p].cap
            self.episodes += ref["episodes"]
            assert [int(got[k][p]) for k in STATS_PUSH] == [ref[k] for k in STATS_PUSH], (p, steps)

    def check(self, vacuous_ok=False):
        m = self.m
        f64, i32 = self.env.f64.cpu(), self.env.i32.cpu()
        obsA, obsB, ep = self.env.obsA.cpu(), self.env.obsB.cpu(), self.pop.ep_reward.cpu()
        for p in range(self.n):
            e, sl = self.solo_env[p], slice(p * m, (p + 1) * m)
            assert torch.equal(f64[:, sl], e.f64.cpu()) and torch.equal(i32[:3, sl], e.i32[:3].cpu()), p  # the ten fields
            assert torch.equal(obsA[sl], e.obsA.cpu()) and torch.equal(obsB[sl], e.obsB.cpu()), p
            assert torch.equal(ep[sl], self.solo[p].ep_reward.cpu()), p
            a, b = self.Rp[p], self.Rs[p]
            assert (a.pos, a.size) == (b.pos, b.size), p
            assert torch.equal(a.trans.view(torch.int32), b.trans.view(torch.int32)), p
            assert torch.equal(a.prios.view(torch.int32), b.prios.view(torch.int32)), p  # bits: a NaN equals itself
            if a.work is not None:
                assert torch.equal(a.work, b.work), p
                _tree_is_rebuild(a)
                _tree_is_oracle(a)
            assert e.counter == self.env.counter
        if not vacuous_ok:
            assert self.episodes > 0 and self.wrapped, (self.episodes, self.wrapped)


def test_state_fields_cover_the_env():
    from pongmi.env import F64_FIELDS, I32_FIELDS
    assert tuple(F64_FIELDS) + tuple(I32_FIELDS[:3]) == FIELDS  # the fourth int field, serves, is not the rollout's


@pytest.mark.parametrize("n,m,steps", [(1, 32, 30), (3, 1, 40), (3, 32, 30), (3, 33, 30), (3, 100, 30)])
def test_tile_edges(n, m, steps):
    """One member; one arena; a whole tile; one arena past a tile; three tiles and a part. The rings start filled,
    so the pushed priority is the maximum of priorities a learner left, and near their ends, so the launch wraps."""
    cap = 40 * m
    P = Pair(n, m, cap, pos=[cap - 7 * m - p for p in range(n)], size=cap, steps_max=steps)
    P.collect(steps)
    P.check(vacuous_ok=m < 32)
    assert P.wrapped


def test_grid_above_the_cu_count():
    """300 members of one tile each: more blocks than compute units, few steps (the members' first episodes end
    after 14-19 steps: 20 steps of 300 x 32 arenas finish some)."""
    P = Pair(300, 32, 32 * 24, pos=32 * 10 + 5, size=32 * 12, steps_max=20)
    P.collect(20)
    P.check()


def test_differing_members():
    """Rings of different lengths and write slots (they wrap at different steps; member 0's launch fills its ring
    exactly: steps * m == cap), epsilon 0, 0.02 and 1, distinct seeds, an opponent shared by two members and one
    of a member's own, an empty ring, priorities that are not 16-byte aligned, and a member that keeps no sum tree."""
    n, m, steps = 4, 40, 32
    nets = _nets(2, 9)
    P = Pair(n, m, [steps * m, 1500, 2048, 1400], pos=[0, 1490, 5, 700], size=[0, 1500, 5, 1400], eps=[0.0, 0.02, 1.0, 0.02],
             seed_env=[3, 1 << 40, 77, 0xFFFFFFFFFFFFFFFF], seed_net=[0, 5, 1 << 33, 9], wA=[nets[0], nets[1], nets[0], nets[0]],
             steps_max=steps, trees=[True, True, True, False], unaligned=(1,))
    tab = P.pop
    assert tab.wA[0].data_ptr() == tab.wA[2].data_ptr() == tab.wA[3].data_ptr() != tab.wA[1].data_ptr()
    P.collect(steps)
    P.check()
    assert P.Rp[3].work is None and P.Rp[0].pos == 0 and P.Rp[0].size == steps * m


def test_two_chained_collects_take_the_new_maximum_on_the_device():
    """advance != 0 in the second launch, the heads' and the draws' counters continue, and the priorities are
    overwritten on the device in between (as update_from does; refresh() then rebuilds the tree): the second
    push stores each member's new maximum, read through prio_dev with no rebind."""
    n, m = 3, 33
    P = Pair(n, m, [33 * 40, 33 * 36, 33 * 50], steps_max=20)
    P.collect(18)
    assert all(float(P.pop.prio[p]) == 1.0 for p in range(n))  # into empty rings
    for p in range(n):
        g = torch.Generator().manual_seed(50 + p)
        new = (torch.rand(P.Rp[p].size, generator=g) * (2 + p) + 0.01).cuda()
        for R in (P.Rp[p], P.Rs[p]):
            R.prios[:R.size] = new
            R.max_prio_stale = True
            R.refresh()
    assert P.pop._advance == 18 * m
    P.collect(20)
    assert P.pop._advance == 38 * m  # no rebind between the two
    for p in range(n):
        assert float(P.pop.prio[p]) == P.Rs[p].max_prio != 1.0
    P.check()


def test_params_are_played_in_place():
    """After the stacked params change in place (an update, exploit()), the next collect plays the new features
    and heads: the solo references are handed the new blocks with set_paramsB."""
    n, m = 2, 32
    P = Pair(n, m, 32 * 30, steps_max=16)
    P.collect(16)
    g = torch.Generator().manual_seed(4)
    P.params.add_((0.1 * torch.randn(P.params.shape, generator=g)).cuda())
    old = P.pop.wB.clone()
    for p in range(n):
        P.solo[p].set_paramsB(P.params[p].clone())
    P.collect(16)
    assert not torch.equal(old, P.pop.wB)
    P.check()


def test_trainer_equals_two_replay_trainers():
    from models.qnet import QNet
    from pongmi.dqn import DQNLearner, DQNPopulation, PopulationTrainer, ReplayTrainer
    from pongmi.env import PongEnv2PBatch
    from pongmi.replay import DeviceReplay
    from pongmi.rollout import STATS_PUSH
    n, m, cap, k = 2, 32, 32 * 20, 4
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
    Rp = [DeviceReplay(cap, "cuda") for _ in range(n)]
    got = PopulationTrainer(env, wA, Pop, Rp, collect_steps=8, updates=2, epsilon=[0.1, 0.3], seed_net=[1, 2], seed=[3, 4]).run(k)
    episodes = 0
    for p in range(n):
        L = DQNLearner(nets[p], seed=7 + p, **kw)
        R = DeviceReplay(cap, "cuda")
        ref = ReplayTrainer(solo_envs[p], wA, L, R, collect_steps=8, updates=2, epsilon=[0.1, 0.3][p], seed_net=1 + p,
                            seed=3 + p).run(k)
        assert [int(got[s][p]) for s in STATS_PUSH] == [ref[s] for s in STATS_PUSH], p
        episodes += ref["episodes"]
        assert (Rp[p].pos, Rp[p].size) == (R.pos, R.size) and R.size == cap
        assert torch.equal(Rp[p].trans.view(torch.int32), R.trans.view(torch.int32)) and torch.equal(Rp[p].prios, R.prios)
        assert torch.equal(Rp[p].work, R.work)
        for name in ("params", "target", "adam_m", "adam_v", "stats_buf"):
            assert torch.equal(getattr(Pop, name)[p], getattr(L, name)), (p, name)
        assert torch.equal(env.f64[:, p * m:(p + 1) * m], solo_envs[p].f64)
    assert episodes > 0 and k * 8 * m > cap  # played to the end of episodes, and the rings wrapped
