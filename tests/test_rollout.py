"""The rollout bookkeeping on the CPU: the contract's numpy statement (rollout_ref.py) against the
project's own host wrappers (the compat VecMonitor and the driver's StatsRecorder) and against the
reference's torch advantage loop, the ring's arithmetic, the C ABI's and the module's argument
checks, and the driver's option check.  The kernels themselves: test_gpu_rollout.py."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from rollout_ref import ROW, EpisodeStatsRef, discount_bound, gae_inputs, gae_ref, gae_torch_loop

NAMES = ["WinLossRewardFunction", "ResourceGatherRewardFunction", "ProduceWorkerRewardFunction", "ProduceBuildingRewardFunction",
         "AttackRewardFunction", "ProduceCombatUnitRewardFunction"]
RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])


def load_driver():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


class StreamEnv:
    """A vec env that replays given (reward, done, raw) streams: what the host wrappers wrap."""

    def __init__(self, rewards, dones, raws):
        self.rewards, self.dones, self.raws = rewards, dones, raws
        self.num_envs = rewards.shape[1]
        self.observation_space = self.action_space = None
        self.rfs = NAMES
        self.t = 0

    def reset(self):
        self.t = 0
        return None

    def step_async(self, actions):
        pass

    def step_wait(self):
        t = self.t
        self.t += 1
        return None, self.rewards[t].copy(), self.dones[t].copy(), [{"raw_rewards": r} for r in self.raws[t].copy()]

    def close(self):
        pass


def host_wrappers(rewards, dones, raws, gamma=0.99):
    """The compat VecMonitor around the driver's StatsRecorder over the streams: the infos that
    carry "episode", in the order the reference's scan meets them, as (step, env, info)."""
    from gym_microrts.run_driver import install

    install()
    from stable_baselines3.common.vec_env import VecMonitor

    envs = VecMonitor(load_driver().StatsRecorder(StreamEnv(rewards, dones, raws), gamma))
    envs.reset()
    out = []
    for t in range(rewards.shape[0]):
        _, _, _, infos = envs.step(None)
        out += [(t, e, info) for e, info in enumerate(infos) if "episode" in info]
    return out


def streams(T, N, seed, p=0.12, integral=False):
    """Raw rewards (real-valued, or the engine's kind: small integers and zeros), dones with
    probability p, reward = raw @ RW as the engine's tensor contract computes it (a sequential dot)."""
    rng = np.random.default_rng(seed)
    raws = rng.integers(-2, 4, (T, N, 6)).astype(np.float64) if integral else rng.standard_normal((T, N, 6)) * 3
    raws[rng.random((T, N, 6)) < 0.4] = 0
    dones = rng.random((T, N)) < p
    rewards = np.zeros((T, N))
    for k in range(6):
        rewards = rewards + raws[..., k] * RW[k]
    return rewards, dones, raws


def compare_with_wrappers(records, host, raws, dones):
    """records: rows [k, ROW] in record order; host: host_wrappers' list.  Exact on the order, r, l
    and the raw sums; the discounted sums within discount_bound of the episode's own rows."""
    from gym_microrts import rollout

    recs = rollout.records_of(records, NAMES)
    assert [(r["step"], r["env"]) for r in recs] == [(t, e) for t, e, _ in host]
    start = {}
    for rec, (t, e, info) in zip(recs, host):
        assert rec["episode"]["r"] == info["episode"]["r"] and rec["episode"]["l"] == info["episode"]["l"], (t, e)
        ms, hs = rec["microrts_stats"], info["microrts_stats"]
        assert list(ms) == list(hs)
        for k in NAMES:
            assert ms[k] == hs[k], (t, e, k)
        t0 = start.get(e, 0)
        rows = raws[t0:t + 1, e]
        assert len(rows) == rec["episode"]["l"]
        bound = discount_bound(np.concatenate([rows, rows.sum(1, keepdims=True)], 1))
        for j, k in enumerate(["discounted_" + k for k in NAMES] + ["discounted"]):
            assert abs(ms[k] - hs[k]) <= bound[j], (t, e, k, ms[k], hs[k], bound[j])
        start[e] = t + 1
    return len(recs)


@pytest.mark.parametrize("integral", [False, True])
def test_numpy_update_equals_the_host_wrappers(integral):
    T, N = 70, 7
    rewards, dones, raws = streams(T, N, 11 + integral, integral=integral)
    dones[3] = True        # every env ends in one step
    dones[4] = False
    dones[4, 0] = True     # an episode of length 1, env 0 alone
    dones[9, N - 1] = True
    ref = EpisodeStatsRef(N, 0.99)
    for t in range(T):
        ref.update(rewards[t], dones[t], raws[t])
    assert ref.count == int(dones.sum()) == len(ref.records) and ref.count > 40
    np.testing.assert_array_equal(ref.ring[:ref.count], np.array(ref.records))
    assert compare_with_wrappers(ref.ring[:ref.count], host_wrappers(rewards, dones, raws), raws, dones) == ref.count
    lens = [int(r[3]) for r in ref.records]
    assert min(lens) == 1 and max(lens) > 15


def test_float32_return_is_numpys_inplace_add():
    """ret = (float)((double)ret + reward): what `float32_array += float64_array` computes, and not
    the float32 sum of the float32-rounded reward."""
    a = np.array([0.1], np.float32)
    r = np.array([1e-9 + 1.0 / 3.0])
    b = a.copy()
    b += r
    ref = EpisodeStatsRef(1)
    ref.ret[:] = a
    ref.update(r, [False], np.zeros((1, 6)))
    assert ref.ret[0] == b[0]
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000)
    assert ((x.astype(np.float64) + y).astype(np.float32) != x + y.astype(np.float32)).any()


@pytest.mark.parametrize("use_gae", [True, False])
def test_numpy_gae_equals_the_reference_torch_loop(use_gae):
    import torch

    for T, N, seed in ((37, 129, 5), (1, 3, 6), (2, 1, 7)):
        r, v, d, lv, ld = gae_inputs(T, N, seed, ends=[(0, 0), (T - 1, N - 1), (T, N // 2)])
        adv, ret = gae_ref(r, v, d, lv, ld, 0.99, 0.95, use_gae)
        ta, tr = gae_torch_loop(*(torch.from_numpy(x) for x in (r, v, d, lv, ld)), 0.99, 0.95, use_gae)
        assert ta.dtype == torch.float32 and tr.dtype == torch.float32
        np.testing.assert_array_equal(adv.view(np.int32), ta.numpy().view(np.int32))
        np.testing.assert_array_equal(ret.view(np.int32), tr.numpy().view(np.int32))
        # bool dones read as float32 give the same bits
        a2, r2 = gae_ref(r, v, d.astype(bool), lv, ld.astype(bool), 0.99, 0.95, use_gae)
        np.testing.assert_array_equal(adv.view(np.int32), a2.view(np.int32))
        np.testing.assert_array_equal(ret.view(np.int32), r2.view(np.int32))


def test_ring_arithmetic():
    from gym_microrts import rollout

    span = rollout.ring_span
    assert span(0, 0, 4) == (0, 0, [])
    assert span(0, 3, 4) == (0, 0, [(0, 3)])
    assert span(3, 6, 4) == (3, 0, [(3, 4), (0, 2)])            # wraps
    assert span(0, 4, 4) == (0, 0, [(0, 4)])
    assert span(0, 10, 4) == (6, 6, [(2, 4), (0, 2)])           # 10 finished, 4 rows: the oldest 6 lost
    assert span(6, 10, 4) == (6, 0, [(2, 4), (0, 2)])
    assert span(2, 13, 4) == (9, 7, [(1, 4), (0, 1)])
    assert span(5, 5, 4) == (5, 0, [])
    assert span(8, 12, 4) == (8, 0, [(0, 4)])
    with pytest.raises(ValueError):
        span(5, 4, 4)
    # against a ring filled the contract's way, every (drained, count) pair
    cap = 5
    for count in range(0, 23):
        ring = np.full(cap, -1)
        for k in range(count):
            ring[k % cap] = k
        for drained in range(0, count + 1):
            first, dropped, slices = span(drained, count, cap)
            got = [int(x) for a, b in slices for x in ring[a:b]]
            assert got == list(range(first, count)) and dropped == first - drained == max(0, count - drained - cap)
    # the numpy contract's ring, read through ring_span after 10 finishes into 4 rows, two drains
    ref = EpisodeStatsRef(3, 0.99, capacity=4)
    done_at = {0: [0], 1: [1, 2], 2: [0, 1, 2], 4: [2], 5: [0, 1], 6: [1]}
    drained, seen = 0, []
    for t in range(8):
        d = np.zeros(3, bool)
        d[done_at.get(t, [])] = True
        ref.update(np.ones(3), d, np.ones((3, 6)))
        if t in (3, 7):
            first, dropped, slices = span(drained, ref.count, 4)
            rows = np.concatenate([ref.ring[a:b] for a, b in slices])
            np.testing.assert_array_equal(rows, np.array(ref.records[first:ref.count]))
            seen.append((first, dropped, len(rows)))
            drained = ref.count
    assert ref.count == 10 and seen == [(2, 2, 4), (6, 0, 4)]
    recs = rollout.records_of(ref.ring, NAMES)
    assert set(recs[0]) == {"env", "step", "episode", "microrts_stats"} and len(recs[0]["microrts_stats"]) == 13
    assert list(recs[0]["microrts_stats"])[6:] == ["discounted_" + k for k in NAMES] + ["discounted"]
    # one call that ends more episodes than the ring holds keeps its last `capacity`
    ref = EpisodeStatsRef(7, 0.99, capacity=3)
    ref.update(np.ones(7), np.ones(7, bool), np.ones((7, 6)))
    first, dropped, slices = span(0, ref.count, 3)
    assert (first, dropped) == (4, 4) and [int(x) for a, b in slices for x in ref.ring[a:b, 0]] == [4, 5, 6]


def test_layout_matches_the_library():
    from gym_microrts import _native, rollout

    L = _native.lib()
    for n, cap in ((1, 1), (3, 4), (63, 1024), (1025, 7), (8192, 32768)):
        lay = rollout.layout(n, cap)
        assert L.mrts_episode_stats_bytes(n, cap) == lay["bytes"]
        assert lay["ring"] % 16 == 0 and lay["ring"] >= 32 + 120 * n and lay["bytes"] == lay["ring"] + cap * ROW * 8
        assert lay["factor"] % 8 == 0 and lay["rawsum"] % 8 == 0 and lay["disc"] % 8 == 0
    assert rollout.ROW == ROW == _native.MRTS_EPISODE_RECORD_DOUBLES


def test_entry_points_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: null pointers, N < 1, T < 1, capacity < 1, a bad
    done_elem / mode, step < 0, a misaligned state or element pointer."""
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    EINVAL = -1
    assert L.mrts_episode_stats_bytes(0, 4) == EINVAL and L.mrts_episode_stats_bytes(4, 0) == EINVAL
    assert L.mrts_episode_stats_bytes(-1, 4) == EINVAL and L.mrts_episode_stats_bytes(4, -3) == EINVAL
    assert L.mrts_episode_stats_bytes(2, 3) == ((32 + 240 + 15) & ~15) + 3 * 144

    def init(state=p, n=4, cap=4):
        return L.mrts_episode_stats_init(None, state, n, cap)

    assert init(state=None) == EINVAL and init(state=p + 8) == EINVAL and init(n=0) == EINVAL and init(cap=0) == EINVAL

    def update(state=p, n=4, cap=4, step=0, reward=p, done0=p, raw=p):
        return L.mrts_episode_stats_update(None, state, n, cap, 0.99, step, reward, done0, raw)

    for name in ("state", "reward", "done0", "raw"):
        assert update(**{name: None}) == EINVAL, name
    assert update(state=p + 8) == EINVAL and update(state=p + 4) == EINVAL
    assert update(reward=p + 4) == EINVAL and update(raw=p + 4) == EINVAL
    assert update(n=0) == EINVAL and update(n=-5) == EINVAL and update(cap=0) == EINVAL and update(step=-1) == EINVAL

    def gae(T=2, N=3, rewards=p, values=p, dones=p, elem=0, last_value=p, last_done=p, mode=0, adv=p, ret=p):
        return L.mrts_gae(None, T, N, rewards, values, dones, elem, last_value, last_done, 0.99, 0.95, mode, adv, ret)

    for name in ("rewards", "values", "dones", "last_value", "last_done", "adv", "ret"):
        assert gae(**{name: None}) == EINVAL, name
        if name not in ("dones", "last_done"):
            assert gae(**{name: p + 2}) == EINVAL, name
    assert gae(T=0) == EINVAL and gae(N=0) == EINVAL and gae(T=-1) == EINVAL and gae(N=-1) == EINVAL
    for bad in (-1, 2, 7):
        assert gae(elem=bad) == EINVAL and gae(mode=bad) == EINVAL
    assert gae(dones=p + 2) == EINVAL and gae(last_done=p + 1) == EINVAL    # float32 dones: 4-byte aligned
    del buf


def test_module_checks_its_inputs():
    """Type, dtype, shape and layout of every tensor, then the device: a CPU tensor is an error."""
    import torch

    from gym_microrts import rollout

    T, n = 3, 4
    r, v, d = torch.zeros(T, n), torch.zeros(T, n), torch.zeros(T, n)
    lv, ld = torch.zeros(n), torch.zeros(n)
    wide = torch.zeros(T, 2 * n)
    with pytest.raises(ValueError, match="rewards is on cpu"):
        rollout.gae(r, v, d, lv, ld)
    with pytest.raises(ValueError, match="rewards is on cpu"):
        rollout.gae(r, v, d.bool(), lv, ld.bool(), out=(torch.zeros(T, n), torch.zeros(T, n)))
    with pytest.raises(ValueError, match="must be a torch.Tensor"):
        rollout.gae(r.numpy(), v, d, lv, ld)
    with pytest.raises(ValueError, match="values must be a torch.Tensor"):
        rollout.gae(r, v.numpy(), d, lv, ld)
    with pytest.raises(ValueError, match="rewards must be torch.float32"):
        rollout.gae(r.double(), v, d, lv, ld)
    with pytest.raises(ValueError, match=r"rewards must be \[T, N\]"):
        rollout.gae(r[0], v, d, lv, ld)
    with pytest.raises(ValueError, match=r"rewards must be \[T, N\]"):
        rollout.gae(r[:0], v, d, lv, ld)
    with pytest.raises(ValueError, match=r"values must be \[3, 4\]"):
        rollout.gae(r, v[:2], d, lv, ld)
    with pytest.raises(ValueError, match="dones must be torch.float32 or torch.bool or torch.uint8"):
        rollout.gae(r, v, d.long(), lv, ld)
    with pytest.raises(ValueError, match="last_done must be torch.bool or torch.uint8"):   # dones and last_done: one kind
        rollout.gae(r, v, d.bool(), lv, ld)
    with pytest.raises(ValueError, match="last_done must be torch.float32"):
        rollout.gae(r, v, d, lv, ld.bool())
    with pytest.raises(ValueError, match=r"last_value must be \[4\]"):
        rollout.gae(r, v, d, lv.reshape(1, n), ld)
    with pytest.raises(ValueError, match="rewards must be contiguous"):
        rollout.gae(wide[:, ::2], v, d, lv, ld)
    with pytest.raises(ValueError, match="dones must be contiguous"):
        rollout.gae(r, v, wide[:, ::2], lv, ld)
    with pytest.raises(ValueError, match=r"out\[1\] must be \[3, 4\]"):
        rollout.gae(r, v, d, lv, ld, out=(torch.zeros(T, n), torch.zeros(T, n + 1)))
    with pytest.raises(ValueError, match=r"out\[0\] must be contiguous"):
        rollout.gae(r, v, d, lv, ld, out=(wide[:, ::2], torch.zeros(T, n)))
    with pytest.raises(ValueError, match="device is cpu"):
        rollout.EpisodeStats(4, NAMES, device="cpu")
    with pytest.raises(ValueError, match="names must hold the 6"):
        rollout.EpisodeStats(4, NAMES[:5])
    with pytest.raises(ValueError, match="num_envs must be >= 1"):
        rollout.EpisodeStats(0, NAMES)
    with pytest.raises(ValueError, match="capacity must be >= 1"):
        rollout.EpisodeStats(4, NAMES, capacity=0)
    rew, done, raw = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bool), torch.zeros(n, 6, dtype=torch.float64)
    with pytest.raises(ValueError, match="reward is on cpu"):
        rollout.check_update(n, rew, done, raw)
    with pytest.raises(ValueError, match="reward is on cpu"):
        rollout.check_update(n, rew, done.to(torch.uint8), raw)
    with pytest.raises(ValueError, match="reward must be torch.float64"):
        rollout.check_update(n, rew.float(), done, raw)
    with pytest.raises(ValueError, match=r"reward must be \[5\]"):
        rollout.check_update(5, rew, done, raw)
    with pytest.raises(ValueError, match="done must be torch.bool or torch.uint8"):
        rollout.check_update(n, rew, done.float(), raw)
    with pytest.raises(ValueError, match=r"raw must be \[4, 6\]"):
        rollout.check_update(n, rew, done, raw[:, :5])
    with pytest.raises(ValueError, match="raw must be contiguous"):
        rollout.check_update(n, rew, done, torch.zeros(n, 12, dtype=torch.float64)[:, ::2])
    with pytest.raises(ValueError, match="must be a torch.Tensor"):
        rollout.check_update(n, rew.numpy(), done, raw)

    class Infos:   # what step() returns: a LazyInfos contributes its _raw, unread
        _raw = raw[:, :5]

    with pytest.raises(ValueError, match=r"raw must be \[4, 6\]"):
        rollout.check_update(n, rew, done, Infos())


def test_driver_refuses_device_bookkeeping_without_the_tensor_api():
    drv = load_driver()
    with pytest.raises(ValueError, match="--bookkeeping device needs --api tensor"):
        drv.run(bookkeeping="device", api="numpy", device="no-such-device")   # raised before the device is touched
    with pytest.raises(ValueError, match="--bookkeeping device needs --api tensor"):
        drv.run(bookkeeping="device", api="hybrid", device="no-such-device")
    with pytest.raises(ValueError, match="bookkeeping must be"):
        drv.run(bookkeeping="gpu", device="no-such-device")
