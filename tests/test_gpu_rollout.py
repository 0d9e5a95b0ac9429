"""The rollout bookkeeping on the MI355X (csrc/mrts_rollout.hip, gym_microrts.rollout), every
comparison with the contract bit-exact: k_gae against rollout_ref.gae_ref and against the
reference's torch loop run on the device; k_episode_update's state and records against
rollout_ref.EpisodeStatsRef; EpisodeStats fed a stepped engine's tensors against the host wrappers
fed host copies of them; the driver's run() and evaluate() with bookkeeping="device" against
their host arms."""
import numpy as np
import pytest

from rollout_ref import ROW, EpisodeStatsRef, gae_inputs, gae_ref, gae_torch_loop
from test_rollout import NAMES, RW, compare_with_wrappers, host_wrappers, load_driver, streams

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

M8 = "maps/8x8/basesWorkers8x8.xml"


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------ k_gae
@pytest.mark.parametrize("N", [1, 63, 65, 257, 1025])
@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_gae_equals_the_contract_and_the_torch_loop(T, N):
    """Both modes, dones as float32 and as bool, episode ends at t = 0, at t = T - 1 and in
    last_done, results into fresh tensors and into `out=` buffers (with guard rows around them)."""
    import torch

    from gym_microrts import rollout

    r, v, d, lv, ld = gae_inputs(T, N, 100 * T + N, ends=[(0, 0), (T - 1, N - 1), (T, N // 2), (0, N - 1), (T - 1, 0)])
    gr, gv, gd, glv, gld = (dev(x) for x in (r, v, d, lv, ld))
    for use_gae in (True, False):
        want_a, want_r = gae_ref(r, v, d, lv, ld, 0.99, 0.95, use_gae)
        ta, tr = gae_torch_loop(gr, gv, gd, glv, gld, 0.99, 0.95, use_gae)
        assert np.array_equal(bits(ta), want_a.view(np.int32)) and np.array_equal(bits(tr), want_r.view(np.int32)), "torch loop on the device"
        a, rt = rollout.gae(gr, gv, gd, glv, gld, 0.99, 0.95, use_gae)
        assert a.shape == (T, N) and a.dtype == torch.float32 and rt.shape == (T, N) and rt.dtype == torch.float32
        assert np.array_equal(bits(a), want_a.view(np.int32)), ("advantages", use_gae)
        assert np.array_equal(bits(rt), want_r.view(np.int32)), ("returns", use_gae)
        big = torch.full((2, T + 2, N), -7.0, device="cuda")
        out = (big[0, 1:T + 1], big[1, 1:T + 1])
        a2, r2 = rollout.gae(gr, gv, gd.bool(), glv, gld.bool(), 0.99, 0.95, use_gae, out=out)
        assert a2 is out[0] and r2 is out[1]
        assert np.array_equal(bits(a2), want_a.view(np.int32)) and np.array_equal(bits(r2), want_r.view(np.int32)), ("bool dones, out=", use_gae)
        assert bool((big[:, 0] == -7).all()) and bool((big[:, T + 1] == -7).all()), "guard rows"
        a3, _ = rollout.gae(gr, gv, gd.to(torch.uint8), glv, gld.to(torch.uint8), 0.99, 0.95, use_gae)
        assert np.array_equal(bits(a3), want_a.view(np.int32)), ("uint8 dones", use_gae)
    # another gamma / lambda: g = (float)gamma, gl = (float)(gamma * lambda), the product in double
    want_a, want_r = gae_ref(r, v, d, lv, ld, 0.97, 0.9, True)
    a, rt = rollout.gae(gr, gv, gd, glv, gld, 0.97, 0.9)
    assert np.array_equal(bits(a), want_a.view(np.int32)) and np.array_equal(bits(rt), want_r.view(np.int32))


# ------------------------------------------------------------------ k_episode_update
def update_streams(N, calls=40, seed=0):
    """Real-valued raw rewards; call 5: no env ends, 6: every env ends, 7: env 0 alone, 8: env N - 1
    alone, 9: none again (so 7 and 8 end episodes of length 1 and 2 in those envs)."""
    rewards, dones, raws = streams(calls, N, 1000 + N + seed, p=0.1)
    dones[5] = dones[7] = dones[8] = dones[9] = False
    dones[6] = True
    dones[7, 0] = dones[8, N - 1] = True
    return rewards, dones, raws


def state_equal(stats, ref):
    st = {k: v.cpu().numpy() for k, v in stats.state().items()}
    assert np.array_equal(st["ret"].view(np.int32), ref.ret.view(np.int32)), "ret"
    assert np.array_equal(st["len"], ref.len), "len"
    for k in ("factor", "rawsum", "disc"):
        assert np.array_equal(st[k].view(np.int64), getattr(ref, k).view(np.int64)), k


@pytest.mark.parametrize("N", [1, 63, 65, 1023, 1025, 2049])
def test_episode_update_equals_the_contract(N):
    """40 calls: the running state after calls 8, 20 and 39 and every record, bit for bit; drains
    after several updates each (records in the reference's scan order); 1023 / 1025 / 2049 envs
    span 4, 5 and 9 workgroups of the cross-block count.  A second run gives the same bytes."""
    import torch

    from gym_microrts import rollout

    rewards, dones, raws = update_streams(N)
    ref = EpisodeStatsRef(N, 0.99)
    stats = rollout.EpisodeStats(N, NAMES, gamma=0.99)
    twin = rollout.EpisodeStats(N, NAMES, gamma=0.99)
    assert stats.capacity == max(4 * N, 1024) == ref.capacity
    state_equal(stats, ref)
    g = [(dev(rewards[t]), dev(dones[t]), dev(raws[t])) for t in range(len(rewards))]
    got, drained = [], 0
    for t, (rew, done, raw) in enumerate(g):
        ref.update(rewards[t], dones[t], raws[t])
        stats.update(rew, done if t % 2 else done.to(torch.uint8), raw)
        if t in (8, 20, 39):
            state_equal(stats, ref)
        if t in (4, 6, 13, 27, 39):
            rows = stats.drain_rows()
            want = np.array(ref.records[drained:ref.count]).reshape(-1, ROW)
            assert rows.shape == want.shape and np.array_equal(rows.view(np.int64), want.view(np.int64)), f"records drained after call {t}"
            drained = ref.count
            got.append(len(rows))
    assert stats.dropped == 0 and stats.steps == 40 and sum(got) == ref.count == int(dones.sum())
    assert got[0] + got[1] >= N and got[1] >= N   # call 6 ended every env
    assert stats.drain() == [] and stats.dropped == 0
    for rew, done, raw in g:
        twin.update(rew, done, raw)
    assert torch.equal(twin._buf, stats._buf), "two identical runs, identical bytes"
    # the ring holds record k in row k % capacity
    ring = stats._ring.cpu().numpy()
    for k in range(max(0, ref.count - ref.capacity), ref.count):
        assert np.array_equal(ring[k % ref.capacity].view(np.int64), ref.records[k].view(np.int64)), k
    stats.reset()
    state_equal(stats, EpisodeStatsRef(N, 0.99))
    assert stats.steps == 0 and int(stats._buf[:2].abs().sum()) == 0 and not bool(stats._ring.any())


@pytest.mark.parametrize("N,offset", [(65, 1), (1025, 3), (1031, 4), (600, 8)])
def test_episode_update_with_a_done_tensor_off_its_allocation_base(N, offset):
    """`done` as a slice of a longer byte tensor (contiguous, so it passes the module's check): at
    offsets 1, 3 and 4 the kernel counts the done bytes one by one, at 8 with 8-byte loads and a
    tail.  State and records equal the contract's over 12 calls, and the bytes around the slice
    are left alone."""
    import torch

    from gym_microrts import rollout

    rewards, dones, raws = update_streams(N, calls=12, seed=offset)
    ref = EpisodeStatsRef(N, 0.99)
    stats = rollout.EpisodeStats(N, NAMES, gamma=0.99)
    held = torch.zeros(offset + N + 9, dtype=torch.bool, device="cuda")
    held[:offset] = True      # set bytes just outside the slice must not be counted
    held[offset + N:] = True
    done = held[offset:offset + N]
    assert done.is_contiguous() and done.data_ptr() % 8 == offset % 8
    for t in range(12):
        ref.update(rewards[t], dones[t], raws[t])
        done.copy_(dev(dones[t]))
        stats.update(dev(rewards[t]), done, dev(raws[t]))
    state_equal(stats, ref)
    rows = stats.drain_rows()
    want = np.array(ref.records).reshape(-1, ROW)
    assert rows.shape == want.shape and np.array_equal(rows.view(np.int64), want.view(np.int64))
    assert bool(held[:offset].all()) and bool(held[offset + N:].all())


def test_small_ring_wraps_and_counts_what_it_dropped():
    """capacity 4, 10 finishes, two drains: the first sees 6 finishes and keeps the last 4, the
    second the next 4 in order; records_of's keys; then one call that ends 7 episodes into 3 rows."""
    from gym_microrts import rollout

    ref = EpisodeStatsRef(3, 0.99, capacity=4)
    stats = rollout.EpisodeStats(3, NAMES, gamma=0.99, capacity=4)
    done_at = {0: [0], 1: [1, 2], 2: [0, 1, 2], 4: [2], 5: [0, 1], 6: [1]}
    rng = np.random.default_rng(9)
    seen = []
    for t in range(8):
        d = np.zeros(3, bool)
        d[done_at.get(t, [])] = True
        raw = rng.standard_normal((3, 6))
        rew = raw @ RW
        ref.update(rew, d, raw)
        stats.update(dev(rew), dev(d), dev(raw))
        if t in (3, 7):
            recs = stats.drain()
            want = rollout.records_of(np.array(ref.records[ref.count - 4:ref.count]), NAMES)
            assert recs == want
            seen.append((len(recs), stats.dropped, [(r["step"], r["env"]) for r in recs]))
    assert ref.count == 10
    assert seen == [(4, 2, [(1, 2), (2, 0), (2, 1), (2, 2)]), (4, 2, [(4, 2), (5, 0), (5, 1), (6, 1)])]
    assert set(recs[0]) == {"env", "step", "episode", "microrts_stats"} and set(recs[0]["episode"]) == {"r", "l"}
    assert list(recs[0]["microrts_stats"]) == NAMES + ["discounted_" + k for k in NAMES] + ["discounted"]
    assert np.array_equal(stats._ring.cpu().numpy().view(np.int64), ref.ring.view(np.int64))
    ref = EpisodeStatsRef(7, 0.99, capacity=3)
    stats = rollout.EpisodeStats(7, NAMES, gamma=0.99, capacity=3)
    raw = rng.standard_normal((7, 6))
    ref.update(raw @ RW, np.ones(7, bool), raw)
    stats.update(dev(raw @ RW), dev(np.ones(7, bool)), dev(raw))
    recs = stats.drain()
    assert [r["env"] for r in recs] == [4, 5, 6] and stats.dropped == 4
    assert np.array_equal(stats._ring.cpu().numpy().view(np.int64), ref.ring.view(np.int64))


# ------------------------------------------------------------------ with the engine
def test_episode_stats_on_a_stepped_engine_equal_the_host_wrappers():
    """4 selfplay + 2 workerRushAI envs of 8x8, max_steps 16, 80 steps under the stand-in sampler:
    EpisodeStats is fed the tensor contract's outputs as they are; the compat VecMonitor and the
    driver's StatsRecorder are fed host copies of the same tensors.  Exact on order, r, l and the
    raw sums; the discounted sums within rollout_ref.discount_bound."""
    import ctypes

    import torch

    from gym_microrts import _native, microrts_ai, rollout
    from gym_microrts.envs.vec_env import LazyInfos, MicroRTSGridModeVecEnv

    env = MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=2, max_steps=16, ai2s=[microrts_ai.workerRushAI] * 2,
                                 map_paths=[M8], reward_weight=RW, return_tensors=True)
    assert [str(rf) for rf in env.rfs] == NAMES
    stats = rollout.EpisodeStats.for_env(env, 0.99)
    assert stats.num_envs == 6 and stats.names == NAMES and stats.capacity == 1024 and stats.device == env._rew.device
    env.reset()
    act = torch.empty((6, 64, 7), dtype=torch.int64, device="cuda")
    rewards, dones, raws = [], [], []
    for s in range(80):
        env.get_action_mask()
        _native.check(_native.lib().mrts_sample_actions_src(env._stream(), env._mask.data_ptr(), env._src.data_ptr(), 6, 64, 0,
                                                            ctypes.c_uint64(23), s, act.data_ptr()))
        _, rew, done, infos = env.step(act)
        assert isinstance(infos, LazyInfos) and infos._np is None
        stats.update(rew, done, infos)
        assert infos._np is None, "update materialised the infos"
        rewards.append(rew.cpu().numpy().copy())
        dones.append(done.cpu().numpy().copy())
        raws.append(infos._raw.cpu().numpy().copy())
    assert env.error_flags() == 0
    rewards, dones, raws = np.array(rewards), np.array(dones), np.array(raws)
    rows = stats.drain_rows()
    env.close()
    host = host_wrappers(rewards, dones, raws)
    assert len(host) >= 6 * 4 and len(rows) == len(host)   # max_steps 16: every env resets at least four times
    assert compare_with_wrappers(rows, host, raws, dones) == len(host)
    assert np.abs(rows[:, 4:17]).sum() > 0
    # and the contract itself, bit for bit, on the engine's streams
    ref = EpisodeStatsRef(6, 0.99)
    for t in range(80):
        ref.update(rewards[t], dones[t], raws[t])
    assert np.array_equal(rows.view(np.int64), np.array(ref.records).view(np.int64))
    state_equal(stats, ref)


# ------------------------------------------------------------------ the driver
def test_driver_with_device_bookkeeping():
    """2 updates x 8 steps with max_steps 8: episodes are reported, every one with its
    microrts_stats, the losses are finite; and under one seed the first rollout's actions equal the
    host arm's: bookkeeping does not touch the rollout."""
    import torch

    drv = load_driver()
    out = {}
    for bk in ("device", "host"):
        out[bk] = drv.run(num_selfplay_envs=4, num_bot_envs=0, num_steps=8, updates=2, api="tensor", head="fused", max_steps=8,
                          bookkeeping=bk, keep_first_rollout=True, log=lambda s: None)
        assert out[bk]["finite"] and out[bk]["engine_error_flags"] == 0, bk
    d, h = out["device"], out["host"]
    assert d["episodes"] > 0 and d["microrts_stats_infos"] == d["episodes"] and d["bookkeeping"] == "device"
    assert d["episodes"] == h["episodes"] and h["microrts_stats_infos"] == 0
    assert torch.equal(d["first_rollout"]["actions"], h["first_rollout"]["actions"])
    assert torch.equal(d["first_rollout"]["obs"], h["first_rollout"]["obs"])


@pytest.mark.parametrize("ai", ["", "coacAI"])
def test_driver_evaluate_with_device_bookkeeping_tallies_what_the_host_arm_does(ai):
    """evaluate() under one seed with max_steps 16, 2 x 16 steps: every game ends by its time limit
    twice, and the device arm (tensor contract, EpisodeStats drained once per 16 steps) logs the
    same WinLoss lines in the same order and returns the same records as the wrappers' arm."""
    drv = load_driver()
    out, lines = {}, {}
    for bk in ("host", "device"):
        lines[bk] = []
        out[bk] = drv.evaluate(ai=ai, num_steps=16, total_timesteps=32 * (1 if ai else 2), log=lines[bk].append, render=False,
                               bookkeeping=bk, max_steps=16)
        assert out[bk]["engine_error_flags"] == 0, bk
    assert out["host"]["results"] and out["device"]["results"] == out["host"]["results"]
    assert lines["device"] == lines["host"] and len(lines["host"]) == len(out["host"]["results"])
    assert out["device"]["global_step"] == out["host"]["global_step"]
    with pytest.raises(ValueError, match="bookkeeping must be"):
        drv.evaluate(bookkeeping="gpu", device="no-such-device")
