"""Packed observations on the MI355X, every comparison bit-exact: an engine of
obs_format="packed" in lock-step with the oracle and with a dense float32 twin, every launch
that writes obs, the grouped and size-cycling envs, the converters (k_unpack_obs /
k_pack_obs) against the numpy reference, and the driver's packed rollout buffer.  The
format and its numpy statement (pack_obs_ref / unpack_obs_ref): test_packed_obs.py.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import MAPS, REPO, obs_bits_equal
from random_maps import write_random_map
from test_packed_obs import pack_obs_ref, unpack_obs_ref

pytestmark = pytest.mark.gpu

RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"
M16A = "maps/16x16/basesWorkers16x16A.xml"


def _torch():
    import torch

    return torch


def bits(x):
    torch = _torch()
    return x.view(torch.int16) if x.element_size() == 2 else x if x.dtype == torch.int32 else x.view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and _torch().equal(bits(a), bits(b))


def words_equal_dense(pk, dense, tag):
    """A packed env's obs against its dense float32 twin's, both ways through the converters."""
    torch = _torch()
    from gym_microrts import packed_obs

    P = dense.shape[-1]
    assert pk.dtype == torch.int32 and pk.shape == dense.shape[:-1] and pk.is_cuda, tag
    assert torch.equal(packed_obs.pack_obs(dense), pk), f"{tag}: pack_obs(twin obs) != packed obs"
    assert same_bits(packed_obs.unpack_obs(pk, P), dense), f"{tag}: unpack_obs(packed obs) != twin obs"
    assert not bool((pk >> P).any()), f"{tag}: a bit at or above {P}"   # (an arithmetic shift: bit 31 would show too)


# ------------------------------------------------------------------ 1. the engine in lock-step
#         name             map (None: random w x h)  w   h   bots   partial fusion
ENGINE = [("8x8",          M8,                       8,  8,  True,  False, True),    # HW = 64: the 64-lane step; fused with bots: 128 lanes
          ("9x13_random",  None,                     9,  13, True,  False, True),    # HW % 4 != 0: the per-word path
          ("16x16",        M16,                      16, 16, True,  False, True),
          ("16x16_fog",    M16,                      16, 16, True,  True,  True),    # P = 31: bits 29 / 30
          ("24x24",        M24,                      24, 24, True,  False, True),    # several cells per lane
          ("47x24_random", None,                     47, 24, False, False, True),    # the unprefetched boundary shape, no bots
          ("16x16_unfused", M16,                     16, 16, True,  False, False)]   # bot_fusion=False: k_bot + the unfused step


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,rel,w,h,bots,partial,fusion", ENGINE, ids=[c[0] for c in ENGINE])
def test_packed_engine_lockstep_with_the_oracle_and_a_dense_twin(tmp_path, name, rel, w, h, bots, partial, fusion):
    """40 ticks, 4 selfplay envs + (workerRush, coacAI) bot envs where the size allows bots,
    max_steps 25 (auto-resets inside).  Every tick the packed obs equals pack_obs_ref of the
    oracle's obs, has no bit at or above P, equals pack_obs of a dense float32 twin env's obs
    and unpacks to that obs bit for bit; masks, source, rewards and dones equal the twin's."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import OracleVecEnv, sample_actions

    if rel is None:
        path = gpath = write_random_map(str(tmp_path / f"{name}.xml"), w, h, 5, n_units=60 if w * h > 200 else 24, wall_frac=0.1)
    else:
        path, gpath = os.path.join(MAPS, rel), rel
    ais = ["workerRushAI", "coacAI"] if bots else []
    P = 31 if partial else 29

    def engine(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=len(ais), max_steps=25, partial_obs=partial,
                                      ai2s=[getattr(microrts_ai, a) for a in ais], map_paths=[gpath], reward_weight=RW,
                                      return_tensors=True, bot_fusion=fusion, **kw)

    g, twin = engine(obs_format="packed"), engine(obs_dtype=torch.float32)
    assert g.obs_format == "packed" and twin.obs_format == "dense" and g.observation_space.shape == (h, w, P)
    o = OracleVecEnv(4, len(ais), [path], max_steps=25, partial_obs=partial, ai2s=ais or None, reward_weight=RW)
    pk, dense, oo = g.reset(), twin.reset(), o.reset()
    for s in range(41):
        tag = f"tick {s}"
        assert pk.shape == (g.num_envs, h, w)
        got, want = pk.cpu().numpy(), pack_obs_ref(oo)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{tag}: {len(bad)} words differ from the oracle, first (env, y, x) {bad[:8].tolist()}")
        assert not (got.view(np.uint32) >> P).any(), f"{tag}: a bit at or above {P}"
        assert obs_bits_equal(dense, oo), f"{tag}: the twin's obs"
        words_equal_dense(pk, dense, tag)
        mo = o.get_action_mask()
        assert torch.equal(g.get_action_mask(), twin.get_action_mask()) and torch.equal(g.source_unit_mask, twin.source_unit_mask), tag
        assert torch.equal(g.get_action_mask().cpu(), torch.from_numpy(mo)), f"{tag}: masks against the oracle"
        if s == 40:
            break
        a = sample_actions(mo, 17, s)
        at = torch.from_numpy(a).to(g.device)
        (pk, rew, done, infos), (dense, rew2, done2, infos2) = g.step(at), twin.step(at)
        oo = o.step(a)[0]
        assert torch.equal(rew, rew2) and torch.equal(done, done2) and torch.equal(infos._raw, infos2._raw), f"{tag}: rewards / dones"
    assert int(g.game_stats()[:, 5].sum()) > 0, "no auto-reset in the rollout"
    assert g.error_flags() == 0 and twin.error_flags() == 0
    g.close(), twin.close(), o.close()


# ------------------------------------------------------------------ 2. every obs writer
@pytest.mark.timeout(120)
def test_every_obs_writer_writes_the_words():
    """Right after reset, steps, reset_games, park_games (the parked envs read the zero word,
    the others do not), an unpark, set_state (the obs at the save) and map cycling: the packed
    env against a dense float32 twin put through the same calls.  A packed state does not load
    into a dense env, nor a dense one into a packed env."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts._native import MicroRTSError
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import sample_actions

    def engine(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=8, num_bot_envs=2, max_steps=2000, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI],
                                      map_paths=[M16], reward_weight=RW, return_tensors=True, **kw)

    g, twin = engine(obs_format="packed"), engine(obs_dtype=torch.float32)
    tick = [0]

    def check(tag):
        words_equal_dense(g._obs, twin._obs, tag)
        assert torch.equal(g.get_action_mask(), twin.get_action_mask()), tag
        return g._obs

    def steps(n):
        for _ in range(n):
            a = torch.from_numpy(sample_actions(g.get_action_mask().cpu().numpy(), 23, tick[0])).to(g.device)
            g.step(a), twin.step(a)
            tick[0] += 1

    g._obs.fill_(-1)   # every launch below writes every word it owns
    assert g.reset() is g._obs and twin.reset() is twin._obs
    check("reset")
    steps(12)
    before = check("steps").clone()
    for e in (g, twin):
        e.reset_games([0, 3])
    after = check("reset_games")
    assert not torch.equal(before[0:2], after[0:2]) and torch.equal(before[2:6], after[2:6])
    steps(3)
    g._obs.fill_(-1)
    for e in (g, twin):
        e.park_games([1, 5])   # game 1 = envs 2, 3; game 5 = bot env 9
    pk = g._obs
    assert int(pk[[2, 3, 9]].abs().sum()) == 0 and bool((pk[[0, 1, 4, 5, 6, 7, 8]] == -1).all()), "park_games writes the parked envs' words only"
    steps(3)
    pk = check("parked, stepped")
    assert int(pk[[2, 3, 9]].abs().sum()) == 0 and bool((pk[[0, 1, 4, 8]] != 0).all())
    for e in (g, twin):
        e.reset_games([1])
    pk = check("unpark")
    assert bool((pk[[2, 3]] != 0).all()) and int(pk[9].abs().sum()) == 0
    snap, snap_twin = g.get_state(), twin.get_state()
    saved = pk.clone()
    steps(8)
    assert not torch.equal(check("after the save"), saved)
    out = g.set_state(snap)
    twin.set_state(snap_twin)
    assert out is g._obs and torch.equal(check("set_state"), saved)
    for env, other in ((g, snap_twin), (twin, snap)):
        kept = env._obs.clone()
        with pytest.raises(MicroRTSError, match="another configuration"):
            env.set_state(other)
        assert torch.equal(env._obs, kept)
    steps(2)
    check("on from the restored state")
    assert g.error_flags() == 0 and twin.error_flags() == 0
    g.close(), twin.close()

    # map cycling (reset_games on next(cycle_maps) inside step) with short episodes
    def cycling(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=2, max_steps=12, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI],
                                      map_paths=[M16], cycle_maps=[M16A, "maps/16x16/basesWorkers16x16C.xml"], reward_weight=RW,
                                      return_tensors=True, **kw)

    g, twin = cycling(obs_format="packed"), cycling(obs_dtype=torch.float32)
    g.reset(), twin.reset()
    for s in range(30):
        a = torch.from_numpy(sample_actions(g.get_action_mask().cpu().numpy(), 29, s)).to(g.device)
        g.step(a), twin.step(a)
        words_equal_dense(g._obs, twin._obs, f"map cycling, tick {s}")
    assert g._game_map == twin._game_map and set(g._game_map) != {0}, "no game moved to a cycle map"
    g.close(), twin.close()


@pytest.mark.timeout(60)
def test_packed_obs_on_the_numpy_and_hybrid_contracts_and_the_dtype_check():
    torch = _torch()
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    def engine(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=2, num_bot_envs=0, max_steps=2000, map_paths=[M8], reward_weight=RW, **kw)

    e, d = engine(return_tensors=False, obs_format="packed"), engine(return_tensors=False)
    pk, dense = e.reset(), d.reset()
    assert isinstance(pk, np.ndarray) and pk.dtype == np.int32 and pk.shape == (2, 8, 8)
    np.testing.assert_array_equal(pk, pack_obs_ref(dense))
    a = np.zeros((2, 64 * 7), np.int64)
    pk, dense = e.step(a)[0], d.step(a)[0]
    assert isinstance(pk, np.ndarray) and pk.dtype == np.int32 and pk.shape == (2, 8, 8)
    np.testing.assert_array_equal(unpack_obs_ref(pk, 29), dense)
    e.close(), d.close()
    e = engine(return_tensors="hybrid", obs_format="packed", obs_dtype=torch.int32)
    pk = e.reset()
    assert torch.is_tensor(pk) and pk.is_cuda and pk.dtype == torch.int32 and pk.shape == (2, 8, 8) and e.obs_format == "packed"
    e.close()
    with pytest.raises(ValueError, match="obs_dtype must be None or torch.int32"):
        engine(return_tensors=True, obs_format="packed", obs_dtype=torch.float32)
    with pytest.raises(ValueError, match="obs_format must be"):
        engine(return_tensors=True, obs_format="bits")


# ------------------------------------------------------------------ 3. grouped and cycling envs
@pytest.mark.timeout(120)
def test_mixed_map_and_size_cycling_envs_pass_the_format_on():
    """MicroRTSMixedMapVecEnv (8x8 + 16x16 buckets in one grouped launch) and
    MicroRTSSizeCyclingVecEnv with obs_format="packed", ten ticks, each bucket against its
    dense twin; mrts_step_group refuses a group of a packed and a dense engine."""
    torch = _torch()
    from gym_microrts import _native, microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSMixedMapVecEnv, MicroRTSSizeCyclingVecEnv
    from oracle_py import sample_actions

    def mixed(**kw):
        return MicroRTSMixedMapVecEnv([dict(map_paths=[M8], num_selfplay_envs=4, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI]),
                                       dict(map_paths=[M16], num_selfplay_envs=2, ai2s=[microrts_ai.coacAI])],
                                      max_steps=2000, reward_weight=RW, return_tensors=True, **kw)

    def cycling(**kw):
        return MicroRTSSizeCyclingVecEnv(4, 2, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI], map_paths=[M8],
                                         cycle_maps=[M16, M8], max_steps=6, reward_weight=RW, **kw)

    for make in (mixed, cycling):
        g, twin = make(obs_format="packed"), make(obs_dtype=torch.float32)
        assert all(e.obs_format == "packed" for e in g.envs) and all(e.obs_format == "dense" for e in twin.envs)
        if make is mixed:
            assert g.grouped and g.launch_plan() == ([0, 0], 1)
        else:
            assert g.obs_format == "packed"
        obs, dense = g.reset(), twin.reset()
        for s in range(11):
            for k, (pk, dn) in enumerate(zip(obs, dense)):
                words_equal_dense(pk, dn, f"{make.__name__}, bucket {k}, tick {s}")
            masks = g.get_action_mask()
            acts = [torch.from_numpy(sample_actions(np.ascontiguousarray(m.cpu().numpy()), 31, s)).to(m.device) for m in masks]
            (obs, rew, done, _), (dense, rew2, done2, _) = g.step(acts), twin.step(acts)
            for x, y in zip(rew, rew2) if make is mixed else ((rew, rew2),):
                assert torch.equal(x, y)
        if make is cycling:
            assert (g.bucket == twin.bucket).all() and len(set(g.bucket.tolist())) == 2, "no env moved to the other size"
            assert any(int(o.abs().sum(dim=(1, 2)).eq(0).sum()) > 0 for o in obs), "a parked env reads zero words"
        else:   # a packed and a dense engine in one group
            e0, e1 = g.envs[0], twin.envs[1]
            for e, a in ((e0, acts[0]), (e1, acts[1])):
                e.step_async(a)
            before = e0._obs.clone(), e1._obs.clone()
            io = (_native.StepIO * 2)(e0._step_io(), e1._step_io())
            hs = (ctypes.c_void_p * 2)(e0._h, e1._h)
            for policy in (0, 1 | 4, 2):
                assert _native.lib().mrts_step_group(hs, 2, e0._stream(), io, policy) == -1
                assert b"packed and dense" in _native.lib().mrts_last_error(e0._h)
            torch.cuda.synchronize()
            assert torch.equal(e0._obs, before[0]) and torch.equal(e1._obs, before[1]), "a refused group steps nothing"
        assert g.error_flags() == 0 and twin.error_flags() == 0
        g.close(), twin.close()


# ------------------------------------------------------------------ 4. the converters
ROWS = [1, 117 * 3, 64 * 9 + 1, 256 * 5 + 1]   # one row; odd (the 2-byte tail); a lone row in a wave / in a workgroup behind several
_words = {}


def words(rows):
    """Random words with random bits at and above P too (shared by the cases of one row count)."""
    if rows not in _words:
        _words[rows] = np.random.default_rng(rows).integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return _words[rows]


@pytest.mark.timeout(60)
@pytest.mark.parametrize("dtype", ["int32", "float32", "float16", "bfloat16"])
@pytest.mark.parametrize("P", [29, 31])
def test_converters_equal_the_numpy_reference(P, dtype):
    """unpack_obs == unpack_obs_ref in every element type (a one is 1, 0x3f800000, 0x3c00 or
    0x3f80, a zero all-zero bits), into a destination pre-filled with -1, 16-byte aligned and
    off by one element (the per-element path); pack_obs(unpack_obs(w)) == w & ((1 << P) - 1);
    pack_obs counts any non-zero element, -0.0 as zero; zero rows launch nothing."""
    torch = _torch()
    from gym_microrts import _native, packed_obs

    dt = getattr(torch, dtype)
    one = {"int32": 1, "float32": 0x3f800000, "float16": 0x3c00, "bfloat16": 0x3f80}[dtype]
    idt = torch.int16 if dt.itemsize == 2 else torch.int32
    for rows in ROWS:
        w = words(rows)
        wd = torch.from_numpy(w).cuda().reshape(1, rows)
        ref01 = unpack_obs_ref(w, P)
        want = torch.from_numpy(ref01 * one).to(idt).cuda().reshape(1, rows, P)
        got = packed_obs.unpack_obs(wd, P, dtype=dt)
        assert got.dtype == dt and got.shape == (1, rows, P)
        assert torch.equal(got.view(idt), want), f"{rows} rows"
        for off in (0, 1):   # a view 16-byte aligned, and one an element off it
            big = torch.full((rows * P + 16,), -1, dtype=idt, device="cuda").view(dt)
            base = (-big.data_ptr() // dt.itemsize) % (16 // dt.itemsize) + off
            assert (big[base:].data_ptr() % 16 == 0) == (off == 0)
            out = big[base:base + rows * P].view(1, rows, P)
            assert packed_obs.unpack_obs(wd, P, dtype=dt, out=out) is out
            assert torch.equal(out.view(idt), want), f"{rows} rows, offset {off}"
            guard = big.view(idt)
            assert bool((guard[:base] == -1).all()) and bool((guard[base + rows * P:] == -1).all()), f"{rows} rows, offset {off}: guards"
        back = packed_obs.pack_obs(got)
        assert back.dtype == torch.int32 and back.shape == (1, rows)
        np.testing.assert_array_equal(back.cpu().numpy().reshape(-1).view(np.uint32), w.view(np.uint32) & np.uint32((1 << P) - 1))
        # any non-zero element counts; -0.0 does not
        vals = torch.from_numpy(np.random.default_rng(7).integers(1, 100, (1, rows, P))).cuda()
        other = (got != 0) * (vals if dtype == "int32" else -vals.to(dt) / 8)
        if dtype != "int32":
            other = torch.where(got != 0, other, torch.tensor(-0.0, dtype=dt, device="cuda"))
        assert torch.equal(packed_obs.pack_obs(other.to(dt).contiguous()), back), f"{rows} rows: other non-zero values"
    # zero rows: MRTS_OK, nothing launched, nothing written
    L, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    g = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    assert L.mrts_unpack_obs(st, g.data_ptr(), 0, P, packed_obs.ELEM[dt], g.data_ptr()) == 0
    assert L.mrts_pack_obs(st, g.data_ptr(), 0, P, packed_obs.ELEM[dt], g.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((g == -1).all())
    assert packed_obs.unpack_obs(torch.empty((0, 4, 4), dtype=torch.int32, device="cuda"), P, dtype=dt).shape == (0, 4, 4, P)


@pytest.mark.timeout(60)
def test_module_checks_on_device_tensors():
    torch = _torch()
    from gym_microrts import packed_obs as po

    pk = torch.zeros(2, 4, 6, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="packed must be contiguous"):
        po.unpack_obs(pk.transpose(1, 2), 29)
    with pytest.raises(ValueError, match=r"packed must be \[\.\.\., H, W\]"):
        po.unpack_obs(pk.reshape(-1), 29)
    with pytest.raises(ValueError, match="out must be torch.float32"):
        po.unpack_obs(pk, 29, out=torch.zeros(2, 4, 6, 29, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        po.unpack_obs(pk, 29, out=torch.zeros(2, 4, 6, 31, device="cuda"))
    with pytest.raises(ValueError, match="out is on cpu"):
        po.unpack_obs(pk, 29, out=torch.zeros(2, 4, 6, 29))
    with pytest.raises(ValueError, match="obs must be contiguous"):
        po.pack_obs(torch.zeros(2, 4, 29, 6, device="cuda").transpose(2, 3))
    with pytest.raises(ValueError, match=r"obs must be \[\.\.\., H, W, 29 or 31\]"):
        po.pack_obs(torch.zeros(2, 4, 6, 30, device="cuda"))
    assert po.pack_obs(po.unpack_obs(pk, 31)).shape == (2, 4, 6)


# ------------------------------------------------------------------ 5. the driver
@pytest.mark.timeout(180)
def test_driver_rollout_with_packed_obs_equals_the_dense_one():
    """One update of examples/ppo_gridnet_driver.py under one seed with obs="packed" and
    obs="dense" (fused head, packed masks, 4 selfplay + 6 bot envs, 8 steps): the first
    rollouts' actions and log-probs are equal, the packed obs buffer unpacks to the dense
    buffer bit for bit, and the final losses are equal -- both runs' networks see the same
    float32 inputs."""
    torch = _torch()
    from gym_microrts import packed_obs

    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    out = {}
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    # torch's default backward kernels add in an order that changes from run to run: two dense runs of one seed
    # differ in the last bits of the loss too (profiles/packed_obs/README.md), so both runs take the deterministic ones
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for obs in ("packed", "dense"):
            out[obs] = drv.run(num_selfplay_envs=4, num_bot_envs=6, num_steps=8, updates=1, api="tensor", head="fused", masks="packed",
                               obs=obs, keep_first_rollout=True, log=lambda s: None)
            assert out[obs]["finite"] and out[obs]["engine_error_flags"] == 0, obs
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    p, d = out["packed"]["first_rollout"], out["dense"]["first_rollout"]
    assert p["obs"].shape == (8, 10, 16, 16) and p["obs"].dtype == torch.int32
    assert d["obs"].shape == (8, 10, 16, 16, 29) and d["obs"].dtype == torch.float32
    assert torch.equal(p["actions"], d["actions"]) and same_bits(p["logprob"], d["logprob"])
    assert same_bits(packed_obs.unpack_obs(p["obs"], 29), d["obs"])
    assert int(p["obs"].ne(0).sum()) == p["obs"].numel()
    for k in ("loss", "policy_loss", "value_loss", "entropy"):
        assert out["packed"][k] == out["dense"][k], k
