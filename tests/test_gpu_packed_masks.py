"""Packed 79-bit action masks on the MI355X, every comparison bit-exact: the engine's
packed output (k_masks_packed) in lock-step with the oracle, its freshness after resets,
parking and checkpoints, the converters (k_pack_masks / k_unpack_masks), the action head
over packed masks against the dense head, and the driver's packed rollout buffer.  The
format and its numpy statement (pack_ref / unpack_ref): test_packed_masks.py.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import MAPS, REPO
from random_maps import write_random_map
from test_packed_masks import WORDS, pack_ref, unpack_ref
from test_policy_head import CH, INPUT_IDS, LP_INVALID, Reference, inputs, philox_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"
_dev = {}


def _torch():
    import torch

    return torch


def bits(x):
    torch = _torch()
    return x if x.dtype in (torch.int64, torch.int32) else x.view(torch.int32)


def same_bits(a, b):
    return _torch().equal(bits(a), bits(b))


def dev_inputs(name):
    """The input set on the device (built once): logits [n*hw, 78] f32, mask, source i32, packed i32 (from pack_ref)."""
    if name not in _dev:
        torch = _torch()
        d = inputs(name)
        _dev[name] = tuple(torch.from_numpy(x).cuda() for x in (d["logits"], d["mask"], d["source"], pack_ref(d["mask"], d["source"])))
    return _dev[name]


# ------------------------------------------------------------------ 1. the engine's packed output
#         name             map (None: random w x h)  w   h   bots  partial
ENGINE = [("8x8",          M8,                       8,  8,  True,  False),   # HW = 64: exactly one wave
          ("9x13_random",  None,                     9,  13, True,  False),   # odd HW: envs not 16-byte aligned
          ("16x16",        M16,                      16, 16, True,  False),
          ("16x16_fog",    M16,                      16, 16, True,  True),    # masks do not depend on fog
          ("24x24",        M24,                      24, 24, True,  False),   # the workgroup loops over cells
          ("47x24_random", None,                     47, 24, False, False)]   # a boundary shape: several cells per lane, no bots


@pytest.mark.parametrize("name,rel,w,h,bots,partial", ENGINE, ids=[c[0] for c in ENGINE])
def test_engine_packed_masks_lockstep_with_the_oracle(tmp_path, name, rel, w, h, bots, partial):
    """40 ticks, 4 selfplay envs + (workerRush, coacAI) bot envs where the size allows bots,
    max_steps 25 (auto-resets inside).  Every tick get_action_mask_packed() equals pack_ref
    of the oracle's masks and source, equals pack_masks of the engine's own dense tensors,
    and has no bit at 79..95; the dense tensors equal those of a twin env that never calls
    the packed getter (eager, delta masks on: the bound buffers and what the engine knows
    about them are untouched)."""
    torch = _torch()
    from gym_microrts import microrts_ai, policy_head
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import OracleVecEnv, sample_actions

    if rel is None:
        path = gpath = write_random_map(str(tmp_path / f"{name}.xml"), w, h, 5, n_units=60 if w * h > 200 else 24, wall_frac=0.1)
    else:
        path, gpath = os.path.join(MAPS, rel), rel
    ais = ["workerRushAI", "coacAI"] if bots else []

    def engine():
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=len(ais), max_steps=25, partial_obs=partial,
                                      ai2s=[getattr(microrts_ai, a) for a in ais], map_paths=[gpath], reward_weight=RW,
                                      return_tensors=True)

    g, twin = engine(), engine()
    o = OracleVecEnv(4, len(ais), [path], max_steps=25, partial_obs=partial, ai2s=ais or None, reward_weight=RW)
    assert g.eager_masks and g.mask_delta
    g.reset(), twin.reset(), o.reset()
    hw = w * h
    for s in range(40):
        mo = o.get_action_mask()
        want = pack_ref(mo, o.source_unit_mask)
        pk = g.get_action_mask_packed()
        assert pk.shape == (g.num_envs, hw, WORDS) and pk.dtype == torch.int32 and pk.is_cuda
        got = pk.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.argwhere((got != want).any(-1))
            raise AssertionError(f"tick {s}: {len(bad)} packed rows differ from the oracle, first (env, cell) {bad[:8].tolist()}")
        assert not (got.view(np.uint32)[..., 2] >> 15).any(), f"tick {s}: bits 79..95"
        assert g._mask_fresh, "the packed getter is not to touch the dense masks' bookkeeping"
        dense, src = g.get_action_mask(), g.source_unit_mask
        assert torch.equal(policy_head.pack_masks(dense, src), pk), f"tick {s}: pack_masks(dense) != packed"
        assert torch.equal(dense.cpu(), torch.from_numpy(mo)), f"tick {s}: dense masks"
        assert torch.equal(twin.get_action_mask(), dense) and torch.equal(twin.source_unit_mask, src), f"tick {s}: twin"
        a = sample_actions(mo, 17, s)
        at = torch.from_numpy(a).to(g.device)
        g.step(at), twin.step(at), o.step(a)
    assert int(g.game_stats()[:, 5].sum()) > 0, "no auto-reset in the rollout"
    assert g.error_flags() == 0
    g.close(), twin.close(), o.close()


# ------------------------------------------------------------------ 2. freshness, parking
def _kmasks_packed(e):
    """pack_ref of the standalone dense mask kernel into scratch tensors: the state's masks now."""
    torch = _torch()
    from gym_microrts import _native

    hw = e.height * e.width
    m = torch.full((e.num_envs, hw, CH), -1, dtype=torch.int32, device=e.device)
    s = torch.full((e.num_envs, hw), -1, dtype=torch.int32, device=e.device)
    _native.check(_native.lib().mrts_get_masks(e._h, e._stream(), m.data_ptr(), s.data_ptr()), e._h, "get_masks")
    return pack_ref(m.cpu().numpy(), s.cpu().numpy())


def test_packed_getter_is_never_stale():
    """Right after reset, steps, reset_games, park_games (parked games' rows all zero), an
    unpark and set_state the packed getter gives the current state's masks; two calls in a
    row give equal tensors."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    e = MicroRTSGridModeVecEnv(num_selfplay_envs=8, num_bot_envs=2, max_steps=2000, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI],
                               map_paths=[M16], reward_weight=RW, return_tensors=True)
    from oracle_py import sample_actions

    tick = [0]

    def check(tag):
        one = e.get_action_mask_packed().clone()
        two = e.get_action_mask_packed()
        assert torch.equal(one, two), f"{tag}: two calls differ"
        np.testing.assert_array_equal(two.cpu().numpy(), _kmasks_packed(e), err_msg=tag)
        return two

    def steps(n):
        for _ in range(n):
            a = sample_actions(e.get_action_mask().cpu().numpy(), 23, tick[0])
            e.step(torch.from_numpy(a).to(e.device))
            tick[0] += 1

    e.reset()
    check("reset")
    steps(12)
    before = check("steps").clone()
    e.reset_games([0, 3])
    after = check("reset_games")
    assert not torch.equal(before[0:2], after[0:2]), "game 0 was reset: its rows are the map's again"
    steps(3)
    e.park_games([1, 5])   # game 1 = envs 2, 3; game 5 = bot env 9
    pk = check("park_games")
    assert int(pk[[2, 3, 9]].abs().sum()) == 0 and int(pk[[0, 1, 4, 8]].abs().sum()) > 0
    steps(3)
    pk = check("parked, stepped")
    assert int(pk[[2, 3, 9]].abs().sum()) == 0
    e.reset_games([1])
    pk = check("unpark")
    assert int(pk[[2, 3]].abs().sum()) > 0 and int(pk[9].abs().sum()) == 0
    snap = e.get_state()
    saved = pk.clone()
    steps(8)
    assert not torch.equal(check("after the save"), saved)
    e.set_state(snap)
    assert torch.equal(check("set_state"), saved)
    assert e.error_flags() == 0
    e.close()


def test_packed_getter_on_the_numpy_contract_and_the_size_cycling_env():
    """A numpy array on the numpy contract; the per-bucket list on the size-cycling env,
    whose parked rows are zero."""
    torch = _torch()
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv, MicroRTSSizeCyclingVecEnv

    e = MicroRTSGridModeVecEnv(num_selfplay_envs=2, num_bot_envs=0, max_steps=2000, map_paths=[M8], reward_weight=RW, return_tensors=False)
    e.reset()
    pk = e.get_action_mask_packed()
    assert isinstance(pk, np.ndarray) and pk.dtype == np.int32 and pk.shape == (2, 64, WORDS)
    np.testing.assert_array_equal(pk, pack_ref(e.get_action_mask(), e.source_unit_mask))
    assert pk.any()
    e.close()
    c = MicroRTSSizeCyclingVecEnv(2, 0, map_paths=[M8], cycle_maps=[M8, M16], reward_weight=RW)
    c.reset()
    pks, masks = c.get_action_mask_packed(), c.get_action_mask()
    assert len(pks) == len(c.sizes) == 2
    for pk, m, sub in zip(pks, masks, c.envs):
        assert torch.equal(pk.cpu(), torch.from_numpy(pack_ref(m.cpu().numpy(), sub.source_unit_mask.cpu().numpy())))
    assert int(pks[0].abs().sum()) > 0 and int(pks[1].abs().sum()) == 0   # both envs play on 8x8
    for sub in c.envs:
        sub.close()


# ------------------------------------------------------------------ 3. converters
@pytest.mark.parametrize("name", INPUT_IDS)
def test_converters_equal_the_numpy_reference(name):
    """pack_masks == pack_ref; unpack_masks(pack_masks(m, s)) == (m != 0, s != 0), stray rows
    included; buffers pre-filled with 0x55555555 are overwritten in full; non-zero values
    other than 1 count as set."""
    torch = _torch()
    from gym_microrts import _native, policy_head

    d = inputs(name)
    n, hw = d["n"], d["hw"]
    _, m, s, want = dev_inputs(name)
    got = policy_head.pack_masks(m, s)
    assert got.shape == (n, hw, WORDS) and got.dtype == torch.int32
    assert torch.equal(got, want)
    assert torch.equal(policy_head.pack_masks(m * -3, s * 0x40000000), want)
    um, us = policy_head.unpack_masks(got)
    assert um.shape == (n, hw, CH) and us.shape == (n, hw) and um.dtype == us.dtype == torch.int32
    assert torch.equal(um, (m != 0).int()) and torch.equal(us, (s != 0).int())
    # straight through the C ABI into poisoned buffers
    L, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    POISON = 0x55555555
    pk = torch.full((n, hw, WORDS), POISON, dtype=torch.int32, device="cuda")
    _native.check(L.mrts_pack_masks(st, m.data_ptr(), s.data_ptr(), n, hw, pk.data_ptr()))
    assert torch.equal(pk, want)
    dm = torch.full((n, hw, CH), POISON, dtype=torch.int32, device="cuda")
    ds = torch.full((n, hw), POISON, dtype=torch.int32, device="cuda")
    garbage = want | torch.tensor([0, 0, -1 << 15], dtype=torch.int32, device="cuda")   # bits 79..95 set: ignored
    _native.check(L.mrts_unpack_masks(st, garbage.data_ptr(), n, hw, dm.data_ptr(), ds.data_ptr()))
    assert torch.equal(dm, um) and torch.equal(ds, us)
    # a mask buffer that is only 4-byte aligned takes the per-element path
    off = torch.full((n * hw * CH + 1,), POISON, dtype=torch.int32, device="cuda")
    _native.check(L.mrts_unpack_masks(st, want.data_ptr(), n, hw, off[1:].data_ptr(), ds.data_ptr()))
    assert torch.equal(off[1:].reshape(n, hw, CH), um) and int(off[0]) == POISON
    ref_m, ref_s = unpack_ref(want.cpu().numpy())
    np.testing.assert_array_equal(um.cpu().numpy(), ref_m)
    np.testing.assert_array_equal(us.cpu().numpy(), ref_s)


def test_converters_across_workgroups_with_an_odd_row_count():
    """1027 rows (four 256-row workgroups and a 3-row one whose last row's channels 76, 77
    fall to the per-element tail), every bit pattern random, guard words around the outputs."""
    torch = _torch()
    from gym_microrts import _native

    rng = np.random.default_rng(77)
    n, hw = 13, 79
    m = (rng.random((n, hw, CH)) < 0.5).astype(np.int32)
    s = (rng.random((n, hw)) < 0.5).astype(np.int32)
    want = pack_ref(m, s)
    L, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    G = 0x5A5A5A5A
    pk = torch.full((n * hw * WORDS + 8,), G, dtype=torch.int32, device="cuda")
    md, sd = torch.from_numpy(m).cuda(), torch.from_numpy(s).cuda()
    _native.check(L.mrts_pack_masks(st, md.data_ptr(), sd.data_ptr(), n, hw, pk[4:].data_ptr()))
    np.testing.assert_array_equal(pk[4:-4].cpu().numpy().reshape(n, hw, WORDS), want)
    assert bool((pk[:4] == G).all()) and bool((pk[-4:] == G).all())
    dm = torch.full((n * hw * CH + 8,), G, dtype=torch.int32, device="cuda")
    ds = torch.full((n * hw + 8,), G, dtype=torch.int32, device="cuda")
    wd = torch.from_numpy(want).cuda()
    _native.check(L.mrts_unpack_masks(st, wd.data_ptr(), n, hw, dm[4:].data_ptr(), ds[4:].data_ptr()))
    np.testing.assert_array_equal(dm[4:-4].cpu().numpy().reshape(n, hw, CH), m)
    np.testing.assert_array_equal(ds[4:-4].cpu().numpy().reshape(n, hw), s)
    for t in (dm, ds):
        assert bool((t[:4] == G).all()) and bool((t[-4:] == G).all())


# ------------------------------------------------------------------ 4. the head over packed masks
@pytest.mark.parametrize("name", INPUT_IDS)
def test_head_packed_equals_dense_bit_for_bit(name):
    """sample (actions, logprob, entropy), evaluate and evaluate's gradient under random
    g_lp / g_ent: packed against dense, as bits.  Garbage in bits 79..95 changes nothing."""
    torch = _torch()
    from gym_microrts import policy_head

    d = inputs(name)
    n = d["n"]
    lg, m, s, pk = dev_inputs(name)
    dense = policy_head.sample(lg, m, s, seed=d["seed"], step=d["step"])
    packed = policy_head.sample(lg, pk, seed=d["seed"], step=d["step"])
    for x, y, what in zip(dense, packed, ("actions", "logprob", "entropy")):
        assert x.shape == y.shape and x.dtype == y.dtype and same_bits(x, y), f"sample: {what}"
    a = dense[0]
    rng = np.random.default_rng(d["seed"] + 1000)
    glp = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    gent = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()

    def run(mask, source):
        x = lg.clone().requires_grad_(True)
        lp, ent = policy_head.evaluate(x, mask, source, actions=a)
        (lp * glp + ent * gent).sum().backward()
        return lp.detach(), ent.detach(), x.grad

    want = run(m, s)
    assert same_bits(want[0], dense[1]) and same_bits(want[1], dense[2])
    garbage = pk | torch.tensor([0, 0, -1 << 15], dtype=torch.int32, device="cuda")
    for tag, p in (("clean", pk), ("garbage in bits 79..95", garbage)):
        got = run(p, None)
        for x, y, what in zip(want, got, ("logprob", "entropy", "grad")):
            assert x.shape == y.shape and same_bits(x, y), f"evaluate, {tag}: {what}"
    dirty = policy_head.sample(lg, garbage, seed=d["seed"], step=d["step"])
    for x, y in zip(dense, dirty):
        assert same_bits(x, y)
    # the rollout buffer's forms: [N, HW, 78] logits, flat actions
    lp3, ent3 = policy_head.evaluate(lg.reshape(n, d["hw"], CH), pk, actions=a.reshape(n, -1))
    assert same_bits(lp3, want[0]) and same_bits(ent3, want[1])


@pytest.mark.parametrize("name", ["9x13_sparse", "16x16_sparse", "24x24_sparse"])
def test_packed_shard_equals_its_slice(name):
    torch = _torch()
    from gym_microrts import policy_head

    d = inputs(name)
    lg, _, _, pk = dev_inputs(name)
    lg = lg.reshape(d["n"], d["hw"], CH)
    one = policy_head.sample(lg, pk, seed=d["seed"], step=d["step"])
    shard = policy_head.sample(lg[20:].contiguous(), pk[20:].contiguous(), seed=d["seed"], step=d["step"], env0=20)
    for x, y in zip(one, shard):
        assert same_bits(x[20:], y)
    keep = d["keep"][20:]
    np.testing.assert_array_equal(shard[0].cpu().numpy()[keep], d["actions"][20:][keep])
    r = philox_rows(d["n"] - 20, d["hw"], d["seed"], d["step"], env0=20)   # the non-source rows' draw is the shard's own stream
    nosrc = d["source"][20:] == 0
    want = ((r[..., :7].astype(np.uint64) * np.array([6, 4, 4, 4, 4, 7, 49], np.uint64)) >> np.uint64(32)).astype(np.int64)
    np.testing.assert_array_equal(shard[0].cpu().numpy()[nosrc], want[nosrc])


def test_packed_invalid_actions_give_minus_1e8_and_no_fault():
    """test_invalid_actions_give_minus_1e8_and_no_fault's case through the packed entry
    points: a masked entry, an index one past its component, a negative and a huge one each
    contribute exactly -1e8 and are never used as an index; bit-equal to the dense head."""
    torch = _torch()
    from gym_microrts import policy_head
    from test_gpu_policy_head import ulp32

    hw = 117
    rng = np.random.default_rng(5)
    mask = np.zeros((1, hw, CH), np.int32)
    mask[0, :, 0] = 1
    mask[0, :, [6, 8]] = 1
    mask[0, :, 29:40] = 1
    src = np.ones((1, hw), np.int32)
    lg = rng.standard_normal((hw, CH)).astype(np.float32)
    a = np.zeros((1, hw, 7), np.int64)
    a[0, :, 1] = 2
    a[0, :, 6] = 5
    ref = Reference(lg, mask, src)
    a[0, 3, 1] = 1                 # masked
    a[0, 7, 6] = 49                # one past the component
    a[0, 9, 6] = -1
    a[0, 11, 6] = 2 ** 40
    a[0, 13, 2] = 77               # a component without valid entries ignores its action
    want = ref.logprob(a)[0]
    assert -4.0e8 - 1e3 < want < -4.0e8 + 1e3
    assert 4 * LP_INVALID == -4.0e8
    pk = torch.from_numpy(pack_ref(mask, src)).cuda()
    ad = torch.from_numpy(a).cuda()
    x = torch.from_numpy(lg).cuda().requires_grad_(True)
    lp, ent = policy_head.evaluate(x, pk, actions=ad)
    assert abs(float(lp[0].detach()) - want) <= 2 * float(ulp32(want))
    assert abs(float(ent[0].detach()) - ref.entropy()[0]) <= 2 * float(ulp32(ref.entropy()[0]))
    lp.sum().backward()
    g = x.grad.cpu().numpy()
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g[7, 29:40], -ref.comp[6]["p"][0, 7, :11], rtol=1e-5, atol=1e-7)   # no indicator term
    np.testing.assert_allclose(g[3, [6, 8]], -ref.comp[1]["p"][0, 3, [0, 2]], rtol=1e-5, atol=1e-7)
    assert (g[13, 10:14] == 0).all()
    y = torch.from_numpy(lg).cuda().requires_grad_(True)
    lpd, entd = policy_head.evaluate(y, torch.from_numpy(mask).cuda(), torch.from_numpy(src).cuda(), ad)
    lpd.sum().backward()
    assert same_bits(lp.detach(), lpd.detach()) and same_bits(ent.detach(), entd.detach()) and same_bits(x.grad, y.grad)


# ------------------------------------------------------------------ 5. the driver
def test_driver_rollout_with_packed_masks_equals_the_dense_one():
    """One update of examples/ppo_gridnet_driver.py under one seed with masks="packed" and
    masks="dense": the first rollouts' actions and log-probs are bit-equal, the packed
    buffer unpacks to the dense buffer and source, the stats are finite, no engine flag."""
    torch = _torch()
    from gym_microrts import policy_head

    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    out = {}
    for masks in ("packed", "dense"):
        out[masks] = drv.run(num_selfplay_envs=4, num_steps=4, updates=1, api="tensor", head="fused", keep_first_rollout=True,
                             masks=masks, log=lambda s: None)
        assert out[masks]["finite"] and out[masks]["engine_error_flags"] == 0, masks
    p, d = out["packed"]["first_rollout"], out["dense"]["first_rollout"]
    assert p["source"] is None and p["mask"].shape == (4, 4, 256, WORDS) and p["mask"].dtype == torch.int32
    assert d["mask"].shape == (4, 4, 256, CH)
    assert torch.equal(p["actions"], d["actions"]) and same_bits(p["logprob"], d["logprob"])
    assert int(d["source"].sum()) > 0
    um, us = policy_head.unpack_masks(p["mask"].reshape(16, 256, WORDS))
    assert torch.equal(um, d["mask"].reshape(16, 256, CH)) and torch.equal(us, d["source"].reshape(16, 256))
