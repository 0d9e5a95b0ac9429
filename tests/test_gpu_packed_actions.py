"""Packed actions on the MI355X, every comparison bit-exact: an engine of
action_format="packed" in lock-step with the oracle and with a dense-action twin, adversarial
word and row streams, the converters (k_pack_actions / k_unpack_actions) against the numpy
reference, the packed stand-in sampler, the action head writing and reading words over both
mask formats, the grouped and size-cycling envs, checkpoints across formats, and the
driver's packed action buffer.  The format and its numpy statement (pack_actions_ref /
unpack_actions_ref): test_packed_actions.py.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import MAPS, REPO, obs_bits_equal
from random_maps import write_random_map
from test_gpu_packed_obs import ENGINE
from test_packed_actions import FLAG, pack_actions_ref, unpack_actions_ref
from test_policy_head import inputs

pytestmark = pytest.mark.gpu

RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"


def _torch():
    import torch

    return torch


def same_bits(a, b):
    torch = _torch()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def outputs_equal(x, y, tag):
    """Two envs' step outputs (obs, reward, done, infos) and next masks."""
    torch = _torch()
    (o1, r1, d1, i1), (o2, r2, d2, i2) = x, y
    assert torch.equal(o1, o2), f"{tag}: obs"
    assert torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1._raw, i2._raw), f"{tag}: rewards / dones"


def masks_equal(g, twin, tag):
    torch = _torch()
    assert torch.equal(g.get_action_mask(), twin.get_action_mask()) and torch.equal(g.source_unit_mask, twin.source_unit_mask), f"{tag}: masks"


# ------------------------------------------------------------------ 1. the engine in lock-step
@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,rel,w,h,bots,partial,fusion", ENGINE, ids=[c[0] for c in ENGINE])
def test_packed_action_engine_lockstep_with_the_oracle_and_a_dense_twin(tmp_path, name, rel, w, h, bots, partial, fusion):
    """40 ticks, 4 selfplay envs + (workerRush, coacAI) bot envs where the size allows bots,
    max_steps 25 (auto-resets inside).  The packed-action env takes pack_actions_ref of the rows
    its dense twin and the oracle take; every tick obs, masks, source, raw and weighted rewards
    and dones are equal across the three."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import OracleVecEnv, sample_actions

    if rel is None:
        path = gpath = write_random_map(str(tmp_path / f"{name}.xml"), w, h, 5, n_units=60 if w * h > 200 else 24, wall_frac=0.1)
    else:
        path, gpath = os.path.join(MAPS, rel), rel
    ais = ["workerRushAI", "coacAI"] if bots else []

    def engine(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=len(ais), max_steps=25, partial_obs=partial,
                                      ai2s=[getattr(microrts_ai, a) for a in ais], map_paths=[gpath], reward_weight=RW,
                                      return_tensors=True, bot_fusion=fusion, obs_dtype=torch.int32, **kw)

    g, twin = engine(action_format="packed"), engine()
    assert g.action_format == "packed" and twin.action_format == "dense"
    assert g._actions.shape == (g.num_envs, w * h) and g._actions.dtype == torch.int32
    o = OracleVecEnv(4, len(ais), [path], max_steps=25, partial_obs=partial, ai2s=ais or None, reward_weight=RW)
    og, ot, oo = g.reset(), twin.reset(), o.reset()
    for s in range(40):
        tag = f"tick {s}"
        assert torch.equal(og, ot) and obs_bits_equal(og, oo), f"{tag}: obs"
        mo = o.get_action_mask()
        masks_equal(g, twin, tag)
        assert torch.equal(g.get_action_mask().cpu(), torch.from_numpy(mo)), f"{tag}: masks against the oracle"
        assert torch.equal(g.source_unit_mask.cpu(), torch.from_numpy(o.source_unit_mask).reshape(g.num_envs, -1)), f"{tag}: source"
        a = sample_actions(mo, 17, s)
        words = dev(pack_actions_ref(a))
        if s % 2:
            words = words.reshape(g.num_envs, h, w)   # [N, H, W] is taken too
        x, y = g.step(words), twin.step(dev(a))
        outputs_equal(x, y, tag)
        og, ot = x[0], y[0]
        oo, rew_o, done_o, infos_o = o.step(a)
        assert np.array_equal(x[2].cpu().numpy(), done_o), f"{tag}: oracle done"
        assert np.array_equal(x[3]._raw.cpu().numpy(), np.array([i["raw_rewards"] for i in infos_o])), f"{tag}: oracle raw rewards"
    assert torch.equal(og, ot) and obs_bits_equal(og, oo)
    assert int(g.game_stats()[:, 5].sum()) > 0, "no auto-reset in the rollout"
    assert g.error_flags() == 0 and twin.error_flags() == 0
    g.close(), twin.close(), o.close()


# ------------------------------------------------------------------ 2. adversarial streams
@pytest.mark.timeout(120)
@pytest.mark.parametrize("rel,hw", [(M8, 64), (M24, 576)], ids=["8x8", "24x24"])
def test_adversarial_words_and_rows(rel, hw):
    """Stream 1: uniformly random 32-bit words at every cell every tick (flags and bits 27..31
    included): the packed env equals a dense twin stepped with unpack_actions_ref of them, and the
    oracle.  Stream 2: int64 rows drawn from {-3..70, +-2^40} through pack_actions (the kernel):
    the packed env equals the dense twin stepped with the rows themselves."""
    torch = _torch()
    from gym_microrts import microrts_ai, packed_actions
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import OracleVecEnv

    ais = ["workerRushAI", "coacAI"]

    def engine(**kw):
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=2, max_steps=25, ai2s=[getattr(microrts_ai, a) for a in ais],
                                      map_paths=[rel], reward_weight=RW, return_tensors=True, obs_dtype=torch.int32, **kw)

    rng = np.random.default_rng(hw)
    g, twin = engine(action_format="packed"), engine()
    o = OracleVecEnv(4, 2, [os.path.join(MAPS, rel)], max_steps=25, ai2s=ais, reward_weight=RW)
    og, ot, oo = g.reset(), twin.reset(), o.reset()
    for s in range(30):
        tag = f"words, tick {s}"
        assert torch.equal(og, ot) and obs_bits_equal(og, oo), f"{tag}: obs"
        masks_equal(g, twin, tag)
        assert torch.equal(g.get_action_mask().cpu(), torch.from_numpy(o.get_action_mask())), f"{tag}: masks against the oracle"
        w = rng.integers(0, 2 ** 32, (6, hw), dtype=np.uint64).astype(np.uint32).view(np.int32)
        rows = unpack_actions_ref(w)
        x, y = g.step(dev(w)), twin.step(dev(rows))
        outputs_equal(x, y, tag)
        og, ot = x[0], y[0]
        oo, _, done_o, infos_o = o.step(rows)
        assert np.array_equal(x[2].cpu().numpy(), done_o), f"{tag}: oracle done"
        assert np.array_equal(x[3]._raw.cpu().numpy(), np.array([i["raw_rewards"] for i in infos_o])), f"{tag}: oracle raw rewards"
    o.close()
    values = np.concatenate([np.arange(-3, 71), [2 ** 40, -2 ** 40]]).astype(np.int64)
    for s in range(30):
        tag = f"rows, tick {s}"
        rows = dev(values[rng.integers(0, len(values), (6, hw, 7))])
        words = packed_actions.pack_actions(rows)
        assert np.array_equal(words.cpu().numpy(), pack_actions_ref(rows.cpu().numpy())), f"{tag}: pack_actions"
        outputs_equal(g.step(words), twin.step(rows), tag)
        masks_equal(g, twin, tag)
    assert g.error_flags() == 0 and twin.error_flags() == 0
    g.close(), twin.close()


# ------------------------------------------------------------------ 3. the converters
ROWS = [1, 63, 64, 65, 351, 4099]


@pytest.mark.timeout(60)
@pytest.mark.parametrize("rows", ROWS)
def test_converters_equal_the_numpy_reference(rows):
    """unpack_actions == unpack_actions_ref on random words (flags and high bits included), into a
    destination between guard elements, 16-byte aligned and 8 bytes off it; pack_actions ==
    pack_actions_ref on rows of in-field and out-of-field values, the source aligned and 8 bytes
    off, the words' destination aligned and 4 bytes off; pack of the unpacked rows stands for the same rows."""
    torch = _torch()
    from gym_microrts import _native, packed_actions

    rng = np.random.default_rng(rows)
    w = rng.integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32).view(np.int32)
    want = dev(unpack_actions_ref(w))
    repacked = pack_actions_ref(unpack_actions_ref(w))   # a flagged component's field comes back as 0, bits 27..31 as 0
    assert np.array_equal(unpack_actions_ref(repacked), unpack_actions_ref(w))
    L, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    for woff in (0, 1):        # the words 16-byte aligned / 4 bytes off
        wbig = torch.zeros(rows + 8, dtype=torch.int32, device="cuda")
        wb = (-wbig.data_ptr() // 4) % 4 + woff
        wd = wbig[wb:wb + rows]
        wd.copy_(dev(w))
        for aoff in (0, 1):    # the rows 16-byte aligned / 8 bytes off
            big = torch.full((rows * 7 + 8,), 7, dtype=torch.int64, device="cuda")
            base = (-big.data_ptr() // 8) % 2 + aoff
            assert (big[base:].data_ptr() % 16 == 0) == (aoff == 0)
            out = big[base:base + rows * 7].view(rows, 7)
            assert packed_actions.unpack_actions(wd, out=out) is out
            assert torch.equal(out, want), f"unpack, offsets {woff} {aoff}"
            assert bool((big[:base] == 7).all()) and bool((big[base + rows * 7:] == 7).all()), "unpack: guards"
            # pack from this (offset) buffer into an offset words buffer
            pbig = torch.full((rows + 8,), -1, dtype=torch.int32, device="cuda")
            pb = (-pbig.data_ptr() // 4) % 4 + woff
            pw = pbig[pb:pb + rows]
            assert L.mrts_pack_actions(st, out.data_ptr(), rows, pw.data_ptr()) == 0
            assert np.array_equal(pw.cpu().numpy(), repacked), f"pack of the unpacked rows, offsets {woff} {aoff}"
            assert bool((pbig[:pb] == -1).all()) and bool((pbig[pb + rows:] == -1).all()), "pack: guards"
    values = np.concatenate([np.arange(-3, 71), [2 ** 40, -2 ** 40]]).astype(np.int64)
    a = values[rng.integers(0, len(values), (rows, 7))]
    for aoff in (0, 1):
        big = torch.zeros(rows * 7 + 8, dtype=torch.int64, device="cuda")
        base = (-big.data_ptr() // 8) % 2 + aoff
        src = big[base:base + rows * 7].view(rows, 7)
        src.copy_(dev(a))
        got = packed_actions.pack_actions(src)
        assert got.dtype == torch.int32 and got.shape == (rows,)
        assert np.array_equal(got.cpu().numpy(), pack_actions_ref(a)), f"pack, offset {aoff}"
    assert packed_actions.pack_actions(torch.empty((0, 5, 7), dtype=torch.int64, device="cuda")).shape == (0, 5)
    assert packed_actions.unpack_actions(torch.empty((0, 5), dtype=torch.int32, device="cuda")).shape == (0, 5, 7)


# ------------------------------------------------------------------ 4. the sampler
@pytest.mark.timeout(60)
@pytest.mark.parametrize("shape", ["9x13", "16x16"])
def test_packed_sampler_equals_pack_of_the_dense_sampler(tmp_path, shape):
    """mrts_sample_actions_src_packed == pack of mrts_sample_actions_src's rows on real masks of a
    stepped game (3 envs of 9x13 = 351 rows: a tail wave; 4 of 16x16), env0 != 0, and == pack of
    the oracle's sampler."""
    torch = _torch()
    from gym_microrts import _native
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import sample_actions

    if shape == "9x13":
        gpath, n, hw = write_random_map(str(tmp_path / "m.xml"), 9, 13, 5, n_units=24, wall_frac=0.1), 4, 117
    else:
        gpath, n, hw = M16, 4, 256
    env = MicroRTSGridModeVecEnv(num_selfplay_envs=n, num_bot_envs=0, max_steps=2000, map_paths=[gpath], reward_weight=RW, return_tensors=True)
    env.reset()
    for s in range(12):
        env.step(dev(sample_actions(env.get_action_mask().cpu().numpy(), 5, s)))
    use = 3 if shape == "9x13" else n
    mask, src = env.get_action_mask()[:use].contiguous(), env.source_unit_mask[:use].contiguous()
    assert int(src.sum()) > 0
    L, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    rows = torch.full((use, hw, 7), -9, dtype=torch.int64, device="cuda")
    big = torch.full((use * hw + 2,), -9, dtype=torch.int32, device="cuda")
    words = big[1:1 + use * hw]
    for env0, step in ((5, 3), (1, 0)):
        u64 = ctypes.c_uint64(77)
        assert L.mrts_sample_actions_src(st, mask.data_ptr(), src.data_ptr(), use, hw, env0, u64, step, rows.data_ptr()) == 0
        assert L.mrts_sample_actions_src_packed(st, mask.data_ptr(), src.data_ptr(), use, hw, env0, u64, step, words.data_ptr()) == 0
        want = pack_actions_ref(rows.cpu().numpy()).reshape(-1)
        assert np.array_equal(words.cpu().numpy(), want), (env0, step)
        assert np.array_equal(want, pack_actions_ref(sample_actions(mask.cpu().numpy(), 77, step, env0=env0)).reshape(-1))
        assert not (want.view(np.uint32) >> FLAG).any()
        assert int(big[0]) == -9 and int(big[-1]) == -9, "guards"
    env.close()


# ------------------------------------------------------------------ 5. the action head
@pytest.mark.timeout(60)
@pytest.mark.parametrize("name,envs", [("8x8_sparse", 3), ("9x13_sparse", 3)], ids=["8x8", "9x13x3"])
@pytest.mark.parametrize("masks", ["dense", "packed"])
def test_action_head_writes_and_reads_words(name, envs, masks):
    """sample(action_format="packed") gives words whose unpack is the dense call's actions, with
    identical log-prob and entropy; evaluate and its gradient are identical from words and from
    rows for the sampled actions, for actions the mask forbids, and for flagged / out-of-range
    words against their unpacked rows."""
    torch = _torch()
    from gym_microrts import packed_actions
    from gym_microrts import policy_head as ph

    d = inputs(name)
    n, hw = envs, d["hw"]
    lg = dev(d["logits"][:n * hw])
    m, s = dev(d["mask"][:n]), dev(d["source"][:n])
    assert int(s.sum()) > 0
    margs = (ph.pack_masks(m, s),) if masks == "packed" else (m, s)
    a, lp, ent = ph.sample(lg, *margs, seed=d["seed"], step=3, env0=2)
    w, lpw, entw = ph.sample(lg, *margs, seed=d["seed"], step=3, env0=2, action_format="packed")
    assert w.dtype == torch.int32 and w.shape == (n, hw)
    assert np.array_equal(unpack_actions_ref(w.cpu().numpy()), a.cpu().numpy()), "unpack(words) != the dense call's actions"
    assert torch.equal(packed_actions.unpack_actions(w), a) and torch.equal(packed_actions.pack_actions(a), w)
    assert same_bits(lp, lpw) and same_bits(ent, entw)

    rng = np.random.default_rng(9)
    forbidden = (a + 1 + torch.from_numpy(rng.integers(0, 3, tuple(a.shape))).cuda()) % torch.tensor([8, 4, 4, 4, 4, 8, 64], device="cuda")
    wild = dev(rng.integers(0, 2 ** 32, (n, hw), dtype=np.uint64).astype(np.uint32).view(np.int32))
    cases = [("sampled", w, a), ("forbidden", packed_actions.pack_actions(forbidden), forbidden),
             ("wild words", wild, dev(unpack_actions_ref(wild.cpu().numpy())))]
    glp, gent = dev(rng.standard_normal(n).astype(np.float32)), dev(rng.standard_normal(n).astype(np.float32))
    for tag, words, rows in cases:
        res = []
        for act in (rows, words, words.reshape(-1)):
            x = lg.clone().requires_grad_(True)
            l, e = ph.evaluate(x, *margs, actions=act)
            (l * glp + e * gent).sum().backward()
            res.append((l.detach(), e.detach(), x.grad))
        for other in res[1:]:
            for u, v in zip(res[0], other):
                assert same_bits(u, v), f"{tag}: evaluate from words differs from evaluate from rows"
        if tag == "sampled":
            assert same_bits(res[1][0], lp) and same_bits(res[1][1], ent)
        else:
            assert bool((res[1][0] <= -1e8).any()), f"{tag}: nothing was forbidden"


# ------------------------------------------------------------------ 6. grouped and cycling envs, checkpoints
@pytest.mark.timeout(120)
def test_mixed_map_and_size_cycling_envs_pass_the_format_on():
    """MicroRTSMixedMapVecEnv (8x8 + 16x16 in one grouped launch; then a packed and a dense
    engine in one group) for 30 ticks and MicroRTSSizeCyclingVecEnv through one cycle, with
    action_format="packed", each bucket against its dense twin."""
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

    for make, ticks in ((mixed, 30), (cycling, 14)):
        g, twin = make(action_format="packed"), make()
        assert all(e.action_format == "packed" for e in g.envs) and all(e.action_format == "dense" for e in twin.envs)
        if make is mixed:
            assert g.grouped and g.launch_plan() == ([0, 0], 1)
        else:
            assert g.action_format == "packed"
        obs, dense = g.reset(), twin.reset()
        for s in range(ticks):
            masks = g.get_action_mask()
            for k, (x, y, mg, mt) in enumerate(zip(obs, dense, masks, twin.get_action_mask())):
                assert torch.equal(x, y) and torch.equal(mg, mt), f"{make.__name__}, bucket {k}, tick {s}"
            rows = [sample_actions(np.ascontiguousarray(m.cpu().numpy()), 31, s) for m in masks]
            (obs, rew, done, _), (dense, rew2, done2, _) = g.step([dev(pack_actions_ref(a)) for a in rows]), twin.step([dev(a) for a in rows])
            for x, y in zip(rew, rew2) if make is mixed else ((rew, rew2),):
                assert torch.equal(x, y)
        if make is cycling:
            assert (g.bucket == twin.bucket).all() and len(set(g.bucket.tolist())) == 2, "no env moved to the other size"
        else:   # one grouped launch of a packed-action and a dense-action engine
            e0, e1, t0, t1 = g.envs[0], twin.envs[1], twin.envs[0], g.envs[1]
            rows = [sample_actions(np.ascontiguousarray(e.get_action_mask().cpu().numpy()), 37, 0) for e in (e0, e1)]
            e0.step_async(dev(pack_actions_ref(rows[0]))), e1.step_async(dev(rows[1]))
            io = (_native.StepIO * 2)(e0._step_io(), e1._step_io())
            hs = (ctypes.c_void_p * 2)(e0._h, e1._h)
            lo, nl = (ctypes.c_int32 * 2)(), ctypes.c_int32()
            assert _native.lib().mrts_step_group_plan(hs, 2, g.group_policy, lo, ctypes.byref(nl)) == 0 and nl.value == 1
            assert _native.lib().mrts_step_group(hs, 2, e0._stream(), io, g.group_policy) == 0
            t0.step(dev(rows[0])), t1.step(dev(pack_actions_ref(rows[1])))
            assert torch.equal(e0._obs, t0._obs) and torch.equal(e1._obs, t1._obs), "a group of both formats"
        assert g.error_flags() == 0 and twin.error_flags() == 0
        g.close(), twin.close()


@pytest.mark.timeout(120)
def test_checkpoints_move_between_the_formats_and_the_input_checks():
    """get_state on a packed-action env, set_state on a dense one, and back, continuing in
    lock-step; the numpy and hybrid contracts take numpy words; the other format's dtype or
    element count is a ValueError naming both shapes; the shared-memory env and the JNI-shaped
    client refuse the keyword."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeSharedMemVecEnv, MicroRTSGridModeVecEnv
    from gym_microrts.jni_client import JNIGridnetVecClient
    from oracle_py import sample_actions

    def engine(**kw):
        kw.setdefault("return_tensors", True)
        return MicroRTSGridModeVecEnv(num_selfplay_envs=4, num_bot_envs=2, max_steps=2000, ai2s=[microrts_ai.workerRushAI, microrts_ai.coacAI],
                                      map_paths=[M16], reward_weight=RW, obs_dtype=torch.int32, **kw)

    g, twin = engine(action_format="packed"), engine()
    g.reset(), twin.reset()
    tick = [0]

    def steps(k, tag):
        for _ in range(k):
            a = sample_actions(g.get_action_mask().cpu().numpy(), 41, tick[0])
            outputs_equal(g.step(dev(pack_actions_ref(a))), twin.step(dev(a)), f"{tag}, tick {tick[0]}")
            masks_equal(g, twin, tag)
            tick[0] += 1

    steps(10, "before")
    snap = g.get_state()
    steps(5, "on")
    later = twin.get_state()
    assert torch.equal(twin.set_state(snap), g.set_state(snap))   # the packed env's state into the dense env
    tick[0] = 10
    steps(5, "packed -> dense")
    assert torch.equal(g.set_state(later), twin.set_state(later))   # and the dense env's into the packed one
    steps(5, "dense -> packed")

    n, hw = g.num_envs, 256
    rows, words = torch.zeros(n, hw, 7, dtype=torch.int64, device="cuda"), torch.zeros(n, hw, dtype=torch.int32, device="cuda")
    for env, bad in ((g, rows), (g, rows.int()), (g, words.long()), (g, rows.cpu().numpy()), (g, words.cpu().numpy().astype(np.int64)),
                     (twin, words), (twin, words.cpu().numpy())):
        with pytest.raises(ValueError, match=r"\[N, HW, 7\] = \(6, 256, 7\).*\[N, HW\] = \(6, 256\)|\[N, HW\] = \(6, 256\).*\[N, HW, 7\] = \(6, 256, 7\)"):
            env.step_async(bad)
    steps(2, "after the refused calls")
    assert g.error_flags() == 0 and twin.error_flags() == 0
    g.close(), twin.close()

    for contract in (False, "hybrid"):
        e, d = engine(action_format="packed", return_tensors=contract), engine(return_tensors=contract)
        e.reset(), d.reset()
        for s in range(4):
            m = e.get_action_mask()
            a = sample_actions(m if isinstance(m, np.ndarray) else m.cpu().numpy(), 43, s)
            w = pack_actions_ref(a)
            x, y = e.step(w if s % 2 else w.reshape(6, 16, 16)), d.step(a.reshape(6, -1))
            assert np.array_equal(np.asarray(x[0].cpu() if torch.is_tensor(x[0]) else x[0]), np.asarray(y[0].cpu() if torch.is_tensor(y[0]) else y[0]))
            assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), (contract, s)
        assert e._act_stage.dtype == torch.int32 and e._act_stage.shape == (6, 256)   # staged at 4 bytes a cell
        e.close(), d.close()
    with pytest.raises(ValueError, match="action_format must be"):
        engine(action_format="words")
    with pytest.raises(ValueError, match="action_format='packed' is not available"):
        MicroRTSGridModeSharedMemVecEnv(2, 0, map_paths=[M8], action_format="packed")
    with pytest.raises(ValueError, match="action_format='packed' is not available"):
        JNIGridnetVecClient(2, 0, 2000, [], MAPS, [M8], [], action_format="packed")


# ------------------------------------------------------------------ 7. the driver
@pytest.mark.timeout(120)
def test_driver_rollout_with_packed_actions_equals_the_dense_one():
    """One update of examples/ppo_gridnet_driver.py under one seed with actions="packed" and
    actions="dense" (fused head, packed masks, packed obs, 16 envs, 8 steps): the first rollout's
    action words unpack to the dense run's actions, log-probs and the update's losses are equal."""
    torch = _torch()
    from gym_microrts import packed_actions

    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    out = {}
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    # torch's default backward kernels add in an order that changes from run to run: both runs take the deterministic ones
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for actions in ("packed", "dense"):
            out[actions] = drv.run(num_selfplay_envs=16, num_steps=8, updates=1, api="tensor", head="fused", masks="packed", obs="packed",
                                   actions=actions, keep_first_rollout=True, log=lambda s: None)
            assert out[actions]["finite"] and out[actions]["engine_error_flags"] == 0, actions
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    p, d = out["packed"]["first_rollout"], out["dense"]["first_rollout"]
    assert p["actions"].shape == (8, 16, 256) and p["actions"].dtype == torch.int32
    assert d["actions"].shape == (8, 16, 256, 7) and d["actions"].dtype == torch.int64
    assert torch.equal(packed_actions.unpack_actions(p["actions"]), d["actions"])
    assert torch.equal(p["obs"], d["obs"]) and same_bits(p["logprob"], d["logprob"])
    for k in ("loss", "policy_loss", "value_loss", "entropy"):
        assert out["packed"][k] == out["dense"][k], (k, out["packed"][k], out["dense"][k])
