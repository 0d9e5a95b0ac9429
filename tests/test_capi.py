"""The drop-in boundary on CPU: libmicrorts_amd.so loads, exports every entry
point include/microrts_amd.h declares, and its host-only calls (config
validation, map XML loading, unit-type JSON) behave -- no kernel launches."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import MAPS, REPO

HEADER = os.path.join(REPO, "include", "microrts_amd.h")


def declared_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(mrts_[a-z_]+)\s*\(", txt)))


def test_header_declares_the_api():
    syms = declared_symbols()
    for s in ["mrts_create", "mrts_reset", "mrts_step", "mrts_get_masks", "mrts_destroy", "mrts_last_error"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    from gym_microrts import _native

    L = _native.lib()
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    assert not missing, missing
    assert set(_native.SIGNATURES) == set(declared_symbols())


def _create(**kw):
    from gym_microrts import _native

    args = dict(num_selfplay_envs=4, num_bot_envs=2, max_steps=2000, partial_obs=False,
                map_paths=[os.path.join(MAPS, "maps/16x16/basesWorkers16x16.xml")], game_map=[0, 0, 0, 0], bot_ai=[0, 0],
                obs_dtype=1)
    args.update(kw)
    return _native.create(**args)


def test_create_and_info():
    from gym_microrts import _native

    h = _create()
    i = _native.info(h)
    assert (i.height, i.width, i.num_envs, i.num_games, i.obs_planes, i.mask_channels) == (16, 16, 6, 4, 29, 78)
    assert i.workspace_bytes >= 4 * 256 * 16
    utt = json.loads(_native.lib().mrts_utt_json(h).decode())
    names = [u["name"] for u in utt["unitTypes"]]
    assert names == ["Resource", "Base", "Barracks", "Worker", "Light", "Heavy", "Ranged"]
    assert len(utt["unitTypes"]) + 1 == 8   # num_planes unit-type group (vec_env.py:235)
    _native.lib().mrts_destroy(h)


@pytest.mark.parametrize("kw,err", [
    (dict(num_selfplay_envs=3), "MicroRTSError"),
    (dict(max_steps=0), "MicroRTSError"),
    (dict(map_paths=["/nonexistent.xml"]), "MicroRTSError"),
    (dict(bot_ai=[99, 0]), "MicroRTSError"),
])
def test_create_rejects_bad_config(kw, err):
    from gym_microrts import _native

    with pytest.raises(getattr(_native, err)):
        _create(**kw)


def test_mixed_map_sizes_rejected():
    with pytest.raises(Exception, match="share height"):
        _create(map_paths=[os.path.join(MAPS, "maps/16x16/basesWorkers16x16.xml"), os.path.join(MAPS, "maps/8x8/basesWorkers8x8.xml")])


def test_unbound_calls_fail_loudly():
    from gym_microrts import _native

    h = _create()
    rc = _native.lib().mrts_reset(h, None, ctypes.c_void_p(16))
    assert rc != 0 and b"not bound" in _native.lib().mrts_last_error(h)


def test_step_entry_points_front_checks():
    """The three step entry points on a created but unbound handle: MRTS_ESTATE with
    "not bound" in mrts_last_error and no launch; mrts_step with a null handle:
    MRTS_ESTATE; mrts_step_group with a null handle list: MRTS_EINVAL."""
    from gym_microrts import _native

    lib = _native.lib()
    EINVAL, ESTATE, P = -1, -5, ctypes.c_void_p(4096)   # P: a non-null address, never dereferenced
    h = _create()
    assert lib.mrts_step(h, None, P, P, P, P, P) == ESTATE
    assert b"not bound" in lib.mrts_last_error(h)
    assert lib.mrts_reset(h, None, None) != 0 and b"reset" in lib.mrts_last_error(h)   # another message in between
    assert lib.mrts_step_weighted(h, None, P, P, P, P, P, P, P) == ESTATE
    assert b"not bound" in lib.mrts_last_error(h)
    lib.mrts_reset(h, None, None)
    hs, io = (ctypes.c_void_p * 1)(h), (_native.StepIO * 1)(_native.StepIO(*[4096] * 7))
    assert lib.mrts_step_group(hs, 1, None, io, _native.GROUP_BOTS_FIRST) == ESTATE
    assert b"not bound" in lib.mrts_last_error(h)
    assert lib.mrts_step(None, None, P, P, P, P, P) == ESTATE
    assert lib.mrts_step_group(None, 1, None, io, 0) == EINVAL
    lib.mrts_destroy(h)


def test_sampler_and_head_entry_points_check_their_arguments():
    """The three stand-in samplers and the three action-head entry points share one
    argument check and return before any launch: MRTS_EINVAL for a null pointer, for
    num_envs * hw over the 32-bit row bound (2^20 x 2048 = 2^31) and, for the stand-in
    samplers, for an `actions` address of 8 mod 16 (their 16-byte stores); MRTS_OK for
    num_envs == 0.  No pointer is dereferenced on the host, so plain addresses do."""
    from gym_microrts import _native

    lib = _native.lib()
    OK, EINVAL, P = _native.MRTS_OK, -1, 4096   # P: a non-null, 16-byte aligned address

    def group(n, hw, actions=P, mask=P, source=P):
        return lib.mrts_sample_actions_src_group(None, (_native.SampleSeg * 1)(_native.SampleSeg(mask, source, n, hw, 0, actions)), 1, 1, 0)

    # fn(n, hw, **pointers by name): every pointer argument defaults to P
    calls = {
        "sample": (lambda n, hw, mask=P, actions=P: lib.mrts_sample_actions(None, mask, n, hw, 0, 1, 0, actions), ["mask", "actions"]),
        "sample_src": (lambda n, hw, mask=P, source=P, actions=P: lib.mrts_sample_actions_src(None, mask, source, n, hw, 0, 1, 0, actions),
                       ["mask", "source", "actions"]),
        "sample_src_group": (group, ["mask", "source", "actions"]),
        "policy_sample": (lambda n, hw, logits=P, mask=P, source=P, actions=P, logprob=P, entropy=P:
                          lib.mrts_policy_sample(None, logits, mask, source, n, hw, 0, 1, 0, actions, logprob, entropy),
                          ["logits", "mask", "source", "actions", "logprob", "entropy"]),
        "policy_evaluate": (lambda n, hw, logits=P, mask=P, source=P, actions=P, logprob=P, entropy=P:
                            lib.mrts_policy_evaluate(None, logits, mask, source, n, hw, actions, logprob, entropy),
                            ["logits", "mask", "source", "actions", "logprob", "entropy"]),
        "policy_evaluate_backward": (lambda n, hw, logits=P, mask=P, source=P, actions=P, g_lp=P, g_ent=P, grad=P:
                                     lib.mrts_policy_evaluate_backward(None, logits, mask, source, n, hw, actions, g_lp, g_ent, grad),
                                     ["logits", "mask", "source", "actions", "g_lp", "g_ent", "grad"]),
    }
    assert lib.mrts_sample_actions_src_group(None, None, 1, 1, 0) == EINVAL
    for name, (fn, pointers) in calls.items():
        for ptr in pointers:
            assert fn(2, 256, **{ptr: None}) == EINVAL, (name, ptr)
        assert fn(1 << 20, 2048) == EINVAL, name   # n * hw = 2^31: just over the bound
        assert fn(0, 256) == OK, name
        if name.startswith("sample"):
            assert fn(2, 256, actions=P + 8) == EINVAL, name
            assert fn(0, 256, actions=P + 8) == EINVAL, name
    # the action head's sampler takes any int64-aligned actions (per-element path)
    assert calls["policy_sample"][0](0, 256, actions=P + 8) == OK


def test_map_loader_matches_python_parser():
    """C++ PhysicalGameState loader vs the oracle harness' python parser on every
    authored map: same size and unit count (workspace size reflects maps)."""
    from gym_microrts import _native
    from oracle_py import parse_map

    for root, _, files in os.walk(os.path.join(MAPS, "maps")):
        for f in files:
            p = os.path.join(root, f)
            m = parse_map(p)
            h = _native.create(2, 0, 100, False, [p], [0], [], 1)
            i = _native.info(h)
            assert (i.height, i.width) == (m["height"], m["width"])
            _native.lib().mrts_destroy(h)
            assert len(m["units"]) > 0 and np.all(m["units"][:, 5] >= 1)


def test_env_requires_gpu_when_absent():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    with pytest.raises(RuntimeError, match="GPU"):
        MicroRTSGridModeVecEnv(num_selfplay_envs=2, num_bot_envs=0, map_paths=["maps/16x16/basesWorkers16x16.xml"])


def test_fused_early_bot_layout_is_race_free_for_every_size():
    """the bot-fused k_step's early bot (wave 0) runs beside
    emit_outputs' phase A (waves 1..).  For every map size the engine fuses (W <= 32,
    H <= 64, H*W > 64, LDS within 160 KB) the bot's LDS writes must miss phase A's
    reads (unit / act / wall / scalars) and phase A's writes (output words, counter)
    must miss everything the bot touches -- in particular on sizes whose cell count
    is not a multiple of 4, where the bot's own wall slot lands inside the step's
    terrain (the bot now reads the step's terrain in place).  Checked by the
    library from the two LDS carves the kernels use."""
    from gym_microrts import _native

    f = _native.lib().mrts_fused_layout_ok
    fusable = [(w, h) for w in range(1, 33) for h in range(1, 65) if f(w, h) >= 0]
    # every size up to 32 x 64 whose fused LDS fits and whose bot LDS mrts_create accepts (<= 64 KB:
    # HW <= ~1130); maps of <= 64 cells take a 128-lane step
    assert 1700 < len(fusable) < 1900 and f(32, 32) == 1 and f(32, 64) == -1
    bad = [(w, h) for w, h in fusable if f(w, h) != 1]
    assert not bad, bad[:20]
    odd = [(w, h) for w, h in fusable if (w * h) % 4]
    assert (15, 15) in odd and (9, 13) in odd and (3, 5) in odd
    assert f(8, 8) == 1 and f(4, 4) == 1 and f(33, 16) == -1 and f(0, 5) == -1


def test_lds_layout_bytes_are_pinned():
    """The step, bot and fused LDS layouts are stated once (one carve each) and their sizes are
    the carves' end offsets.  These rows were read from a build of the commit before that change
    (profiles/lds_layout/): an array added to a carve moves them, and a size that does not follow
    its carve is an out-of-bounds LDS access that no GPU test is guaranteed to hit."""
    from gym_microrts import _native

    bot = _native.lib().mrts_engine_bot_lds_bytes
    bot.restype, bot.argtypes = ctypes.c_size_t, [ctypes.c_int] * 2

    def lay(w, h, fused=0, partial=0, NT=0):
        r = _native.step_layout(w * h, w, fused, partial, NT)
        return r.NT, r.lds_bytes, r.early

    # 8x8: its own workgroup is 64 lanes unfused, 128 fused; a wider launch's ballot words cost a few bytes
    assert lay(8, 8) == (64, 3904, 0) and lay(8, 8, NT=256) == (256, 3936, 0)
    assert lay(8, 8, fused=1) == (128, 4528, 1) and lay(8, 8, fused=1, NT=256) == (256, 4544, 1)
    #        (w, h): unfused, fused, fused + fog, bot
    rows = {(15, 15): (13344, 15792, 16688, 13072), (16, 16): (15008, 17888, 18912, 14800),
            (24, 24): (33520, 40096, 42400, None), (32, 32): (59376, 71264, 75360, 58960),
            (47, 24): (65408, None, None, None), (33, 33): (63296, None, None, None)}
    for (w, h), (unfused, fused, fog, b) in rows.items():
        assert lay(w, h) == (256, unfused, 0), (w, h)
        if fused is not None:
            assert lay(w, h, fused=1) == (256, fused, 1), (w, h)
            assert lay(w, h, fused=1, partial=1) == (256, fog, 0), (w, h)   # fog: never the early path
        if b is not None:
            assert bot(w * h, w) == b, (w, h)
    assert lay(47, 24)[1] <= 65536 < lay(48, 24)[1]   # the 64 KB limit of mrts_create
    for w, h in [(8, 8), (47, 24), (33, 33)]:   # the early flag at the size's own fused workgroup
        assert lay(w, h, fused=1)[2] == 1, (w, h)


def test_step_group_plan_merges_what_fits():
    """mrts_step_group_plan (host logic, no workspace needed): configs[4]'s buckets -- 8x8
    and 16x16 share a launch under merge-fit (members that keep >= 6 workgroups per CU),
    24x24 (40 KB fused workgroups: four per CU) and 32x32 keep their own; merge-all puts
    all in one; separate gives one each; engines of other planes or bot fusion never share;
    a handle listed twice is rejected."""
    from gym_microrts import _native

    lib = _native.lib()

    def mk(m, bots=2, partial=False):
        return _create(map_paths=[os.path.join(MAPS, m)], game_map=[0] * (2 + bots), bot_ai=[4] * bots, num_bot_envs=bots,
                       partial_obs=partial)

    def plan(hs, policy):
        arr = (ctypes.c_void_p * len(hs))(*hs)
        lo, nl = (ctypes.c_int32 * len(hs))(), ctypes.c_int32()
        rc = lib.mrts_step_group_plan(arr, len(hs), policy, lo, ctypes.byref(nl))
        return rc, list(lo), nl.value

    h8, h16, h24 = mk("maps/8x8/basesWorkers8x8.xml"), mk("maps/16x16/basesWorkers16x16.xml"), mk("maps/24x24/basesWorkers24x24.xml")
    hs = [h8, h16, h24]
    assert plan(hs, _native.GROUP_MERGE_FIT | _native.GROUP_BOTS_FIRST) == (0, [0, 0, 1], 2)
    h32 = mk("maps/32x32/basesWorkers32x32.xml")
    assert plan([h8, h16, h32], _native.GROUP_MERGE_FIT) == (0, [0, 0, 1], 2)
    assert plan([h8, h16, h32], _native.GROUP_MERGE_ALL) == (0, [0, 0, 0], 1)
    lib.mrts_destroy(h32)
    assert plan(hs, _native.GROUP_MERGE_ALL) == (0, [0, 0, 0], 1)
    assert plan(hs, _native.GROUP_SEPARATE) == (0, [0, 1, 2], 3)
    hp = mk("maps/10x10/basesTwoWorkers10x10.xml", partial=True)   # 31 planes: its own launch
    hsp = mk("maps/4x4/baseTwoWorkers4x4.xml", bots=0)             # no bots: not fused, its own launch
    assert plan([h16, hp, hsp], _native.GROUP_MERGE_ALL) == (0, [0, 1, 2], 3)
    rc, _, _ = plan([h16, h16], _native.GROUP_MERGE_ALL)
    assert rc != 0 and b"twice" in lib.mrts_last_error(h16)
    for bad in (3, 8):
        rc, _, _ = plan(hs, bad)
        assert rc != 0 and b"policy" in lib.mrts_last_error(h8)
    for h in hs + [hp, hsp]:
        lib.mrts_destroy(h)
