"""Packed observations on the CPU: a numpy statement of the format (include/microrts_amd.h,
csrc/mrts_rules.h cell_onehot), the oracle's obs seen through it, the C ABI's and the
module's argument checks for the converters, and the driver's option check.  pack_obs_ref /
unpack_obs_ref are what the GPU tests (test_gpu_packed_obs.py) compare the kernels with.

The format: packed_obs [N, H, W] int32 holding uint32 bit patterns; bit i of a cell's word is
plane i of the dense obs of that env and cell for i < P (29, or 31 with partial obs); bits
P..31 are zero in what the library writes and ignored by what reads.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import MAPS, REPO

GROUPS = (5, 5, 3, 8, 6, 2)   # hp, resources, owner, unit type, action, terrain (+ 2: visibility, with partial obs)
EMPTY = 1 | 1 << 5 | 1 << 10 | 1 << 13 | 1 << 21 | 1 << 27   # the empty cell that is no wall
M16 = "maps/16x16/basesWorkers16x16.xml"


def pack_obs_ref(obs):
    """Dense [..., P] (P = 29 or 31, any numeric dtype) -> int32 [...]: bit i is set where
    plane i's element is non-zero."""
    obs = np.asarray(obs)
    P = obs.shape[-1]
    assert P in (29, 31)
    w = ((obs != 0).astype(np.uint64) << np.arange(P, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


def unpack_obs_ref(packed, planes, dtype=np.int32):
    """int32 [...] -> dense [..., planes] of 0 / 1 in `dtype`; bits >= planes are ignored."""
    w = np.ascontiguousarray(packed).view(np.uint32)
    return ((w[..., None] >> np.arange(planes, dtype=np.uint32)) & np.uint32(1)).astype(dtype)


def group_counts(words, P):
    """Set bits per plane group of every word: [..., len(groups)]."""
    groups = GROUPS + ((2,) if P == 31 else ())
    bits = unpack_obs_ref(words, P)
    edges = np.cumsum((0,) + groups)
    assert edges[-1] == P
    return np.stack([bits[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], -1)


# ------------------------------------------------------------------ the format
@pytest.mark.parametrize("P", [29, 31])
def test_reference_round_trip(P):
    """Random one-hot planes, then arbitrary non-zero values (negative, huge, fractional):
    unpack_obs_ref(pack_obs_ref(x)) == (x != 0), and no bit at or above P."""
    rng = np.random.default_rng(P)
    groups = GROUPS + ((2,) if P == 31 else ())
    onehot = np.concatenate([np.eye(g, dtype=np.int32)[rng.integers(0, g, (3, 7, 5))] for g in groups], -1)
    assert onehot.shape == (3, 7, 5, P)
    w = pack_obs_ref(onehot)
    assert w.shape == (3, 7, 5) and w.dtype == np.int32
    np.testing.assert_array_equal(unpack_obs_ref(w, P), onehot)
    assert (group_counts(w, P) == 1).all()
    anyv = rng.standard_normal((4, 6, 6, P)) * (rng.random((4, 6, 6, P)) < 0.4) * 1e6
    anyv[0, 0, 0, :3] = [-0.0, -1e-30, 2.0 ** 40]
    w = pack_obs_ref(anyv)
    np.testing.assert_array_equal(unpack_obs_ref(w, P), (anyv != 0).astype(np.int32))
    assert (w.view(np.uint32)[0, 0, 0] & 7) == 6   # -0.0 is zero, a denormal-sized value is not
    assert not (w.view(np.uint32) >> P).any()
    np.testing.assert_array_equal(unpack_obs_ref(w, P, np.float32), (anyv != 0).astype(np.float32))


def test_hand_written_words():
    empty = np.zeros(29, np.int32)
    empty[[0, 5, 10, 13, 21, 27]] = 1   # hp 0, resources 0, no owner, no unit, no action, no wall
    assert int(pack_obs_ref(empty).view(np.uint32)) == EMPTY
    for i in range(31):
        one = np.zeros(31, np.float32)
        one[i] = -2.5   # any non-zero value
        assert int(pack_obs_ref(one).view(np.uint32)) == 1 << i
    garbage = np.array([EMPTY | 0b111 << 29], np.uint32).view(np.int32)
    np.testing.assert_array_equal(unpack_obs_ref(garbage, 29)[0], empty)   # bits >= P are nobody's
    fog = unpack_obs_ref(garbage, 31)[0]
    assert fog[29] == 1 and fog[30] == 1 and fog.sum() == 8                # with P = 31 bits 29, 30 are planes; bit 31 is not


@pytest.mark.parametrize("partial", [False, True], ids=["full", "fog"])
def test_the_oracles_obs_as_words(partial):
    """pack_obs_ref of the oracle's obs on the 16x16 map over 30 ticks of random play: exactly
    one bit in each plane group of every word, no bit at or above P, and the round trip."""
    from oracle_py import OracleVecEnv, sample_actions

    P = 31 if partial else 29
    o = OracleVecEnv(4, 2, [os.path.join(MAPS, M16)], max_steps=2000, partial_obs=partial, ai2s=["workerRushAI", "coacAI"])
    obs = o.reset()
    seen = set()
    for s in range(30):
        assert obs.shape == (6, 16, 16, P)
        w = pack_obs_ref(obs)
        assert (group_counts(w, P) == 1).all(), f"tick {s}"
        assert not (w.view(np.uint32) >> P).any(), f"tick {s}"
        np.testing.assert_array_equal(unpack_obs_ref(w, P), obs)
        seen.update(np.unique(w.view(np.uint32)).tolist())
        obs = o.step(sample_actions(o.get_action_mask(), 3, s))[0]
    assert (EMPTY | (1 << 29 if partial else 0)) in seen and len(seen) > 8
    o.close()


# ------------------------------------------------------------------ C ABI (host only)
def test_obs_converters_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: a null pointer, rows < 0 or beyond
    2^31 - 257, planes other than 29 / 31, an unknown element type, an obs pointer off its
    element size; rows == 0 launches nothing."""
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    EINVAL = -1

    def unpack(packed=p, rows=1, planes=29, elem=_native.MRTS_ELEM_FLOAT32, obs=p):
        return L.mrts_unpack_obs(None, packed, rows, planes, elem, obs)

    def pack(obs=p, rows=1, planes=29, elem=_native.MRTS_ELEM_FLOAT32, packed=p):
        return L.mrts_pack_obs(None, obs, rows, planes, elem, packed)

    for fn in (unpack, pack):
        assert fn(packed=None) == EINVAL and fn(obs=None) == EINVAL, fn.__name__
        assert fn(rows=-1) == EINVAL and fn(rows=-2 ** 40) == EINVAL, fn.__name__
        assert fn(rows=2 ** 31 - 256) == EINVAL and fn(rows=2 ** 40) == EINVAL, fn.__name__   # beyond the samplers' row bound
        for planes in (0, 28, 30, 32, -29, 78):
            assert fn(planes=planes) == EINVAL, (fn.__name__, planes)
        for elem in (-1, 4, 29):
            assert fn(elem=elem) == EINVAL, (fn.__name__, elem)
        for elem, size in ((_native.MRTS_ELEM_INT32, 4), (_native.MRTS_ELEM_FLOAT32, 4), (_native.MRTS_ELEM_FLOAT16, 2),
                           (_native.MRTS_ELEM_BFLOAT16, 2)):
            for off in range(1, size):
                assert fn(elem=elem, obs=p + off) == EINVAL, (fn.__name__, elem, off)
            for planes in (29, 31):
                assert fn(rows=0, planes=planes, elem=elem) == 0, (fn.__name__, elem)   # nothing to launch
                assert fn(rows=0, planes=planes, elem=elem, obs=p + size) == 0          # element-aligned is enough
    del buf


# ------------------------------------------------------------------ the module's checks
def test_module_checks_for_packed_obs():
    import torch

    from gym_microrts import packed_obs as po

    pk = torch.zeros(2, 4, 4, dtype=torch.int32)
    ob = torch.zeros(2, 4, 4, 29)
    with pytest.raises(ValueError, match="packed is on cpu"):
        po.unpack_obs(pk, 29)
    with pytest.raises(ValueError, match="planes must be 29 or 31"):
        po.unpack_obs(pk, 30)
    with pytest.raises(ValueError, match="dtype must be one of"):
        po.unpack_obs(pk, 29, dtype=torch.float64)
    with pytest.raises(ValueError, match="packed must be torch.int32"):
        po.unpack_obs(pk.long(), 29)
    with pytest.raises(ValueError, match="packed must be torch.int32"):
        po.unpack_obs(pk.float(), 29)
    with pytest.raises(ValueError, match="packed must be a torch.Tensor"):
        po.unpack_obs(pk.numpy(), 29)
    with pytest.raises(ValueError, match="obs is on cpu"):
        po.pack_obs(ob)
    with pytest.raises(ValueError, match="obs must be a torch.Tensor"):
        po.pack_obs(ob.numpy())
    with pytest.raises(ValueError, match="obs must be torch.int32 or"):
        po.pack_obs(ob.double())
    assert set(po.ELEM) == {torch.int32, torch.float32, torch.float16, torch.bfloat16} and po.PLANES == (29, 31)


# ------------------------------------------------------------------ the driver's option
def test_driver_refuses_packed_obs_without_the_tensor_api():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    for api in ("numpy", "hybrid"):
        with pytest.raises(ValueError, match="--obs packed needs --api tensor"):
            drv.run(obs="packed", api=api, device="no-such-device")   # raised before the device is touched
    with pytest.raises(ValueError, match="obs must be"):
        drv.run(obs="bits", api="tensor", device="no-such-device")
