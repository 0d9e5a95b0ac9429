"""Packed 79-bit action masks on the CPU: a numpy statement of the format
(include/microrts_amd.h, csrc/mrts_actions.h), the C ABI's and the module's argument
checks for the packed entry points, and the driver's option check.  pack_ref /
unpack_ref are what the GPU tests (test_gpu_packed_masks.py) compare the kernels with.

The format: packed [N, HW, 3] int32 holding uint32 bit patterns; word j, bit b of a row
is bit 32 j + b of getMasks' 79-bit word; bit 0 is the source channel, bit ch + 1 is mask
channel ch; bits 79..95 are zero in what the library writes and ignored by what reads.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from test_policy_head import CH, INPUT_IDS, inputs

WORDS = 3
BITS = CH + 1


def pack_ref(mask, source):
    """Dense (mask [n, hw, 78], source [n, hw]) -> packed int32 [n, hw, 3]: a bit is set
    where the element is non-zero, every row is kept."""
    mask, source = np.asarray(mask), np.asarray(source)
    n, hw = source.shape
    bits = np.zeros((n, hw, 32 * WORDS), np.uint64)
    bits[:, :, 0] = source != 0
    bits[:, :, 1:BITS] = mask.reshape(n, hw, CH) != 0
    words = (bits.reshape(n, hw, WORDS, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def unpack_ref(packed):
    """Packed [n, hw, 3] -> (mask int32 [n, hw, 78], source int32 [n, hw]) of 0 / 1; bits 79..95 are ignored."""
    w = np.ascontiguousarray(packed).view(np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    bits = bits.reshape(w.shape[0], w.shape[1], 32 * WORDS)
    return bits[:, :, 1:BITS].astype(np.int32), bits[:, :, 0].astype(np.int32)


# ------------------------------------------------------------------ the format
@pytest.mark.parametrize("name", INPUT_IDS)
def test_reference_round_trip(name):
    """unpack_ref(pack_ref(m, s)) == (m != 0, s != 0) on every input set -- the synthetic
    sets' non-source rows with stray mask bits included -- and bits 79..95 stay zero."""
    d = inputs(name)
    p = pack_ref(d["mask"], d["source"])
    assert p.shape == (d["n"], d["hw"], WORDS) and p.dtype == np.int32
    m, s = unpack_ref(p)
    np.testing.assert_array_equal(m, (d["mask"] != 0).astype(np.int32))
    np.testing.assert_array_equal(s, (d["source"] != 0).astype(np.int32))
    assert not (p.view(np.uint32)[..., 2] >> 15).any()
    if name in ("9x13_sparse", "16x16_sparse", "24x24_sparse"):
        stray = (d["source"] == 0) & (d["mask"] != 0).any(-1)
        assert stray.any() and (p[stray].view(np.uint32) & ~np.uint32(1)).any()   # kept, not dropped


def test_fixed_bits_of_a_hand_written_row():
    def one(ch=None, src=0):
        m = np.zeros((1, 1, CH), np.int32)
        if ch is not None:
            m[0, 0, ch] = 7   # any non-zero value
        return pack_ref(m, np.full((1, 1), src, np.int32)).view(np.uint32)[0, 0].tolist()

    assert one(src=5) == [1, 0, 0]                 # source -> word 0 bit 0
    assert one(0) == [1 << 1, 0, 0]                # channel 0 -> word 0 bit 1
    assert one(30) == [1 << 31, 0, 0]              # channel 30 -> word 0 bit 31
    assert one(31) == [0, 1 << 0, 0]               # channel 31 -> word 1 bit 0
    assert one(77) == [0, 0, 1 << 14]              # channel 77 -> word 2 bit 14
    garbage = np.array([[[0, 0, (0x1FFFF << 15) | (1 << 14)]]], np.uint32).view(np.int32)
    m, s = unpack_ref(garbage)
    assert m.sum() == 1 and m[0, 0, 77] == 1 and s.sum() == 0   # bits 79..95 are nobody's


# ------------------------------------------------------------------ C ABI (host only)
def test_packed_entry_points_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: null pointers, hw < 1, negative counts,
    num_envs * hw beyond the samplers' row bound; num_envs == 0 launches nothing."""
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    u64 = ctypes.c_uint64
    EINVAL = -1

    def sample(logits=p, packed=p, n=1, hw=16, env0=0, act=p, lp=p, ent=p):
        return L.mrts_policy_sample_packed(None, logits, packed, n, hw, env0, u64(1), 0, act, lp, ent)

    def evaluate(logits=p, packed=p, n=1, hw=16, act=p, lp=p, ent=p):
        return L.mrts_policy_evaluate_packed(None, logits, packed, n, hw, act, lp, ent)

    def backward(logits=p, packed=p, n=1, hw=16, act=p, glp=p, gent=p, grad=p):
        return L.mrts_policy_evaluate_backward_packed(None, logits, packed, n, hw, act, glp, gent, grad)

    def pack(mask=p, source=p, n=1, hw=16, packed=p):
        return L.mrts_pack_masks(None, mask, source, n, hw, packed)

    def unpack(packed=p, n=1, hw=16, mask=p, source=p):
        return L.mrts_unpack_masks(None, packed, n, hw, mask, source)

    for fn, ptrs in ((sample, ("logits", "packed", "act", "lp", "ent")),
                     (evaluate, ("logits", "packed", "act", "lp", "ent")),
                     (backward, ("logits", "packed", "act", "glp", "gent", "grad")),
                     (pack, ("mask", "source", "packed")),
                     (unpack, ("packed", "mask", "source"))):
        for name in ptrs:
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
        assert fn(hw=0) == EINVAL and fn(hw=-3) == EINVAL and fn(n=-1) == EINVAL, fn.__name__
        assert fn(n=2 ** 20, hw=2 ** 11) == EINVAL, fn.__name__            # 2^31 rows
        assert fn(n=(2 ** 31 - 256) // 1128 + 1, hw=1128) == EINVAL, fn.__name__
        assert fn(n=0) == 0, fn.__name__                                   # nothing to launch
    assert sample(env0=-1) == EINVAL
    del buf


def test_get_masks_packed_refuses_null_and_unbound_handles():
    """mrts_get_masks_packed: MRTS_EINVAL for a null handle or output, MRTS_ESTATE while
    no workspace is bound (mrts_get_masks' rule) -- no launch either way."""
    from conftest import MAPS
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert L.mrts_get_masks_packed(None, None, p) == -1
    h = _native.create(num_selfplay_envs=2, num_bot_envs=0, max_steps=2000, partial_obs=False,
                       map_paths=[os.path.join(MAPS, "maps/8x8/basesWorkers8x8.xml")], game_map=[0], bot_ai=[], obs_dtype=0)
    try:
        assert L.mrts_get_masks_packed(h, None, None) == -1
        assert L.mrts_get_masks_packed(h, None, p) == -5
        assert b"not bound" in L.mrts_last_error(h)
    finally:
        L.mrts_destroy(h)


# ------------------------------------------------------------------ the module's checks
def test_module_checks_for_packed_masks():
    import torch

    from gym_microrts import policy_head as ph

    n, hw = 2, 16
    lg = torch.zeros(n * hw, CH)
    pk = torch.zeros(n, hw, WORDS, dtype=torch.int32)
    m = torch.zeros(n, hw, CH, dtype=torch.int32)
    s = torch.zeros(n, hw, dtype=torch.int32)
    a = torch.zeros(n, hw, 7, dtype=torch.int64)
    for call in (lambda **k: ph.sample(k.get("lg", lg), k.get("pk", pk), k.get("s"), seed=1, step=0),
                 lambda **k: ph.evaluate(k.get("lg", lg), k.get("pk", pk), k.get("s"), actions=k.get("a", a))):
        with pytest.raises(ValueError, match="is on cpu"):
            call()
        with pytest.raises(TypeError, match="packed must be torch.int32"):
            call(pk=pk.long())
        with pytest.raises(TypeError, match="packed must be torch.int32"):
            call(pk=pk.float())
        with pytest.raises(TypeError, match="packed must be a torch.Tensor"):
            call(pk=pk.numpy())
        with pytest.raises(ValueError, match=r"packed must be \[N, HW, 3\]"):
            call(pk=pk.reshape(n * hw, WORDS))
        with pytest.raises(ValueError, match="pass source=None"):   # packed together with a source
            call(s=s)
        with pytest.raises(ValueError, match="needs its source"):   # dense without a source
            call(pk=m)
        with pytest.raises(ValueError, match="logits must be"):
            call(lg=lg[:-1])
        with pytest.raises(TypeError, match="logits must be torch.float32"):
            call(lg=lg.double())
    with pytest.raises(TypeError, match="actions must be torch.int64"):
        ph.evaluate(lg, pk, actions=a.int())
    with pytest.raises(ValueError, match="actions must hold"):
        ph.evaluate(lg, pk, actions=a[:, :-1])
    with pytest.raises(TypeError, match="needs the actions"):
        ph.evaluate(lg, pk)
    # the converters
    with pytest.raises(ValueError, match="mask is on cpu"):
        ph.pack_masks(m, s)
    with pytest.raises(TypeError, match="mask must be torch.int32"):
        ph.pack_masks(m.float(), s)
    with pytest.raises(ValueError, match="source must be"):
        ph.pack_masks(m, s.reshape(-1))
    with pytest.raises(ValueError, match="packed is on cpu"):
        ph.unpack_masks(pk)
    with pytest.raises(ValueError, match=r"packed must be \[N, HW, 3\]"):
        ph.unpack_masks(m)
    # the dense forms' messages are what they were
    with pytest.raises(ValueError, match="logits is on cpu"):
        ph.sample(lg, m, s, seed=1, step=0)
    with pytest.raises(ValueError, match=r"mask must be \[N, HW, 78\]"):
        ph.evaluate(lg, m.reshape(n * hw, CH), s, a)
    with pytest.raises(TypeError, match="mask must be torch.int32"):
        ph.sample(lg, m.float(), s, seed=1, step=0)


# ------------------------------------------------------------------ the driver's option
def test_driver_refuses_packed_masks_without_the_fused_head():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    with pytest.raises(ValueError, match="--masks packed needs --head fused"):
        drv.run(masks="packed", head="torch", device="no-such-device")   # raised before the device is touched
    with pytest.raises(ValueError, match="masks must be"):
        drv.run(masks="bits", head="fused", api="tensor", device="no-such-device")
