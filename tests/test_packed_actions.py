"""Packed actions on the CPU: a numpy statement of the format (include/microrts_amd.h,
csrc/mrts_actions.h), the C ABI's and the modules' argument checks for the new entry points,
and the driver's option check.  pack_actions_ref / unpack_actions_ref are what the GPU tests
(test_gpu_packed_actions.py) compare the kernels with.

The format: action_words [N, HW] int32 holding uint32 bit patterns; component k's value in
BITS[k] bits from bit OFF[k] (type 0..2, move 3..4, harvest 5..6, return 7..8, produce
direction 9..10, produce type 11..13, attack cell 14..19); bit 20 + k is component k's
invalid flag; bits 27..31 are zero in what the library writes and ignored by what reads.
A word stands for the row whose component k is -1 when flag k is set, else the field.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import MAPS, REPO

NVEC = (6, 4, 4, 4, 4, 7, 49)
BITS = (3, 2, 2, 2, 2, 3, 6)
OFF = (0, 3, 5, 7, 9, 11, 14)
FLAG = 20


def pack_actions_ref(actions):
    """int64 rows [..., 7] -> words int32 [...]: component k in its field when it lies in
    [0, 2^BITS[k]); otherwise field 0 and flag k set."""
    a = np.asarray(actions).astype(np.int64)
    assert a.shape[-1] == 7
    w = np.zeros(a.shape[:-1], np.uint32)
    for k in range(7):
        v = a[..., k]
        fits = (v >= 0) & (v < (1 << BITS[k]))
        w |= np.where(fits, v, 0).astype(np.uint32) << np.uint32(OFF[k])
        w |= (~fits).astype(np.uint32) << np.uint32(FLAG + k)
    return w.view(np.int32)


def unpack_actions_ref(words):
    """words [...] -> int64 rows [..., 7]: -1 where the flag is set, the field otherwise;
    bits 27..31 are ignored."""
    w = np.ascontiguousarray(words).view(np.uint32)
    out = np.empty(w.shape + (7,), np.int64)
    for k in range(7):
        field = ((w >> np.uint32(OFF[k])) & np.uint32((1 << BITS[k]) - 1)).astype(np.int64)
        out[..., k] = np.where((w >> np.uint32(FLAG + k)) & np.uint32(1), -1, field)
    return out


# ------------------------------------------------------------------ the format
def test_layout_is_the_fewest_bits_laid_end_to_end():
    assert BITS == tuple(int(np.ceil(np.log2(n))) for n in NVEC)
    assert OFF == tuple(int(x) for x in np.concatenate(([0], np.cumsum(BITS)[:-1]))) and sum(BITS) == FLAG and FLAG + 7 == 27
    from gym_microrts import packed_actions

    assert packed_actions.FIELD_BITS == BITS and packed_actions.FLAG_BIT == FLAG and packed_actions.COMPONENTS == 7


def test_round_trip_of_every_in_field_row():
    """unpack(pack(a)) == a for rows whose components fit their fields: a random sample (in-range
    values and the out-of-range-but-in-field ones: type 6 / 7, produce type 7, attack cell 49..63)
    and each component's extremes; no flag, no bit at or above 27."""
    rng = np.random.default_rng(5)
    a = np.stack([rng.integers(0, 1 << b, 20000) for b in BITS], -1).astype(np.int64)
    ext = []
    for k in range(7):
        for v in (0, NVEC[k] - 1, (1 << BITS[k]) - 1):
            row = np.zeros(7, np.int64)
            row[k] = v
            ext.append(row)
    ext.append(np.array([(1 << b) - 1 for b in BITS], np.int64))
    a = np.concatenate([a, np.array(ext)])
    w = pack_actions_ref(a)
    assert w.dtype == np.int32 and w.shape == a.shape[:-1]
    assert not (w.view(np.uint32) >> FLAG).any()
    np.testing.assert_array_equal(unpack_actions_ref(w), a)
    assert int(pack_actions_ref(ext[-1]).view(np.uint32)) == (1 << FLAG) - 1


def test_hand_written_words():
    def word(**kv):
        row = np.zeros(7, np.int64)
        for k, v in kv.items():
            row[int(k[1:])] = v
        return int(pack_actions_ref(row).view(np.uint32))

    assert word() == 0
    assert word(c0=5) == 5                      # attack type
    assert word(c1=3) == 3 << 3
    assert word(c2=1) == 1 << 5
    assert word(c3=2) == 2 << 7
    assert word(c4=3) == 3 << 9
    assert word(c5=6) == 6 << 11
    assert word(c6=48) == 48 << 14
    assert word(c0=4, c4=1, c5=2) == 4 | (1 << 9) | (2 << 11)   # produce a unit of type 2 to the right
    np.testing.assert_array_equal(unpack_actions_ref(np.array([5 | (48 << 14)], np.uint32).view(np.int32))[0], [5, 0, 0, 0, 0, 0, 48])
    np.testing.assert_array_equal(unpack_actions_ref(np.array([(1 << 20) | (1 << 26) | (63 << 14) | 1], np.uint32).view(np.int32))[0],
                                  [-1, 0, 0, 0, 0, 0, -1])


@pytest.mark.parametrize("bad,comp", [(-1, 0), (-1, 3), (2 ** 40, 0), (2 ** 40, 6), (-2 ** 40, 5), (4, 1), (4, 4), (64, 6), (8, 0), (8, 5)])
def test_a_component_outside_its_field_sets_the_flag(bad, comp):
    row = np.array([1, 2, 3, 0, 1, 5, 40], np.int64)
    row[comp] = bad
    w = int(pack_actions_ref(row).view(np.uint32))
    assert (w >> (FLAG + comp)) & 1 and ((w >> OFF[comp]) & ((1 << BITS[comp]) - 1)) == 0
    assert bin(w >> FLAG).count("1") == 1 and w >> 27 == 0
    want = row.copy()
    want[comp] = -1
    np.testing.assert_array_equal(unpack_actions_ref(np.array([w], np.uint32).view(np.int32))[0], want)


def test_high_bits_are_ignored():
    rng = np.random.default_rng(6)
    w = rng.integers(0, 1 << 27, 5000, dtype=np.uint64).astype(np.uint32)
    hi = (rng.integers(1, 32, 5000, dtype=np.uint64).astype(np.uint32)) << np.uint32(27)
    np.testing.assert_array_equal(unpack_actions_ref((w | hi).view(np.int32)), unpack_actions_ref(w.view(np.int32)))
    np.testing.assert_array_equal(unpack_actions_ref(np.array([0xF8000000], np.uint32).view(np.int32))[0], np.zeros(7, np.int64))


def test_the_oracle_samplers_rows_survive_the_round_trip():
    """ovec_sample_actions on real masks (its no-valid-entry draws included: most rows)."""
    from oracle_py import OracleVecEnv, sample_actions

    o = OracleVecEnv(2, 0, [os.path.join(MAPS, "maps/16x16/basesWorkers16x16.xml")], max_steps=2000)
    o.reset()
    for s in range(3):
        m = o.get_action_mask()
        a = sample_actions(m, 11, s, env0=3)
        w = pack_actions_ref(a)
        assert not (w.view(np.uint32) >> FLAG).any()
        np.testing.assert_array_equal(unpack_actions_ref(w), a)
        o.step(a)
    o.close()


# ------------------------------------------------------------------ C ABI (host only)
def test_new_entry_points_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: null pointers, row counts, alignment, a bad
    format value; zero rows launch nothing."""
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    u64 = ctypes.c_uint64
    EINVAL = -1

    def sampler(mask=p, source=p, n=1, hw=16, env0=0, words=p):
        return L.mrts_sample_actions_src_packed(None, mask, source, n, hw, env0, u64(1), 0, words)

    for name in ("mask", "source", "words"):
        assert sampler(**{name: None}) == EINVAL, name
    assert sampler(hw=0) == EINVAL and sampler(n=-1) == EINVAL and sampler(env0=-1) == EINVAL
    assert sampler(n=2 ** 20, hw=2 ** 11) == EINVAL and sampler(words=p + 2) == EINVAL
    assert sampler(n=0) == 0 and sampler(n=0, words=p + 4) == 0

    def pack(act=p, rows=4, words=p):
        return L.mrts_pack_actions(None, act, rows, words)

    def unpack(words=p, rows=4, act=p):
        return L.mrts_unpack_actions(None, words, rows, act)

    for fn in (pack, unpack):
        assert fn(act=None) == EINVAL and fn(words=None) == EINVAL
        assert fn(rows=-1) == EINVAL and fn(rows=2 ** 31 - 256) == EINVAL
        assert fn(act=p + 4) == EINVAL and fn(words=p + 2) == EINVAL          # int64 rows: 8 bytes, words: 4
        assert fn(rows=0) == 0 and fn(rows=0, act=p + 8, words=p + 4) == 0

    def sample(mf=0, af=1, logits=p, mask=p, source=p, n=1, hw=16, env0=0, act=p, lp=p, ent=p):
        return L.mrts_policy_sample_fmt(None, logits, mf, mask, source, n, hw, env0, u64(1), 0, af, act, lp, ent)

    def evaluate(mf=0, af=1, logits=p, mask=p, source=p, n=1, hw=16, act=p, lp=p, ent=p):
        return L.mrts_policy_evaluate_fmt(None, logits, mf, mask, source, n, hw, af, act, lp, ent)

    def backward(mf=0, af=1, logits=p, mask=p, source=p, n=1, hw=16, act=p, glp=p, gent=p, grad=p):
        return L.mrts_policy_evaluate_backward_fmt(None, logits, mf, mask, source, n, hw, af, act, glp, gent, grad)

    for fn, ptrs in ((sample, ("logits", "mask", "act", "lp", "ent")), (evaluate, ("logits", "mask", "act", "lp", "ent")),
                     (backward, ("logits", "mask", "act", "glp", "gent", "grad"))):
        for mf in (0, 1):
            for af in (0, 1):
                for name in ptrs:
                    assert fn(mf=mf, af=af, **{name: None}) == EINVAL, (fn.__name__, mf, af, name)
                assert fn(mf=mf, af=af, n=0) == 0
                assert fn(mf=mf, af=af, hw=0) == EINVAL and fn(mf=mf, af=af, n=-1) == EINVAL
                assert fn(mf=mf, af=af, n=2 ** 20, hw=2 ** 11) == EINVAL
            assert fn(mf=mf, af=0, act=p + 4) == EINVAL and fn(mf=mf, af=1, act=p + 2) == EINVAL
            assert fn(mf=mf, af=1, act=p + 4, n=0) == 0                      # words need 4-byte alignment only
        assert fn(mf=0, source=None) == EINVAL and fn(mf=1, source=None, n=0) == 0   # packed masks carry their source
        for bad in (-1, 2, 7):
            assert fn(mf=bad, n=0) == EINVAL and fn(af=bad, n=0) == EINVAL
    assert sample(env0=-1) == EINVAL
    del buf


def test_set_action_format_checks_its_arguments():
    from gym_microrts import _native

    L = _native.lib()
    assert L.mrts_set_action_format(None, 1) == -1
    h = _native.create(num_selfplay_envs=2, num_bot_envs=0, max_steps=2000, partial_obs=False,
                       map_paths=[os.path.join(MAPS, "maps/8x8/basesWorkers8x8.xml")], game_map=[0], bot_ai=[], obs_dtype=0)
    try:
        for bad in (-1, 2, 3):
            assert L.mrts_set_action_format(h, bad) == -1
            assert b"MRTS_ACT_PACKED" in L.mrts_last_error(h)
        assert L.mrts_set_action_format(h, _native.MRTS_ACT_PACKED) == 0
        assert L.mrts_set_action_format(h, _native.MRTS_ACT_DENSE) == 0
        # the format is no part of the configuration: the snapshot size is the same either way
        n0 = L.mrts_state_bytes(h)
        L.mrts_set_action_format(h, _native.MRTS_ACT_PACKED)
        assert L.mrts_state_bytes(h) == n0
    finally:
        L.mrts_destroy(h)


# ------------------------------------------------------------------ the modules' checks
def test_module_checks_for_packed_actions():
    import torch

    from gym_microrts import packed_actions as pa
    from gym_microrts import policy_head as ph

    a = torch.zeros(2, 16, 7, dtype=torch.int64)
    w = torch.zeros(2, 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="actions is on cpu"):
        pa.pack_actions(a)
    with pytest.raises(ValueError, match="words is on cpu"):
        pa.unpack_actions(w)
    with pytest.raises(ValueError, match="actions must be torch.int64"):
        pa.pack_actions(a.int())
    with pytest.raises(ValueError, match="words must be torch.int32"):
        pa.unpack_actions(w.long())
    with pytest.raises(ValueError, match=r"actions must be \[..., 7\]"):
        pa.pack_actions(a[..., :6].contiguous())
    with pytest.raises(ValueError, match="must be a torch.Tensor"):
        pa.pack_actions(a.numpy())
    n, hw = 2, 16
    lg = torch.zeros(n * hw, 78)
    m = torch.zeros(n, hw, 78, dtype=torch.int32)
    s = torch.zeros(n, hw, dtype=torch.int32)
    pk = torch.zeros(n, hw, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="action_format must be"):
        ph.sample(lg, m, s, seed=1, step=0, action_format="words")
    for call in (lambda x: ph.evaluate(lg, m, s, x), lambda x: ph.evaluate(lg, pk, actions=x)):
        with pytest.raises(ValueError, match="logits is on cpu"):   # words pass the input check: int32, N*HW elements
            call(w)
        with pytest.raises(ValueError, match="logits is on cpu"):
            call(w.reshape(n, 4, 4))
        with pytest.raises(TypeError, match="actions must be torch.int64"):   # int32 of any other size is not words
            call(w[:, :-1])
        with pytest.raises(ValueError, match="actions must hold"):
            call(a[:, :-1])


# ------------------------------------------------------------------ the driver's option
def test_driver_refuses_packed_actions_without_the_fused_head():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    with pytest.raises(ValueError, match="--actions packed needs --head fused"):
        drv.run(actions="packed", head="torch", device="no-such-device")   # raised before the device is touched
    with pytest.raises(ValueError, match="actions must be"):
        drv.run(actions="words", device="no-such-device")
    with pytest.raises(ValueError, match="--head fused needs --api tensor"):
        drv.run(actions="packed", head="fused", api="numpy", device="no-such-device")
