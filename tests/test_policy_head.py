"""The masked action head (gym_microrts.policy_head, csrc/mrts_policy.hip) on the CPU:
the C ABI's and the module's argument checks, and the helpers the GPU tests
(test_gpu_policy_head.py) share -- a numpy Philox4x32-10 pinned to the oracle's stream,
a float64 reference of the head's contract, and the input sets.

The contract (per row of env e, cell c; component k at OFF[k], LEN[k] wide; V = the
entries the mask allows, none when source == 0):
  V empty : log-prob 0, entropy 0, gradient 0; sampled action (r[k] * LEN[k]) >> 32
  else    : M = max_V l, E_j = exp(l_j - M), S = sum_V E_j, p_j = E_j / S,
            log p_a = (l_a - M) - log S for a in V, -1e8 otherwise; H = -sum_V p_j log p_j;
            sampled action: the first j in V with C_j > u * S, u = (r[k] >> 8) * 2^-24
logprob[e] / entropy[e]: the sums over cells and components, rounded once to float32.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import MAPS

OFF = (0, 6, 10, 14, 18, 22, 29)
LEN = (6, 4, 4, 4, 4, 7, 49)
CH = 78
DELTA = 2.0 ** -15       # sampling comparison: u this close to an interior CDF boundary is left out
LEFT_OUT_CAP = 0.01
LP_INVALID = -1.0e8


# ------------------------------------------------------------------ Philox4x32-10
def philox_rows(n, hw, seed, step, env0=0):
    """The eight words of every row: two Philox4x32-10 blocks of counter
    (cell, env0 + env, step, 0|1), key = the seed's two halves.  uint32 [n, hw, 8]."""
    out = np.zeros((n, hw, 8), np.uint64)
    e, c = np.meshgrid(np.arange(env0, env0 + n, dtype=np.uint64), np.arange(hw, dtype=np.uint64), indexing="ij")
    m32 = np.uint64(0xFFFFFFFF)
    for h in range(2):
        c0, c1, c2, c3 = c.copy(), e.copy(), np.full_like(c, step), np.full_like(c, h)
        k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
            c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        for i, w in enumerate((c0, c1, c2, c3)):
            out[:, :, 4 * h + i] = w
    return out.astype(np.uint32)


def no_valid_draw(r):
    """(r[k] * LEN[k]) >> 32: the draw of a component without valid entries.  int64 [..., 7]."""
    return (r[..., :7].astype(np.uint64) * np.array(LEN, np.uint64)) >> np.uint64(32)


# ------------------------------------------------------------------ float64 reference
class Reference:
    """The contract in float64 numpy.  Per component arrays are [n, hw]; `valid` is
    the set V as bool [n, hw, 78]."""

    def __init__(self, logits, mask, source):
        n, hw = source.shape
        self.n, self.hw = n, hw
        self.l = np.asarray(logits, np.float32).reshape(n, hw, CH).astype(np.float64)
        self.valid = (np.asarray(mask).reshape(n, hw, CH) != 0) & (np.asarray(source) != 0)[:, :, None]
        self.comp = []
        for off, ln in zip(OFF, LEN):
            v, l = self.valid[:, :, off:off + ln], self.l[:, :, off:off + ln]
            some = v.any(-1)
            M = np.where(some, np.where(v, l, -np.inf).max(-1), 0.0)
            E = np.where(v, np.exp(np.where(v, l - M[..., None], 0.0)), 0.0)
            S = np.where(some, E.sum(-1), 1.0)
            p = E / S[..., None]
            logp = np.where(v, (l - M[..., None]) - np.log(S)[..., None], 0.0)
            H = -(p * logp).sum(-1)
            self.comp.append(dict(v=v, some=some, E=E, S=S, p=p, logp=logp, H=H))

    def entropy(self):
        return sum(c["H"] for c in self.comp).sum(1)

    def logprob(self, actions):
        a = np.asarray(actions).reshape(self.n, self.hw, 7)
        tot = np.zeros((self.n, self.hw))
        for k, c in enumerate(self.comp):
            ak = a[:, :, k]
            inr = (ak >= 0) & (ak < LEN[k])
            ac = np.where(inr, ak, 0)[..., None]
            ok = inr & np.take_along_axis(c["v"], ac, -1)[..., 0]
            lp = np.where(ok, np.take_along_axis(c["logp"], ac, -1)[..., 0], LP_INVALID)
            tot += np.where(c["some"], lp, 0.0)
        return tot.sum(1)

    def sample(self, r):
        """(actions int64 [n, hw, 7], compare bool [n, hw, 7]): the inverse-CDF picks at
        the words r, and which components the comparison keeps (u farther than DELTA from
        every interior boundary of the CDF; components without valid entries always)."""
        act = no_valid_draw(r).astype(np.int64)
        keep = np.ones(act.shape, bool)
        for k, c in enumerate(self.comp):
            u = (r[:, :, k] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
            C = np.cumsum(c["E"], -1)
            hit = c["v"] & (C > (u * c["S"])[..., None])
            last = LEN[k] - 1 - np.argmax(c["v"][..., ::-1], -1)
            pick = np.where(hit.any(-1), np.argmax(hit, -1), last)
            act[:, :, k] = np.where(c["some"], pick, act[:, :, k])
            interior = c["v"] & (np.arange(LEN[k]) != last[..., None])
            near = interior & (np.abs(C / c["S"][..., None] - u[..., None]) <= DELTA)
            keep[:, :, k] = ~(c["some"] & near.any(-1))
        return act, keep

    def left_out_share(self, keep):
        some = np.stack([c["some"] for c in self.comp], -1)
        return float((~keep).sum()) / max(1, int(some.sum()))


# ------------------------------------------------------------------ input sets
def real_masks(n, ticks=30):
    """Masks and the source channel of a stepped 16x16 game (the oracle's getMasks)."""
    from oracle_py import OracleVecEnv, sample_actions

    o = OracleVecEnv(n + n % 2, 0, [os.path.join(MAPS, "maps/16x16/basesWorkers16x16.xml")], max_steps=2000)
    o.reset()
    for s in range(ticks):
        o.step(sample_actions(o.get_action_mask(), 11, s))
    m = np.array(o.get_action_mask()[:n], np.int32)
    src = np.array(o.source_unit_mask[:n], np.int32).reshape(n, -1)
    o.close()
    return m, src


def synthetic_masks(rng, n, hw, density):
    """Source cells at `density`; a source row's components have no, one, all or a
    random subset of their entries valid.  Some non-source rows carry mask bits too:
    the head must not look at them."""
    src = (rng.random((n, hw)) < density).astype(np.int32)
    m = np.zeros((n, hw, CH), np.int32)
    for off, ln in zip(OFF, LEN):
        kind = rng.integers(0, 4, (n, hw))
        one = np.zeros((n, hw, ln), np.int32)
        np.put_along_axis(one, rng.integers(0, ln, (n, hw, 1)), 1, -1)
        sub = (rng.random((n, hw, ln)) < 0.5).astype(np.int32)
        m[:, :, off:off + ln] = np.select([kind[..., None] == 0, kind[..., None] == 1, kind[..., None] == 2],
                                          [0, one, 1], sub)
    stray = (rng.random((n, hw)) < 0.1) & (src == 0)
    m[(src == 0) & ~stray] = 0
    return m, src


#            name               hw   n   masks    logits    seed
INPUT_SETS = [("4x4_dense",     16,  1, 1.0,    "normal", 101),
              ("8x8_sparse",    64,  3, 0.05,   "normal", 102),
              ("8x8_dense_big", 64,  1, 1.0,    "big",    103),
              ("9x13_dense",    117, 3, 1.0,    "normal", 104),
              ("9x13_sparse",   117, 40, 0.05,  "big",    105),
              ("16x16_sparse",  256, 40, 0.05,  "normal", 106),
              ("16x16_empty",   256, 3, 0.0,    "equal",  107),
              ("16x16_real",    256, 3, "real", "normal", 108),
              ("24x24_dense",   576, 3, 1.0,    "equal",  109),
              ("24x24_sparse",  576, 40, 0.05,  "normal", 110)]
INPUT_IDS = [s[0] for s in INPUT_SETS]
_cache = {}


def inputs(name):
    """One input set, built once: dict(hw, n, seed, step, logits f32 [n*hw, 78], mask i32,
    source i32, ref = Reference, r = the Philox words, actions / keep = the reference's draw)."""
    if name not in _cache:
        _, hw, n, masks, kind, seed = INPUT_SETS[INPUT_IDS.index(name)]
        rng = np.random.default_rng(seed)
        mask, src = real_masks(n) if masks == "real" else synthetic_masks(rng, n, hw, masks)
        if kind == "normal":
            lg = (3.0 * rng.standard_normal((n * hw, CH))).astype(np.float32)
        elif kind == "equal":
            lg = np.full((n * hw, CH), 0.75, np.float32)
        else:   # magnitudes of +-80: exp overflows float32 unless the max is subtracted
            lg = (80.0 * rng.choice([-1.0, 1.0], (n * hw, CH)) + rng.standard_normal((n * hw, CH))).astype(np.float32)
        step = seed % 7
        ref = Reference(lg, mask, src)
        r = philox_rows(n, hw, seed, step)
        actions, keep = ref.sample(r)
        _cache[name] = dict(hw=hw, n=n, seed=seed, step=step, logits=lg, mask=mask, source=src, ref=ref, r=r, actions=actions,
                            keep=keep)
    return _cache[name]


# ------------------------------------------------------------------ the helpers themselves
def test_numpy_philox_is_the_oracles_stream():
    """With an all-zero mask the oracle's sampler returns (r[k] * len_k) >> 32."""
    from oracle_py import sample_actions

    for n, hw, seed, step, env0 in ((3, 117, 0x0123456789ABCDEF, 5, 0), (2, 256, 9, 0, 4096), (1, 16, 2 ** 63 + 12345, 4000000000, 7)):
        want = sample_actions(np.zeros((n, hw, CH), np.int32), seed, step, env0=env0)
        np.testing.assert_array_equal(no_valid_draw(philox_rows(n, hw, seed, step, env0)).astype(np.int64), want)
    np.testing.assert_array_equal(philox_rows(40, 64, 9, 5)[20:], philox_rows(20, 64, 9, 5, env0=20))


def test_reference_matches_the_reference_projects_float32_rules():
    """The contract's two float32 facts, with torch's Categorical over
    where(mask, logits, -1e8) (experiments/ppo_gridnet.py:164-167): a fully masked
    component gives log-prob 0 and entropy 0, a masked action gives -1e8."""
    import torch
    from torch.distributions import Categorical

    lg = torch.tensor([[0.3, -1.2, 2.0, 0.1]])
    none = Categorical(logits=torch.where(torch.zeros(1, 4, dtype=torch.bool), lg, torch.tensor(-1e8)))
    assert float(none.log_prob(torch.tensor([2]))) == 0.0 and float(none.entropy()) == 0.0
    some = Categorical(logits=torch.where(torch.tensor([[True, False, True, False]]), lg, torch.tensor(-1e8)))
    assert float(some.log_prob(torch.tensor([1]))) == -1e8
    mask, src = np.zeros((1, 1, CH), np.int32), np.ones((1, 1), np.int32)
    mask[0, 0, [6, 8]] = 1
    row = np.zeros((1, CH), np.float32)
    row[0, 6:10] = lg.numpy()
    ref = Reference(row, mask, src)
    a = np.zeros((1, 1, 7), np.int64)
    a[0, 0, 1] = 2
    assert abs(ref.logprob(a)[0] - float(some.log_prob(torch.tensor([2])))) < 1e-6
    assert abs(ref.entropy()[0] - float(some.entropy())) < 1e-6
    a[0, 0, 1] = 1
    assert ref.logprob(a)[0] == LP_INVALID
    a[0, 0, 1] = 99   # out of range: the same value, no index
    assert ref.logprob(a)[0] == LP_INVALID


@pytest.mark.parametrize("name", INPUT_IDS)
def test_left_out_share_of_the_sampling_comparison(name):
    """Per input set of the GPU tests, from the reference alone: the components whose
    u lies within DELTA of an interior CDF boundary are at most 1 % (expected worst,
    a full 49-wide component: 2 * DELTA * 48 = 0.3 %), and the reference's draw is valid."""
    d = inputs(name)
    share = d["ref"].left_out_share(d["keep"])
    print(f"{name}: left out {share:.5f}")
    assert share <= LEFT_OUT_CAP
    for k, c in enumerate(d["ref"].comp):
        ak = d["actions"][:, :, k]
        assert ((ak >= 0) & (ak < LEN[k])).all()
        assert np.take_along_axis(c["v"], ak[..., None], -1)[..., 0][c["some"]].all()
    if name in ("9x13_sparse", "16x16_sparse", "24x24_dense", "24x24_sparse"):   # the synthetic component kinds are all there
        wide = d["ref"].comp[6]["v"].sum(-1)[d["source"] != 0]
        assert (wide == 0).any() and (wide == 1).any() and (wide == 49).any()


# ------------------------------------------------------------------ C ABI (host only)
def _abi_args():
    buf = (ctypes.c_uint8 * 4096)()
    return ctypes.addressof(buf), buf


def test_entry_points_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: null pointers, hw < 1, negative
    counts, num_envs * hw beyond the samplers' row bound."""
    from gym_microrts import _native

    L = _native.lib()
    p, keep = _abi_args()
    u64 = ctypes.c_uint64
    EINVAL = -1

    def sample(logits=p, mask=p, source=p, n=1, hw=16, env0=0, act=p, lp=p, ent=p):
        return L.mrts_policy_sample(None, logits, mask, source, n, hw, env0, u64(1), 0, act, lp, ent)

    def evaluate(logits=p, mask=p, source=p, n=1, hw=16, act=p, lp=p, ent=p):
        return L.mrts_policy_evaluate(None, logits, mask, source, n, hw, act, lp, ent)

    def backward(logits=p, mask=p, source=p, n=1, hw=16, act=p, glp=p, gent=p, grad=p):
        return L.mrts_policy_evaluate_backward(None, logits, mask, source, n, hw, act, glp, gent, grad)

    for fn, ptrs in ((sample, ("logits", "mask", "source", "act", "lp", "ent")),
                     (evaluate, ("logits", "mask", "source", "act", "lp", "ent")),
                     (backward, ("logits", "mask", "source", "act", "glp", "gent", "grad"))):
        for name in ptrs:
            assert fn(**{name: None}) == EINVAL, (fn.__name__, name)
        assert fn(hw=0) == EINVAL and fn(hw=-3) == EINVAL and fn(n=-1) == EINVAL
        assert fn(n=2 ** 20, hw=2 ** 11) == EINVAL            # 2^31 rows
        assert fn(n=(2 ** 31 - 256) // 1128 + 1, hw=1128) == EINVAL
        assert fn(n=0) == 0                                   # nothing to launch
    assert sample(env0=-1) == EINVAL
    del keep


# ------------------------------------------------------------------ the module's checks
def test_module_rejects_cpu_tensors_and_wrong_dtypes_or_shapes():
    import torch

    from gym_microrts import policy_head as ph

    n, hw = 2, 16
    lg = torch.zeros(n * hw, CH)
    m = torch.zeros(n, hw, CH, dtype=torch.int32)
    s = torch.zeros(n, hw, dtype=torch.int32)
    a = torch.zeros(n, hw, 7, dtype=torch.int64)
    for call in (lambda **k: ph.sample(k.get("lg", lg), k.get("m", m), k.get("s", s), seed=1, step=0),
                 lambda **k: ph.evaluate(k.get("lg", lg), k.get("m", m), k.get("s", s), k.get("a", a))):
        with pytest.raises(ValueError, match="logits is on cpu"):
            call()
        with pytest.raises(TypeError, match="logits must be torch.float32"):
            call(lg=lg.double())
        with pytest.raises(TypeError, match="mask must be"):
            call(m=m.bool())
        with pytest.raises(TypeError, match="source must be"):
            call(s=s.long())
        with pytest.raises(TypeError, match="mask must be a torch.Tensor"):
            call(m=m.numpy())
        with pytest.raises(ValueError, match="mask must be"):
            call(m=m.reshape(n * hw, CH))
        with pytest.raises(ValueError, match="source must be"):
            call(s=s.reshape(-1))
        with pytest.raises(ValueError, match="logits must be"):
            call(lg=lg[:-1])
        with pytest.raises(ValueError, match="logits must be"):
            call(lg=torch.zeros(n, hw, CH + 1))
    with pytest.raises(TypeError, match="mask must be torch.int32"):   # sample takes the engine's own tensors only
        ph.sample(lg, m.float(), s, seed=1, step=0)
    with pytest.raises(TypeError, match="actions must be torch.int64"):
        ph.evaluate(lg, m, s, a.int())
    with pytest.raises(ValueError, match="actions must hold"):
        ph.evaluate(lg, m, s, a[:, :-1])
    with pytest.raises(ValueError, match="logits is on cpu"):   # the rollout buffer's float copies pass the dtype check
        ph.evaluate(lg, m.float(), s.float(), a)
