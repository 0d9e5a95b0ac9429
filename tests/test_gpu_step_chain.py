"""The step kernel's per-game chain against the CPU oracle, tick by tick, on every path of
k_step: the full-workgroup kernel (16x16 on 256 lanes, k_step's FULL: the map's H*W equals
the workgroup size and is a compile-time constant) in each of its obs kinds, and the general
kernel for every other shape -- including a 16x16 engine that shares a launch with an 8x8 one
and so takes the general kernel at 256 lanes.

Each case steps an engine and the oracle for 96 ticks on random masked actions from the
device sampler and compares, as bytes, every tick: obs, masks, source, raw rewards, weighted
rewards and dones; the engine's error flags stay 0.  Four selfplay envs with max_steps = 24
put auto-resets inside the run; the reward weights are non-trivial.  The shapes: 8x8 (64
lanes), 9x13 (odd H*W, 128 lanes), 15x15 and 16x16 (one cell per lane), 24x24 (wide prefetch,
three cells per lane), 17x16 and 32x32 (the wide prefetch's boundaries: two cells per lane with a
partly idle wave in the second pass, and exactly four), 47x24 (the unprefetched path), 16x16
under fog (31 planes, dense), 16x16 against the device coacAI with bot fusion (the fused
instantiation, early bot), an 8x8 + 16x16 group in one launch, and the 256-lane kernel's other
obs kinds: dense streams (both deltas off), int32 and packed obs.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import MAPS, obs_bits_equal
from random_maps import write_random_map

pytestmark = [pytest.mark.gpu]

RW = np.array([10.0, -1.5, 1.0, 0.2, 3.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"
M9x13, M15 = "maps/9x13/basesWorkersWalls9x13.xml", "maps/15x15/basesWorkersWalls15x15.xml"
TICKS, MAX_STEPS, NSP = 96, 24, 4


def _engine(map_path, bots=(), **kw):
    import torch

    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    if "obs_format" not in kw:
        kw["obs_dtype"] = getattr(torch, kw.pop("obs_dtype", "float32"))
    return MicroRTSGridModeVecEnv(num_selfplay_envs=NSP, num_bot_envs=len(bots), max_steps=MAX_STEPS,
                                  ai2s=[getattr(microrts_ai, b) for b in bots], map_paths=[map_path], reward_weight=RW,
                                  return_tensors=True, **kw)


def _oracle(path, bots, partial_obs):
    from oracle_py import OracleVecEnv

    return OracleVecEnv(NSP, len(bots), [path], max_steps=MAX_STEPS, partial_obs=partial_obs, ai2s=list(bots) or None, reward_weight=RW)


def _obs_equal(e, obs, want):
    if e.obs_format == "packed":
        from gym_microrts.packed_obs import unpack_obs

        import torch

        obs = unpack_obs(obs, want.shape[-1], dtype=torch.int32)
    return obs_bits_equal(obs, want)


class Pair:
    """One engine and its oracle."""

    def __init__(self, e, o):
        import torch

        self.e, self.o = e, o
        self.act = torch.empty((e.num_envs, e.height * e.width, 7), dtype=torch.int64, device=e.device)

    def sample(self, seed, s, tag):
        """the tick's masks against the oracle's, then random masked actions from the device sampler"""
        import torch

        from gym_microrts import _native

        e = self.e
        want = self.o.get_action_mask_full()
        got = e.get_action_mask()
        assert torch.equal(got.cpu(), torch.from_numpy(want[:, :, 1:])), f"{tag}: masks"
        assert torch.equal(e._src.cpu(), torch.from_numpy(want[:, :, 0])), f"{tag}: source"
        self.o.source_unit_mask = np.ascontiguousarray(want[:, :, 0])
        _native.check(_native.lib().mrts_sample_actions_src(e._stream(), e._mask.data_ptr(), e._src.data_ptr(), e.num_envs,
                                                            e.height * e.width, 0, ctypes.c_uint64(seed), s, self.act.data_ptr()))
        return self.act

    def oracle_step(self):
        raw, done = self.o.step_raw(self.act.cpu().numpy())
        return raw, done, self.o.encode(self.o.raw_obs())

    def compare(self, out, want, tag):
        import torch

        e = self.e
        obs, rew, done0, _ = out
        raw, done, oobs = want
        assert _obs_equal(e, obs, oobs), f"{tag}: obs"
        assert np.array_equal(e._raw.cpu().numpy().view(np.uint64), raw.view(np.uint64)), f"{tag}: raw rewards"
        assert np.array_equal(e._done.cpu().numpy().astype(bool), done), f"{tag}: dones"
        weighted = np.zeros(len(raw))
        for k in range(6):   # the reference's raw @ reward_weight, summed in order
            weighted = weighted + raw[:, k] * RW[k]
        assert np.array_equal(rew.cpu().numpy().view(np.uint64), weighted.view(np.uint64)), f"{tag}: weighted rewards"
        assert np.array_equal(done0.cpu().numpy().astype(bool), done[:, 0]), f"{tag}: done[:, 0]"
        assert e.error_flags() == 0, f"{tag}: engine error flags"
        torch.cuda.synchronize()

    def finish(self, tag):
        assert int(self.e.game_stats()[:, 5].sum()) > 0, f"{tag}: no auto-reset in the rollout"
        self.e.close(), self.o.close()


def _lockstep(pairs, step, seed):
    """pairs: one per map size; step(list of action tensors) -> one output tuple per pair"""
    for p in pairs:
        assert _obs_equal(p.e, p.e.reset(), p.o.reset()), "reset obs"
    for s in range(TICKS):
        acts = [p.sample(seed, s, f"tick {s} {p.e.height}x{p.e.width}") for p in pairs]
        want = [p.oracle_step() for p in pairs]
        for p, out, w in zip(pairs, step(acts), want):
            p.compare(out, w, f"tick {s} {p.e.height}x{p.e.width}")
    for p in pairs:
        p.finish(f"{p.e.height}x{p.e.width}")


#        name            map (None: random w x h)  bots        engine kwargs
CASES = [("8x8",           M8,    8,  8,  [],         dict()),
         ("9x13_odd",      M9x13, 9,  13, [],         dict()),
         ("15x15",         M15,   15, 15, [],         dict()),
         ("16x16",         M16,   16, 16, [],         dict()),
         ("24x24_wide",    M24,   24, 24, [],         dict()),
         ("17x16_wide2",   None,  17, 16, [],         dict()),   # two cells per lane, the second pass a quarter of one wave
         ("32x32_wide4",   None,  32, 32, [],         dict()),   # exactly 4 x 256 cells: the last size the prefetch serves
         ("47x24_unpf",    None,  47, 24, [],         dict()),
         ("16x16_fog",     M16,   16, 16, [],         dict(partial_obs=True)),
         ("16x16_coac",    M16,   16, 16, ["coacAI"], dict(bot_fusion=True)),
         ("16x16_coac_unfused", M16, 16, 16, ["coacAI"], dict(bot_fusion=False)),   # the full-workgroup kernel with a bot game
         ("16x16_dense",   M16,   16, 16, [],         dict(obs_delta=False, mask_delta=False)),
         ("16x16_i32",     M16,   16, 16, [],         dict(obs_dtype="int32")),
         ("16x16_packed",  M16,   16, 16, [],         dict(obs_format="packed"))]


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name,rel,w,h,bots,kw", CASES, ids=[c[0] for c in CASES])
def test_step_chain_lockstep_with_the_oracle(tmp_path, name, rel, w, h, bots, kw):
    if rel is None:
        path = gpath = write_random_map(str(tmp_path / f"{name}.xml"), w, h, 5, n_units=60, wall_frac=0.1)
    else:
        path, gpath = os.path.join(MAPS, rel), rel
    e = _engine(gpath, bots, **kw)
    assert (e.height, e.width) == (h, w)
    p = Pair(e, _oracle(path, bots, kw.get("partial_obs", False)))
    _lockstep([p], lambda a: [e.step(a[0])], seed=31)


@pytest.mark.timeout(60)
def test_step_chain_lockstep_mixed_group_in_one_launch():
    """8x8 + 16x16 in one mrts_step_group launch: each segment's games take their own engine's grid."""
    import torch

    from gym_microrts.envs.vec_env import MicroRTSMixedMapVecEnv

    spec = [M8, M16]
    env = MicroRTSMixedMapVecEnv([dict(map_paths=[m], num_selfplay_envs=NSP, ai2s=[]) for m in spec], max_steps=MAX_STEPS,
                                 return_tensors=True, reward_weight=RW, obs_dtype=torch.float32)
    assert env.grouped and env.launch_plan()[1] == 1, "the two buckets must share one launch"
    pairs = [Pair(e, _oracle(os.path.join(MAPS, m), [], False)) for e, m in zip(env.envs, spec)]

    def step(acts):
        out = env.step(acts)   # (obs list, reward list, done list, infos list)
        return [tuple(o[b] for o in out) for b in range(len(spec))]

    _lockstep(pairs, step, seed=32)
