"""Delta masks (mrts_set_mask_delta): k_step stores only the mask rows that can differ
from what the bound buffer holds -- the source rows of the state it loads and of the
state it leaves -- and the buffer still holds getMasks(0) of the current state, bit for
bit, every tick.

The reference for the masks is the standalone mask kernel (mrts_get_masks into scratch
tensors: k_masks' dense path on the stored state) after every step, as in
test_eager_masks_equal_mask_kernel; every rollout also runs a twin env with
mask_delta=False on the same actions and compares obs / rewards / dones / masks.
Actions are random masked ones from the device sampler, so units die and rows go from
source to empty; max_steps is about 40, so time-limit auto-resets recur.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu]

W = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"
M9x13 = "maps/9x13/basesWorkersWalls9x13.xml"


def _engine(map_path, nsp, bots, mask_delta=True, max_steps=40, partial_obs=False, obs_dtype="int32"):
    import torch

    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    return MicroRTSGridModeVecEnv(num_selfplay_envs=nsp, num_bot_envs=len(bots), max_steps=max_steps,
                                  ai2s=[getattr(microrts_ai, b) for b in bots], map_paths=[map_path], reward_weight=W,
                                  partial_obs=partial_obs, return_tensors=True, obs_dtype=getattr(torch, obs_dtype),
                                  mask_delta=mask_delta)


class Checker:
    """One engine's dense reference: mrts_get_masks into scratch tensors of its own."""

    def __init__(self, e):
        import torch

        self.e = e
        hw = e.height * e.width
        self.m = torch.full((e.num_envs, hw, 78), -1, dtype=torch.int32, device=e.device)
        self.s = torch.full((e.num_envs, hw), -1, dtype=torch.int32, device=e.device)
        self.act = torch.empty((e.num_envs, hw, 7), dtype=torch.int64, device=e.device)

    def check(self, tag):
        import torch

        from gym_microrts import _native

        e = self.e
        _native.check(_native.lib().mrts_get_masks(e._h, e._stream(), self.m.data_ptr(), self.s.data_ptr()), e._h, "get_masks")
        assert e._mask_fresh, tag
        if not torch.equal(e._mask, self.m):
            bad = (e._mask != self.m).any(dim=2).nonzero()
            raise AssertionError(f"{tag}: {len(bad)} mask rows differ from k_masks, first (env, cell) {bad[:8].tolist()}")
        assert torch.equal(e._src, self.s), f"{tag}: source"

    def sample(self, seed, s):
        from gym_microrts import _native

        e = self.e
        _native.check(_native.lib().mrts_sample_actions_src(e._stream(), e._mask.data_ptr(), e._src.data_ptr(), e.num_envs,
                                                            e.height * e.width, 0, ctypes.c_uint64(seed), s, self.act.data_ptr()))
        return self.act


def _same_outputs(a, b, tag):
    import torch

    for k, (x, y) in enumerate(zip(a[:3], b[:3])):
        assert torch.equal(x, y), f"{tag}: output {k} (obs, reward, done) differs between delta on and off"


def _lockstep(on, off, ticks, seed):
    """`on` (delta) and `off` (dense) engines, or lists of them stepped by a mixed env."""
    import torch

    on.reset()
    off.reset()
    es_on = getattr(on, "envs", [on])
    es_off = getattr(off, "envs", [off])
    cks = [Checker(e) for e in es_on]
    for c in cks:
        c.check("reset")
    for s in range(ticks):
        on.get_action_mask()
        off.get_action_mask()
        acts = [c.sample(seed, s) for c in cks]
        a = acts if hasattr(on, "envs") else acts[0]
        out_on, out_off = on.step(a), off.step(a)
        if hasattr(on, "envs"):
            for b in range(len(es_on)):
                _same_outputs([o[b] for o in out_on], [o[b] for o in out_off], f"step {s} bucket {b}")
        else:
            _same_outputs(out_on, out_off, f"step {s}")
        for c, eo in zip(cks, es_off):
            c.check(f"step {s} {c.e.height}x{c.e.width}")
            assert torch.equal(c.e._mask, eo._mask), f"step {s}: delta on vs off"
    episodes = sum(int(e.game_stats()[:, 5].sum()) for e in es_on)
    assert episodes > 0, "no auto-reset in the rollout"
    assert on.error_flags() == 0
    on.close()
    off.close()


CASES = {
    # selfplay (masks first), bot-fused and early-bot workgroups in one launch, int32 obs
    "16x16_bots": dict(map_path=M16, nsp=8, bots=["workerRushAI", "workerRushAI", "coacAI", "coacAI"]),
    # odd H*W: rows are 8-byte aligned only
    "9x13_odd": dict(map_path=M9x13, nsp=6, bots=["coacAI"], obs_dtype="float32"),
    # pf_wide: several cells per lane
    "24x24_wide": dict(map_path=M24, nsp=4, bots=["workerRushAI", "coacAI"], obs_dtype="float32"),
    # 31 planes: the sight disks between the mask and the obs stream
    "16x16_partial": dict(map_path=M16, nsp=8, bots=["coacAI", "workerRushAI"], partial_obs=True),
    # one cell per lane in a 64-lane workgroup, no bots
    "8x8_selfplay": dict(map_path=M8, nsp=8, bots=[], obs_dtype="float32"),
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", sorted(CASES))
def test_delta_masks_lockstep(case):
    _lockstep(_engine(mask_delta=True, **CASES[case]), _engine(mask_delta=False, **CASES[case]), 200, seed=11)


@pytest.mark.timeout(180)
def test_delta_masks_lockstep_mixed_sizes_grouped_launch():
    """8x8 / 16x16 / 24x24 buckets in one mrts_step_group call: the delta switch rides per member."""
    import torch

    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSMixedMapVecEnv

    def mk(delta):
        buckets = [dict(map_paths=[m], num_selfplay_envs=nsp, ai2s=[getattr(microrts_ai, a) for a in ais])
                   for m, nsp, ais in [(M8, 4, ["workerRushAI", "coacAI"]), (M16, 4, ["coacAI", "workerRushAI", "coacAI", "workerRushAI"]),
                                       (M24, 2, ["workerRushAI", "coacAI"])]]
        return MicroRTSMixedMapVecEnv(buckets, max_steps=40, return_tensors=True, reward_weight=W, obs_dtype=torch.float32,
                                      mask_delta=delta)

    on, off = mk(True), mk(False)
    assert on.grouped and all(e.mask_delta for e in on.envs) and not any(e.mask_delta for e in off.envs)
    _lockstep(on, off, 200, seed=12)


@pytest.mark.timeout(120)
def test_sync_tracking_across_rebind_resets_parks_and_checkpoints():
    """Poisoned buffers + re-bind: the next step writes every row (dense fallback).  Then
    reset_games, park_games / unpark, a checkpoint save / restore and an explicit
    get_action_mask() after _mask_fresh = False, with steps between: the bound buffers are
    exact after every step."""
    from gym_microrts import _native

    e = _engine(M16, 8, ["workerRushAI", "coacAI", "coacAI", "workerRushAI"], mask_delta=True)
    ck = Checker(e)
    e.reset()
    tick = [0]

    def steps(n, tag):
        for _ in range(n):
            e.get_action_mask()
            e.step(ck.sample(21, tick[0]))
            ck.check(f"{tag}, tick {tick[0]}")
            tick[0] += 1

    steps(10, "start")
    # the caller scribbles over both buffers and hands them back by binding again (the
    # tick's actions are drawn first; the step's source argument is the poisoned buffer,
    # all non-zero, which selects the row of every idle unit: the same rows as before)
    e.get_action_mask()
    act = ck.sample(21, tick[0])
    e._mask.fill_(0x5A5A5A5A)
    e._src.fill_(0x5A5A5A5A)
    _native.check(_native.lib().mrts_bind_mask_outputs(e._h, e._mask.data_ptr(), e._src.data_ptr()), e._h, "bind_mask_outputs")
    e.step(act)
    tick[0] += 1
    ck.check("dense step after the re-bind")
    steps(6, "after the re-bind")
    e.reset_games([0, 5])
    ck.check("reset_games")
    steps(6, "after reset_games")
    e.park_games([1, 4, 6])
    ck.check("park_games")
    steps(6, "parked")
    e.reset_games([1, 6])   # unpark two of them; game 4 stays parked
    ck.check("unpark")
    steps(6, "after the unpark")
    snap = e.get_state()
    steps(9, "after the save")
    e.set_state(snap)
    ck.check("set_state")
    steps(9, "after the restore")
    e._mask_fresh = False
    e.get_action_mask()   # k_masks into the bound buffers
    ck.check("explicit get_action_mask")
    steps(45, "after get_action_mask")   # past max_steps: auto-resets with a parked game beside
    assert e.error_flags() == 0
    e.close()


@pytest.mark.timeout(120)
def test_untouched_rows_are_not_stored_and_rebinding_hands_the_buffer_back():
    """A sentinel in the mask row of a cell that is no source cell before or after the
    step survives a delta step, is overwritten with zeros by a dense step
    (mask_delta=False), and also by a delta-enabled step that follows a re-bind."""
    import torch

    from gym_microrts import _native

    SENT = 0x7EADBEEF

    def run(mask_delta, rebind):
        e = _engine(M16, 4, [], mask_delta=mask_delta, max_steps=2000)
        hw = e.height * e.width
        e.reset()
        e.get_action_mask()
        noop = torch.zeros((e.num_envs, hw, 7), dtype=torch.int64, device=e.device)
        e.step(noop)
        cell = 8 * 16 + 8   # mid-map: empty on basesWorkers16x16
        before = e._src.clone()
        assert int(before[:, cell].abs().sum()) == 0 and int(e._mask[:, cell].abs().sum()) == 0
        e._mask[:, cell, :] = SENT
        if rebind:
            _native.check(_native.lib().mrts_bind_mask_outputs(e._h, e._mask.data_ptr(), e._src.data_ptr()), e._h, "bind")
        e.step(noop)
        assert int(e._src[:, cell].abs().sum()) == 0, "the cell became a source cell"
        row = e._mask[:, cell, :].clone()
        # every other row is what the mask kernel writes
        ck = Checker(e)
        e._mask[:, cell, :] = 0
        ck.check("other rows")
        e.close()
        return row

    assert bool((run(True, False) == SENT).all()), "a delta step stored a row that cannot have changed"
    assert int(run(False, False).abs().sum()) == 0, "a dense step left the sentinel"
    assert int(run(True, True).abs().sum()) == 0, "the step after a re-bind must write every row"
