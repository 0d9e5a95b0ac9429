"""Delta observations (mrts_set_obs_delta): k_step stores only the obs rows -- a cell's P
planes -- whose content differs from the one of the state the step loaded, and the obs
buffer still holds the one-hot of the current state, bit for bit, every tick.

Every rollout runs an obs_delta=True engine, an obs_delta=False twin and the CPU oracle on
the same actions and compares the obs as bytes each tick, twin against twin and against the
oracle.  Before every step the delta engine's whole obs buffer is overwritten with a
sentinel: after the step, every row that still holds the sentinel must be a row the dense
twin did not change (the step skipped it, rightly), every other row must hold the twin's
bytes, and the skipped rows are put back before the next tick.  So a step that stored a
wrong row, skipped a changed one, or silently ran dense fails its case; a case that the host
rule keeps dense -- a size past the kernel's bound (47x24), or fog -- must run dense: no
sentinel survives.
"""
import os

import numpy as np
import pytest

from conftest import MAPS, obs_bits_equal
from random_maps import write_random_map

pytestmark = [pytest.mark.gpu]

RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16, M24 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml", "maps/24x24/basesWorkers24x24.xml"
M9x13, M15 = "maps/9x13/basesWorkersWalls9x13.xml", "maps/15x15/basesWorkersWalls15x15.xml"
SENT = 0x7EADBEEF   # as int32 and as float32 bits: neither 0 nor 1 / 1.0f
NVEC = np.array([6, 4, 4, 4, 4, 7, 49])


def _torch():
    import torch

    return torch


def _engine(map_path, nsp, bots, obs_delta=True, max_steps=25, partial_obs=False, obs_dtype="float32", **kw):
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    torch = _torch()
    if "obs_format" not in kw:
        kw["obs_dtype"] = getattr(torch, obs_dtype)
    return MicroRTSGridModeVecEnv(num_selfplay_envs=nsp, num_bot_envs=len(bots), max_steps=max_steps,
                                  ai2s=[getattr(microrts_ai, b) for b in bots], map_paths=[map_path], reward_weight=RW,
                                  partial_obs=partial_obs, return_tensors=True, obs_delta=obs_delta, **kw)


def _oracle(path, nsp, bots, max_steps, partial_obs):
    from oracle_py import OracleVecEnv

    return OracleVecEnv(nsp, len(bots), [path], max_steps=max_steps, partial_obs=partial_obs, ai2s=list(bots) or None, reward_weight=RW)


def _bits(x):
    return x if x.dtype == _torch().int32 else x.view(_torch().int32)


def _rows(x):
    """obs [N, H, W, P] as int32 bit rows [N * H * W, P]"""
    return _bits(x).reshape(-1, x.shape[-1])


def _actions(mo, seed, s, mode, rng):
    from oracle_py import sample_actions

    a = sample_actions(mo, seed, s)
    if mode == "masked":
        return a
    u = (rng.random(a.shape) * NVEC).astype(np.int64)   # ignores the mask: illegal actions, conflicts, bad rows
    if mode == "uniform":
        return u
    return np.where(rng.random(a.shape[:2] + (1,)) < 0.3, u, a)


class Twin:
    """A delta engine, its dense twin and the oracle of one map size, stepped together."""

    def __init__(self, on, off, oracle, expect_delta=True):
        self.on, self.off, self.o, self.expect_delta = on, off, oracle, expect_delta
        self.changed = self.unchanged = self.skipped = 0

    def reset(self):
        a, b, oo = self.on.reset(), self.off.reset(), self.o.reset()
        assert obs_bits_equal(a, oo) and obs_bits_equal(b, oo), "reset obs"

    def before_step(self):
        self.prev = self.off._obs.clone()
        _bits(self.on._obs).fill_(SENT)   # the caller's write is undone in after_step, before the engine reads on

    def after_step(self, obs_on, obs_off, obs_oracle, tag):
        torch = _torch()
        assert obs_on is self.on._obs and obs_off is self.off._obs
        assert obs_bits_equal(obs_off, obs_oracle), f"{tag}: the dense twin's obs against the oracle"
        got, want, prev = _rows(obs_on), _rows(obs_off), _rows(self.prev)
        kept = (got == SENT).all(dim=1)          # rows the step did not store
        same = (want == prev).all(dim=1)         # rows the tick did not change
        assert bool(same[kept].all()), f"{tag}: {int((kept & ~same).sum())} changed rows were not stored"
        assert torch.equal(got[~kept], want[~kept]), f"{tag}: a stored row differs from the dense twin's"
        assert not bool(((got == SENT).any(dim=1) & ~kept).any()), f"{tag}: a row stored in part"
        if not self.expect_delta:
            assert not bool(kept.any()), f"{tag}: a dense step left rows unwritten"
        got[kept] = prev[kept]                   # put the skipped rows back: the buffer is the engine's again
        assert obs_bits_equal(obs_on, obs_oracle), f"{tag}: the delta engine's obs against the oracle"
        self.changed += int((~same).sum())
        self.unchanged += int(same.sum())
        self.skipped += int(kept.sum())

    def finish(self, tag):
        assert self.changed > 0 and self.unchanged > 0, f"{tag}: {self.changed} rows changed, {self.unchanged} did not"
        if self.expect_delta:
            assert self.skipped > 0, f"{tag}: no row was ever skipped: the engine ran dense"
            assert self.skipped == self.unchanged, f"{tag}: {self.unchanged - self.skipped} unchanged rows were stored"
        else:
            assert self.skipped == 0
        assert int(self.on.game_stats()[:, 5].sum()) > 0, f"{tag}: no auto-reset in the rollout"
        assert self.on.error_flags() == 0 and self.off.error_flags() == 0
        self.on.close(), self.off.close(), self.o.close()


def _run(twins, step_on, step_off, ticks, seed, mode="masked"):
    """twins: one per map size; step_on / step_off(list of action tensors) -> list of obs per twin"""
    torch = _torch()
    rng = np.random.default_rng(seed)
    for t in twins:
        t.reset()
    for s in range(ticks):
        acts, oo = [], []
        for t in twins:
            mo = t.o.get_action_mask()
            mg = t.on.get_action_mask()
            t.off.get_action_mask()
            assert torch.equal(mg.cpu(), torch.from_numpy(mo)), f"tick {s}: masks against the oracle"
            a = _actions(mo, seed, s, mode, rng)
            acts.append(torch.from_numpy(a).to(t.on.device))
            oo.append(t.o.step(a)[0])
            t.before_step()
        obs_on, obs_off = step_on(acts), step_off(acts)
        for t, a, b, o in zip(twins, obs_on, obs_off, oo):
            t.after_step(a, b, o, f"tick {s} {t.on.height}x{t.on.width}")
    for t in twins:
        t.finish(f"{t.on.height}x{t.on.width}")


#        name              map (None: random w x h)  nsp bots                            kwargs
CASES = [("8x8_selfplay",    M8,    8,  8,  8, [],                               dict()),
         ("16x16_selfplay",  M16,   16, 16, 8, [],                               dict(max_steps=40, ticks=90)),
         ("16x16_bots_i32",  M16,   16, 16, 4, ["coacAI", "workerRushAI"],        dict(obs_dtype="int32")),   # bot-fused, early bot
         ("16x16_unfused",   M16,   16, 16, 4, ["coacAI", "workerRushAI"],        dict(bot_fusion=False)),
         ("9x13_odd",        M9x13, 9,  13, 4, ["coacAI"],                        dict()),                     # odd HW: rows off 16 B
         ("15x15_i32",       M15,   15, 15, 4, ["workerRushAI"],                  dict(obs_dtype="int32")),
         ("24x24_wide",      M24,   24, 24, 4, ["workerRushAI", "coacAI"],        dict()),                     # several cells per lane
         ("47x24_random",    None,  47, 24, 4, [],                               dict(expect_delta=False)),   # past the bound: dense
         ("16x16_fog",       M16,   16, 16, 4, ["coacAI", "workerRushAI"],        dict(partial_obs=True, expect_delta=False)),               # fog: dense
         ("16x16_fog_i32",   M16,   16, 16, 8, [],                               dict(partial_obs=True, obs_dtype="int32", expect_delta=False)),
         ("16x16_uniform",   M16,   16, 16, 4, ["coacAI", "workerRushAI"],        dict(mode="uniform")),       # adversarial streams
         ("16x16_mixed_i32", M16,   16, 16, 4, ["workerRushAI", "coacAI"],        dict(mode="mixed", obs_dtype="int32")),
         ("24x24_mixed",     M24,   24, 24, 2, ["coacAI"],                        dict(mode="mixed"))]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name,rel,w,h,nsp,bots,kw", CASES, ids=[c[0] for c in CASES])
def test_delta_obs_lockstep_with_a_dense_twin_and_the_oracle(tmp_path, name, rel, w, h, nsp, bots, kw):
    kw = dict(kw)
    ticks, mode, expect = kw.pop("ticks", 45), kw.pop("mode", "masked"), kw.pop("expect_delta", True)
    if rel is None:
        path = gpath = write_random_map(str(tmp_path / f"{name}.xml"), w, h, 5, n_units=60, wall_frac=0.1)
    else:
        path, gpath = os.path.join(MAPS, rel), rel
    on, off = _engine(gpath, nsp, bots, obs_delta=True, **kw), _engine(gpath, nsp, bots, obs_delta=False, **kw)
    assert on.obs_delta and not off.obs_delta
    o = _oracle(path, nsp, bots, kw.get("max_steps", 25), kw.get("partial_obs", False))
    t = Twin(on, off, o, expect)
    _run([t], lambda a: [on.step(a[0])[0]], lambda a: [off.step(a[0])[0]], ticks, seed=11, mode=mode)


@pytest.mark.timeout(180)
def test_delta_obs_lockstep_mixed_sizes_grouped_launch():
    """8x8 / 16x16 / 24x24 buckets in one mrts_step_group call: the delta switch rides per member."""
    torch = _torch()
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSMixedMapVecEnv

    spec = [(M8, 4, ["workerRushAI", "coacAI"]), (M16, 4, ["coacAI", "workerRushAI"]), (M24, 2, ["workerRushAI", "coacAI"])]

    def mk(delta):
        buckets = [dict(map_paths=[m], num_selfplay_envs=nsp, ai2s=[getattr(microrts_ai, a) for a in ais]) for m, nsp, ais in spec]
        return MicroRTSMixedMapVecEnv(buckets, max_steps=25, return_tensors=True, reward_weight=RW, obs_dtype=torch.float32,
                                      obs_delta=delta)

    on, off = mk(True), mk(False)
    assert on.grouped and all(e.obs_delta for e in on.envs) and not any(e.obs_delta for e in off.envs)
    twins = [Twin(a, b, _oracle(os.path.join(MAPS, m), nsp, ais, 25, False)) for a, b, (m, nsp, ais) in zip(on.envs, off.envs, spec)]
    _run(twins, lambda a: on.step(a)[0], lambda a: off.step(a)[0], 45, seed=12)


def _survivors(e, act):
    """Sentinel over the whole obs buffer, one step: the number of rows the step left alone.
    The buffer is left poisoned in those rows (callers invalidate or repair it)."""
    _bits(e._obs).fill_(SENT)
    e.get_action_mask()
    e.step(act)
    return int((_rows(e._obs) == SENT).all(dim=1).sum())


@pytest.mark.timeout(120)
def test_sync_tracking_across_resets_parks_checkpoints_and_buffers():
    """Every entry point that writes obs or changes the state, with steps between: the delta
    engine's obs equal a dense twin's after every call.  A step given another obs buffer runs
    dense, and so does the next step into the first one; mrts_invalidate_obs and
    mrts_set_obs_delta(0) make the next step dense, mrts_set_obs_delta(1) after a dense step
    runs delta again; a packed-obs engine ignores the flag."""
    torch = _torch()
    from gym_microrts import _native
    from oracle_py import sample_actions

    bots = ["workerRushAI", "coacAI", "coacAI", "workerRushAI"]
    e, d = _engine(M16, 8, bots, obs_delta=True, max_steps=40), _engine(M16, 8, bots, obs_delta=False, max_steps=40)
    lib = _native.lib()
    tick = [0]

    def same(tag):
        assert torch.equal(_bits(e._obs), _bits(d._obs)), f"{tag}: obs differ from the dense twin's"

    def act():
        m = d.get_action_mask()
        e.get_action_mask()
        tick[0] += 1
        return torch.from_numpy(sample_actions(m.cpu().numpy(), 21, tick[0])).to(e.device)

    def steps(n, tag):
        for _ in range(n):
            a = act()
            e.step(a), d.step(a)
            same(f"{tag}, tick {tick[0]}")

    def poisoned_step(tag, dense):
        """a step over a poisoned buffer: dense writes every row; delta leaves rows, which are repaired"""
        a = act()
        d.step(a)
        prev = e._obs.clone()
        n = _survivors(e, a)
        assert (n == 0) == dense, f"{tag}: {n} rows survived, dense expected: {dense}"
        if n:
            kept = (_rows(e._obs) == SENT).all(dim=1)
            _rows(e._obs)[kept] = _rows(prev)[kept]
        same(tag)

    e.reset(), d.reset()
    same("reset")
    steps(5, "start")
    poisoned_step("a delta step", dense=False)
    e.reset_games([0, 5]), d.reset_games([0, 5])
    same("reset_games")
    poisoned_step("after reset_games", dense=False)
    steps(3, "after reset_games")
    e.park_games([1, 4, 6]), d.park_games([1, 4, 6])
    same("park_games")
    assert int(_bits(e._obs)[2:4].abs().sum()) == 0, "a parked game's obs are zero"
    poisoned_step("parked", dense=False)
    steps(3, "parked")
    e.reset_games([1, 6]), d.reset_games([1, 6])   # unpark two of them; game 4 stays parked
    same("unpark")
    poisoned_step("after the unpark", dense=False)
    snap_e, snap_d = e.get_state(), d.get_state()
    steps(4, "after the save")
    e.set_state(snap_e), d.set_state(snap_d)
    same("set_state")
    poisoned_step("after the restore", dense=False)
    e.reset_games([4]), d.reset_games([4])   # every game plays: a dense step writes every row of the buffer
    same("unpark the last")
    # a second obs buffer: that step is dense, and so is the next one into the first buffer
    first, second = e._obs, torch.empty_like(e._obs)
    a = act()
    d.step(a)
    e._obs = second
    assert _survivors(e, a) == 0, "a step into another buffer must write every row"
    same("the second buffer")
    a = act()
    d.step(a)
    e._obs = first
    assert _survivors(e, a) == 0, "back in the first buffer, which missed a tick: every row"
    same("the first buffer again")
    poisoned_step("the first buffer, once current", dense=False)
    # reset_games into another buffer leaves the remembered one stale: the next step is dense
    e._obs = second
    e.reset_games([2]), d.reset_games([2])
    e._obs = first
    poisoned_step("after reset_games into another buffer", dense=True)
    poisoned_step("then", dense=False)
    # the caller's write, handed back
    _bits(e._obs)[:, 3, 3, :] = SENT
    e.invalidate_obs()
    steps(1, "after invalidate_obs")
    e.invalidate_obs()
    poisoned_step("invalidate_obs", dense=True)
    _native.check(lib.mrts_set_obs_delta(e._h, 0), e._h, "set_obs_delta")
    poisoned_step("set_obs_delta(0)", dense=True)
    poisoned_step("set_obs_delta(0) again", dense=True)
    _native.check(lib.mrts_set_obs_delta(e._h, 1), e._h, "set_obs_delta")
    poisoned_step("set_obs_delta(1) after a dense step", dense=False)
    e.park_games([5]), d.park_games([5])
    steps(45, "past max_steps")   # auto-resets with a parked game beside
    assert e.error_flags() == 0
    e.close(), d.close()
    # a packed engine writes its words in full, flag or not
    pk = _engine(M16, 4, [], obs_delta=True, obs_format="packed")
    pk.reset()
    noop = torch.zeros((pk.num_envs, 256, 7), dtype=torch.int64, device=pk.device)
    pk.get_action_mask()
    pk.step(noop)
    pk._obs.fill_(-1)
    pk.get_action_mask()
    pk.step(noop)
    assert not bool((pk._obs == -1).any()) and not bool((pk._obs >> 29).any()), "a packed engine must write every word"
    pk.close()
    assert lib.mrts_set_obs_delta(None, 1) == -1 and lib.mrts_invalidate_obs(None) == -1   # MRTS_EINVAL: null handle


@pytest.mark.timeout(120)
@pytest.mark.parametrize("obs_dtype", ["float32", "int32"])
def test_unchanged_rows_are_not_stored_and_invalidate_hands_the_buffer_back(obs_dtype):
    """A sentinel in obs rows that the next tick leaves unchanged survives a delta step and is
    overwritten by a dense one (obs_delta=False); after invalidate_obs() the next step writes
    every row and the buffer is exact again."""
    torch = _torch()

    def run(obs_delta, invalidate):
        e = _engine(M16, 4, [], obs_delta=obs_delta, max_steps=2000, obs_dtype=obs_dtype)
        e.reset()
        noop = torch.zeros((e.num_envs, 256, 7), dtype=torch.int64, device=e.device)
        e.get_action_mask()
        e.step(noop)
        want = e._obs.clone()
        e.get_action_mask()
        e.step(noop)   # no-ops: a NONE that lasts a tick, issued and done within each step
        assert torch.equal(_bits(e._obs), _bits(want)), "a no-op tick changed the obs"
        cells = [(8, 8), (0, 0), (15, 15), (2, 2)]   # mid-map (empty), the corners, a base's corner of the map
        for y, x in cells:
            _bits(e._obs)[:, y, x, :] = SENT
        if invalidate:
            e.invalidate_obs()
        e.get_action_mask()
        e.step(noop)
        rows = torch.stack([_bits(e._obs)[:, y, x, :] for y, x in cells])
        for y, x in cells:
            _bits(e._obs)[:, y, x, :] = _bits(want)[:, y, x, :]
        assert torch.equal(_bits(e._obs), _bits(want)), "every other row"
        e.close()
        return rows, torch.stack([_bits(want)[:, y, x, :] for y, x in cells])

    rows, want = run(True, False)
    assert bool((rows == SENT).all()), "a delta step stored a row that did not change"
    rows, want = run(False, False)
    assert torch.equal(rows, want), "a dense step left the sentinel"
    rows, want = run(True, True)
    assert torch.equal(rows, want), "the step after invalidate_obs() must write every row"
