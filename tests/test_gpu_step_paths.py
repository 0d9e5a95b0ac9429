"""One step path: mrts_step / mrts_step_weighted are mrts_step_group with one member.

Engine A steps through env.step (mrts_step_weighted); its twin B, of the same
configuration and fed the same device-sampled actions, through a direct
mrts_step_group(hs, 1, ..) built from _step_io(), under policy 0 and under
MERGE_FIT | BOTS_FIRST.  Every tick obs, raw reward, done, reward, done0 and the bound
mask and source tensors are equal bit for bit.  max_steps is 40, so time-limit
auto-resets recur within the 60 ticks.  A's rollout is computed once per case.

And a game list that mrts_reset_games / mrts_park_games reject changes nothing: the
list is validated as a whole before the host mirrors or the device are touched.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu]

W = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M8, M16 = "maps/8x8/basesWorkers8x8.xml", "maps/16x16/basesWorkers16x16.xml"
TICKS, SEED = 60, 5

CASES = {
    # two grid segments (bot games first), fused bots, early bot
    "16x16_fused": dict(map_path=M16, nsp=4, bots=["coacAI", "workerRushAI", "coacAI", "workerRushAI"]),
    # a 64-lane workgroup, one segment
    "8x8_selfplay": dict(map_path=M8, nsp=4, bots=[]),
    # 64 lanes, two segments, a separate k_bot launch
    "8x8_unfused": dict(map_path=M8, nsp=2, bots=["workerRushAI", "workerRushAI"], bot_fusion=False),
}
OUTPUTS = ("_obs", "_raw", "_done", "_rew", "_done0", "_mask", "_src")


def _engine(map_path, nsp, bots, bot_fusion=True, extra_maps=()):
    from gym_microrts import microrts_ai
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv

    return MicroRTSGridModeVecEnv(num_selfplay_envs=nsp, num_bot_envs=len(bots), max_steps=40,
                                  ai2s=[getattr(microrts_ai, b) for b in bots], map_paths=[map_path], reward_weight=W,
                                  return_tensors=True, bot_fusion=bot_fusion, _extra_maps=extra_maps)


def _sample(e, act, s):
    from gym_microrts import _native

    _native.check(_native.lib().mrts_sample_actions_src(e._stream(), e._mask.data_ptr(), e._src.data_ptr(), e.num_envs,
                                                        e.height * e.width, 0, ctypes.c_uint64(SEED), s, act.data_ptr()))


def _outputs(e):
    return {k: getattr(e, k).clone() for k in OUTPUTS}


def _group_step(e, act, policy):
    from gym_microrts import _native

    e.step_async(act)
    io = (_native.StepIO * 1)(e._step_io())
    hs = (ctypes.c_void_p * 1)(e._h)
    e._launch("step", _native.lib().mrts_step_group, hs, 1, e._stream(), io, policy)
    e._tensor_outputs()


def _compare(e, want, tag):
    import torch

    for k in OUTPUTS:
        assert torch.equal(getattr(e, k), want[k]), f"{tag}: {k} differs between mrts_step_weighted and a group of one"


@functools.lru_cache(maxsize=None)
def _rollout_a(case):
    """Engine A's rollout through env.step: per tick the actions it took and every output after the step."""
    import torch

    e = _engine(**CASES[case])
    e.reset()
    ticks = [(None, _outputs(e))]
    for s in range(TICKS):
        act = torch.empty((e.num_envs, e.height * e.width, 7), dtype=torch.int64, device=e.device)
        _sample(e, act, s)
        e.step(act)
        ticks.append((act, _outputs(e)))
    assert e.error_flags() == 0
    assert int(e.game_stats()[:, 5].sum()) > 0, "no auto-reset in the rollout"
    e.close()
    return ticks


@pytest.mark.timeout(60)
@pytest.mark.parametrize("policy", ["separate", "merge_fit_bots_first"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_is_a_group_of_one(case, policy):
    from gym_microrts import _native

    policy = 0 if policy == "separate" else _native.GROUP_MERGE_FIT | _native.GROUP_BOTS_FIRST
    ticks = _rollout_a(case)
    b = _engine(**CASES[case])
    b.reset()
    _compare(b, ticks[0][1], "reset")
    for s, (act, want) in enumerate(ticks[1:]):
        _group_step(b, act, policy)
        _compare(b, want, f"tick {s}")
    assert b.error_flags() == 0
    assert int(b.game_stats()[:, 5].sum()) > 0, "no auto-reset in the rollout"
    b.close()


@pytest.mark.timeout(60)
def test_rejected_game_list_changes_nothing():
    """games [0, 10**6]: the second entry is out of range.  Both calls return MRTS_EINVAL and
    leave game 0's map index and parked flag alone: the snapshot header (the first 256 bytes,
    with both host mirrors, for an engine of at most 8 games) is unchanged, and the next step
    equals the twin's."""
    import torch

    from gym_microrts import _native

    lib = _native.lib()
    cfg = dict(CASES["16x16_fused"], extra_maps=("maps/16x16/basesWorkers16x16A.xml",))
    a, b = _engine(**cfg), _engine(**cfg)
    a.reset()
    b.reset()
    act = torch.empty((a.num_envs, a.height * a.width, 7), dtype=torch.int64, device=a.device)
    for s in range(3):
        _sample(a, act, s)
        a.step(act)
        b.step(act)
    before = a.get_state().tensor[:256].clone()
    games, maps = (ctypes.c_int32 * 2)(0, 10 ** 6), (ctypes.c_int32 * 2)(1, 0)
    assert lib.mrts_reset_games(a._h, a._stream(), games, maps, 2, a._obs.data_ptr()) == -1   # MRTS_EINVAL
    assert lib.mrts_park_games(a._h, a._stream(), games, 2, a._obs.data_ptr()) == -1
    assert torch.equal(a.get_state().tensor[:256], before), "a rejected list changed the host mirrors"
    _sample(a, act, 3)
    a.step(act)
    b.step(act)
    _compare(b, _outputs(a), "the step after the rejected lists")
    assert a.error_flags() == 0
    a.close()
    b.close()
