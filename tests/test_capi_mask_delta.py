"""mrts_set_mask_delta's argument checks (host only, no kernel launch)."""
import os

from conftest import MAPS


def test_set_mask_delta_checks_its_arguments():
    from gym_microrts import _native

    lib = _native.lib()
    assert lib.mrts_set_mask_delta(None, 1) == -1   # MRTS_EINVAL: null handle
    h = _native.create(num_selfplay_envs=4, num_bot_envs=0, max_steps=100, partial_obs=False,
                       map_paths=[os.path.join(MAPS, "maps/16x16/basesWorkers16x16.xml")], game_map=[0, 0], bot_ai=[], obs_dtype=1)
    # a switch, not a launch: needs no workspace, any non-zero value is "on"
    for on in (0, 1, 7, -1, 0):
        assert lib.mrts_set_mask_delta(h, on) == _native.MRTS_OK
        assert lib.mrts_last_error(h) == b""
    lib.mrts_destroy(h)


def test_envs_take_mask_delta_with_no_fixed_default():
    """mask_delta=None leaves the choice to MICRORTS_AMD_MASK_DELTA (how an unchanged bench.py runs both arms)."""
    import inspect

    from gym_microrts.envs import vec_env

    sig = inspect.signature(vec_env.MicroRTSGridModeVecEnv.__init__)
    assert sig.parameters["mask_delta"].default is None
    assert inspect.signature(vec_env.MicroRTSSizeCyclingVecEnv.__init__).parameters["mask_delta"].default is None
