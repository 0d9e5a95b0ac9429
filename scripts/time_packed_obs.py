"""Time the packed-obs paths against their dense float32 twins on the MI355X, with the method
of scripts/time_packed_masks.py: 16x16, real states after a 200-tick pre-roll under the
stand-in sampler, device events, the arms alternating inside one process, medians of 30.

  1. The step launch (mrts_step_weighted; eager, delta masks on) of an engine with
     obs_format="packed" against a float32 engine's, 1024 and 8192 selfplay envs and 8192 envs
     vs device coacAI.  The two engines play the same games (same seed, same sampler stream);
     a repetition is STEP_TICKS ticks per arm, each tick's launch between its own pair of
     events (the sampler launch in front of it is outside them), the arms taking turns tick
     block by tick block.  The float32 engine's device code is the parent's, byte for byte
     (profiles/packed_obs/README.md), so it is the parent's step.
  2. mrts_unpack_obs (float32 and bfloat16) and mrts_pack_obs at the last size's rows, with
     mrts_unpack_masks -- the same write pattern, 312-byte rows -- in the same run; launches
     alone, KERNEL_CALLS back to back.  With --ab-lib (a variant build of the library, loaded
     beside the product one) its mrts_unpack_obs as a second unpack arm; the committed
     timing.json's variant read the words through L1 / L2 instead of staging them in LDS
     (`packed[row0 + min(r, nr - 1)] & keep` in place of `s_w[r]`, no staging loop or barrier).
  3. A PPO minibatch of --minibatch-envs env-steps drawn from a --buffer-steps deep rollout
     buffer and made ready for the network: buf_obs[idx] (float32 planes) against
     unpack_obs(buf_packed[idx]); the two buffers' sizes.
  4. The rollout step's sum: the dense step against the packed step + one float32 unpack.

Algorithmic bytes, from shapes (G games, rows = N * HW, S0 + S1 = the source rows before and
after the tick, the delta masks' stores):
  step    G*HW*32 (state in and out) + rows*4 (source out) + (S0 + S1)*312 + N*66 + obs
          obs = rows*116 dense float32, rows*4 packed
  unpack  rows*(4 + 29*e), e = 4 or 2        pack rows*(4 + 29*4)        unpack_masks rows*328

  python scripts/time_packed_obs.py --out profiles/packed_obs/timing.json [--ab-lib scripts/ab/libs/VARIANT.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from time_policy_head import KERNEL_CALLS, alternate, summary  # noqa: E402  (sets the import path of the package too)
from gym_microrts import _native, microrts_ai, packed_obs, policy_head  # noqa: E402
from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv  # noqa: E402

STEP_TICKS = 20   # ticks per repetition of a step arm
PLANES = 29


class Stepper:
    """An engine stepped by C-ABI launches under the stand-in sampler; step() returns the launch's events."""

    def __init__(self, nsp, nbot, seed, **kw):
        self.env = MicroRTSGridModeVecEnv(num_selfplay_envs=nsp, num_bot_envs=nbot, max_steps=2000, ai2s=[microrts_ai.coacAI] * nbot,
                                          map_paths=["maps/16x16/basesWorkers16x16.xml"],
                                          reward_weight=np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0]), device="cuda:0", return_tensors=True, **kw)
        e = self.env
        assert e.eager_masks and e.mask_delta
        self.n, self.hw, self.seed, self.t = e.num_envs, e.height * e.width, seed, 0
        self.act = torch.empty((self.n, self.hw, 7), dtype=torch.int64, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        e.reset()

    def step(self, timed=False):
        e, L = self.env, _native.lib()
        _native.check(L.mrts_sample_actions_src(self.st, e._mask.data_ptr(), e._src.data_ptr(), self.n, self.hw, 0,
                                                ctypes.c_uint64(self.seed), self.t, self.act.data_ptr()))
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if timed else None
        if timed:
            ev[0].record()
        _native.check(L.mrts_step_weighted(e._h, self.st, self.act.data_ptr(), e._src.data_ptr(), e._obs.data_ptr(), e._raw.data_ptr(),
                                           e._done.data_ptr(), e._rew.data_ptr(), e._done0.data_ptr()), e._h, "step")
        if timed:
            ev[1].record()
        self.t += 1
        return ev


def time_steps(nsp, nbot, a):
    arms = {"dense_f32": Stepper(nsp, nbot, a.seed, obs_dtype=torch.float32), "packed": Stepper(nsp, nbot, a.seed, obs_format="packed")}
    src_rows = {k: [] for k in arms}
    for _ in range(a.ticks):
        for s in arms.values():
            s.step()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for rep in range(a.warmup + a.reps):
        for k, s in arms.items():
            evs = []
            for _ in range(STEP_TICKS):
                src_rows[k].append(s.env._src.sum())   # on both arms alike (outside the events)
                evs.append(s.step(timed=True))
            evs[-1][1].synchronize()
            if rep >= a.warmup:
                times[k].append(sum(x.elapsed_time(y) for x, y in evs) * 1e-3 / STEP_TICKS)
    d, p = arms["dense_f32"].env, arms["packed"].env
    assert torch.equal(packed_obs.unpack_obs(p._obs, PLANES).view(torch.int32), d._obs.view(torch.int32)), "the arms' games diverged"
    assert torch.equal(p._mask, d._mask) and torch.equal(p._rew, d._rew)
    assert d.error_flags() == 0 and p.error_flags() == 0
    n, hw = d.num_envs, d.height * d.width
    G, rows = nsp // 2 + nbot, n * hw
    assert torch.equal(torch.stack(src_rows["packed"]), torch.stack(src_rows["dense_f32"]))
    S = float(torch.stack(src_rows["packed"]).float().mean())   # source rows per tick; a tick stores those before and after it
    common = G * hw * 32 + rows * 4 + 2 * S * 312 + n * 66
    nb = {"dense_f32": common + rows * PLANES * 4, "packed": common + rows * 4}
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"num_selfplay_envs": nsp, "num_bot_envs": nbot, "hw": hw, "pre_roll_ticks": a.ticks, "ticks_timed_per_arm": a.reps * STEP_TICKS,
           "mean_source_rows": round(S, 1), **{k + "_step": summary(v, nb[k]) for k, v in times.items()},
           "packed_over_dense": round(med["packed"] / med["dense_f32"], 3),
           "obs_bytes_not_stored": rows * PLANES * 4 - rows * 4}
    packed_words, mask_words = p._obs.clone(), p.get_action_mask_packed().clone()
    d.close(), p.close()
    return res, packed_words, mask_words, med


def load_ab(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.mrts_unpack_obs.restype, L.mrts_unpack_obs.argtypes = _native.SIGNATURES["mrts_unpack_obs"]
    return L


def time_converters(words, mask_words, a, ab):
    lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    rows = words.numel()
    n, hw = mask_words.shape[0], mask_words.shape[1]
    f32 = torch.empty(words.shape + (PLANES,), dtype=torch.float32, device="cuda")
    bf16 = torch.empty(words.shape + (PLANES,), dtype=torch.bfloat16, device="cuda")
    f32_ab = torch.empty_like(f32)
    back = torch.empty_like(words)
    m2 = torch.empty((n, hw, 78), dtype=torch.int32, device="cuda")
    s2 = torch.empty((n, hw), dtype=torch.int32, device="cuda")
    E = _native
    arms = {
        "unpack_obs_f32_kernel": lambda: lib.mrts_unpack_obs(st, words.data_ptr(), rows, PLANES, E.MRTS_ELEM_FLOAT32, f32.data_ptr()),
        "unpack_obs_bf16_kernel": lambda: lib.mrts_unpack_obs(st, words.data_ptr(), rows, PLANES, E.MRTS_ELEM_BFLOAT16, bf16.data_ptr()),
        "unpack_masks_kernel": lambda: lib.mrts_unpack_masks(st, mask_words.data_ptr(), n, hw, m2.data_ptr(), s2.data_ptr()),
        "pack_obs_f32_kernel": lambda: lib.mrts_pack_obs(st, f32.data_ptr(), rows, PLANES, E.MRTS_ELEM_FLOAT32, back.data_ptr()),
    }
    if ab is not None:
        arms["unpack_obs_f32_direct_words_kernel"] = lambda: ab.mrts_unpack_obs(st, words.data_ptr(), rows, PLANES, E.MRTS_ELEM_FLOAT32,
                                                                                  f32_ab.data_ptr())
        arms["unpack_obs_bf16_direct_words_kernel"] = lambda: ab.mrts_unpack_obs(st, words.data_ptr(), rows, PLANES, E.MRTS_ELEM_BFLOAT16,
                                                                                   bf16.data_ptr())
    nb = {"unpack_obs_f32_kernel": rows * (4 + PLANES * 4), "unpack_obs_bf16_kernel": rows * (4 + PLANES * 2),
          "unpack_masks_kernel": n * hw * 328, "pack_obs_f32_kernel": rows * (4 + PLANES * 4),
          "unpack_obs_f32_direct_words_kernel": rows * (4 + PLANES * 4), "unpack_obs_bf16_direct_words_kernel": rows * (4 + PLANES * 2)}
    ts = alternate(arms, a.warmup, a.reps)
    torch.cuda.synchronize()
    assert torch.equal(back, words) and torch.equal(f32.to(torch.bfloat16).view(torch.int16), bf16.view(torch.int16))
    if ab is not None:
        assert torch.equal(f32_ab.view(torch.int32), f32.view(torch.int32))
    res = {"rows": rows, "planes": PLANES, **{k: summary(v, nb[k]) for k, v in ts.items()}}
    return res, {k: statistics.median(v) for k, v in ts.items()}


def time_minibatch(words, a):
    """words [N, H, W]: a --buffer-steps deep buffer of them (rolled along N), dense float32 and packed."""
    lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    T, mb = a.buffer_steps, a.minibatch_envs
    n, h, w = words.shape
    buf_packed = torch.stack([words.roll(t, 0) for t in range(T)])              # [T, N, H, W] int32
    buf_obs = packed_obs.unpack_obs(buf_packed, PLANES)                         # [T, N, H, W, 29] float32
    fp, fo = buf_packed.reshape(T * n, h, w), buf_obs.reshape(T * n, h, w, PLANES)
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    idx = torch.randperm(T * n, device="cuda", generator=g)[:mb]
    gathered = fp[idx]
    out = torch.empty((mb, h, w, PLANES), dtype=torch.float32, device="cuda")
    keep = {}

    def gather_dense():
        keep["d"] = fo[idx]

    def gather_packed():
        keep["p"] = fp[idx]

    arms = {"gather_dense": gather_dense, "gather_packed": gather_packed,
            "unpack_obs_f32_kernel": lambda: lib.mrts_unpack_obs(st, gathered.data_ptr(), gathered.numel(), PLANES, _native.MRTS_ELEM_FLOAT32,
                                                                 out.data_ptr())}
    ts = alternate(arms, a.warmup, a.reps)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), keep["d"].view(torch.int32)) and torch.equal(keep["p"], gathered)
    rows = mb * h * w
    gb = {"gather_dense": 2 * rows * PLANES * 4, "gather_packed": 2 * rows * 4, "unpack_obs_f32_kernel": rows * (4 + PLANES * 4)}
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"buffer_steps": T, "num_envs": n, "minibatch_env_steps": mb,
            "dense_buffer_bytes": buf_obs.element_size() * buf_obs.nelement(), "packed_buffer_bytes": buf_packed.element_size() * buf_packed.nelement(),
            **{k: summary(v, gb[k]) for k, v in ts.items()},
            "dense_total_us": round(med["gather_dense"] * 1e6, 2),
            "packed_total_us": round((med["gather_packed"] + med["unpack_obs_f32_kernel"]) * 1e6, 2)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--bot-envs", type=int, default=8192, help="a last step table: this many envs vs device coacAI (0: none)")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--buffer-steps", type=int, default=16)
    ap.add_argument("--minibatch-envs", type=int, default=4 * 8192)
    ap.add_argument("--ab-lib", type=str, default="", help="a variant libmicrorts_amd.so whose mrts_unpack_obs is the A/B arm")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_packed_obs.py needs the MI355X: there is no CPU timing")
    ab = load_ab(a.ab_lib) if a.ab_lib else None
    steps = []
    for n in a.num_envs:
        res, words, mask_words, med = time_steps(n, 0, a)
        steps.append(res)
    conv, cmed = time_converters(words, mask_words, a, ab)
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": f"device events; step arms: {STEP_TICKS} ticks per repetition, each launch between its own events, summed and divided; "
                     f"*_kernel arms: {KERNEL_CALLS} C-ABI launches back to back per repetition, divided; arms alternating; median of reps",
           "ab_arm": "direct_words = the --ab-lib build's k_unpack_obs (timing.json's: the words read through L1 / L2, no LDS staging)" if ab else None,
           "step": steps, "converters": conv, "minibatch": time_minibatch(words, a),
           "rollout_step_sum": {"num_envs": a.num_envs[-1],
                                "dense_step_us": round(med["dense_f32"] * 1e6, 2),
                                "packed_step_us": round(med["packed"] * 1e6, 2),
                                "unpack_obs_f32_us": round(cmed["unpack_obs_f32_kernel"] * 1e6, 2),
                                "packed_step_plus_unpack_us": round((med["packed"] + cmed["unpack_obs_f32_kernel"]) * 1e6, 2)}}
    del words, mask_words
    if a.bot_envs:
        doc["step_vs_coac"] = time_steps(0, a.bot_envs, a)[0]
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
