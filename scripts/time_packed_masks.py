"""Time the packed-mask paths against their dense twins on the MI355X, with the method of
scripts/time_policy_head.py: 16x16, real masks after a 200-tick pre-roll under the
stand-in sampler, device events, the arms alternating inside one process, medians of 30.

Per size (1024 and 8192 envs):
  1. the action head's launches alone (KERNEL_CALLS back to back per repetition), packed
     against dense: sample, evaluate, evaluate + backward.  With --ab-lib (a build with
     -DMRTS_PACKED_ROW_LOADS, loaded beside the product library) a third arm per
     operation: "ballot on word 0, then load the three words per source row".
  2. mrts_get_masks_packed (beside mrts_get_masks into scratch tensors), mrts_pack_masks
     and mrts_unpack_masks, with their algorithmic bytes per second.
  3. (the last size only) a PPO minibatch of --minibatch-envs env-steps drawn from a
     --buffer-steps deep rollout buffer: the gather -- buf_mask[idx] + buf_src[idx] against
     buf_packed[idx] -- and then evaluate + backward on the gathered masks; the two
     buffers' sizes.

Algorithmic bytes, from shapes (S = source rows, G = games, rows = N * HW):
  sample    packed rows*(12 + 56) + S*312 + 8N         dense rows*(4 + 56) + S*624 + 8N
  evaluate  packed rows*12 + S*(312 + 56) + 8N         dense rows*4 + S*(624 + 56) + 8N
  evaluate + backward  2 * evaluate + rows*312         (the forward's reads again + the gradient's fill)
  get_masks_packed G*HW*16 + rows*12    get_masks G*HW*16 + rows*316
  pack / unpack rows*(316 + 12)

  bash scripts/ab/build_variant.sh rowloads WORKTREE EXTRA=-DMRTS_PACKED_ROW_LOADS
  python scripts/time_packed_masks.py --out profiles/packed_masks/timing.json --ab-lib scripts/ab/libs/rowloads.so
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

from time_policy_head import alternate, summary  # noqa: E402  (sets the import path of the package too)
from gym_microrts import _native, policy_head  # noqa: E402
from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv  # noqa: E402


def pre_rolled_env(n, ticks, seed):
    env = MicroRTSGridModeVecEnv(num_selfplay_envs=n, num_bot_envs=0, max_steps=2000, map_paths=["maps/16x16/basesWorkers16x16.xml"],
                                 reward_weight=np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0]), device="cuda:0", return_tensors=True)
    hw = env.height * env.width
    env.reset()
    act = torch.empty((n, hw, 7), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for t in range(ticks):
        m = env.get_action_mask()
        _native.check(_native.lib().mrts_sample_actions_src(st, m.data_ptr(), env.source_unit_mask.data_ptr(), n, hw, 0,
                                                            ctypes.c_uint64(seed), t, act.data_ptr()))
        env.step(act)
    return env, hw


def load_ab(path):
    """The A/B build's handle-free entry points, beside the product library."""
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ("mrts_policy_sample_packed", "mrts_policy_evaluate_packed", "mrts_policy_evaluate_backward_packed"):
        f = getattr(L, name)
        f.restype, f.argtypes = _native.SIGNATURES[name]
    return L


def head_arms(lib, ab, st, logits, mask, src, packed, n, hw, seed):
    """name -> {arm -> callable}: the C-ABI launches alone, into preallocated buffers; and a check that the arms agree."""
    u64 = ctypes.c_uint64(seed)
    actions, _, _ = policy_head.sample(logits, mask, src, seed=seed, step=0)
    ones = torch.ones(n, device="cuda")
    out = {}
    for arm, L, ptrs in (("dense", lib, (mask, src)), ("packed", lib, (packed,)), ("packed_row_loads", ab, (packed,))):
        if L is None:
            continue
        sfx = "" if arm == "dense" else "_packed"
        lp, ent, grad, act2 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty_like(logits), torch.empty_like(actions)
        P = [logits.data_ptr()] + [t.data_ptr() for t in ptrs]
        fs, fe, fb = (getattr(L, "mrts_policy_" + k + sfx) for k in ("sample", "evaluate", "evaluate_backward"))

        def k_sample(fs=fs, P=P, act2=act2, lp=lp, ent=ent):
            fs(st, *P, n, hw, 0, u64, 1, act2.data_ptr(), lp.data_ptr(), ent.data_ptr())

        def k_eval(fe=fe, P=P, lp=lp, ent=ent):
            fe(st, *P, n, hw, actions.data_ptr(), lp.data_ptr(), ent.data_ptr())

        def k_eval_bwd(fb=fb, P=P, grad=grad, k_eval=k_eval):
            k_eval()
            fb(st, *P, n, hw, actions.data_ptr(), ones.data_ptr(), ones.data_ptr(), grad.data_ptr())

        out[arm] = dict(sample=k_sample, evaluate=k_eval, evaluate_backward=k_eval_bwd, bufs=(act2, lp, ent, grad))
    for fn in ("sample", "evaluate_backward"):   # every arm writes the same bits
        for arm in out:
            out[arm][fn]()
    torch.cuda.synchronize()
    for arm in out:
        for x, y in zip(out["dense"]["bufs"], out[arm]["bufs"]):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), arm
    return {op: {arm + "_kernel": out[arm][op] for arm in out} for op in ("sample", "evaluate", "evaluate_backward")}, actions


def head_bytes(rows, S, n):
    p = {"sample": rows * (12 + 56) + S * 312 + 8 * n, "evaluate": rows * 12 + S * (312 + 56) + 8 * n}
    d = {"sample": rows * (4 + 56) + S * 624 + 8 * n, "evaluate": rows * 4 + S * (624 + 56) + 8 * n}
    p["evaluate_backward"] = 2 * p["evaluate"] + rows * 312
    d["evaluate_backward"] = 2 * d["evaluate"] + rows * 312
    return {"dense": d, "packed": p, "packed_row_loads": p}


def ratios(ts, base):
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {f"{k[:-7]}_over_{base}": round(med[k] / med[base + "_kernel"], 3) for k in med if k != base + "_kernel"}


def measure(n, a, ab, minibatch):
    env, hw = pre_rolled_env(n, a.ticks, a.seed)
    lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    mask, src = env.get_action_mask().clone(), env.source_unit_mask.clone()
    packed = env.get_action_mask_packed().clone()
    assert torch.equal(policy_head.pack_masks(mask, src), packed)
    rows, S, G = n * hw, int((src != 0).sum()), n // 2
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    logits = 3.0 * torch.randn((rows, 78), device="cuda", generator=g)
    res = {"num_envs": n, "hw": hw, "source_rows": S, "source_share": round(S / rows, 5), "pre_roll_ticks": a.ticks}

    # 1. the head's launches
    ops, _ = head_arms(lib, ab, st, logits, mask, src, packed, n, hw, a.seed)
    nb = head_bytes(rows, S, n)
    for op, arms in ops.items():
        ts = alternate(arms, a.warmup, a.reps)
        res[op] = {k: summary(v, nb[k[:-7]][op]) for k, v in ts.items()}
        res[op].update(ratios(ts, "dense"))

    # 2. the engine's packed output and the converters
    m2, s2, p2 = torch.empty_like(mask), torch.empty_like(src), torch.empty_like(packed)
    arms = {
        "get_masks_packed_kernel": lambda: lib.mrts_get_masks_packed(env._h, st, p2.data_ptr()),
        "get_masks_kernel": lambda: lib.mrts_get_masks(env._h, st, m2.data_ptr(), s2.data_ptr()),   # into scratch: the env's own buffers stay
        "pack_masks_kernel": lambda: lib.mrts_pack_masks(st, mask.data_ptr(), src.data_ptr(), n, hw, p2.data_ptr()),
        "unpack_masks_kernel": lambda: lib.mrts_unpack_masks(st, packed.data_ptr(), n, hw, m2.data_ptr(), s2.data_ptr()),
    }
    cb = {"get_masks_packed_kernel": G * hw * 16 + rows * 12, "get_masks_kernel": G * hw * 16 + rows * 316,
          "pack_masks_kernel": rows * 328, "unpack_masks_kernel": rows * 328}
    ts = alternate(arms, a.warmup, a.reps)
    res["masks"] = {k: summary(v, cb[k]) for k, v in ts.items()}
    torch.cuda.synchronize()
    assert torch.equal(m2, mask) and torch.equal(s2, src) and torch.equal(p2, packed)
    assert env.error_flags() == 0
    env.close()

    # 3. the minibatch: gather from the rollout buffer, then evaluate + backward
    if minibatch:
        T, mb = a.buffer_steps, a.minibatch_envs
        buf_mask = torch.stack([mask.roll(t, 0) for t in range(T)])     # [T, N, HW, 78] int32
        buf_src = torch.stack([src.roll(t, 0) for t in range(T)])
        buf_packed = torch.stack([packed.roll(t, 0) for t in range(T)])
        fm, fs, fp = buf_mask.reshape(T * n, hw, 78), buf_src.reshape(T * n, hw), buf_packed.reshape(T * n, hw, 3)
        idx = torch.randperm(T * n, device="cuda", generator=g)[:mb]
        lg = 3.0 * torch.randn((mb * hw, 78), device="cuda", generator=g)
        gm, gs, gp = fm[idx], fs[idx], fp[idx]
        assert torch.equal(policy_head.pack_masks(gm, gs), gp)
        S2 = int((gs != 0).sum())
        ops, _ = head_arms(lib, None, st, lg, gm, gs, gp, mb, hw, a.seed)
        keep = {}

        def gather_dense():
            keep["d"] = (fm[idx], fs[idx])

        def gather_packed():
            keep["p"] = fp[idx]

        arms = {"gather_dense": gather_dense, "gather_packed": gather_packed,
                "evaluate_backward_dense_kernel": ops["evaluate_backward"]["dense_kernel"],
                "evaluate_backward_packed_kernel": ops["evaluate_backward"]["packed_kernel"]}
        ts = alternate(arms, a.warmup, a.reps)
        nbm = head_bytes(mb * hw, S2, mb)
        gb = {"gather_dense": 2 * mb * hw * 316, "gather_packed": 2 * mb * hw * 12,
              "evaluate_backward_dense_kernel": nbm["dense"]["evaluate_backward"],
              "evaluate_backward_packed_kernel": nbm["packed"]["evaluate_backward"]}
        med = {k: statistics.median(v) for k, v in ts.items()}
        res["minibatch"] = {"buffer_steps": T, "minibatch_env_steps": mb, "source_rows": S2,
                            "dense_buffer_bytes": buf_mask.element_size() * buf_mask.nelement() + buf_src.element_size() * buf_src.nelement(),
                            "packed_buffer_bytes": buf_packed.element_size() * buf_packed.nelement(),
                            **{k: summary(v, gb[k]) for k, v in ts.items()},
                            "dense_total_us": round((med["gather_dense"] + med["evaluate_backward_dense_kernel"]) * 1e6, 2),
                            "packed_total_us": round((med["gather_packed"] + med["evaluate_backward_packed_kernel"]) * 1e6, 2)}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--buffer-steps", type=int, default=16)
    ap.add_argument("--minibatch-envs", type=int, default=4 * 8192)
    ap.add_argument("--ab-lib", type=str, default="", help="a libmicrorts_amd.so built with -DMRTS_PACKED_ROW_LOADS: the A/B arm")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_packed_masks.py needs the MI355X: there is no CPU timing")
    ab = load_ab(a.ab_lib) if a.ab_lib else None
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": "device events; *_kernel arms: 20 C-ABI launches back to back per repetition, divided by 20; arms alternating; median of reps",
           "ab_arm": "packed_row_loads = -DMRTS_PACKED_ROW_LOADS: ballot on word 0, then the three words loaded per source row" if ab else None,
           "sizes": [measure(n, a, ab, i == len(a.num_envs) - 1) for i, n in enumerate(a.num_envs)]}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
