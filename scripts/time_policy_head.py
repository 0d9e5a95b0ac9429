"""Time the fused masked action head (gym_microrts.policy_head) against the driver's
torch `policy()` on identical inputs, on the MI355X.

Per size (1024 and 8192 envs, 16x16, real masks after a 200-tick pre-roll under the
stand-in sampler) and per operation -- sample, evaluate, evaluate + backward -- the arms
alternate inside one process; each repetition is timed with device events after a
warm-up, and the median is reported with the spread.  "fused" and "torch" time one call
of the Python entry point (at these sizes the fused call is bounded by its host work,
not by the kernel); "fused_kernel" times the C-ABI launch alone, KERNEL_CALLS launches
back to back into preallocated buffers per repetition, divided by their number.  The
stand-in sampler (`mrts_sample_actions_src`) is timed beside `sample`, launch against
launch: it reads the same mask rows and writes the same actions, without the S logit
rows.  Algorithmic bytes are counted from shapes (S = source rows of the timed masks):

  sample             N*HW*(4 + 56) + S*624 + 8N
  evaluate           N*HW*4 + S*(624 + 56) + 8N
  evaluate+backward  evaluate + N*HW*(4 + 312) + S*(624 + 56) + 8N

  python scripts/time_policy_head.py --out profiles/policy_head/timing.json
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
sys.path.insert(0, os.path.join(REPO, "microrts-py_amd"))
sys.path.insert(0, os.path.join(REPO, "examples"))

from gym_microrts import _native, policy_head  # noqa: E402
from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv  # noqa: E402
import ppo_gridnet_driver as drv  # noqa: E402


def real_inputs(n, ticks, seed):
    """Masks / source of n selfplay envs after `ticks` steps of the stand-in sampler, and N(0, 3) logits."""
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
    mask, src = env.get_action_mask().clone(), env.source_unit_mask.clone()
    assert env.error_flags() == 0
    env.close()
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = 3.0 * torch.randn((n * hw, 78), device="cuda", generator=g)
    return logits, mask, src, hw


KERNEL_CALLS = 20   # launches per repetition of a "*_kernel" arm


def timed(fn, calls=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / calls


def alternate(arms, warmup, reps):
    """arms: name -> callable.  Warm every arm, then `reps` rounds of one timed call per arm in turn."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(timed(fn, KERNEL_CALLS if k.endswith("_kernel") else 1))
    return times


def summary(ts, nbytes=None):
    med = statistics.median(ts)
    out = {"median_us": round(med * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2), "reps": len(ts)}
    if nbytes is not None:
        out["algorithmic_bytes"] = int(nbytes)
        out["bytes_per_s"] = round(nbytes / med, 1)
    return out


def measure(n, ticks, warmup, reps, seed):
    logits, mask, src, hw = real_inputs(n, ticks, seed)
    S, rows = int((src != 0).sum()), n * hw
    maskf = mask.float()   # the torch head's rollout buffer holds the float copy
    stub = lambda _obs: (logits, None)   # noqa: E731  policy() with the network taken out
    actions, _, _ = policy_head.sample(logits, mask, src, seed=seed, step=0)
    act_src = torch.empty_like(actions)
    st = torch.cuda.current_stream().cuda_stream
    lib = _native.lib()
    nb = {"sample": rows * (4 + 56) + S * 624 + 8 * n, "evaluate": rows * 4 + S * (624 + 56) + 8 * n}
    nb["evaluate_backward"] = nb["evaluate"] + rows * (4 + 312) + S * (624 + 56) + 8 * n
    res = {"num_envs": n, "hw": hw, "source_rows": S, "source_share": round(S / rows, 5), "pre_roll_ticks": ticks}

    def torch_sample():
        with torch.no_grad():
            drv.policy(stub, None, maskf, hw)

    def torch_eval():
        with torch.no_grad():
            drv.policy(stub, None, maskf, hw, action=actions)

    lg = logits.clone().requires_grad_(True)
    stub_g = lambda _obs: (lg, None)   # noqa: E731

    def torch_bwd():
        lg.grad = None
        _, lp, ent, _ = drv.policy(stub_g, None, maskf, hw, action=actions)
        (lp.sum() + ent.sum()).backward()

    def fused_bwd():
        lg.grad = None
        lp, ent = policy_head.evaluate(lg, mask, src, actions)
        (lp.sum() + ent.sum()).backward()

    # the C-ABI launches alone, into preallocated buffers
    lp, ent = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    ones, grad, act2 = torch.ones(n, device="cuda"), torch.empty_like(logits), torch.empty_like(actions)
    P = [t.data_ptr() for t in (logits, mask, src)]
    u64 = ctypes.c_uint64(seed)

    def k_sample():
        lib.mrts_policy_sample(st, *P, n, hw, 0, u64, 1, act2.data_ptr(), lp.data_ptr(), ent.data_ptr())

    def k_eval():
        lib.mrts_policy_evaluate(st, *P, n, hw, actions.data_ptr(), lp.data_ptr(), ent.data_ptr())

    def k_eval_bwd():
        k_eval()
        lib.mrts_policy_evaluate_backward(st, *P, n, hw, actions.data_ptr(), ones.data_ptr(), ones.data_ptr(), grad.data_ptr())

    def k_standin():
        lib.mrts_sample_actions_src(st, mask.data_ptr(), src.data_ptr(), n, hw, 0, u64, 1, act_src.data_ptr())

    ops = {
        "sample": {"fused": lambda: policy_head.sample(logits, mask, src, seed=seed, step=1), "torch": torch_sample,
                   "fused_kernel": k_sample, "standin_sampler_kernel": k_standin},
        "evaluate": {"fused": lambda: policy_head.evaluate(logits, mask, src, actions), "torch": torch_eval, "fused_kernel": k_eval},
        "evaluate_backward": {"fused": fused_bwd, "torch": torch_bwd, "fused_kernel": k_eval_bwd},
    }
    for op, arms in ops.items():
        ts = alternate(arms, warmup, reps)
        res[op] = {k: summary(v, nb[op] if k.startswith("fused") else None) for k, v in ts.items()}
        med = {k: statistics.median(v) for k, v in ts.items()}
        res[op]["torch_over_fused"] = round(med["torch"] / med["fused"], 2)
        res[op]["torch_over_fused_kernel"] = round(med["torch"] / med["fused_kernel"], 2)
        if "standin_sampler_kernel" in ts:
            res[op]["fused_kernel_over_standin_sampler_kernel"] = round(med["fused_kernel"] / med["standin_sampler_kernel"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_policy_head.py needs the MI355X: there is no CPU timing")
    doc = {"device": torch.cuda.get_device_name(0), "timing": "device events around one call, arms alternating, median of reps",
           "sizes": [measure(n, a.ticks, a.warmup, a.reps, a.seed) for n in a.num_envs]}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
