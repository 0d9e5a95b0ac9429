"""Time the fused first encoder stage on packed obs (gym_microrts.obs_conv: conv3x3 + max-pool +
ReLU straight from the words) against the path it replaces -- packed_obs.unpack_obs and the
network's own torch stage -- on the MI355X, with the method of scripts/time_packed_obs.py: 16x16,
real states after a 200-tick pre-roll under the stand-in sampler, the reference agent's
first-layer weights (tests/golden/agent_sota_policy.npz), device events, the arms alternating
inside one process, medians of 30.  The torch arm of the same run is the yardstick.

  a. The forward under no_grad at 1024 and 8192 envs: unpack_obs, Conv2d, MaxPool2d and ReLU
     each alone (the torch arm's four launches), their chain, and obs_conv.encode.
  b. A PPO minibatch of --minibatch-envs env-steps gathered from a --buffer-steps deep packed
     buffer, then the stage's forward and its backward to the parameters: gather + unpack +
     torch stage against gather + encode, with torch.cuda.max_memory_allocated above what was
     allocated before the arm.
  c. The rollout step's sum: the packed step + encode against the float32 step + the torch
     stage on its dense obs (the step launches timed as in time_packed_obs.py).

Algorithmic bytes, from shapes (rows = N * H * W, out = N * C * Ho * Wo floats, tbl = C * P * 9
floats): encode rows*4 + out*4 + tbl*4; its backward rows*4 + out*4 + tbl*4 (in) + the
workspace written and read once + tbl*4 (out); the torch stage rows*P*4 (unpack out) +
rows*P*4 + rows*C*4 (conv) + rows*C*4 + out*4 (pool) + 2*out*4 (relu).

  python scripts/time_obs_conv.py --out profiles/obs_conv/timing.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from time_policy_head import KERNEL_CALLS, alternate, summary  # noqa: E402  (sets the import path of the package too)
from time_packed_obs import STEP_TICKS, time_steps  # noqa: E402
from gym_microrts import _native, obs_conv, packed_obs  # noqa: E402

PLANES, C = 29, 32


def first_stage():
    """The network's first stage as the driver's GridNet builds it, with the reference agent's weights."""
    with np.load(os.path.join(REPO, "tests", "golden", "agent_sota_policy.npz")) as z:
        w, b = torch.from_numpy(z["encoder.1.weight"]), torch.from_numpy(z["encoder.1.bias"])
    enc = nn.Sequential(nn.Conv2d(PLANES, C, 3, padding=1), nn.MaxPool2d(3, 2, 1), nn.ReLU()).cuda()
    with torch.no_grad():
        enc[0].weight.copy_(w)
        enc[0].bias.copy_(b)
    return enc


def stage_bytes(n, h, w):
    rows, out, tbl = n * h * w, n * C * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1), C * PLANES * 9
    return {"unpack_obs_f32_kernel": rows * (4 + PLANES * 4), "conv2d_kernel": rows * (PLANES + C) * 4 + tbl * 4,
            "max_pool2d_kernel": rows * C * 4 + out * 4, "relu_kernel": 2 * out * 4,
            "torch_stage_kernel": rows * (4 + PLANES * 4) + rows * (PLANES + C) * 4 + tbl * 4 + rows * C * 4 + out * 4 + 2 * out * 4,
            "encode_kernel": rows * 4 + out * 4 + tbl * 4}


def time_forward(words, enc, a):
    n, h, w = words.shape
    dense = torch.empty((n, h, w, PLANES), device="cuda")
    keep = {}
    with torch.no_grad():
        packed_obs.unpack_obs(words, PLANES, out=dense)
        x = dense.permute(0, 3, 1, 2)
        conv = enc[0](x)
        pooled = enc[1](conv)

        def chain():
            keep["torch"] = enc(packed_obs.unpack_obs(words, PLANES, out=dense).permute(0, 3, 1, 2))

        def fused():
            keep["fused"] = obs_conv.encode(words, enc[0].weight, enc[0].bias)

        arms = {"unpack_obs_f32_kernel": lambda: packed_obs.unpack_obs(words, PLANES, out=dense),
                "conv2d_kernel": lambda: enc[0](x), "max_pool2d_kernel": lambda: enc[1](conv), "relu_kernel": lambda: enc[2](pooled),
                "torch_stage_kernel": chain, "encode_kernel": fused}
        ts = alternate(arms, a.warmup, a.reps)
    torch.cuda.synchronize()
    diff = float((keep["torch"] - keep["fused"]).abs().max())
    assert diff < 1e-4, diff
    nb = stage_bytes(n, h, w)
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"num_envs": n, "hw": h * w, "max_abs_diff_of_the_arms": diff, **{k: summary(v, nb[k]) for k, v in ts.items()},
            "torch_launches_sum_us": round(sum(med[k] for k in ("unpack_obs_f32_kernel", "conv2d_kernel", "max_pool2d_kernel", "relu_kernel")) * 1e6, 2),
            "encode_over_torch_stage": round(med["encode_kernel"] / med["torch_stage_kernel"], 3)}, med


def time_minibatch(words, enc, a):
    T, mb = a.buffer_steps, a.minibatch_envs
    n, h, w = words.shape
    buf = torch.stack([words.roll(t, 0) for t in range(T)]).reshape(T * n, h, w)
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    idx = torch.randperm(T * n, device="cuda", generator=g)[:mb]
    gout = torch.randn((mb, C, (h - 1) // 2 + 1, (w - 1) // 2 + 1), device="cuda", generator=g)
    params = list(enc.parameters())
    grads, peak = {}, {}

    fwd = {"torch": lambda o: enc(packed_obs.unpack_obs(o, PLANES).permute(0, 3, 1, 2)),
           "fused": lambda o: obs_conv.encode(o, enc[0].weight, enc[0].bias)}

    def arm(name):
        def run():
            for p in params:
                p.grad = None
            fwd[name](buf[idx]).backward(gout)
        return run

    arms = {k: arm(k) for k in fwd}
    ts = alternate(arms, a.warmup, a.reps)
    for k, run in arms.items():   # the peak of one more call of each, outside the timing
        torch.cuda.synchronize()
        for p in params:
            p.grad = None
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
        grads[k] = [p.grad.clone() for p in params]
    rel = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(grads["fused"], grads["torch"])]
    assert max(rel) < 1e-3, rel
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"buffer_steps": T, "num_envs": n, "minibatch_env_steps": mb, "what": "gather + stage forward + backward to weight and bias",
            "gradients_max_rel_diff_of_the_arms": rel, **{k: summary(v) for k, v in ts.items()},
            "peak_bytes_above_start": {k: int(v) for k, v in peak.items()},
            "fused_over_torch": round(med["fused"] / med["torch"], 3),
            "fused_peak_over_torch_peak": round(peak["fused"] / peak["torch"], 4),
            "workspace_bytes": int(_native.lib().mrts_obs_conv_workspace_bytes(mb, h, w, PLANES, C))}


def time_dense_stage(words, enc, a):
    """The torch stage on a float32 engine's own dense obs (no unpack): the dense arm of the rollout step."""
    dense = packed_obs.unpack_obs(words, PLANES)
    with torch.no_grad():
        ts = alternate({"torch_stage_on_dense_kernel": lambda: enc(dense.permute(0, 3, 1, 2))}, a.warmup, a.reps)
    return statistics.median(ts["torch_stage_on_dense_kernel"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--buffer-steps", type=int, default=16)
    ap.add_argument("--minibatch-envs", type=int, default=4 * 8192)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_obs_conv.py needs the MI355X: there is no CPU timing")
    enc = first_stage()
    forward, sums = [], []
    for n in a.num_envs:
        step, words, _, smed = time_steps(n, 0, a)
        res, fmed = time_forward(words, enc, a)
        forward.append(res)
        dense_stage = time_dense_stage(words, enc, a)
        packed_sum, dense_sum = smed["packed"] + fmed["encode_kernel"], smed["dense_f32"] + dense_stage
        sums.append({"num_envs": n, "packed_step_us": round(smed["packed"] * 1e6, 2), "encode_us": round(fmed["encode_kernel"] * 1e6, 2),
                     "dense_step_us": round(smed["dense_f32"] * 1e6, 2), "torch_stage_on_dense_us": round(dense_stage * 1e6, 2),
                     "packed_step_plus_unpack_plus_torch_stage_us": round((smed["packed"] + fmed["torch_stage_kernel"]) * 1e6, 2),
                     "packed_step_plus_encode_us": round(packed_sum * 1e6, 2), "dense_step_plus_torch_stage_us": round(dense_sum * 1e6, 2),
                     "packed_fused_over_dense_torch": round(packed_sum / dense_sum, 3)})
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": f"device events; step arms: {STEP_TICKS} ticks per repetition, each launch between its own events, summed and divided; "
                     f"*_kernel arms: {KERNEL_CALLS} calls back to back per repetition, divided; the minibatch arms: one call per "
                     f"repetition; arms alternating; median of reps",
           "weights": "tests/golden/agent_sota_policy.npz encoder.1", "forward": forward, "minibatch": time_minibatch(words, enc, a),
           "rollout_step_sum": sums}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
