"""Time the device rollout bookkeeping (gym_microrts.rollout) against the torch code it replaces in
examples/ppo_gridnet_driver.py, on identical inputs, on the MI355X.

Per size (1024 and 8192 envs, T = 256; neither kernel sees the map, so the inputs are synthetic:
float32 N(0, 1) rewards / values, an episode end with probability 1/64 per env-step, raw rewards
of small integers as a 16x16 game's are) the arms alternate inside one process; each repetition is
timed with device events after a warm-up and the median is reported with the spread, and the
whole-call arms also report the host's wall time per call (perf_counter around the call, which for
the host arm of the update includes its sync).

  gae     "device": rollout.gae into preallocated outputs (the whole Python call);
          "device_kernel": the C-ABI launch alone, KERNEL_CALLS back to back, divided by their number;
          "torch": the driver's loop over T (7 torch ops per time step), then adv + values.
          Algorithmic bytes T * N * 20 (three float32 loads, two stores per element).
  update  "device": EpisodeStats.update (the whole call); "device_kernel": the launch alone;
          "torch": the driver's lines -- ep_ret += (raw @ w).float(), next_done.any() read on the
          host, the masked read and reset when an env ended.
          Algorithmic bytes N * (8 + 1 + 48) in, 2 * 120 * N of state read and written, 144 per record.

  python scripts/time_rollout.py --out profiles/rollout/timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "microrts-py_amd"))

from gym_microrts import _native, rollout  # noqa: E402

KERNEL_CALLS = 20   # launches per repetition of a "*_kernel" arm
NAMES = ["WinLossRewardFunction", "ResourceGatherRewardFunction", "ProduceWorkerRewardFunction", "ProduceBuildingRewardFunction",
         "AttackRewardFunction", "ProduceCombatUnitRewardFunction"]


def timed(fn, calls=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    wall = time.perf_counter() - t0
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / calls, wall / calls


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
            torch.cuda.synchronize()
    return times


def summary(ts, nbytes=None, wall=True):
    dev, host = [t[0] for t in ts], [t[1] for t in ts]
    med = statistics.median(dev)
    out = {"median_us": round(med * 1e6, 2), "min_us": round(min(dev) * 1e6, 2), "max_us": round(max(dev) * 1e6, 2), "reps": len(ts)}
    if wall:
        out["host_wall_median_us"] = round(statistics.median(host) * 1e6, 2)
    if nbytes is not None:
        out["algorithmic_bytes"] = int(nbytes)
        out["bytes_per_s"] = round(nbytes / med, 1)
    return out


def torch_gae(rew, val, done, last_v, next_done):
    """The driver's advantage loop (gamma 0.99, lambda 0.95)."""
    T = rew.shape[0]
    adv = torch.zeros_like(rew)
    gae = torch.zeros(rew.shape[1], device=rew.device)
    for t in reversed(range(T)):
        nv, nd = (last_v, next_done) if t == T - 1 else (val[t + 1], done[t + 1])
        delta = rew[t] + 0.99 * nv * (1 - nd) - val[t]
        gae = delta + 0.99 * 0.95 * (1 - nd) * gae
        adv[t] = gae
    return adv, adv + val


def measure(n, T, warmup, reps, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, device="cuda", generator=g)   # noqa: E731
    uni = lambda *shape: torch.rand(shape, device="cuda", generator=g)    # noqa: E731
    res = {"num_envs": n, "T": T}
    lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream

    # ---- GAE
    rew, val, last_v = rnd(T, n), rnd(T, n), rnd(n)
    done, next_done = (uni(T, n) < 1 / 64).float(), (uni(n) < 1 / 64).float()
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    ta, tr = torch_gae(rew, val, done, last_v, next_done)
    rollout.gae(rew, val, done, last_v, next_done, out=(adv, ret))
    res["gae_equal_bits"] = bool(torch.equal(adv.view(torch.int32), ta.view(torch.int32)) and torch.equal(ret.view(torch.int32), tr.view(torch.int32)))
    P = [t.data_ptr() for t in (rew, val, done)]

    def k_gae():
        lib.mrts_gae(st, T, n, *P, 0, last_v.data_ptr(), next_done.data_ptr(), 0.99, 0.95, 0, adv.data_ptr(), ret.data_ptr())

    arms = {"device": lambda: rollout.gae(rew, val, done, last_v, next_done, out=(adv, ret)), "device_kernel": k_gae,
            "torch": lambda: torch_gae(rew, val, done, last_v, next_done)}
    ts = alternate(arms, warmup, reps)
    nb = T * n * 20
    res["gae"] = {k: summary(v, nb if k.startswith("device") else None, wall=not k.endswith("_kernel")) for k, v in ts.items()}
    med = {k: statistics.median(t[0] for t in v) for k, v in ts.items()}
    res["gae"]["torch_over_device"] = round(med["torch"] / med["device"], 2)
    res["gae"]["torch_over_device_kernel"] = round(med["torch"] / med["device_kernel"], 2)

    # ---- one rollout step's bookkeeping
    raw = torch.randint(-1, 3, (n, 6), device="cuda", generator=g).double() * (uni(n, 6) < 0.2)
    w = torch.tensor([10.0, 1.0, 1.0, 0.2, 1.0, 4.0], dtype=torch.float64, device="cuda")
    reward = raw @ w
    done0 = uni(n) < 1 / 64
    nd = done0.float()
    stats = rollout.EpisodeStats(n, NAMES, 0.99)
    kstats = rollout.EpisodeStats(n, NAMES, 0.99)   # the launch-alone arm's own buffer and serial numbers
    ep_ret, finished = torch.zeros(n, device="cuda"), []
    ended = int(done0.sum())

    def host_lines():
        nonlocal finished
        ep_ret.add_((raw @ w).float())
        if bool(nd.any()):
            finished += ep_ret[nd.bool()].tolist()
            ep_ret[nd.bool()] = 0
        finished = []

    def k_update():
        lib.mrts_episode_stats_update(st, kstats._buf.data_ptr(), n, kstats.capacity, 0.99, kstats.steps, reward.data_ptr(),
                                      done0.data_ptr(), raw.data_ptr())
        kstats.steps += 1

    arms = {"device": lambda: stats.update(reward, done0, raw), "device_kernel": k_update, "torch": host_lines}
    ts = alternate(arms, warmup, reps)
    nb = n * (8 + 1 + 48) + 2 * 120 * n + 144 * ended
    res["update"] = {k: summary(v, nb if k.startswith("device") else None, wall=not k.endswith("_kernel")) for k, v in ts.items()}
    res["update"]["episodes_ended_per_call"] = ended
    med = {k: statistics.median(t[0] for t in v) for k, v in ts.items()}
    res["update"]["torch_over_device"] = round(med["torch"] / med["device"], 2)
    res["update"]["torch_over_device_kernel"] = round(med["torch"] / med["device_kernel"], 2)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--num-steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_rollout.py needs the MI355X: there is no CPU timing")
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": "device events around one call (a *_kernel arm: 20 launches, divided), arms alternating, median of reps",
           "sizes": [measure(n, a.num_steps, a.warmup, a.reps, a.seed) for n in a.num_envs]}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
