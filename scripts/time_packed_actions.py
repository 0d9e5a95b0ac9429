"""Time the packed-action paths against their dense (int64 row) twins on the MI355X, with the
method of scripts/time_packed_obs.py: 16x16, real states after a 200-tick pre-roll under the
stand-in sampler, device events, the arms alternating inside one process, medians of 30, the
dense arm in the same run.  Per size (1024 and 8192 selfplay envs):

  1. k_step and k_sample_src: a dense-action engine under mrts_sample_actions_src and a
     packed-action engine under mrts_sample_actions_src_packed playing the same games (same
     seed, same stream); a repetition is STEP_TICKS ticks per arm, each tick's sampler launch and
     step launch (mrts_step_weighted; eager, delta masks and delta obs on) between their own pairs
     of events, the arms taking turns tick block by tick block.  The dense engine's step runs
     the int64 branch of the same kernel (profiles/packed_actions/README.md: its resources are
     the parent's).
  2. The action head's three launches (mrts_policy_sample_fmt / _evaluate_fmt /
     _evaluate_backward_fmt) on the final state's dense masks and N(0, 3) logits, writing /
     reading int64 rows against words; and the converters mrts_pack_actions /
     mrts_unpack_actions; launches alone, KERNEL_CALLS back to back.
  3. A PPO minibatch gather of --minibatch-envs env-steps from a --buffer-steps deep action
     buffer: buf_act[idx] int64 rows against words; the two buffers' sizes.

Algorithmic bytes, from shapes (rows = N * HW, S = source rows):
  k_sample_src   rows*4 (source) + S*312 (mask rows) + rows*56 dense | rows*4 packed
  k_step         G*HW*32 + rows*4 + (S0 + S1)*312 + N*66 + obs (delta: not counted) + S*56 dense | S*4 packed
  head sample    rows*4 + S*624 + 8 N + rows*56 | rows*4;   evaluate rows*4 + S*624 + 8 N + S*56 | S*4
  backward       evaluate + rows*312 + S*312
  pack / unpack  rows*60;   gather 2 * mb*HW*56 | 2 * mb*HW*4

  python scripts/time_packed_actions.py --out profiles/packed_actions/timing.json
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
from gym_microrts import _native, packed_actions  # noqa: E402
from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv  # noqa: E402

STEP_TICKS = 20   # ticks per repetition of a step arm


class Stepper:
    """An engine stepped by C-ABI launches under the stand-in sampler; step() returns the sampler's and the step's events."""

    def __init__(self, nsp, seed, words):
        self.env = MicroRTSGridModeVecEnv(num_selfplay_envs=nsp, num_bot_envs=0, max_steps=2000, map_paths=["maps/16x16/basesWorkers16x16.xml"],
                                          reward_weight=np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0]), device="cuda:0", return_tensors=True,
                                          action_format="packed" if words else "dense")
        e = self.env
        assert e.eager_masks and e.mask_delta
        self.n, self.hw, self.seed, self.t, self.words = e.num_envs, e.height * e.width, seed, 0, words
        self.act = torch.empty((self.n, self.hw) if words else (self.n, self.hw, 7), dtype=torch.int32 if words else torch.int64, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        e.reset()

    def step(self, timed=False):
        e, L = self.env, _native.lib()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timed else None
        sampler = L.mrts_sample_actions_src_packed if self.words else L.mrts_sample_actions_src
        if timed:
            ev[0].record()
        _native.check(sampler(self.st, e._mask.data_ptr(), e._src.data_ptr(), self.n, self.hw, 0, ctypes.c_uint64(self.seed), self.t,
                              self.act.data_ptr()))
        if timed:
            ev[1].record()
            ev[2].record()
        _native.check(L.mrts_step_weighted(e._h, self.st, self.act.data_ptr(), e._src.data_ptr(), e._obs.data_ptr(), e._raw.data_ptr(),
                                           e._done.data_ptr(), e._rew.data_ptr(), e._done0.data_ptr()), e._h, "step")
        if timed:
            ev[3].record()
        self.t += 1
        return ev


def time_steps(nsp, a):
    arms = {"dense": Stepper(nsp, a.seed, False), "packed": Stepper(nsp, a.seed, True)}
    src_rows = []
    for _ in range(a.ticks):
        for s in arms.values():
            s.step()
    torch.cuda.synchronize()
    t_s, t_k = {k: [] for k in arms}, {k: [] for k in arms}
    for rep in range(a.warmup + a.reps):
        for k, s in arms.items():
            evs = []
            for _ in range(STEP_TICKS):
                rows = s.env._src.sum()   # on both arms alike (outside the events)
                if k == "packed":
                    src_rows.append(rows)
                evs.append(s.step(timed=True))
            evs[-1][3].synchronize()
            if rep >= a.warmup:
                t_s[k].append(sum(x[0].elapsed_time(x[1]) for x in evs) * 1e-3 / STEP_TICKS)
                t_k[k].append(sum(x[2].elapsed_time(x[3]) for x in evs) * 1e-3 / STEP_TICKS)
    d, p = arms["dense"].env, arms["packed"].env
    assert torch.equal(p._obs.view(torch.int32), d._obs.view(torch.int32)) and torch.equal(p._mask, d._mask) and torch.equal(p._rew, d._rew), \
        "the arms' games diverged"
    assert torch.equal(packed_actions.unpack_actions(arms["packed"].act), arms["dense"].act)
    assert d.error_flags() == 0 and p.error_flags() == 0
    n, hw = d.num_envs, d.height * d.width
    G, rows = nsp // 2, n * hw
    S = float(torch.stack(src_rows).float().mean())
    common = G * hw * 32 + rows * 4 + 2 * S * 312 + n * 66
    res = {"num_selfplay_envs": nsp, "hw": hw, "pre_roll_ticks": a.ticks, "ticks_timed_per_arm": a.reps * STEP_TICKS, "mean_source_rows": round(S, 1),
           "k_sample_src": {"dense": summary(t_s["dense"], rows * 4 + S * 312 + rows * 56), "packed": summary(t_s["packed"], rows * 4 + S * 312 + rows * 4)},
           "k_step": {"dense": summary(t_k["dense"], common + S * 56), "packed": summary(t_k["packed"], common + S * 4)}}
    for kern in ("k_sample_src", "k_step"):
        res[kern]["packed_over_dense"] = round(res[kern]["packed"]["median_us"] / res[kern]["dense"]["median_us"], 3)
    mask, src, words = d._mask.clone(), d._src.clone(), arms["packed"].act.clone()
    d.close(), p.close()
    return res, mask, src, words


def time_head_and_converters(mask, src, a):
    lib, st = _native.lib(), torch.cuda.current_stream().cuda_stream
    n, hw = src.shape
    rows, S = n * hw, int((src != 0).sum())
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    logits = 3.0 * torch.randn((rows, 78), device="cuda", generator=g)
    act, words = torch.empty((n, hw, 7), dtype=torch.int64, device="cuda"), torch.empty((n, hw), dtype=torch.int32, device="cuda")
    act2, words2 = torch.empty_like(act), torch.empty_like(words)
    lp, ent, lp2, ent2 = (torch.empty(n, device="cuda") for _ in range(4))
    ones, grad, grad2 = torch.ones(n, device="cuda"), torch.empty_like(logits), torch.empty_like(logits)
    u64 = ctypes.c_uint64(a.seed)
    D, P = _native.MRTS_ACT_DENSE, _native.MRTS_ACT_PACKED
    lm = (logits.data_ptr(), _native.MRTS_MASK_DENSE, mask.data_ptr(), src.data_ptr(), n, hw)

    def sample(fmt, out, l, e):
        return lambda: lib.mrts_policy_sample_fmt(st, *lm, 0, u64, 0, fmt, out.data_ptr(), l.data_ptr(), e.data_ptr())

    def evaluate(fmt, x, l, e):
        return lambda: lib.mrts_policy_evaluate_fmt(st, *lm, fmt, x.data_ptr(), l.data_ptr(), e.data_ptr())

    def backward(fmt, x, gr):
        return lambda: lib.mrts_policy_evaluate_backward_fmt(st, *lm, fmt, x.data_ptr(), ones.data_ptr(), ones.data_ptr(), gr.data_ptr())

    arms = {"sample_dense_kernel": sample(D, act, lp, ent), "sample_packed_kernel": sample(P, words, lp2, ent2),
            "evaluate_dense_kernel": evaluate(D, act, lp, ent), "evaluate_packed_kernel": evaluate(P, words, lp2, ent2),
            "backward_dense_kernel": backward(D, act, grad), "backward_packed_kernel": backward(P, words, grad2),
            "pack_actions_kernel": lambda: lib.mrts_pack_actions(st, act.data_ptr(), rows, words2.data_ptr()),
            "unpack_actions_kernel": lambda: lib.mrts_unpack_actions(st, words.data_ptr(), rows, act2.data_ptr())}
    ts = alternate(arms, a.warmup, a.reps)
    torch.cuda.synchronize()
    assert torch.equal(act2, act) and torch.equal(words2, words), "the head's words are not pack of its rows"
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(ent.view(torch.int32), ent2.view(torch.int32))
    assert torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    head = rows * 4 + S * 624 + 8 * n
    nb = {"sample_dense_kernel": head + rows * 56, "sample_packed_kernel": head + rows * 4,
          "evaluate_dense_kernel": head + S * 56, "evaluate_packed_kernel": head + S * 4,
          "backward_dense_kernel": head + S * 56 + rows * 312 + S * 312, "backward_packed_kernel": head + S * 4 + rows * 312 + S * 312,
          "pack_actions_kernel": rows * 60, "unpack_actions_kernel": rows * 60}
    res = {"num_envs": n, "hw": hw, "source_rows": S, **{k: summary(v, nb[k]) for k, v in ts.items()}}
    for op in ("sample", "evaluate", "backward"):
        res[op + "_packed_over_dense"] = round(res[op + "_packed_kernel"]["median_us"] / res[op + "_dense_kernel"]["median_us"], 3)
    return res


def time_minibatch(words, a):
    """words [N, HW]: a --buffer-steps deep buffer of them (rolled along N), as int64 rows and as words."""
    T, n, hw = a.buffer_steps, words.shape[0], words.shape[1]
    mb = min(a.minibatch_envs, T * n)
    buf_w = torch.stack([words.roll(t, 0) for t in range(T)])   # [T, N, HW] int32
    buf_a = packed_actions.unpack_actions(buf_w)                # [T, N, HW, 7] int64
    fw, fa = buf_w.reshape(T * n, hw), buf_a.reshape(T * n, hw, 7)
    g = torch.Generator(device="cuda").manual_seed(a.seed)
    idx = torch.randperm(T * n, device="cuda", generator=g)[:mb]
    keep = {}

    def gather_dense():
        keep["d"] = fa[idx]

    def gather_packed():
        keep["p"] = fw[idx]

    ts = alternate({"gather_dense": gather_dense, "gather_packed": gather_packed}, a.warmup, a.reps)
    torch.cuda.synchronize()
    assert torch.equal(packed_actions.unpack_actions(keep["p"]), keep["d"])
    gb = {"gather_dense": 2 * mb * hw * 56, "gather_packed": 2 * mb * hw * 4}
    return {"buffer_steps": T, "num_envs": n, "minibatch_env_steps": mb,
            "dense_buffer_bytes": buf_a.element_size() * buf_a.nelement(), "packed_buffer_bytes": buf_w.element_size() * buf_w.nelement(),
            **{k: summary(v, gb[k]) for k, v in ts.items()},
            "packed_over_dense": round(statistics.median(ts["gather_packed"]) / statistics.median(ts["gather_dense"]), 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--buffer-steps", type=int, default=32)
    ap.add_argument("--minibatch-envs", type=int, default=4 * 8192)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_packed_actions.py needs the MI355X: there is no CPU timing")
    sizes = []
    for n in a.num_envs:
        res, mask, src, words = time_steps(n, a)
        res["head_and_converters"] = time_head_and_converters(mask, src, a)
        res["minibatch"] = time_minibatch(words, a)
        sizes.append(res)
        del mask, src, words
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": f"device events; k_sample_src / k_step arms: {STEP_TICKS} ticks per repetition, each launch between its own events, summed and "
                     f"divided; *_kernel arms: {KERNEL_CALLS} C-ABI launches back to back per repetition, divided; arms alternating; median of reps",
           "sizes": sizes}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
