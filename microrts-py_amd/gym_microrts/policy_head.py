"""The masked action head of a GridNet policy on the device.

`sample` and `evaluate` replace the seven `CategoricalMasked` chains of the
reference's `Agent.get_action_and_value` (experiments/ppo_gridnet.py:164-167,
215-247) with the HIP kernels of csrc/mrts_policy.hip, which read only the mask and
logit rows of cells that hold a unit that can act:

    actions, logprob, entropy = policy_head.sample(logits, mask, source, seed=s, step=t)
    logprob, entropy = policy_head.evaluate(logits, mask, source, actions)   # differentiable in logits

`mask` and `source` are what `get_action_mask()` and `source_unit_mask` return on the
tensor contract ([N, HW, 78] and [N, HW] int32 device tensors); `logits` is [N*HW, 78]
or [N, HW, 78] float32.  A component with no valid entry (every component of a
non-source cell) contributes 0 to the log-prob and the entropy, as the reference's
float32 arithmetic does.  There is no CPU path: a CPU tensor is an error.
"""
import ctypes

import torch

from . import _native

CHANNELS = 78      # sum of the action plane's nvec (vec_env.py:234)
COMPONENTS = 7


def _need(t, name, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")


def _on_gpu(ref, **tensors):
    """Every tensor on one GPU (checked after the shapes, so a shape error names the shape)."""
    for name, t in tensors.items():
        if t.device.type != "cuda":
            raise ValueError(f"{name} is on {t.device}: the action head runs on the GPU only (no CPU fallback)")
        if t.device != ref.device:
            raise ValueError(f"{name} is on {t.device}, logits on {ref.device}")


def _as_int32(t):
    """int32 as the engine writes it, or the float copy a rollout buffer holds."""
    return (t if t.dtype == torch.int32 else t.to(torch.int32)).contiguous()


def _inputs(logits, mask, source, float_masks, actions=None):
    """Check the three inputs; returns (logits, mask, source, N, HW) contiguous, mask / source int32."""
    _need(logits, "logits", (torch.float32,))
    mdt = (torch.int32, torch.float32) if float_masks else (torch.int32,)
    _need(mask, "mask", mdt)
    _need(source, "source", mdt)
    if mask.dim() != 3 or mask.shape[2] != CHANNELS or mask.shape[1] < 1:
        raise ValueError(f"mask must be [N, HW, {CHANNELS}], not {tuple(mask.shape)}")
    n, hw = int(mask.shape[0]), int(mask.shape[1])
    if tuple(source.shape) != (n, hw):
        raise ValueError(f"source must be [N, HW] = {(n, hw)}, not {tuple(source.shape)}")
    if tuple(logits.shape) not in ((n * hw, CHANNELS), (n, hw, CHANNELS)):
        raise ValueError(f"logits must be [N*HW, {CHANNELS}] or [N, HW, {CHANNELS}] with N, HW = {(n, hw)}, not {tuple(logits.shape)}")
    if actions is not None:
        _need(actions, "actions", (torch.int64,))
        if actions.numel() != n * hw * COMPONENTS:
            raise ValueError(f"actions must hold N*HW*{COMPONENTS} = {n * hw * COMPONENTS} elements, not {tuple(actions.shape)}")
        _on_gpu(logits, logits=logits, mask=mask, source=source, actions=actions)
    else:
        _on_gpu(logits, logits=logits, mask=mask, source=source)
    return logits.contiguous(), _as_int32(mask), _as_int32(source), n, hw


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def sample(logits, mask, source, *, seed, step, env0=0):
    """Draw one action per component and cell: (actions [N, HW, 7] int64, what
    `step()` takes zero-copy; logprob [N]; entropy [N], float32).  The draw is the
    inverse CDF of the masked softmax at the Philox words keyed by (cell, env0 + env,
    step) under `seed` -- the stream of the engine's stand-in sampler, so a shard
    [env0, env0 + N) draws exactly its slice of one larger batch.  No grad."""
    lg, m, s, n, hw = _inputs(logits, mask, source, False)
    dev = lg.device
    actions = torch.empty((n, hw, COMPONENTS), dtype=torch.int64, device=dev)
    logprob = torch.empty((n,), dtype=torch.float32, device=dev)
    entropy = torch.empty((n,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_policy_sample(_stream(dev), lg.detach().data_ptr(), m.data_ptr(), s.data_ptr(), n, hw, int(env0),
                                              ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(step) & 0xFFFFFFFF, actions.data_ptr(),
                                              logprob.data_ptr(), entropy.data_ptr())
    _native.check(rc, None, "policy_sample")
    return actions, logprob, entropy


class _Evaluate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, mask, source, actions, n, hw):
        dev = logits.device
        logprob = torch.empty((n,), dtype=torch.float32, device=dev)
        entropy = torch.empty((n,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _native.lib().mrts_policy_evaluate(_stream(dev), logits.data_ptr(), mask.data_ptr(), source.data_ptr(), n, hw,
                                                    actions.data_ptr(), logprob.data_ptr(), entropy.data_ptr())
        _native.check(rc, None, "policy_evaluate")
        ctx.save_for_backward(logits, mask, source, actions)
        ctx.shape = (n, hw)
        return logprob, entropy

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        logits, mask, source, actions = ctx.saved_tensors
        n, hw = ctx.shape
        dev = logits.device
        zero = None
        if g_lp is None or g_ent is None:
            zero = torch.zeros((n,), dtype=torch.float32, device=dev)
        g_lp = zero if g_lp is None else g_lp.to(torch.float32).contiguous()
        g_ent = zero if g_ent is None else g_ent.to(torch.float32).contiguous()
        grad = torch.empty_like(logits)   # the kernel writes every element
        with torch.cuda.device(dev):
            rc = _native.lib().mrts_policy_evaluate_backward(_stream(dev), logits.data_ptr(), mask.data_ptr(), source.data_ptr(), n, hw,
                                                             actions.data_ptr(), g_lp.data_ptr(), g_ent.data_ptr(), grad.data_ptr())
        _native.check(rc, None, "policy_evaluate_backward")
        return grad, None, None, None, None, None


def evaluate(logits, mask, source, actions):
    """(logprob [N], entropy [N]) of `actions` ([N, HW, 7] or [N, HW*7] int64) under the
    masked softmax; differentiable in `logits` (the backward is a kernel too).  `mask` /
    `source` may also be the float32 copies a rollout buffer holds: they are converted
    to int32 once per call.  An action the mask forbids contributes -1e8, the
    reference's float32 value."""
    lg, m, s, n, hw = _inputs(logits, mask, source, True, actions)
    return _Evaluate.apply(lg, m, s, actions.contiguous(), n, hw)
