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

Packed masks: getMasks' 79-bit word per cell in three int32 words, [N, HW, 3] -- bit 0
the source channel, bit ch + 1 mask channel ch (include/microrts_amd.h).  It is what
`get_action_mask_packed()` returns and what a rollout buffer can afford to keep (12
bytes a row against 316).  `sample` and `evaluate` take it in place of `mask` with no
`source`, and give the dense calls' results bit for bit:

    packed = policy_head.pack_masks(mask, source)          # or env.get_action_mask_packed()
    mask, source = policy_head.unpack_masks(packed)
    actions, logprob, entropy = policy_head.sample(logits, packed, seed=s, step=t)
    logprob, entropy = policy_head.evaluate(logits, packed, actions=actions)

Packed actions: a row's seven components in one int32 word per cell, [N, HW]
(gym_microrts.packed_actions; 4 bytes a cell against 56).  `sample(..., action_format="packed")`
writes them -- what an `action_format="packed"` env's step() takes zero-copy -- and
`evaluate` recognises them by dtype int32 and N*HW elements.  With either mask format the
results are the dense-action calls' bit for bit: log-prob, entropy, gradient, and
`packed_actions.unpack_actions` of the words.
"""
import ctypes

import torch

from . import _native

CHANNELS = 78      # sum of the action plane's nvec (vec_env.py:234)
COMPONENTS = 7
PACKED_WORDS = 3   # a packed row: the source bit + 78 channels in 96 bits


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


def _is_packed(mask):
    """A packed tensor by its shape: [N, HW, 3] (a dense mask ends in 78)."""
    return isinstance(mask, torch.Tensor) and mask.dim() == 3 and mask.shape[2] == PACKED_WORDS


def _format(mask, source):
    """True for a packed call (packed masks, no source), False for a dense one (mask and
    source); ValueError for the two mixed forms."""
    if source is None:
        if isinstance(mask, torch.Tensor) and mask.dim() >= 1 and mask.shape[-1] == CHANNELS:
            raise ValueError(f"a dense mask [N, HW, {CHANNELS}] needs its source [N, HW]; only packed masks "
                             f"[N, HW, {PACKED_WORDS}] come without one")
        return True
    if _is_packed(mask):
        raise ValueError(f"packed masks [N, HW, {PACKED_WORDS}] hold the source channel (bit 0): pass source=None")
    return False


def _dense(mask, source):
    """Check a dense pair's shapes; returns (N, HW)."""
    if mask.dim() != 3 or mask.shape[2] != CHANNELS or mask.shape[1] < 1:
        raise ValueError(f"mask must be [N, HW, {CHANNELS}], not {tuple(mask.shape)}")
    n, hw = int(mask.shape[0]), int(mask.shape[1])
    if tuple(source.shape) != (n, hw):
        raise ValueError(f"source must be [N, HW] = {(n, hw)}, not {tuple(source.shape)}")
    return n, hw


def _packed(packed):
    """Check a packed tensor's type and shape; returns (N, HW)."""
    _need(packed, "packed", (torch.int32,))
    if packed.dim() != 3 or packed.shape[2] != PACKED_WORDS or packed.shape[1] < 1:
        raise ValueError(f"packed must be [N, HW, {PACKED_WORDS}], not {tuple(packed.shape)}")
    return int(packed.shape[0]), int(packed.shape[1])


def _inputs(logits, mask, source, float_masks, actions=None):
    """Check a call's inputs, dense (mask and source) or packed (source is None: `mask` is the
    packed words); returns (logits, mask, source or None, N, HW) contiguous, the masks int32."""
    _need(logits, "logits", (torch.float32,))
    if source is None:
        n, hw = _packed(mask)
        tensors = {"logits": logits, "packed": mask}
    else:
        mdt = (torch.int32, torch.float32) if float_masks else (torch.int32,)
        _need(mask, "mask", mdt)
        _need(source, "source", mdt)
        n, hw = _dense(mask, source)
        tensors = {"logits": logits, "mask": mask, "source": source}
    if tuple(logits.shape) not in ((n * hw, CHANNELS), (n, hw, CHANNELS)):
        raise ValueError(f"logits must be [N*HW, {CHANNELS}] or [N, HW, {CHANNELS}] with N, HW = {(n, hw)}, not {tuple(logits.shape)}")
    if actions is not None:
        # packed action words: int32 with N*HW elements; anything else is held to the int64 rows' rules
        words = isinstance(actions, torch.Tensor) and actions.dtype == torch.int32 and actions.numel() == n * hw
        if not words:
            _need(actions, "actions", (torch.int64,))
            if actions.numel() != n * hw * COMPONENTS:
                raise ValueError(f"actions must hold N*HW*{COMPONENTS} = {n * hw * COMPONENTS} elements (int64 rows; or N*HW = {n * hw} "
                                 f"packed int32 words), not {tuple(actions.shape)}")
        tensors["actions"] = actions
    _on_gpu(logits, **tensors)
    return logits.contiguous(), _as_int32(mask), None if source is None else _as_int32(source), n, hw


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _head(name, logits, mask, source, n, hw, head, actions, *tail):
    """Call the action head's entry point mrts_`name`_fmt on the logits' device and current
    stream: packed masks when source is None, packed action words when `actions` is int32.
    `head`: the arguments between the shape and the actions."""
    dev = logits.device
    mfmt, src = (_native.MRTS_MASK_PACKED, None) if source is None else (_native.MRTS_MASK_DENSE, source.data_ptr())
    afmt = _native.MRTS_ACT_PACKED if actions.dtype == torch.int32 else _native.MRTS_ACT_DENSE
    with torch.cuda.device(dev):
        rc = getattr(_native.lib(), f"mrts_{name}_fmt")(_stream(dev), logits.data_ptr(), mfmt, mask.data_ptr(), src, n, hw, *head,
                                                       afmt, actions.data_ptr(), *tail)
    _native.check(rc, None, name)


def pack_masks(mask, source):
    """Dense -> packed: `mask` [N, HW, 78] and `source` [N, HW] int32 device tensors ->
    [N, HW, 3] int32.  A bit is set where the element is non-zero; every row is kept, a
    non-source row's stray bits too."""
    _need(mask, "mask", (torch.int32,))
    _need(source, "source", (torch.int32,))
    n, hw = _dense(mask, source)
    _on_gpu(mask, mask=mask, source=source)
    dev = mask.device
    m, s = mask.contiguous(), source.contiguous()
    packed = torch.empty((n, hw, PACKED_WORDS), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_pack_masks(_stream(dev), m.data_ptr(), s.data_ptr(), n, hw, packed.data_ptr())
    _native.check(rc, None, "pack_masks")
    return packed


def unpack_masks(packed):
    """Packed [N, HW, 3] int32 -> (mask [N, HW, 78], source [N, HW]) int32 of 0 / 1, the
    tensors `get_action_mask()` and `source_unit_mask` return on the tensor contract."""
    n, hw = _packed(packed)
    _on_gpu(packed, packed=packed)
    dev = packed.device
    p = packed.contiguous()
    mask = torch.empty((n, hw, CHANNELS), dtype=torch.int32, device=dev)
    source = torch.empty((n, hw), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_unpack_masks(_stream(dev), p.data_ptr(), n, hw, mask.data_ptr(), source.data_ptr())
    _native.check(rc, None, "unpack_masks")
    return mask, source


def sample(logits, mask, source=None, *, seed, step, env0=0, action_format="dense"):
    """Draw one action per component and cell: (actions [N, HW, 7] int64, what
    `step()` takes zero-copy -- or, with action_format="packed", the same actions as packed
    words [N, HW] int32, what an action_format="packed" env takes; logprob [N]; entropy [N], float32).  The draw is the
    inverse CDF of the masked softmax at the Philox words keyed by (cell, env0 + env,
    step) under `seed` -- the stream of the engine's stand-in sampler, so a shard
    [env0, env0 + N) draws exactly its slice of one larger batch.  No grad.
    `mask` with `source`: the dense tensors; `mask` alone: packed [N, HW, 3] int32."""
    if action_format not in ("dense", "packed"):
        raise ValueError(f"action_format must be 'dense' or 'packed', not {action_format!r}")
    _format(mask, source)
    lg, m, s, n, hw = _inputs(logits, mask, source, False)
    dev = lg.device
    if action_format == "packed":
        actions = torch.empty((n, hw), dtype=torch.int32, device=dev)
    else:
        actions = torch.empty((n, hw, COMPONENTS), dtype=torch.int64, device=dev)
    logprob = torch.empty((n,), dtype=torch.float32, device=dev)
    entropy = torch.empty((n,), dtype=torch.float32, device=dev)
    _head("policy_sample", lg.detach(), m, s, n, hw, (int(env0), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), int(step) & 0xFFFFFFFF),
          actions, logprob.data_ptr(), entropy.data_ptr())
    return actions, logprob, entropy


class _Evaluate(torch.autograd.Function):
    """`source` is None for packed masks, which `mask` then holds."""

    @staticmethod
    def forward(ctx, logits, mask, source, actions, n, hw):
        logprob = torch.empty((n,), dtype=torch.float32, device=logits.device)
        entropy = torch.empty((n,), dtype=torch.float32, device=logits.device)
        _head("policy_evaluate", logits, mask, source, n, hw, (), actions, logprob.data_ptr(), entropy.data_ptr())
        ctx.save_for_backward(logits, mask, source, actions)
        ctx.shape = (n, hw)
        return logprob, entropy

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        logits, mask, source, actions = ctx.saved_tensors
        n, hw = ctx.shape
        zero = None
        if g_lp is None or g_ent is None:
            zero = torch.zeros((n,), dtype=torch.float32, device=logits.device)
        g_lp = zero if g_lp is None else g_lp.to(torch.float32).contiguous()
        g_ent = zero if g_ent is None else g_ent.to(torch.float32).contiguous()
        grad = torch.empty_like(logits)   # the kernel writes every element
        _head("policy_evaluate_backward", logits, mask, source, n, hw, (), actions, g_lp.data_ptr(), g_ent.data_ptr(),
              grad.data_ptr())
        return grad, None, None, None, None, None


def evaluate(logits, mask, source=None, actions=None):
    """(logprob [N], entropy [N]) of `actions` ([N, HW, 7] or [N, HW*7] int64, or packed action
    words: int32 with N*HW elements, read as the rows they stand for) under the
    masked softmax; differentiable in `logits` (the backward is a kernel too).  `mask` /
    `source` may also be the float32 copies a rollout buffer holds: they are converted
    to int32 once per call.  An action the mask forbids contributes -1e8, the
    reference's float32 value.  `mask` alone (source=None, `actions` by keyword): packed
    [N, HW, 3] int32, as it comes out of the rollout buffer."""
    if actions is None:
        raise TypeError("evaluate() needs the actions to evaluate")
    _format(mask, source)
    lg, m, s, n, hw = _inputs(logits, mask, source, True, actions)
    return _Evaluate.apply(lg, m, s, actions.contiguous(), n, hw)
