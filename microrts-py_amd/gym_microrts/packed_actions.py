"""Packed actions: an action row's seven components as one 32-bit word per env and cell.

    bits 0..2 action type, 3..4 move direction, 5..6 harvest direction, 7..8 return
    direction, 9..10 produce direction, 11..13 produce type, 14..19 attack cell;
    bit 20 + k is the INVALID flag of component k; bits 27..31 are zero in what the
    library writes and ignored by every reader (include/microrts_amd.h).

A word stands for the dense row whose component k is -1 when flag k is set and the field's
value otherwise.  Packing puts component k into its field when it lies in [0, 2^bits_k);
otherwise the field is 0 and the flag is set -- such a component is out of range in the
dense row too, so step() and the action head treat pack(a) exactly as they treat a.
It is what `MicroRTSGridModeVecEnv(..., action_format="packed").step()` takes and what
`policy_head.sample(..., action_format="packed")` returns -- [N, HW] int32 -- and what a
rollout buffer can afford to keep: 4 bytes a cell against the int64 row's 56.

    words = packed_actions.pack_actions(actions)      # [..., 7] int64 -> [...] int32
    actions = packed_actions.unpack_actions(words)    # the reverse

The converters are the HIP kernels of csrc/mrts_sampler.hip on the current stream.  There
is no CPU path: a CPU tensor is an error.
"""
import torch

from . import _native

COMPONENTS = 7
FIELD_BITS = (3, 2, 2, 2, 2, 3, 6)   # the fewest bits that hold 0 .. nvec[k] - 1, nvec = (6, 4, 4, 4, 4, 7, 49)
FLAG_BIT = sum(FIELD_BITS)           # 20: component k's invalid flag is bit FLAG_BIT + k


def _check(t, name, dtype, last=None):
    """Type, dtype, the last dimension when given, then device and layout (so a shape error names the shape)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
    if last is not None and (t.dim() < 1 or t.shape[-1] != last):
        raise ValueError(f"{name} must be [..., {last}], not {tuple(t.shape)}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} is on {t.device}: the action converters run on the GPU only (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def pack_actions(actions):
    """`actions` [..., 7] int64 device tensor -> words [...] int32.  A component outside its
    field's range (negative, or >= 4 in a direction, >= 8 in the type or produce type, >= 64
    in the attack cell) sets its invalid flag."""
    _check(actions, "actions", torch.int64, COMPONENTS)
    dev = actions.device
    words = torch.empty(tuple(actions.shape[:-1]), dtype=torch.int32, device=dev)
    if words.numel() == 0:   # an empty tensor has no pointer to pass
        return words
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_pack_actions(_stream(dev), actions.data_ptr(), words.numel(), words.data_ptr())
    _native.check(rc, None, "pack_actions")
    return words


def unpack_actions(words, out=None):
    """`words` [...] int32 device tensor -> actions [..., 7] int64, every element written: -1
    where the component's flag is set, the field's value otherwise.  `out`: a contiguous int64
    tensor of the result's shape on the same device to write into."""
    _check(words, "words", torch.int32)
    shape = tuple(words.shape) + (COMPONENTS,)
    dev = words.device
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=dev)
    else:
        _check(out, "out", torch.int64)
        if tuple(out.shape) != shape or out.device != dev:
            raise ValueError(f"out must be {shape} on {dev}, not {tuple(out.shape)} on {out.device}")
    if words.numel() == 0:
        return out
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_unpack_actions(_stream(dev), words.data_ptr(), words.numel(), out.data_ptr())
    _native.check(rc, None, "unpack_actions")
    return out
