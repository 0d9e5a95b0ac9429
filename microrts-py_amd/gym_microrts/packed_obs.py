"""Packed observations: the one-hot obs as one 32-bit word per env and cell.

Bit i of a cell's word is plane i of the dense obs, i < P (P = 29, or 31 with partial
obs); bits P..31 are zero in what the engine writes and ignored by every reader
(include/microrts_amd.h).  It is what `MicroRTSGridModeVecEnv(..., obs_format="packed")`
returns from reset() / step() -- [N, H, W] int32 -- and what a rollout buffer can afford
to keep: 4 bytes a cell against the dense float32 form's 116 or 124.  The network still
reads dense planes, so the rollout unpacks once per forward, straight into the
network's input dtype:

    dense = packed_obs.unpack_obs(packed, planes, dtype=torch.float32, out=dense)   # [N, H, W, planes]
    packed = packed_obs.pack_obs(dense)                                              # the reverse

The converters are the HIP kernels of csrc/mrts_obs.hip on the current stream.  There
is no CPU path: a CPU tensor is an error.
"""
import torch

from . import _native

PLANES = (29, 31)
ELEM = {torch.int32: _native.MRTS_ELEM_INT32, torch.float32: _native.MRTS_ELEM_FLOAT32,
        torch.float16: _native.MRTS_ELEM_FLOAT16, torch.bfloat16: _native.MRTS_ELEM_BFLOAT16}


def _check(t, name, dtypes):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} is on {t.device}: the obs converters run on the GPU only (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def unpack_obs(packed, planes, dtype=torch.float32, out=None):
    """`packed` [..., H, W] int32 device tensor -> [..., H, W, planes] of 0 / 1 in `dtype`
    (int32, float32, float16 or bfloat16); planes is 29 or 31, bits at or above it are
    ignored.  int32 and float32 results are a dense engine's own obs bit for bit.
    `out`: a contiguous tensor of the result's shape and dtype on the same device to write
    into (every element is written), so a rollout reuses one dense tensor."""
    if planes not in PLANES:
        raise ValueError(f"planes must be 29 or 31, not {planes!r}")
    if dtype not in ELEM:
        raise ValueError(f"dtype must be one of {', '.join(str(d) for d in ELEM)}, not {dtype}")
    _check(packed, "packed", (torch.int32,))
    if packed.dim() < 2:
        raise ValueError(f"packed must be [..., H, W], not {tuple(packed.shape)}")
    shape = tuple(packed.shape) + (planes,)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=packed.device)
    else:
        _check(out, "out", (dtype,))
        if tuple(out.shape) != shape or out.device != packed.device:
            raise ValueError(f"out must be {shape} on {packed.device}, not {tuple(out.shape)} on {out.device}")
    dev = packed.device
    if packed.numel() == 0:   # an empty tensor has no pointer to pass
        return out
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_unpack_obs(_stream(dev), packed.data_ptr(), packed.numel(), planes, ELEM[dtype], out.data_ptr())
    _native.check(rc, None, "unpack_obs")
    return out


def pack_obs(obs):
    """Dense [..., H, W, planes] device tensor (int32, float32, float16 or bfloat16; planes
    = obs.shape[-1] is 29 or 31) -> [..., H, W] int32: bit i is set where plane i's
    element is non-zero."""
    _check(obs, "obs", tuple(ELEM))
    if obs.dim() < 3 or obs.shape[-1] not in PLANES:
        raise ValueError(f"obs must be [..., H, W, 29 or 31], not {tuple(obs.shape)}")
    planes = int(obs.shape[-1])
    dev = obs.device
    packed = torch.empty(tuple(obs.shape[:-1]), dtype=torch.int32, device=dev)
    if packed.numel() == 0:
        return packed
    with torch.cuda.device(dev):
        rc = _native.lib().mrts_pack_obs(_stream(dev), obs.data_ptr(), packed.numel(), planes, ELEM[obs.dtype], packed.data_ptr())
    _native.check(rc, None, "pack_obs")
    return packed
