"""The first encoder stage of a GridNet policy on packed observations.

`encode(packed, weight, bias)` is `Conv2d(P, C, 3, padding=1) -> MaxPool2d(3, 2, 1) -> ReLU`
computed straight from the packed obs words (packed_obs.py: one int32 per env and cell,
bit i = plane i), with no dense obs in between:

    x = obs_conv.encode(packed, conv.weight, conv.bias)   # [N, C, (H-1)//2+1, (W-1)//2+1] float32

Over a one-hot input the convolution has no multiplies, so an output is the bias plus the
weights that the set bits of nine words select (include/microrts_amd.h states the order of
the adds).  The backward reaches `weight` and `bias` only -- the words carry no gradient --
and recomputes the forward from the words, so autograd keeps nothing but the three inputs.
Both directions are the HIP kernels of csrc/mrts_conv.hip on the current stream.  There is
no CPU path: a CPU tensor is an error.
"""
import torch

from . import _native
from .packed_obs import PLANES, _check, _stream

MAX_CHANNELS = 64


def _shapes(packed, weight, bias):
    _check(packed, "packed", (torch.int32,))
    _check(weight, "weight", (torch.float32,))
    _check(bias, "bias", (torch.float32,))
    if packed.dim() < 2:
        raise ValueError(f"packed must be [..., H, W], not {tuple(packed.shape)}")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] not in PLANES:
        raise ValueError(f"weight must be [C, 29 or 31, 3, 3], not {tuple(weight.shape)}")
    c, planes = int(weight.shape[0]), int(weight.shape[1])
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"weight has {c} output channels: 1..{MAX_CHANNELS} are supported")
    if tuple(bias.shape) != (c,):
        raise ValueError(f"bias must be [{c}], not {tuple(bias.shape)}")
    if weight.device != packed.device or bias.device != packed.device:
        raise ValueError(f"packed, weight and bias must share a device, not {packed.device}, {weight.device}, {bias.device}")
    h, w = int(packed.shape[-2]), int(packed.shape[-1])
    n = packed.numel() // (h * w) if h * w else 0
    if _native.lib().mrts_obs_conv_workspace_bytes(n, h, w, planes, c) < 0:
        raise ValueError(f"packed {tuple(packed.shape)} is outside the supported sizes (a map of 1..4096 cells, "
                         f"all cells together below 2**31 - 256)")
    return n, h, w, planes, c


class _Encode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed, weight, bias):
        n, h, w, planes, c = ctx.shape = _shapes(packed, weight, bias)
        dev = packed.device
        out = torch.empty(tuple(packed.shape[:-2]) + (c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=dev)
        if n:
            with torch.cuda.device(dev):
                rc = _native.lib().mrts_obs_conv_forward(_stream(dev), packed.data_ptr(), n, h, w, planes, weight.data_ptr(),
                                                         bias.data_ptr(), c, out.data_ptr())
            _native.check(rc, None, "obs_conv_forward")
        ctx.save_for_backward(packed, weight, bias)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            return None, None, None
        packed, weight, bias = ctx.saved_tensors
        n, h, w, planes, c = ctx.shape
        dev = packed.device
        if n == 0:
            gw, gb = torch.zeros_like(weight), torch.zeros_like(bias)
        else:
            gw, gb = torch.empty_like(weight), torch.empty_like(bias)
            g = grad_out.to(torch.float32).contiguous()
            lib = _native.lib()
            nbytes = lib.mrts_obs_conv_workspace_bytes(n, h, w, planes, c)
            ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                rc = lib.mrts_obs_conv_backward(_stream(dev), packed.data_ptr(), n, h, w, planes, weight.data_ptr(), bias.data_ptr(),
                                                c, g.data_ptr(), ws.data_ptr(), nbytes, gw.data_ptr(), gb.data_ptr())
            _native.check(rc, None, "obs_conv_backward")
        return None, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None


def encode(packed, weight, bias):
    """`packed` [..., H, W] int32 device tensor (any leading dimensions are the batch),
    `weight` [C, P, 3, 3] and `bias` [C] float32 on the same device, all contiguous; P is 29
    or 31 and bits of a word at or above it are ignored, C is 1..64.  Returns
    relu(max_pool2d(conv2d(unpacked planes, weight, bias, padding=1), 3, 2, 1)) as
    [..., C, (H-1)//2+1, (W-1)//2+1] float32, differentiable in `weight` and `bias`; the
    backward launch is skipped when neither needs a gradient."""
    _shapes(packed, weight, bias)
    return _Encode.apply(packed, weight, bias)
