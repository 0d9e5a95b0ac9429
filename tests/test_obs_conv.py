"""The fused first encoder stage on packed obs (conv3x3 + max-pool + ReLU from the words), the
parts that need no GPU: the numpy statement of its contract (obs_conv_ref.py) against torch on
the CPU, the C ABI's argument checks, the module's and the driver's input checks.  The kernels
themselves: test_gpu_obs_conv.py.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from obs_conv_ref import conv_ref, gamma, grad_ref, pool_ref, sota_first_layer, words
from test_packed_obs import unpack_obs_ref


def weights_of(kind, P, rng):
    if kind == "sota":
        w, b = sota_first_layer()
        assert w.shape == (32, 29, 3, 3) and P == 29
        return w, b
    return (rng.normal(0, 0.1, (5, P, 3, 3)).astype(np.float32), rng.normal(0, 0.1, (5,)).astype(np.float32))


def torch_stage64(packed, P, weight, bias, grad_out=None):
    """float64 torch on the CPU from the unpacked planes: conv, the error bound of a float32
    evaluation of each conv output (gamma_64 * (|bias| + sum |selected weights|): at most
    1 + 9 * 7 terms), the pool with its indices, and -- given grad_out -- autograd's gradients."""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(unpack_obs_ref(packed, P, np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(weight.astype(np.float64)).requires_grad_(grad_out is not None)
    b = torch.from_numpy(bias.astype(np.float64)).requires_grad_(grad_out is not None)
    conv = F.conv2d(x, w, b, padding=1)
    bound = gamma(64) * F.conv2d(x, w.detach().abs(), b.detach().abs(), padding=1)
    m, idx = F.max_pool2d(conv, 3, 2, 1, return_indices=True)
    out = torch.relu(m)
    grads = None
    if grad_out is not None:
        out.backward(torch.from_numpy(np.asarray(grad_out, np.float64)))
        grads = (w.grad.numpy(), b.grad.numpy())
    pooled_bound = F.max_pool2d(bound, 3, 2, 1)
    return conv.detach().numpy(), bound.numpy(), idx.numpy(), out.detach().numpy(), pooled_bound.numpy(), grads


@pytest.mark.parametrize("kind,P", [("sota", 29), ("normal", 29), ("normal", 31)])
@pytest.mark.parametrize("H,W", [(8, 8), (9, 13), (16, 16)])
def test_the_statement_against_torch(H, W, kind, P):
    """conv_ref is within gamma_64 * (|bias| + sum |selected weights|) of float64 conv2d on the
    unpacked planes, pool_ref's argmax is max_pool2d's index on every output (tied empty
    regions included), grad_ref is torch's float64 autograd to 1e-12, and both ReLU branches
    are taken (the share of outputs with m > 0 was 0.70-0.84 for these inputs)."""
    rng = np.random.default_rng(H * 100 + W + P)
    weight, bias = weights_of(kind, P, rng)
    packed = words(rng, (4, H, W), P)
    conv = conv_ref(packed, weight, bias)
    out, m, arg = pool_ref(conv)
    assert conv.dtype == np.float32 and out.dtype == np.float32
    gout = rng.standard_normal(out.shape)
    # the gradient flows where the float32 forward says m > 0: give torch that forward's sign
    # pattern only if it agrees, which it must away from m = 0 (asserted below)
    t_conv, t_bound, t_idx, t_out, t_pbound, (t_gw, t_gb) = torch_stage64(packed, P, weight, bias, gout)
    assert (np.abs(conv - t_conv) <= t_bound).all()
    np.testing.assert_array_equal(arg, t_idx)
    assert (np.abs(out - t_out) <= t_pbound).all()
    share = float((m > 0).mean())
    print(f"share of outputs with m > 0: {share:.3f}")
    assert 0.05 < share < 0.95
    t_m = np.take_along_axis(t_conv.reshape(t_conv.shape[:2] + (-1,)), t_idx.reshape(t_idx.shape[:2] + (-1,)), -1).reshape(m.shape)
    assert ((m > 0) == (t_m > 0)).all(), "a maximum within rounding of zero: choose another seed"
    gw, gb, Kw, Kb, Sw, Sb = grad_ref(packed, P, m, arg, gout)
    np.testing.assert_allclose(gw, t_gw, rtol=1e-12, atol=1e-12 * max(1.0, float(Sw.max())))
    np.testing.assert_allclose(gb, t_gb, rtol=1e-12, atol=1e-12 * max(1.0, float(Sb.max())))
    assert (Kb == (m > 0).sum((0, 2, 3))).all() and (Sw <= Sb[:, None, None, None] + 1e-9).all()
    assert (gw[Kw == 0] == 0).all()


def test_zero_words_and_high_bits_in_the_statement():
    """A zero word adds nothing (zero padding), bits at or above P are nobody's, and an
    all-ones word selects every plane."""
    rng = np.random.default_rng(5)
    weight, bias = weights_of("normal", 29, rng)
    packed = words(rng, (2, 8, 8), 29).view(np.uint32).copy()
    packed[0, 2:5, 3] = 0
    packed[1, 0, 0] = 0xFFFFFFFF
    packed[1, 7, 6] |= 0xE0000000
    a = conv_ref(packed.view(np.int32), weight, bias)
    b = conv_ref((packed & np.uint32((1 << 29) - 1)).view(np.int32), weight, bias)
    np.testing.assert_array_equal(a, b)
    t_conv, t_bound = torch_stage64(packed.view(np.int32), 29, weight, bias)[:2]
    assert (np.abs(a - t_conv) <= t_bound * gamma(1 + 9 * 29) / gamma(64)).all()   # all-ones words: up to 1 + 9 * 29 terms


# ------------------------------------------------------------------ C ABI (host only)
def test_obs_conv_entry_points_refuse_bad_arguments():
    """MRTS_EINVAL on the host, before any launch: a null pointer, planes other than 29 / 31,
    channels outside 1..64, height or width below 1, a map over 4096 cells, n < 0 or
    n * height * width beyond 2^31 - 257, a workspace smaller than the query says; n == 0 is
    MRTS_OK and launches nothing."""
    from gym_microrts import _native

    L = _native.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    EINVAL = -1
    BIG = 1 << 40

    def query(n=2, h=16, w=16, planes=29, c=32):
        return L.mrts_obs_conv_workspace_bytes(n, h, w, planes, c)

    def fwd(packed=p, n=2, h=16, w=16, planes=29, weight=p, bias=p, c=32, out=p):
        return L.mrts_obs_conv_forward(None, packed, n, h, w, planes, weight, bias, c, out)

    def bwd(packed=p, n=2, h=16, w=16, planes=29, weight=p, bias=p, c=32, gout=p, ws=p, ws_bytes=BIG, gw=p, gb=p):
        return L.mrts_obs_conv_backward(None, packed, n, h, w, planes, weight, bias, c, gout, ws, ws_bytes, gw, gb)

    assert query() > 0 and query(n=0) == 0
    assert query(n=1, h=1, w=1, c=1) > 0 and query(h=47, w=24, planes=31, c=64) > 0 and query(h=1, w=1128) > 0
    for fn in (query, fwd, bwd):
        for planes in (0, 28, 30, 32, -29, 78):
            assert fn(planes=planes) == EINVAL, (fn.__name__, planes)
        for c in (0, -1, 65, 1 << 20):
            assert fn(c=c) == EINVAL, (fn.__name__, c)
        assert fn(h=0) == EINVAL and fn(w=0) == EINVAL and fn(h=-16) == EINVAL and fn(w=-1) == EINVAL, fn.__name__
        assert fn(h=64, w=65) == EINVAL and fn(h=4097, w=1) == EINVAL and fn(h=1 << 20, w=1 << 20) == EINVAL, fn.__name__
        assert fn(n=-1) == EINVAL, fn.__name__
        assert fn(n=(2 ** 31 - 256) // 256 + 1) == EINVAL and fn(n=2 ** 31 - 1) == EINVAL, fn.__name__   # rows beyond 32 bits
    for name in ("packed", "weight", "bias", "out"):
        assert fwd(**{name: None}) == EINVAL, name
    for name in ("packed", "weight", "bias", "gout", "ws", "gw", "gb"):
        assert bwd(**{name: None}) == EINVAL, name
    need = query()
    assert bwd(ws_bytes=need - 1) == EINVAL and bwd(ws_bytes=0) == EINVAL and bwd(ws_bytes=-1) == EINVAL
    for planes in (29, 31):   # nothing to launch
        assert fwd(n=0, planes=planes) == 0 and bwd(n=0, planes=planes, ws_bytes=0) == 0
    del buf


# ------------------------------------------------------------------ the module's and the driver's checks
def test_module_checks_for_obs_conv():
    import torch

    from gym_microrts import obs_conv

    packed = torch.zeros((2, 8, 8), dtype=torch.int32)
    weight, bias = torch.zeros((32, 29, 3, 3)), torch.zeros((32,))
    with pytest.raises(ValueError, match="GPU only"):
        obs_conv.encode(packed, weight, bias)
    with pytest.raises(ValueError, match="torch.int32"):
        obs_conv.encode(packed.float(), weight, bias)
    with pytest.raises(ValueError, match="torch.Tensor"):
        obs_conv.encode(packed.numpy(), weight, bias)
    if not torch.cuda.is_available():
        return
    dev = "cuda"
    with pytest.raises(ValueError, match="GPU only"):
        obs_conv.encode(packed.to(dev), weight, bias.to(dev))
    packed, weight, bias = packed.to(dev), weight.to(dev), bias.to(dev)
    with pytest.raises(ValueError, match="torch.float32"):
        obs_conv.encode(packed, weight.double(), bias)
    for bad_w in (torch.zeros((32, 30, 3, 3), device=dev), torch.zeros((32, 29, 3), device=dev), torch.zeros((65, 29, 3, 3), device=dev),
                  torch.zeros((32, 29, 5, 5), device=dev)):
        with pytest.raises(ValueError, match="weight"):
            obs_conv.encode(packed, bad_w, bias)
    with pytest.raises(ValueError, match="bias"):
        obs_conv.encode(packed, weight, bias[:31].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        obs_conv.encode(packed.transpose(1, 2), weight, bias)
    with pytest.raises(ValueError, match=r"\[\.\.\., H, W\]"):
        obs_conv.encode(packed[0, 0], weight, bias)
    with pytest.raises(ValueError, match="supported sizes"):
        obs_conv.encode(torch.zeros((1, 65, 64), dtype=torch.int32, device=dev), weight, bias)


def _driver():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_fused_encoder_needs_packed_obs():
    drv = _driver()
    with pytest.raises(ValueError, match="--encoder fused needs --obs packed"):
        drv.run(api="tensor", head="fused", encoder="fused")
    with pytest.raises(ValueError, match="--encoder fused needs --obs packed"):
        drv.run(api="tensor", obs="dense", encoder="fused")
    with pytest.raises(ValueError, match="encoder must be"):
        drv.run(encoder="hip")
