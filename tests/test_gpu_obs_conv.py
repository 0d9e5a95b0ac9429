"""The fused first encoder stage on packed obs on the MI355X (csrc/mrts_conv.hip through
gym_microrts.obs_conv): the forward element for element against the numpy statement of the
contract (obs_conv_ref.py) and, independently of it, within the float32 error bound of float64
torch on the CPU; the backward within the summation bound of the float64 gradients, exact
zeros, the same bits twice; autograd; and the driver's --encoder fused.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from obs_conv_ref import conv_ref, gamma, grad_ref, pool_ref, sota_first_layer, words
from test_obs_conv import torch_stage64

pytestmark = pytest.mark.gpu

RW = np.array([10.0, 1.0, 1.0, 0.2, 1.0, 4.0])
M16 = "maps/16x16/basesWorkers16x16.xml"
#        N  H   W   P   C
CASES = [(3, 1, 1, 29, 32),
         (2, 2, 3, 29, 5),
         (4, 8, 8, 29, 32),
         (3, 9, 13, 31, 32),
         (2, 16, 16, 29, 32),    # the sota weights; words from a packed engine after 60 ticks
         (2, 24, 24, 31, 64),
         (1, 47, 24, 29, 32),
         (2, 8, 8, 29, 32)]      # zero words, all-ones words, bits at or above P
IDS = ["x".join(str(v) for v in c) for c in CASES[:-1]] + ["2x8x8x29x32_odd_words"]
ODD = len(CASES) - 1


def _torch():
    import torch

    return torch


def engine_words(ticks=60):
    """[2, 16, 16] words of a packed engine's two selfplay envs after `ticks` of random play."""
    torch = _torch()
    from gym_microrts.envs.vec_env import MicroRTSGridModeVecEnv
    from oracle_py import sample_actions

    g = MicroRTSGridModeVecEnv(num_selfplay_envs=2, num_bot_envs=0, max_steps=2000, ai2s=[], map_paths=[M16], reward_weight=RW,
                               return_tensors=True, obs_format="packed")
    pk = g.reset()
    for s in range(ticks):
        a = torch.from_numpy(sample_actions(g.get_action_mask().cpu().numpy(), 31, s)).to(g.device)
        pk = g.step(a)[0]
    out = pk.cpu().numpy().copy()
    g.close()
    assert out.shape == (2, 16, 16) and out.dtype == np.int32 and len(np.unique(out)) > 4
    return out


@functools.lru_cache(maxsize=None)
def case(k):
    """A case's inputs and its references, computed once: the statement's forward (conv, out,
    m, arg), float64 torch's forward with its bound, a N(0, 1) grad_out and the float64
    gradients with their term counts and magnitudes."""
    N, H, W, P, C = CASES[k]
    rng = np.random.default_rng(1000 + k)
    if (H, W, C, P) == (16, 16, 32, 29):
        weight, bias = sota_first_layer()
        packed = engine_words()
    else:
        weight = rng.normal(0, 0.1, (C, P, 3, 3)).astype(np.float32)
        bias = rng.normal(0, 0.1, (C,)).astype(np.float32)
        packed = words(rng, (N, H, W), P)
    if k == ODD:
        u = packed.view(np.uint32).copy()
        u[0, 0, 0] = u[0, 3, 2:6] = u[1, 7, 7] = 0                 # zero words: a corner, a run, the last cell
        u[0, 5, 5] = u[1, 0, 7] = 0xFFFFFFFF                       # all-ones
        u[1, 2, 1:4] |= np.uint32(0xE0000000)                      # bits at or above P
        u[0, 7, 0] = 0x80000000                                    # only a bit above P: a zero word to every reader
        packed = u.view(np.int32)
    conv = conv_ref(packed, weight, bias)
    out, m, arg = pool_ref(conv)
    gout = rng.standard_normal(out.shape).astype(np.float32)
    t64 = torch_stage64(packed, P, weight, bias)
    grads = grad_ref(packed, P, m, arg, gout)
    return dict(packed=packed, weight=weight, bias=bias, conv=conv, out=out, m=m, arg=arg, gout=gout, t_out=t64[3], t_pbound=t64[4],
                grads=grads, P=P)


def dev(*arrays):
    torch = _torch()
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def raw_backward(packed, weight, bias, gout, fill=float("nan")):
    """The C ABI's backward into gradients pre-filled with `fill` (it overwrites)."""
    torch = _torch()
    from gym_microrts import _native

    L = _native.lib()
    n, h, w = packed.shape
    c, planes = weight.shape[:2]
    nbytes = L.mrts_obs_conv_workspace_bytes(n, h, w, planes, c)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
    gw, gb = torch.full_like(weight, fill), torch.full_like(bias, fill)
    rc = L.mrts_obs_conv_backward(torch.cuda.current_stream().cuda_stream, packed.data_ptr(), n, h, w, planes, weight.data_ptr(),
                                  bias.data_ptr(), c, gout.data_ptr(), ws.data_ptr(), nbytes, gw.data_ptr(), gb.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return gw.cpu().numpy(), gb.cpu().numpy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_forward(k):
    """encode == pool_ref(conv_ref(...)) as float32 values element for element with no stored
    -0.0, and within the float32 bound (gamma_64 * (|bias| + sum |selected weights|), its
    maximum over each pool window; the odd-words case: gamma_262, an all-ones word's term
    count) of float64 torch's conv2d -> max_pool2d -> relu on the CPU from unpack_obs_ref."""
    torch = _torch()
    from gym_microrts import obs_conv

    d = case(k)
    N, H, W, P, C = CASES[k]
    packed, weight, bias = dev(d["packed"], d["weight"], d["bias"])
    with torch.no_grad():
        got = obs_conv.encode(packed, weight, bias)
    assert got.shape == (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu().numpy()
    share = float((d["m"] > 0).mean())
    err = np.abs(got - d["t_out"])
    print(f"{IDS[k]}: share m > 0 {share:.3f}, max |gpu - float64 torch| {err.max():.3e}, max bound {d['t_pbound'].max():.3e}, "
          f"mismatches against the statement {(got != d['out']).sum()}")
    np.testing.assert_array_equal(got, d["out"])
    assert not np.signbit(got[got == 0]).any(), "a stored -0.0"
    scale = gamma(1 + 9 * 29) / gamma(64) if k == ODD else 1.0
    assert (err <= d["t_pbound"] * scale).all()
    if k == ODD:   # bits at or above P are ignored: the same words masked to P bits
        masked = (d["packed"].view(np.uint32) & np.uint32((1 << P) - 1)).view(np.int32)
        with torch.no_grad():
            again = obs_conv.encode(dev(masked)[0], weight, bias)
        np.testing.assert_array_equal(again.cpu().numpy(), got)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_backward(k):
    """With a N(0, 1) grad_out: every grad_weight / grad_bias element within gamma_{K-1} * S of
    grad_ref (K terms of magnitudes summing to S: the bound of any summation order, 0 for a
    single term), elements with no term exactly +0.0, and a second call gives the same bits."""
    d = case(k)
    packed, weight, bias, gout = dev(d["packed"], d["weight"], d["bias"], d["gout"])
    gw, gb = raw_backward(packed, weight, bias, gout)
    r_gw, r_gb, Kw, Kb, Sw, Sb = d["grads"]
    for name, got, ref, K, S in (("grad_weight", gw, r_gw, Kw, Sw), ("grad_bias", gb, r_gb, Kb, Sb)):
        assert np.isfinite(got).all(), name
        # the float32 result of K terms in any order: gamma_{K-1} * S off the exact sum, which grad_ref's float64 is to 2^-53 * K * S
        bound = gamma(np.maximum(K - 1, 0)) * S
        err = np.abs(got.astype(np.float64) - ref)
        slack = 2.0 ** -52 * K * S
        print(f"{IDS[k]} {name}: max K {K.max()}, elements with K = 0: {(K == 0).sum()}, worst err / bound "
              f"{np.max(err[K > 1] / bound[K > 1]) if (K > 1).any() else 0.0:.3f}")
        assert (err <= bound + slack).all(), name
        zero = got[K == 0]
        assert (zero == 0).all() and not np.signbit(zero).any(), f"{name}: an element without a term is not +0.0"
        one = K == 1
        np.testing.assert_array_equal(got[one], ref[one].astype(np.float32), err_msg=f"{name}: a single term is exact")
    gw2, gb2 = raw_backward(packed, weight, bias, gout, fill=7.0)
    assert gw.tobytes() == gw2.tobytes() and gb.tobytes() == gb2.tobytes()


@pytest.mark.timeout(120)
def test_autograd():
    """encode(...).backward(g) fills .grad on both parameters with the raw backward's values;
    with one parameter frozen only the other gets a gradient; under no_grad or with both
    frozen the result carries no graph; leading dimensions fold into the batch; a
    non-default current stream is honoured; an empty batch works."""
    torch = _torch()
    from gym_microrts import obs_conv

    k = 3   # 3 x 9 x 13, P = 31
    d = case(k)
    packed, weight, bias, gout = dev(d["packed"], d["weight"], d["bias"], d["gout"])
    want_w, want_b = raw_backward(packed, weight, bias, gout)
    w, b = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    out = obs_conv.encode(packed, w, b)
    assert out.requires_grad
    out.backward(gout)
    assert w.grad.cpu().numpy().tobytes() == want_w.tobytes() and b.grad.cpu().numpy().tobytes() == want_b.tobytes()
    w2, b2 = weight.clone().requires_grad_(True), bias.clone()
    obs_conv.encode(packed, w2, b2).backward(gout)
    assert b2.grad is None and w2.grad.cpu().numpy().tobytes() == want_w.tobytes()
    w3, b3 = weight.clone(), bias.clone().requires_grad_(True)
    obs_conv.encode(packed, w3, b3).backward(gout)
    assert w3.grad is None and b3.grad.cpu().numpy().tobytes() == want_b.tobytes()
    with torch.no_grad():
        assert not obs_conv.encode(packed, w, b).requires_grad
    assert not obs_conv.encode(packed, weight, bias).requires_grad
    # a second stage on top: the gradient reaches the parameters through the graph
    w4, b4 = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    (obs_conv.encode(packed, w4, b4) * gout).sum().backward()
    assert w4.grad.cpu().numpy().tobytes() == want_w.tobytes() and b4.grad.cpu().numpy().tobytes() == want_b.tobytes()
    # leading dimensions
    two = torch.stack([packed, packed]).contiguous()
    with torch.no_grad():
        o2 = obs_conv.encode(two, weight, bias)
    assert o2.shape == (2,) + tuple(out.shape) and torch.equal(o2[0], out.detach()) and torch.equal(o2[1], out.detach())
    # a non-default stream: the work is ordered after what that stream did before
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        late = torch.empty_like(packed)
        late.copy_(packed, non_blocking=True)
        ws, bs = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        os_ = obs_conv.encode(late, ws, bs)
        os_.backward(gout)
    s.synchronize()
    assert torch.equal(os_.detach(), out.detach()) and ws.grad.cpu().numpy().tobytes() == want_w.tobytes()
    # no rows
    we, be = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    e = obs_conv.encode(torch.empty((0, 9, 13), dtype=torch.int32, device="cuda"), we, be)
    assert e.shape == (0, 32, 5, 7)
    e.sum().backward()
    assert not bool(we.grad.any()) and not bool(be.grad.any())


@pytest.mark.timeout(120)
def test_gridnet_takes_the_words():
    """GridNet.forward on the packed words against its forward on the unpacked planes: the first
    stages differ by float32 rounding (test_forward holds each to its bound) and the later
    layers are the same torch modules, so logits and values agree to 1e-3; the state dict's
    names are what they were."""
    torch = _torch()
    from gym_microrts import packed_obs

    drv = _driver()
    torch.manual_seed(3)
    d = case(4)
    net = drv.GridNet(29, 16, 16).cuda()
    net.load_reference_state(drv.load_weights(drv.SOTA))
    packed = dev(d["packed"])[0]
    with torch.no_grad():
        lg_w, v_w = net(packed)
        lg_d, v_d = net(packed_obs.unpack_obs(packed, 29))
    assert lg_w.shape == lg_d.shape == (2 * 256, 78) and v_w.shape == v_d.shape
    assert torch.allclose(lg_w, lg_d, rtol=1e-3, atol=1e-3) and torch.allclose(v_w, v_d, rtol=1e-3, atol=1e-3)
    assert [k for k in net.state_dict()] == [k for k in drv.GridNet(29, 16, 16).state_dict()]


def _driver():
    spec = importlib.util.spec_from_file_location("ppo_gridnet_driver", os.path.join(REPO, "examples", "ppo_gridnet_driver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.timeout(120)
def test_driver_with_the_fused_encoder(monkeypatch):
    """One update of the driver with --encoder fused (fused head, packed masks, packed obs):
    finite losses, no engine error, stats["encoder"] == "fused", and packed_obs.unpack_obs is
    never called -- no forward of the rollout, the GAE or the update unpacks anything."""
    from gym_microrts import packed_obs

    calls = []
    real = packed_obs.unpack_obs

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(packed_obs, "unpack_obs", counting)
    drv = _driver()
    assert drv.packed_obs.unpack_obs is counting
    stats = drv.run(num_selfplay_envs=4, num_steps=4, updates=1, api="tensor", head="fused", masks="packed", obs="packed",
                    encoder="fused", log=lambda s: None)
    assert stats["finite"] and stats["engine_error_flags"] == 0 and stats["encoder"] == "fused"
    assert not calls
