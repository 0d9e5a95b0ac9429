"""The numpy statement of the fused first encoder stage on packed obs words (the contract of
include/microrts_amd.h's mrts_obs_conv_forward / mrts_obs_conv_backward): what test_obs_conv.py
holds against torch on the CPU and test_gpu_obs_conv.py holds the kernels against.

    conv_ref  the convolution, every add one float32 round-to-nearest add in the stated order
    pool_ref  the 3x3 / stride 2 / padding 1 first maximum (strict >) and the ReLU
    grad_ref  the parameter gradients in float64 from the float32 forward's argmax and m > 0,
              with each element's term count K and S = sum |g|
    words     a word generator: one set bit per plane group, about 12 % occupied cells
"""
import os

import numpy as np

from conftest import REPO

GROUPS = (5, 5, 3, 8, 6, 2)   # hp, resources, owner, unit type, action, terrain (+ 2: visibility, with partial obs)
EMPTY = 1 | 1 << 5 | 1 << 10 | 1 << 13 | 1 << 21 | 1 << 27
U = 2.0 ** -24                # float32 unit roundoff


def gamma(k):
    """gamma_k = k u / (1 - k u): the relative error bound of k float32 roundings."""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1 - k * U)


def sota_first_layer():
    """The reference agent's first conv layer: weight [32, 29, 3, 3], bias [32], float32."""
    with np.load(os.path.join(REPO, "tests", "golden", "agent_sota_policy.npz")) as z:
        return np.ascontiguousarray(z["encoder.1.weight"], dtype=np.float32), np.ascontiguousarray(z["encoder.1.bias"], dtype=np.float32)


def words(rng, shape, P, occupied=0.12):
    """int32 `shape` of obs words: empty cells, and about `occupied` of them with one random
    bit per plane group."""
    groups = GROUPS + ((2,) if P == 31 else ())
    w = np.zeros(shape, np.uint32)
    lo = 0
    for g in groups:
        w |= np.uint32(1) << (lo + rng.integers(0, g, shape)).astype(np.uint32)
        lo += g
    empty = np.uint32(EMPTY | (1 << 29 if P == 31 else 0))
    return np.where(rng.random(shape) < occupied, w, empty).astype(np.uint32).view(np.int32)


def _shifted(a, ky, kx, fill=0):
    """b[..., y, x] = a[..., y + ky - 1, x + kx - 1], `fill` outside."""
    H, W = a.shape[-2:]
    b = np.full_like(a, fill)
    ys, yd = (slice(max(ky - 1, 0), H + min(ky - 1, 0)), slice(max(1 - ky, 0), H + min(1 - ky, 0)))
    xs, xd = (slice(max(kx - 1, 0), W + min(kx - 1, 0)), slice(max(1 - kx, 0), W + min(1 - kx, 0)))
    b[..., yd, xd] = a[..., ys, xs]
    return b


def conv_ref(packed, weight, bias):
    """packed [N, H, W] int32, weight [C, P, 3, 3] float32, bias [C] float32 -> conv [N, C, H, W]
    float32: acc = bias; per tap in row-major order, skipped when the neighbour is outside
    the map or its word (masked to P bits) is zero, t = the selected weights summed in
    ascending plane order from the first one, acc = acc + t.  float32 throughout."""
    weight, bias = np.asarray(weight, np.float32), np.asarray(bias, np.float32)
    C, P = weight.shape[:2]
    w = np.ascontiguousarray(packed).view(np.uint32) & np.uint32((1 << P) - 1)
    N, H, W = w.shape
    acc = np.broadcast_to(bias[None, :, None, None], (N, C, H, W)).astype(np.float32)
    for ky in range(3):
        for kx in range(3):
            nb = _shifted(w, ky, kx)                     # zero outside the map: skipped like a zero word
            t = np.zeros((N, C, H, W), np.float32)
            started = np.zeros((N, 1, H, W), bool)
            for p in range(P):
                bit = ((nb >> np.uint32(p)) & np.uint32(1)).astype(bool)[:, None]
                wt = weight[None, :, p, ky, kx, None, None]
                t = np.where(bit, np.where(started, t + wt, wt), t).astype(np.float32)
                started = started | bit
            acc = np.where(started, acc + t, acc).astype(np.float32)
    return acc


def pool_ref(conv):
    """conv [N, C, H, W] float32 -> (out, m, arg): the first maximum m (strict >) over rows
    2 i - 1 .. 2 i + 1 and columns 2 j - 1 .. 2 j + 1 in row-major order, positions outside
    the map left out; arg = y * W + x of it; out = m where m > 0, else +0.0."""
    N, C, H, W = conv.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    m = np.full((N, C, Ho, Wo), -np.inf, np.float32)
    arg = np.full((N, C, Ho, Wo), -1, np.int64)
    ii, jj = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    for dy in range(3):
        for dx in range(3):
            y, x = 2 * ii - 1 + dy, 2 * jj - 1 + dx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            v = conv[:, :, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
            better = ok[None, None] & (v > m)
            m = np.where(better, v, m)
            arg = np.where(better, (y * W + x)[None, None], arg)
    assert (arg >= 0).all()
    out = np.where(m > 0, m, np.float32(0.0)).astype(np.float32)
    return out, m, arg


def grad_ref(packed, P, m, arg, grad_out):
    """The gradients in float64 from the float32 forward's (m, arg) of pool_ref: for every
    output with m > 0, g = grad_out's element goes to grad_bias[c] and to
    grad_weight[c, p, ky, kx] for every tap of the argmax position whose neighbour is
    inside the map and has bit p set.  Returns (gw, gb, Kw, Kb, Sw, Sb): the gradients, the
    number of terms of each element and the sum of the terms' magnitudes."""
    w = np.ascontiguousarray(packed).view(np.uint32) & np.uint32((1 << P) - 1)
    N, H, W = w.shape
    C = m.shape[1]
    on = m > 0
    g = np.where(on, np.asarray(grad_out, np.float64), 0.0)
    n_i, c_i = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    at = (np.broadcast_to(n_i[:, :, None, None], arg.shape), np.broadcast_to(c_i[:, :, None, None], arg.shape), arg)
    G, A, K = (np.zeros((N, C, H * W), np.float64) for _ in range(3))
    np.add.at(G, at, g)
    np.add.at(A, at, np.abs(g))
    np.add.at(K, at, on.astype(np.float64))
    G, A, K = (a.reshape(N, C, H, W) for a in (G, A, K))
    gw, Sw, Kw = (np.zeros((C, P, 3, 3), np.float64) for _ in range(3))
    for ky in range(3):
        for kx in range(3):
            nb = _shifted(w, ky, kx)
            bits = ((nb[..., None] >> np.arange(P, dtype=np.uint32)) & np.uint32(1)).astype(np.float64)   # [N, H, W, P]
            for dst, src in ((gw, G), (Sw, A), (Kw, K)):
                dst[:, :, ky, kx] = np.einsum("nchw,nhwp->cp", src, bits)
    return gw, G.sum((0, 2, 3)), np.rint(Kw).astype(np.int64), np.rint(K.sum((0, 2, 3))).astype(np.int64), Sw, A.sum((0, 2, 3))
