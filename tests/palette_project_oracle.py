"""Helper of tests/test_palette_project_*.py: the palette projection of DESIGN.md "palette projection" restated in torch (float64 by
default, any dtype: in float32 on the CPU it is the yardstick the kernels' deviations are measured against; the forward runs
under autograd), the closed-form VJP, the hard forward on tests/palette_snap_oracle.py, and the inputs the tests share."""
import numpy as np
import torch

from tests import palette_oracle as PO
from tests import palette_snap_oracle as SO

# (B, H, W, K), sizes: a ragged last chunk of 1024 pixels (60, 231 and 256 pixels; 4096 gives four chunks), a full and a nearly
# empty palette, an invalid image in the middle of a batch
CASES = {"3x6x10x40": ((3, 6, 10, 40), [1, 37, 40]), "2x16x16x256": ((2, 16, 16, 256), [2, 256]),
         "2x64x64x40": ((2, 64, 64, 40), [40, 33]), "3x6x10x40-skip": ((3, 6, 10, 40), [37, -1, 40]),
         "1x33x7x256": ((1, 33, 7, 256), [256])}
TAUS = (1e-3, 5e-2)


def _sizes(sizes, B, K):
    return [K] * B if sizes is None else [min(max(int(s), 0), K) for s in sizes]


def weights(xb, cb, tau):
    """xb (P, 4), cb (n, 4) in one dtype -> w (P, n) = softmax_k(-(d - min_j d_j) / tau), written as the definition reads"""
    d = ((xb[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
    e = torch.exp(-(d - d.min(dim=1, keepdim=True).values) / tau)
    return e / e.sum(dim=1, keepdim=True)


def soft_project(img, palette, sizes, tau, dtype=torch.float64):
    """img (B,H,W,4) tensor in [-1,1] (autograd flows through it), palette (B,K,4) ints 0..255, sizes (B,) ints or None ->
    y (B,H,W,4) = 2 sum_k w_k c_k - 1 in `dtype`; an image without valid slots is returned as it is"""
    img = torch.as_tensor(img)
    palette = torch.as_tensor(np.asarray(palette))
    B, K = int(palette.shape[0]), int(palette.shape[1])
    x = img.to(dtype) * 0.5 + 0.5
    c = palette.to(dtype) / 255
    out = []
    for b, n in enumerate(_sizes(sizes, B, K)):
        if n == 0:
            out.append(img[b].to(dtype))
            continue
        w = weights(x[b].reshape(-1, 4), c[b, :n], tau)
        out.append((2 * (w @ c[b, :n]) - 1).reshape(img[b].shape))
    return torch.stack(out)


def closed_form_vjp(img, palette, sizes, tau, g, dtype=torch.float64):
    """dL/dimg = (2 / tau) Cov_w(c) g per pixel, Cov_w(c) = sum_k w_k c_k c_k^T - (sum_k w_k c_k)(sum_k w_k c_k)^T, as written
    (uncentred); g itself for an image without valid slots"""
    img = torch.as_tensor(img).detach()
    palette = torch.as_tensor(np.asarray(palette))
    B, K = int(palette.shape[0]), int(palette.shape[1])
    x = img.to(dtype) * 0.5 + 0.5
    c = palette.to(dtype) / 255
    g = torch.as_tensor(g).to(dtype)
    out = []
    for b, n in enumerate(_sizes(sizes, B, K)):
        if n == 0:
            out.append(g[b])
            continue
        cb = c[b, :n]
        w = weights(x[b].reshape(-1, 4), cb, tau)
        mean = w @ cb                                                                  # (P, 4)
        second = torch.einsum("pk,ki,kj->pij", w, cb, cb)
        cov = second - mean[:, :, None] * mean[:, None, :]
        out.append(((2 / tau) * torch.einsum("pij,pj->pi", cov, g[b].reshape(-1, 4))).reshape(img[b].shape))
    return torch.stack(out)


def hard_project(img, palette, sizes=None):
    """the snap's image (numpy float32): tests/palette_snap_oracle.snap, which passes an image without valid slots through"""
    return SO.snap(img, palette, sizes).image


def evaluate(img, pal, sizes, tau, g, dtype):
    """(y, dimg) of the restatement in `dtype` on the CPU, the VJP of g by autograd, as float64 numpy"""
    x = torch.tensor(img).to(dtype).requires_grad_(True)          # f32 -> f64 is exact
    y = soft_project(x, pal, sizes, tau, dtype)
    y.backward(torch.tensor(g).to(dtype))
    return y.detach().double().numpy(), x.grad.double().numpy()


_cases = {}


def case(name):
    """(img, pal, sizes, g) of a case, drawn once and shared (never modified): tests/palette_oracle.noisy_palette_case, then row 0
    of every image with at least two valid slots overwritten by the midpoint of its first and last valid colour (where the Jacobian
    is largest), and an upstream gradient g ~ N(0, 1)"""
    if name not in _cases:
        (B, H, W, K), sizes = CASES[name]
        img, pal, sz, _, _ = PO.noisy_palette_case(300 + len(name) + K, B, H, W, K, sizes)
        img = img.copy()
        for b, n in enumerate(_sizes(sizes, B, K)):
            if n >= 2:
                mid = (pal[b, 0].astype(np.float64) + pal[b, n - 1].astype(np.float64)) / 2
                img[b, 0] = (mid / 127.5 - 1.0).astype(np.float32)
        g = np.random.default_rng(17 + K + H).normal(size=img.shape).astype(np.float32)
        _cases[name] = (img, pal, sz, g)
    return _cases[name]


_refs = {}


def reference(name, tau):
    """(inputs, (y64, g64), yardstick (forward max abs, gradient of its max-norm)): the float64 restatement and the float32
    restatement's deviation from it, computed once, shared, never modified"""
    key = (name, tau)
    if key not in _refs:
        inputs = case(name)
        y64, g64 = evaluate(*inputs[:3], tau, inputs[3], torch.float64)
        y32, g32 = evaluate(*inputs[:3], tau, inputs[3], torch.float32)
        yard = (np.abs(y32 - y64).max(), np.abs(g32 - g64).max() / np.abs(g64).max())
        _refs[key] = (inputs, (y64, g64), yard)
    return _refs[key]
