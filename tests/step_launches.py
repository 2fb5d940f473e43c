"""Launch harvest and float64 references for tests/test_step_launches_gpu.py.

The host half (the references) needs no GPU: tests/test_step_launches_cpu.py checks it against oracle/reference_graph.py.

Convolutions are written in the tap form of include/p2pgan.h:
  op G: lo[n,y,x,d]  = sum_{kh,kw,g} hi[n, s*y+kh-1, s*x+kw-1, g] W[kh,kw,g,d]
  op P: hi[n,Y,X,g] += lo[n,y,x,d] W[kh,kw,g,d]      at Y = s*y+kh-1, X = s*x+kw-1
  op W: dW[kh,kw,g,d] = sum_{n,y,x} hi[n, s*y+kh-1, s*x+kw-1, g] lo[n,y,x,d]
with a zero border of 1 pixel before and 2 after (TF SAME for k=4: (1,1) at stride 2, (1,2) at stride 1).
"""
import math

import numpy as np
import torch

F64 = torch.float64
CHUNK = 16          # images per im2col chunk of the whole-batch weight gradient


def _padded(hi):
    """hi [n,H,W,g] (f64 tensor) -> zero border 1 before / 2 after"""
    return torch.nn.functional.pad(hi, (0, 0, 1, 2, 1, 2))


def conv_g(hi, w, stride):
    """op G in float64: hi [n, s*LH, s*LW, Cg], w [4,4,Cg,Cd] -> [n, LH, LW, Cd]"""
    hi, w = torch.as_tensor(hi, dtype=F64), torch.as_tensor(w, dtype=F64)
    n, H, W_, _ = hi.shape
    lh, lw = H // stride, W_ // stride
    hp = _padded(hi)
    out = torch.zeros((n, lh, lw, w.shape[3]), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            out += hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :] @ w[kh, kw]
    return out.numpy()


def conv_p(lo, w, stride):
    """op P in float64: lo [n, LH, LW, Cd], w [4,4,Cg,Cd] -> [n, s*LH, s*LW, Cg]"""
    lo, w = torch.as_tensor(lo, dtype=F64), torch.as_tensor(w, dtype=F64)
    n, lh, lw, _ = lo.shape
    hp = torch.zeros((n, stride * lh + 3, stride * lw + 3, w.shape[2]), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :] += lo @ w[kh, kw].T
    return hp[:, 1:1 + stride * lh, 1:1 + stride * lw, :].numpy()


def conv_w(hi, lo, stride):
    """op W in float64 over the whole batch, CHUNK images at a time (im2col of one tap x f64 GEMM):
    hi [n, s*LH, s*LW, Cg], lo [n, LH, LW, Cd] -> dW [4,4,Cg,Cd]"""
    n, lh, lw, cd = lo.shape
    cg = hi.shape[3]
    dw = torch.zeros((4, 4, cg, cd), dtype=F64)
    for a in range(0, n, CHUNK):
        hp = _padded(torch.as_tensor(hi[a:a + CHUNK], dtype=F64))
        lo_c = torch.as_tensor(lo[a:a + CHUNK], dtype=F64).reshape(-1, cd)
        for kh in range(4):
            for kw in range(4):
                cols = hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :].reshape(-1, cg)
                dw[kh, kw] += cols.T @ lo_c
    return dw.numpy()


def act(x, kind, alpha):
    """kind 0 none, 1 LeakyReLU(alpha), 2 ReLU (p2p_act)"""
    if kind == 1:
        return np.where(x > 0, x, alpha * x)
    if kind == 2:
        return np.maximum(x, 0.0)
    return x


def norm_act(x, gamma, beta, eps, kind, alpha, mask=None):
    """y = act(drop(gamma * (x - mean) / sqrt(var + eps) + beta)) per (image, channel); x [n,H,W,C] (f64); gamma/beta may be None
    (no normalisation); mask 0/1 keeps and scales by 2 (keras Dropout(0.5))"""
    x = np.asarray(x, np.float64)
    if gamma is not None:
        mu = x.mean(axis=(1, 2), keepdims=True)
        var = ((x - mu) ** 2).mean(axis=(1, 2), keepdims=True)
        x = (x - mu) / np.sqrt(var + eps) * gamma + beta
    if mask is not None:
        x = x * mask * 2.0
    return act(x, kind, alpha)


def pooled_moments(sp, cnt):
    """slot partials [n, slots, C, 2] = (mean, centred sum of squares) of cnt pixels each -> per (image, channel) mean and variance
    (parallel-variance rule)"""
    sp = np.asarray(sp, np.float64)
    mean = sp[..., 0].mean(axis=1)
    m2 = sp[..., 1].sum(axis=1) + cnt * ((sp[..., 0] - mean[:, None, :]) ** 2).sum(axis=1)
    return mean, m2 / (cnt * sp.shape[1])


def image_set(n, seed=0, extra=4):
    """Images whose per-image outputs are compared in full: the first and last, both sides of every power-of-two boundary from
    either end (tile / workgroup groupings of 1, 2, 4 ... images, and tiles of 256 rows that span 256 / (H*W) images), and a few
    seeded random ones."""
    s = {0, n - 1}
    t = 1
    while t < n:
        s.update({t - 1, t, n - 1 - t, n - t})
        t *= 2
    rng = np.random.default_rng(seed)
    s.update(int(i) for i in rng.integers(0, n, size=extra))
    return sorted(i for i in s if 0 <= i < n)


def per_image_err(got, ref):
    """max over images of max|got - ref| / max|ref| within the image"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    axes = tuple(range(1, got.ndim))
    return float((np.abs(got - ref).max(axis=axes) / (np.abs(ref).max(axis=axes) + 1e-30)).max())


def per_image_channel_err(got, ref, scale=None):
    """max over (image, channel) of max|got - ref| / max|scale| within the (image, channel) plane, [n,H,W,C].  scale defaults to
    ref; a normalised output passes the value in front of its activation and dropout (a plane that ReLU and dropout leave nearly
    empty is measured against what the kernel computed, not against its few surviving small values)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref if scale is None else np.asarray(scale, np.float64))
    return float((np.abs(got - ref).max(axis=(1, 2)) / (scale.max(axis=(1, 2)) + 1e-30)).max())


def moment_err(mean, var, x, eps=0.0):
    """per (image, channel) moments [n, C] against those of x [n,H,W,C] in float64: max of |mean error| / standard deviation and
    |variance error| / (variance + eps) / 5"""
    x = np.asarray(x, np.float64)
    m, v = x.mean(axis=(1, 2)), x.var(axis=(1, 2))
    e_mean = np.abs(np.asarray(mean, np.float64) - m) / np.sqrt(v + eps)
    e_var = np.abs(np.asarray(var, np.float64) - v) / (v + eps) / 5
    return float(max(e_mean.max(), e_var.max()))


def per_tap_err(got, ref):
    """weight gradient [4,4,Cg,Cd]: max over taps of max|got - ref| / max|ref| within the tap"""
    got, ref = np.asarray(got, np.float64).reshape(16, -1), np.asarray(ref, np.float64).reshape(16, -1)
    return float((np.abs(got - ref).max(axis=1) / (np.abs(ref).max(axis=1) + 1e-30)).max())


# ---------------------------------------------------------------------------------------------------------------- step plumbing
def keras_adam(p, g, m, v, t, lr, b1, b2, eps):
    """one Keras (OptimizerV2) Adam step in float64, t = iteration count after the increment (pix2pix_model.py:28-29): returns
    (p, m, v).  eps is added to sqrt(v) outside the bias correction, which lives in the step size lr_t.  The arrays are float64
    numpy arrays or torch tensors (the GPU test evaluates the whole flat buffers on the device)."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return p - lr_t * m / (v ** 0.5 + eps), m, v


def bf16_round(x):
    """float32 values rounded to the nearest bfloat16, ties to even (what the kernels' from_f32 and torch's cast do), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


_M64 = (1 << 64) - 1


def dropout_mask(n, seed, counter, group0=0):
    """the keep mask of p2p_dropout_mask(_dev) (optim.hip dropout_mask_kernel): element 8*i+k is bit 8*k+3 of
    z = splitmix64(seed * 0x9E3779B97F4A7C15 + counter * 0xD1B54A32D192ED03 + (i + group0)), with the generator's increment
    0x9E3779B97F4A7C15 added before the finaliser; counter = counter_dev * 16 + salt for the device form.  uint8 [n]."""
    base = (int(seed) * 0x9E3779B97F4A7C15 + int(counter) * 0xD1B54A32D192ED03 + int(group0) + 0x9E3779B97F4A7C15) & _M64
    with np.errstate(over="ignore"):
        z = np.uint64(base) + np.arange((n + 7) // 8, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    bits = (z[:, None] >> (np.arange(8, dtype=np.uint64) * np.uint64(8) + np.uint64(3))) & np.uint64(1)
    return bits.reshape(-1)[:n].astype(np.uint8)
