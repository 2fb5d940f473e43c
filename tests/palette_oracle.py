"""Helper of tests/test_palette_*.py: the palette definitions of DESIGN.md "palette loss" restated in torch (float64 by default, any
dtype: in float32 on the CPU it is the yardstick the kernels' deviations are measured against), the closed-form VJP, the palette
extraction with numpy, and the inputs the forward/backward tests share."""
import numpy as np
import torch

K_MAX = 256


def soft_palette(img, palette, sizes, tau, dtype=torch.float64):
    """img (B,H,W,4) tensor in [-1,1] (autograd flows through it), palette (B,K,4) ints 0..255, sizes (B,) ints or None ->
    (hist (B,K), conformance (B,)) in `dtype`.  Every operation is done in `dtype`, written as the definitions read."""
    img = torch.as_tensor(img)
    palette = torch.as_tensor(np.asarray(palette))
    B, K = int(palette.shape[0]), int(palette.shape[1])
    sizes = [K] * B if sizes is None else [int(s) for s in sizes]
    x = img.to(dtype) * 0.5 + 0.5
    c = palette.to(dtype) / 255
    hist, conf = [], []
    for b in range(B):
        n = min(sizes[b], K)
        if n <= 0:
            hist.append(torch.zeros(K, dtype=dtype) + 0 * x[b].sum())
            conf.append(0 * x[b].sum())
            continue
        d = ((x[b].reshape(-1, 1, 4) - c[b, :n].reshape(1, n, 4)) ** 2).sum(-1)          # (HW, n)
        e = torch.exp(-(d - d.min(dim=1, keepdim=True).values) / tau)
        w = e / e.sum(dim=1, keepdim=True)
        hist.append(torch.cat([w.mean(0), torch.zeros(K - n, dtype=dtype)]))
        conf.append((w * d).sum(1).mean())
    return torch.stack(hist), torch.stack(conf)


def closed_form_vjp(img, palette, sizes, tau, gh, gm, dtype=torch.float64):
    """dL/dimg for upstream gradients gh (B,K), gm (B,), by the closed form:
    a_k = (gh_k + gm d_pk) / HW, abar = sum_k w_pk a_k,
    dL/dx_p = (2/tau) sum_k w_pk (a_k - abar) c_k + (2 gm / HW) (x_p - sum_k w_pk c_k),  dL/dimg = 0.5 dL/dx."""
    img = torch.as_tensor(img).detach()
    palette = torch.as_tensor(np.asarray(palette))
    B, H, W, _ = img.shape
    K = int(palette.shape[1])
    sizes = [K] * B if sizes is None else [int(s) for s in sizes]
    x = img.to(dtype) * 0.5 + 0.5
    c = palette.to(dtype) / 255
    gh, gm = torch.as_tensor(gh).to(dtype), torch.as_tensor(gm).to(dtype)
    out = torch.zeros((B, H * W, 4), dtype=dtype)
    for b in range(B):
        n = min(sizes[b], K)
        if n <= 0:
            continue
        xb, cb = x[b].reshape(-1, 4), c[b, :n]
        d = ((xb[:, None, :] - cb[None, :, :]) ** 2).sum(-1)
        e = torch.exp(-(d - d.min(dim=1, keepdim=True).values) / tau)
        w = e / e.sum(dim=1, keepdim=True)
        a = (gh[b, :n][None, :] + gm[b] * d) / (H * W)
        abar = (w * a).sum(1, keepdim=True)
        gx = (2 / tau) * ((w * (a - abar)) @ cb) + (2 * gm[b] / (H * W)) * (xb - w @ cb)
        out[b] = 0.5 * gx
    return out.reshape(B, H, W, 4)


def palette_histogram_loss(h_true, h_pred):
    return 0.5 * (h_pred - h_true).abs().sum(-1).mean()


def extract_palette(images, cap=K_MAX):
    """numpy (B,H,W,4) float32 in [-1,1] -> (palette int32 (B,cap,4), sizes int32 (B,)): q = clamp(floor((img*0.5+0.5)*255+0.5), 0,
    255) with every step in float32, the distinct keys r + 256 g + 65536 b + 2^24 a in ascending order; more than `cap`: -1, zeros."""
    img = np.asarray(images, np.float32)
    f = np.float32
    q = np.clip(np.floor((img * f(0.5) + f(0.5)) * f(255) + f(0.5)), 0, 255).astype(np.uint32)
    keys = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)
    B = img.shape[0]
    pal, sizes = np.zeros((B, cap, 4), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        u = np.unique(keys[b])
        if len(u) > cap:
            sizes[b] = -1
            continue
        sizes[b] = len(u)
        pal[b, :len(u)] = np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255, u >> 24], axis=1).astype(np.int32)
    return pal, sizes


def noisy_palette_case(seed, B, H, W, K, sizes):
    """Inputs of the forward/backward tests: random RGBA palettes (B,K,4), images whose pixels are colours of their image's valid
    slots, half of them with N(0, 0.05) noise added, clipped to [-1,1]; random upstream gradients.  An image with sizes[b] <= 0 draws
    from all K slots (its palette is ignored)."""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, size=(B, K, 4)).astype(np.int32)
    img = np.zeros((B, H, W, 4), np.float32)
    for b in range(B):
        n = sizes[b] if sizes[b] > 0 else K
        idx = rng.integers(0, n, size=(H, W))
        img[b] = pal[b][idx].astype(np.float32) / 127.5 - 1.0
    noisy = rng.random((B, H, W, 1)) < 0.5
    img = np.clip(img + noisy * rng.normal(0.0, 0.05, size=img.shape), -1.0, 1.0).astype(np.float32)
    gh = rng.normal(size=(B, K)).astype(np.float32)
    gm = rng.normal(size=(B,)).astype(np.float32)
    return img, pal, np.asarray(sizes, np.int32), gh, gm


def evaluate(img, pal, sizes, tau, gh, gm, dtype):
    """(hist, conf, dimg) of the restatement in `dtype` on the CPU under autograd, as float64 numpy"""
    x = torch.tensor(img).to(dtype).requires_grad_(True)          # f32 -> f64 is exact
    h, m = soft_palette(x, pal, sizes, tau, dtype)
    ((h * torch.tensor(gh).to(dtype)).sum() + (m * torch.tensor(gm).to(dtype)).sum()).backward()
    return h.detach().double().numpy(), m.detach().double().numpy(), x.grad.double().numpy()
