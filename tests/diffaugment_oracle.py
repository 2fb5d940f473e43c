"""Plain torch restatement of the differentiable augmentation (DESIGN.md "differentiable augmentation"), written from the formulas:
differentiable by autograd, any float dtype, CPU.  Shares no code with palette_and_histo_gan_amd/diffaugment.py.

Per image, with x (H, W, 4), a colour row (b, s, k), a geometry row (ty, tx, y0, x0) and a box ch x cw, in this order:
    colour       u = x[..., :3] + b;  v = (u - mean_c u) s + mean_c u;  y = (v - mean(v)) k + mean(v);  alpha untouched
    translation  out[r, c] = y[r - ty, c - tx] where that pixel exists, else fill (all four channels)
    cutout       out[r, c] = fill for y0 <= r < y0 + ch and x0 <= c < x0 + cw
"""
import numpy as np
import torch


def stages(policy):
    return {p.strip() for p in policy.split(",") if p.strip()}


def _kept(H, W, ty, tx, y0, x0, ch, cw, on):
    """(bool (H, W): output pixel is not a fill, source row per output row, source column per output column), python ints throughout"""
    ty, tx = (int(ty), int(tx)) if "translation" in on else (0, 0)
    rows, cols = np.arange(H, dtype=np.int64) - ty, np.arange(W, dtype=np.int64) - tx
    kept = ((rows >= 0) & (rows < H))[:, None] & ((cols >= 0) & (cols < W))[None, :]
    if "cutout" in on:
        r, c = np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64)
        box = ((r >= int(y0)) & (r < int(y0) + ch))[:, None] & ((c >= int(x0)) & (c < int(x0) + cw))[None, :]
        kept &= ~box
    return kept, np.clip(rows, 0, H - 1), np.clip(cols, 0, W - 1)


def diff_augment(x, color, geometry, ch, cw, policy, fill=-1.0):
    """x: torch (B, H, W, 4) of the dtype to evaluate in; color (B, 3) / geometry (B, 4): arrays or tensors"""
    on = stages(policy)
    color = torch.as_tensor(np.asarray(color, dtype=np.float64)).to(x.dtype)          # f32 table values are exact in either dtype
    geometry = np.asarray(geometry, dtype=np.int64)
    B, H, W, _ = x.shape
    out = []
    for i in range(B):
        img = x[i]
        if "color" in on:
            b, s, k = color[i]
            u = img[..., :3] + b
            sbar = u.mean(dim=-1, keepdim=True)
            v = (u - sbar) * s + sbar
            m = v.mean()
            img = torch.cat([(v - m) * k + m, img[..., 3:]], dim=-1)
        kept, rows, cols = _kept(H, W, *geometry[i], ch, cw, on)
        moved = img[torch.as_tensor(rows)][:, torch.as_tensor(cols)]
        out.append(torch.where(torch.as_tensor(kept)[..., None], moved, torch.full_like(moved, fill)))
    return torch.stack(out)


def vjp_closed_form(g, color, geometry, ch, cw, policy):
    """the VJP as the design states it: g' = g carried back to the source positions (0 where the output was a fill), Gamma its sum over
    pixels and colour channels, M = 3 H W;  dv = k g' + (1 - k) Gamma / M;  dx_c = s dv_c + (1 - s) / 3 sum_c' dv_c';  dx_3 = g'_3"""
    on = stages(policy)
    color = torch.as_tensor(np.asarray(color, dtype=np.float64)).to(g.dtype)
    geometry = np.asarray(geometry, dtype=np.int64)
    B, H, W, _ = g.shape
    out = []
    for i in range(B):
        kept, rows, cols = _kept(H, W, *geometry[i], ch, cw, on)
        gp = torch.zeros_like(g[i])
        rr, cc = np.nonzero(kept)
        gp[torch.as_tensor(rows[rr]), torch.as_tensor(cols[cc])] = g[i][torch.as_tensor(rr), torch.as_tensor(cc)]
        if "color" in on:
            _, s, k = color[i]
            dv = k * gp[..., :3] + (1 - k) * gp[..., :3].sum() / (3 * H * W)
            gp = torch.cat([s * dv + (1 - s) / 3 * dv.sum(dim=-1, keepdim=True), gp[..., 3:]], dim=-1)
        out.append(gp)
    return torch.stack(out)


def evaluate(x, g, color, geometry, ch, cw, policy, dtype, fill=-1.0):
    """(out, d<out, g>/dx) as float64 numpy arrays, evaluated in `dtype`"""
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    out = diff_augment(xt, color, geometry, ch, cw, policy, fill)
    (out * torch.tensor(np.asarray(g), dtype=dtype)).sum().backward()
    return out.detach().numpy().astype(np.float64), xt.grad.numpy().astype(np.float64)
