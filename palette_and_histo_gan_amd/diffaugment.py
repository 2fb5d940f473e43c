"""Differentiable augmentation in front of the discriminator (build-added: DiffAugment, Zhao et al., NeurIPS 2020; DESIGN.md
"differentiable augmentation" holds the definitions).

The reference's only remedy for its 250 pairs is Pix2PixAugmentedModel, which augments the DATASET.  Here the same random colour
change, translation and cutout are applied to the real and to the generated image just before the discriminator sees them, and the
generator's gradient flows back through them:

    params = draw_parameters(batch, height, width, policy, seed, step)        # host side, stateless
    out = diff_augment(images, params, policy)                                # HIP forward, HIP VJP (csrc/diffaugment.hip)

`diff_augment` is one torch.autograd.Function, differentiable with respect to the images only, so it can stand between
`self.generator(...)` and `self.discriminator([...])` of a tf.GradientTape step (Pix2PixDiffAugmentModel).  The kernels launch on the
current stream; there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .configuration import SEED

POLICIES = ("color", "translation", "cutout")          # also the order in which the stages are applied
_ALL = ",".join(POLICIES)


def policy_bits(policy):
    """the kernels' bit set (1 colour, 2 translation, 4 cutout) of a comma-separated subset of POLICIES ("" is the identity)"""
    if not isinstance(policy, str):
        raise ValueError(f"policy is a comma-separated subset of {POLICIES}, got {policy!r}")
    bits = 0
    for name in (p.strip() for p in policy.split(",")):
        if name == "":
            continue
        if name not in POLICIES:
            raise ValueError(f"unknown augmentation {name!r} in policy {policy!r}: choose from {POLICIES}")
        bits |= 1 << POLICIES.index(name)
    return bits


class AugmentParameters:
    """One row per image: `color` f32 (B, 3) = brightness offset b, saturation factor s, contrast factor k; `geometry` int32 (B, 4) =
    translation ty, tx and the cutout box's corner y0, x0; `ch`, `cw` the box size.  Host or device tensors (or anything
    torch.as_tensor takes, of exactly these dtypes); a host table is uploaded once per device, without blocking, and kept."""

    def __init__(self, color, geometry, ch, cw):
        color, geometry = torch.as_tensor(color), torch.as_tensor(geometry)
        if color.dim() != 2 or color.shape[1] != 3 or color.dtype != torch.float32:
            raise ValueError(f"color: expected a float32 (B, 3) table, got {color.dtype} {tuple(color.shape)}")
        if geometry.dim() != 2 or geometry.shape[1] != 4 or geometry.dtype != torch.int32:
            raise ValueError(f"geometry: expected an int32 (B, 4) table, got {geometry.dtype} {tuple(geometry.shape)}")
        if color.shape[0] != geometry.shape[0]:
            raise ValueError(f"color has {color.shape[0]} rows, geometry {geometry.shape[0]}")
        if int(ch) != ch or int(cw) != cw or ch < 0 or cw < 0:
            raise ValueError(f"the cutout box is ch x cw non-negative integers, got {ch!r} x {cw!r}")
        self.color, self.geometry, self.ch, self.cw = color.detach(), geometry.detach(), int(ch), int(cw)
        self._on = {}

    @property
    def batch(self):
        return int(self.color.shape[0])

    def on(self, dev):
        """(color, geometry) as dense tensors on `dev`"""
        got = self._on.get(dev)
        if got is None:
            got = self._on[dev] = tuple(self._upload(t, dev) for t in (self.color, self.geometry))
        return got

    @staticmethod
    def _upload(t, dev):
        if t.device == dev:
            return t.contiguous()
        if t.device.type == "cpu":
            # a pageable source would make the copy wait for the stream.  The pinned temporary is dropped at once: torch's caching
            # host allocator keeps its block until the copy recorded on this stream has run, so this is safe as it stands
            t = t.contiguous().pin_memory()
        return t.to(dev, non_blocking=True)


def draw_parameters(batch, height, width, policy=_ALL, seed=SEED, step=0):
    """The parameter table of one step, on the host.  Stateless: it is drawn from np.random.default_rng([seed, step]) and so depends on
    (seed, step, batch, height, width) alone -- a run resumed at a step draws what the uninterrupted run drew.  Every column is drawn
    whatever the policy (which is only checked), so switching a stage off does not move the others' values.  Ranges of the paper:
    b ~ U[-0.5, 0.5), s ~ U[0, 2), k ~ U[0.5, 1.5); ty uniform in [-H//8, H//8], tx likewise; box ch x cw = H//2 x W//2 with its corner
    y0 uniform in [-(ch//2), H - ch + ch//2], x0 likewise (the box's centre is uniform over the image)."""
    policy_bits(policy)
    B, H, W = int(batch), int(height), int(width)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"expected a batch of at least one H x W image, got {batch} x {height} x {width}")
    rng = np.random.default_rng([int(seed), int(step)])
    u = rng.random((B, 3))
    color = np.stack([u[:, 0] - 0.5, u[:, 1] * 2.0, u[:, 2] + 0.5], axis=1).astype(np.float32)
    ch, cw = H // 2, W // 2
    geometry = np.stack([rng.integers(-(H // 8), H // 8 + 1, size=B), rng.integers(-(W // 8), W // 8 + 1, size=B),
                         rng.integers(-(ch // 2), H - ch + ch // 2 + 1, size=B), rng.integers(-(cw // 2), W - cw + cw // 2 + 1, size=B)],
                        axis=1).astype(np.int32)
    return AugmentParameters(torch.from_numpy(color), torch.from_numpy(geometry), ch, cw)


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _workspace(bits, B, H, W, dev):
    if not bits & 1:
        return None          # only the colour stage sums
    return torch.empty(max(int(L.lib().p2p_diffaug_workspace_bytes(B, H, W)) // 4, 1), dtype=torch.float32, device=dev)


class DiffAugment(torch.autograd.Function):
    """img: dense f32 (B, H, W, 4) device tensor; color f32 (B, 3), geometry int32 (B, 4): dense, on img's device.  Backward: the
    gradient with respect to img only (p2p_diffaug_bwd needs the tables, not the image); single backward."""

    @staticmethod
    def forward(ctx, img, color, geometry, ch, cw, bits, fill):
        B, H, W, _ = (int(x) for x in img.shape)
        dev = img.device
        out = torch.empty_like(img)
        ws = _workspace(bits, B, H, W, dev)
        with torch.cuda.device(dev):
            L.call("p2p_diffaug_fwd", B, H, W, _p(img), _p(color), _p(geometry), ch, cw, bits, fill, _p(out), _p(ws), _stream(dev))
        ctx.save_for_backward(color, geometry)
        ctx.args = (ch, cw, bits, fill)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        color, geometry = ctx.saved_tensors
        ch, cw, bits, fill = ctx.args
        g = grad.to(torch.float32).contiguous()
        B, H, W, _ = (int(x) for x in g.shape)
        dev = g.device
        dimg = torch.empty_like(g)
        ws = _workspace(bits, B, H, W, dev)
        with torch.cuda.device(dev):
            L.call("p2p_diffaug_bwd", B, H, W, _p(g), _p(color), _p(geometry), ch, cw, bits, fill, _p(dimg), _p(ws), _stream(dev))
        return dimg, None, None, None, None, None, None


def diff_augment(images, params, policy=_ALL, fill=-1.0, device=None):
    """`images` (B, H, W, 4) RGBA in [-1, 1] (a torch tensor, or anything torch.as_tensor takes) augmented image by image with the rows
    of `params` (AugmentParameters: draw_parameters, or built by hand): an f32 (B, H, W, 4) device tensor, differentiable with respect
    to `images`, not to `params`.  The stages of `policy` are applied in the order colour, translation, cutout whatever their order in
    the string; per image, with M = 3 H W:
        colour       channels 0..2 of every pixel: u = x + b;  v = (u - mean_c u) s + mean_c u;  y = (v - m) k + m with m the mean of v
                     over the image (= mean_rgb(x) + b).  Alpha is untouched.
        translation  out[r, c] = y[r - ty, c - tx] where that pixel exists, `fill` in all four channels elsewhere
        cutout       out[r, c] = fill for y0 <= r < y0 + ch and x0 <= c < x0 + cw (the box may hang over the border)
    `fill` = -1 is the blackened transparent pixel of the datasets' normalisation.  Without "color" the result is a bit-exact
    copy / move / fill of the input; the empty policy returns the (converted) input itself."""
    bits = policy_bits(policy)
    if not isinstance(params, AugmentParameters):
        raise ValueError(f"params: expected AugmentParameters (draw_parameters), got {type(params).__name__}")
    img = torch.as_tensor(images)
    if img.dim() != 4 or img.shape[3] != 4 or img.numel() == 0:
        raise ValueError(f"expected a non-empty (B, H, W, 4) RGBA batch, got {tuple(img.shape)}")
    if params.batch != img.shape[0]:
        raise ValueError(f"the parameter table has {params.batch} rows for a batch of {img.shape[0]} images")
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    if device is not None:
        dev = torch.device(device)
    else:
        dev = img.device if img.is_cuda else torch.device("cuda:0")
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    img = img.to(device=dev, dtype=torch.float32).contiguous()          # stays on the autograd graph
    if bits == 0:
        return img
    color, geometry = params.on(dev)
    return DiffAugment.apply(img, color, geometry, params.ch, params.cw, bits, float(fill))
