"""Module-level functions with the reference's names (histogram.py:35-97) for callers outside the fused train step.

`calculate_rgbuv_histogram` runs the HIP forward kernels (p2p_rgbuv_hist_fwd + p2p_hist_normalize at the reference's arguments,
p2p_rgbuv_hist_general otherwise) and is differentiable, as the reference's function is: on an input that requires grad it is
one torch.autograd.Function whose backward is HIP as well (p2p_hist_normalize_bwd, then p2p_rgbuv_hist_bwd at the reference's
arguments or p2p_rgbuv_hist_general_bwd otherwise).  Engine.rgbuv_histogram goes through the same Function, so a loss hook written
with either (Pix2PixHistogramModel.generator_loss and its overrides) reaches the generator.  The scalar distances are a handful of
elementwise torch ops on the (B,S,S,3) result.  Inside the fused train step none of this is used: the loss and its gradient are
computed by the fused kernels without materialising the normalised histogram.
"""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

METHODS = {"inverse-quadratic": 0, "RBF": 1}       # any other string: code 2, no kernel function (histogram.py:20-27)


def _is_default(size, code, sigma):
    return size == 64 and code == 0 and abs(sigma - 0.02) <= 1e-12


class RGBuvHistogram(torch.autograd.Function):
    """img: contiguous f32 (B, H, W, >= 3) device tensor in [-1, 1] -> normalised (B, size, size, 3) f32.  Backward: the gradient
    with img's shape, channels >= 3 zero.  Launches on the current stream; single backward only."""

    @staticmethod
    def forward(ctx, img, size, code, sigma):
        B, H, W, ch = (int(x) for x in img.shape)
        dev = img.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        view = L.Tensor(img.data_ptr(), H * W, W, ch)
        raw = torch.empty(B * 3 * size * size, dtype=torch.float32, device=dev)
        if _is_default(size, code, sigma):
            out = torch.empty((B, 64, 64, 3), dtype=torch.float32, device=dev)
            L.call("p2p_rgbuv_hist_fwd", L.F32, B, H, W, C.byref(view), C.c_void_p(raw.data_ptr()), stream)
            L.call("p2p_hist_normalize", C.c_void_p(raw.data_ptr()), B, C.c_void_p(out.data_ptr()), stream)
        else:
            L.call("p2p_rgbuv_hist_general", L.F32, B, H, W, C.byref(view), size, code, sigma, C.c_void_p(raw.data_ptr()), stream)
            h = raw.view(B, 3, size, size).permute(0, 2, 3, 1)            # the reference stacks the components last (histogram.py:75)
            out = (h / h.sum(dim=(1, 2, 3), keepdim=True)).contiguous()     # :78-79
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(img, raw)
            ctx.args = (size, code, sigma)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        img, raw = ctx.saved_tensors
        size, code, sigma = ctx.args
        B, H, W, ch = (int(x) for x in img.shape)
        dev = img.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        g = grad_out.to(dtype=torch.float32).contiguous()
        gh = torch.empty(B * 3 * size * size, dtype=torch.float32, device=dev)
        L.call("p2p_hist_normalize_bwd", C.c_void_p(raw.data_ptr()), C.c_void_p(g.data_ptr()), B, size, C.c_void_p(gh.data_ptr()), stream)
        view = L.Tensor(img.data_ptr(), H * W, W, ch)
        dimg = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
        if _is_default(size, code, sigma):
            L.call("p2p_rgbuv_hist_bwd", L.F32, B, H, W, C.byref(view), C.c_void_p(gh.data_ptr()), C.c_void_p(dimg.data_ptr()), stream)
        else:
            L.call("p2p_rgbuv_hist_general_bwd", L.F32, B, H, W, C.byref(view), size, code, sigma, C.c_void_p(gh.data_ptr()),
                   C.c_void_p(dimg.data_ptr()), stream)
        if ch == 4:
            return dimg, None, None, None                                   # the kernels write the alpha gradient as 0
        grad = torch.zeros_like(img)
        grad[..., :3] = dimg[..., :3]
        return grad, None, None, None


def rgbuv_histogram(img, size=64, method="inverse-quadratic", sigma=0.02):
    """RGBuvHistogram on a contiguous f32 (B, H, W, >= 3) device tensor (callers convert dtype and device first, outside the
    Function, so autograd carries the gradient back through the conversion)."""
    size, sigma = int(size), float(sigma)
    code = METHODS.get(method, 2)
    if not _is_default(size, code, sigma) and (not 2 <= size <= 128 or sigma <= 0):
        raise ValueError("size must be in 2..128 and sigma positive")
    with torch.cuda.device(img.device):
        return RGBuvHistogram.apply(img, size, code, sigma)


def calculate_rgbuv_histogram(image_batch, size=64, method="inverse-quadratic", sigma=0.02, device="cuda:0"):
    """histogram.py:35-81.  (B, S, S, 4) values in [-1, 1] -> normalised (B, size, size, 3) f32 device tensor, differentiable with
    respect to `image_batch` when that is a tensor which requires grad (the gradient has its shape, dtype and device; channels >= 3
    get zero).  The reference's only call (size 64, inverse-quadratic kernel, sigma 0.02) runs the specialised kernels; any other size
    (2..128), sigma or method goes through the general kernels -- method "RBF", "inverse-quadratic", or anything else, for which the
    reference applies NO kernel function (histogram.py:20-27 has no third branch; "thresholding" is documented there but not
    implemented) and so does this.  Launches on the current stream; no engine, no parameters are created."""
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    dev = torch.device(device)
    img = torch.as_tensor(image_batch).to(device=dev, dtype=torch.float32).contiguous()
    if img.dim() != 4 or img.shape[3] < 3:
        raise ValueError(f"expected a (B, H, W, >= 3) batch, got {tuple(img.shape)}")
    return rgbuv_histogram(img, size, method, sigma)


def hellinger_loss(y_true, y_pred):
    """histogram.py:84-89"""
    b = y_true.shape[0]
    return (1.0 / math.sqrt(2.0)) * torch.sqrt(((torch.sqrt(y_pred) - torch.sqrt(y_true)) ** 2).sum()) / b


def l1_loss(y_true, y_pred):
    """histogram.py:92-93"""
    return (y_true - y_pred).abs().mean()


def l2_loss(y_true, y_pred):
    """histogram.py:96-97"""
    return ((y_true - y_pred) ** 2).mean()
