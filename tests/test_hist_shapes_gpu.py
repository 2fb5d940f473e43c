"""-m gpu: every histogram entry point of csrc/hist.hip at ragged pixel counts and odd bin counts (cases, geometry and float64
references: tests/hist_cases.py, shown to reach every class and to be able to fail by tests/test_hist_cases_cpu.py).

Everything goes through the C ABI.  Every output sits NaN-filled between guard elements holding a sentinel: the guards must be
intact, every element of the extent finite, and a second launch must give identical bits.  The image is read through three views
in both dtypes: dense with 4 channels (NaN in alpha), dense with 3, and a window of a larger NaN-filled buffer (row_stride > W,
img_stride > H W, ld = 8 behind a channel offset of 4), so that a read outside the view poisons the result.  For a bf16 view the
float64 reference takes the bf16-rounded image: the kernels widen bf16 to f32 exactly, so the f32 bounds apply unchanged.

Bounds: forward 1e-4 of the max-norm, VJP 1e-4 (mid-range images) / 2e-3 (sprites with near-black pixels: 1 / (x + 1e-6)) in
max-norm and L2 -- the suite's figures.  The general kernels at small bin counts, method 2 and wide sigma have no figure of
their own: they get max(that figure, 1.5 x the deviation of the same oracle expression evaluated in float32 on the CPU from
float64), DESIGN.md section 2's yardstick.  Every figure is printed before it is asserted."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import histogram as H
from tests import gpu_util as U
from tests import hist_cases as HC

pytestmark = pytest.mark.gpu
GUARD, SENTINEL, CAP = 64, -12345.0, 2048


class Out:
    """`n` elements, NaN (float32) or -7 (int32), between two guards of GUARD sentinels; 256 bytes keep the extent 16-byte aligned"""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.t = torch.full((n + 2 * GUARD,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device=U.DEV)
        self.t[GUARD:GUARD + n] = float("nan") if dtype.is_floating_point else -7
        self.ptr = C.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    def read(self, what, finite=True):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == a.dtype.type(SENTINEL)).all() and (a[GUARD + self.n:] == a.dtype.type(SENTINEL)).all(), f"{what}: write outside the extent"
        a = a[GUARD:GUARD + self.n].copy()
        if finite:
            assert np.isfinite(a).all(), f"{what}: {np.count_nonzero(~np.isfinite(a))} of {a.size} elements not written or not finite"
        return a


def twice(fn):
    """two launches on fresh outputs: identical bits"""
    a, b = fn(), fn()
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k}: the second launch differs"
    return a


def make_view(img, kind, dtype):
    """float32 (N, H, W, 3) host image -> (the device buffer, to be kept alive; the p2p_tensor view of it)"""
    N, Hh, W, _ = img.shape
    x = torch.tensor(img).to(U.DEV).to(U.tdt(dtype))
    if kind == "dense3":
        buf = x.contiguous()
        return buf, L.Tensor(buf.data_ptr(), Hh * W, W, 3)
    if kind == "dense4":
        buf = torch.full((N, Hh, W, 4), float("nan"), dtype=U.tdt(dtype), device=U.DEV)
        buf[..., :3] = x
        return buf, L.Tensor(buf.data_ptr(), Hh * W, W, 4)
    Hb, Wb, Cb, y0, x0, c0 = Hh + 2, W + 3, 8, 1, 2, 4
    buf = torch.full((N, Hb, Wb, Cb), float("nan"), dtype=U.tdt(dtype), device=U.DEV)
    buf[:, y0:y0 + Hh, x0:x0 + W, c0:c0 + 3] = x
    return buf, L.Tensor(buf.data_ptr() + ((y0 * Wb + x0) * Cb + c0) * buf.element_size(), Hb * Wb, Wb, Cb)


def dims(img):
    N, Hh, W, _ = img.shape
    return N, Hh, W


def report(what, got, limit):
    print(f"{what}: {' / '.join(f'{g:.3g}' for g in np.atleast_1d(got))} (bound {limit:.3g})")


def check_forward(what, got_raw, got_out, ref, limit_raw, limit_out):
    raw_err, out_err = U.rel_err(got_raw, ref[0]), U.rel_err(got_out, ref[1])
    report(f"{what} raw", raw_err, limit_raw)
    report(f"{what} normalised", out_err, limit_out)
    assert raw_err < limit_raw and out_err < limit_out, (what, raw_err, out_err)


def check_vjp(what, got, ref, limit, yard=(0.0, 0.0)):
    """got (N, H, W, 4): alpha exactly 0, RGB against the float64 VJP in max-norm and L2, each within max(limit, 1.5 x its yardstick)"""
    assert np.count_nonzero(got[..., 3]) == 0, f"{what}: alpha gradient"
    dev = HC.deviation(got[..., :3], ref)
    limits = [HC.bound(limit, y) for y in yard]
    report(what, dev, max(limits))
    assert dev[0] < limits[0] and dev[1] < limits[1], (what, dev, limits)


# ---- launches ------------------------------------------------------------------------------------------------------------------------

def run_fwd(img, vk, dtype):
    N, Hh, W = dims(img)
    keep, view = make_view(img, vk, dtype)
    raw, out = Out(N * 3 * 64 * 64), Out(N * 64 * 64 * 3)
    L.call("p2p_rgbuv_hist_fwd", dtype, N, Hh, W, C.byref(view), raw.ptr, U.stream())
    L.call("p2p_hist_normalize", raw.ptr, N, out.ptr, U.stream())
    return dict(raw=raw.read("hist_fwd raw").reshape(N, 3, 64, 64), out=out.read("hist_normalize").reshape(N, 64, 64, 3))


def run_fwd3(img, vk, dtype, listed):
    N, Hh, W = dims(img)
    keep, view = make_view(img, vk, dtype)
    raw, out = Out(N * 3 * 64 * 64), Out(N * 64 * 64 * 3)
    ws = Out(L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4)
    pts, npts = Out(N * CAP * 4), Out(N, torch.int32)
    if listed:
        L.call("p2p_rgbuv_points", dtype, N, Hh, W, C.byref(view), CAP, pts.ptr, npts.ptr, U.stream())
    L.call("p2p_rgbuv_hist_fwd3", dtype, N, Hh, W, C.byref(view), pts.ptr if listed else None, npts.ptr if listed else None, CAP,
           raw.ptr, ws.ptr, U.stream())
    L.call("p2p_hist_normalize", raw.ptr, N, out.ptr, U.stream())
    res = dict(raw=raw.read("hist_fwd3 raw").reshape(N, 3, 64, 64), out=out.read("hist_normalize").reshape(N, 64, 64, 3),
               ws=ws.read("hist_fwd3 workspace"))
    if listed:
        res["npts"] = npts.read("npoints", finite=False)
        res["pts"] = pts.read("points", finite=False).reshape(N, CAP, 4)
    return res


def run_general(img, vk, dtype, args):
    size, method, sigma = args
    N, Hh, W = dims(img)
    keep, view = make_view(img, vk, dtype)
    raw = Out(N * 3 * size * size)
    L.call("p2p_rgbuv_hist_general", dtype, N, Hh, W, C.byref(view), size, HC.METHOD_CODE[method], sigma, raw.ptr, U.stream())
    return dict(raw=raw.read("hist_general raw").reshape(N, 3, size, size))


def run_bwd(img, vk, dtype, gh, args=HC.DEFAULT, general=False):
    size, method, sigma = args
    N, Hh, W = dims(img)
    keep, view = make_view(img, vk, dtype)
    g = U.dev(gh)
    dimg = Out(N * Hh * W * 4)
    if general:
        L.call("p2p_rgbuv_hist_general_bwd", dtype, N, Hh, W, C.byref(view), size, HC.METHOD_CODE[method], sigma, U.ptr(g), dimg.ptr,
               U.stream())
    else:
        L.call("p2p_rgbuv_hist_bwd", dtype, N, Hh, W, C.byref(view), U.ptr(g), dimg.ptr, U.stream())
    return dict(dimg=dimg.read("hist backward dimg").reshape(N, Hh, W, 4))


def run_hellinger(real, fake, vk, dtype, slabs):
    """p2p_rgbuv_hist_fwd of both images, p2p_hellinger_fwd / _finish, then the shared-row backward (one slab) or the per-component
    one (three slabs, summed here)"""
    N, Hh, W = dims(fake)
    keep_r, vr = make_view(real, vk, dtype)
    keep_f, vf = make_view(fake, vk, dtype)
    n = N * 3 * 64 * 64
    h_r, h_f, gh = Out(n), Out(n), Out(n)
    tot_r, tot_f, sqp, sq, loss = Out(N), Out(N), Out(N), Out(1), Out(1)
    dimg = Out((3 if slabs else 1) * N * Hh * W * 4)
    L.call("p2p_rgbuv_hist_fwd", dtype, N, Hh, W, C.byref(vr), h_r.ptr, U.stream())
    L.call("p2p_rgbuv_hist_fwd", dtype, N, Hh, W, C.byref(vf), h_f.ptr, U.stream())
    L.call("p2p_hellinger_fwd", h_r.ptr, h_f.ptr, N, tot_r.ptr, tot_f.ptr, sqp.ptr, sq.ptr, U.stream())
    L.call("p2p_hellinger_finish", sq.ptr, 1.0 / N, loss.ptr, U.stream())
    L.call("p2p_rgbuv_hist_hellinger_bwd" if slabs else "p2p_rgbuv_hist_hellinger_bwd3", dtype, N, Hh, W, C.byref(vf), h_r.ptr, h_f.ptr,
           tot_r.ptr, tot_f.ptr, sq.ptr, 1.0 / (2.0 * math.sqrt(2.0) * N), gh.ptr, dimg.ptr, U.stream())
    d = dimg.read("hellinger backward dimg")
    res = dict(loss=loss.read("loss"), gh=gh.read("gh workspace"), tot=np.concatenate([tot_r.read("tot"), tot_f.read("tot")]),
               sq=np.concatenate([sqp.read("sq_part"), sq.read("sq_sum")]))
    res["dimg"] = d.reshape(3, N, Hh, W, 4).sum(0) if slabs else d.reshape(N, Hh, W, 4)
    res["slabs"] = d
    return res


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(HC.SHAPES))
def test_default_forward_and_normalisation(shape):
    """p2p_rgbuv_hist_fwd (batches of 96 pixels) + p2p_hist_normalize against float64, raw and normalised"""
    for kind, dtype, vk in HC.variants(shape):
        got = twice(lambda: run_fwd(HC.image(shape, kind, dtype), vk, dtype))
        check_forward((shape, kind, dtype, vk), got["raw"], got["out"], HC.forward(shape, kind, dtype), HC.FWD_BOUND, HC.FWD_BOUND)


@pytest.mark.parametrize("shape", list(HC.SHAPES))
def test_shared_row_forward_dense_and_listed(shape):
    """p2p_rgbuv_hist_fwd3 over the pixels (three ranges of 64-pixel batches) and over the colour list of p2p_rgbuv_points (tiles
    of 1024 pixels): both against float64 and against each other; the list is the restated one, row for row"""
    for kind, dtype, vk in HC.variants(shape):
        img, ref = HC.image(shape, kind, dtype), HC.forward(shape, kind, dtype)
        dense = twice(lambda: run_fwd3(img, vk, dtype, listed=False))
        check_forward((shape, kind, dtype, vk, "dense"), dense["raw"], dense["out"], ref, HC.FWD_BOUND, HC.FWD_BOUND)
    listed_cases = [("mid", 0, "dense4"), ("mid", 1, "strided")]
    if HC.has_sprite(shape):
        listed_cases += [(k, dt, vk) for k in ("sprite", "rich") for dt, vk in ((0, "strided"), (1, "dense3"), (0, "dense4"))]
    for kind, dtype, vk in listed_cases:
        img, ref = HC.image(shape, kind, dtype), HC.forward(shape, kind, dtype)
        N, Hh, W = dims(img)
        listed = twice(lambda: run_fwd3(img, vk, dtype, listed=True))
        dense = run_fwd3(img, vk, dtype, listed=False)
        check_forward((shape, kind, dtype, vk, "listed"), listed["raw"], listed["out"], ref, HC.FWD_BOUND, HC.FWD_BOUND)
        assert np.abs(listed["out"] - dense["out"]).max() <= 1e-4 * dense["out"].max()
        for n, want in enumerate(HC.colour_points(img)):
            k, pts = int(listed["npts"][n]), listed["pts"][n]
            if len(want) > CAP:                                      # more colours than the list holds: contracted densely
                assert k == -1
                continue
            assert k == len(want) and np.array_equal(pts[:k], want), (shape, kind, n, k, len(want))
            assert np.isnan(pts[k:]).all()                          # nothing beyond the list
            assert pts[:k, 3].sum() == Hh * W and (pts[:k, 3] >= 1).all()
            tiles = len(HC.point_tiles(Hh * W))
            colours = len(np.unique(img[n].reshape(-1, 3), axis=0))
            assert colours <= k <= colours * tiles and len(np.unique(pts[:k, :3], axis=0)) == colours


@pytest.mark.parametrize("size,method,sigma", HC.BIN_CASES)
def test_general_forward_at_odd_bin_counts(size, method, sigma):
    """p2p_rgbuv_hist_general (batches of 32 pixels, size^2 / 256 bins per thread, clamped duplicates) on the tail shapes and
    one without a tail"""
    args = (size, method, sigma)
    for shape in HC.GENERAL_SHAPES:
        for kind, dtype, vk in HC.variants(shape):
            got = twice(lambda: run_general(HC.image(shape, kind, dtype), vk, dtype, args))
            ref, yard = HC.forward(shape, kind, dtype, args), HC.forward_yardstick(shape, kind, dtype, args)
            print("yardstick raw / normalised", yard)
            norm = HC._np(HC.normalise(torch.as_tensor(got["raw"], dtype=torch.float64)))
            check_forward((shape, kind, dtype, vk, args), got["raw"], norm, ref, HC.bound(HC.FWD_BOUND, yard[0]),
                          HC.bound(HC.FWD_BOUND, yard[1]))


@pytest.mark.parametrize("size", HC.NORMALIZE_BWD_SIZES)
def test_normalize_bwd_at_odd_sizes(size):
    """p2p_hist_normalize_bwd against the float64 VJP of raw^T / sum(raw)"""
    raw, g, ref = HC.normalize_bwd(size)
    yard = HC.deviation(HC.normalize_bwd(size, HC.F32)[2], ref)

    def run():
        gh, raw_d, g_d = Out(raw.size), U.dev(raw), U.dev(g)
        L.call("p2p_hist_normalize_bwd", U.ptr(raw_d), U.ptr(g_d), raw.shape[0], size, gh.ptr, U.stream())
        return dict(gh=gh.read("hist_normalize_bwd").reshape(raw.shape))

    dev = HC.deviation(twice(run)["gh"], ref)
    print("yardstick", yard)
    report(("normalize_bwd", size), dev, HC.bound(HC.VJP_MID_BOUND, max(yard)))
    assert dev[0] < HC.bound(HC.VJP_MID_BOUND, yard[0]) and dev[1] < HC.bound(HC.VJP_MID_BOUND, yard[1])


@pytest.mark.parametrize("shape", list(HC.SHAPES))
def test_shared_row_backward_every_pixel(shape):
    """p2p_rgbuv_hist_bwd (rgbuv_hist_bwd3_kernel: nsplit ranges of 64-pixel batches, pipelined) with a random raw-histogram
    gradient: every pixel's gradient against float64 -- the empty split included, dimg must still be complete -- alpha exactly 0"""
    for kind, dtype, vk in HC.variants(shape):
        gh, ref = HC.raw_vjp(shape, kind, dtype)
        got = twice(lambda: run_bwd(HC.image(shape, kind, dtype), vk, dtype, gh))
        check_vjp((shape, kind, dtype, vk), got["dimg"], ref, HC.vjp_bound(kind))


@pytest.mark.parametrize("shape", list(HC.SHAPES))
def test_hellinger_loss_and_shared_row_gradient(shape):
    """p2p_hellinger_fwd / _finish and p2p_rgbuv_hist_hellinger_bwd3 against the closed form in float64"""
    for kind, dtype, vk in HC.variants(shape):
        real, fake, loss, grad = HC.hellinger(shape, kind, dtype)
        got = twice(lambda: run_hellinger(real, fake, vk, dtype, slabs=False))
        report((shape, kind, dtype, vk, "loss"), abs(float(got["loss"][0]) - loss) / loss, 1e-4)
        assert abs(float(got["loss"][0]) - loss) < 1e-4 * loss
        check_vjp((shape, kind, dtype, vk), got["dimg"], grad, HC.vjp_bound(kind))


@pytest.mark.parametrize("shape", HC.TAIL_SHAPES)
def test_hellinger_gradient_in_three_slabs(shape):
    """p2p_rgbuv_hist_hellinger_bwd (rgbuv_hist_bwd_kernel, one slab per component, batches of 64 pixels) on the tail shapes: the
    slabs summed against the same closed form"""
    for kind, dtype, vk in HC.variants(shape):
        real, fake, loss, grad = HC.hellinger(shape, kind, dtype)
        got = twice(lambda: run_hellinger(real, fake, vk, dtype, slabs=True))
        check_vjp((shape, kind, dtype, vk), got["dimg"], grad, HC.vjp_bound(kind))


@pytest.mark.parametrize("size,method,sigma", HC.BIN_CASES)
def test_general_backward_at_odd_bin_counts(size, method, sigma):
    """p2p_rgbuv_hist_general_bwd (64 pixels per workgroup, gh and the kernel rows padded to Sp = 4 ceil(size / 4) and read in
    float4 pieces, wave w owning row blocks w, w + 4, ...) on the tail shapes"""
    args = (size, method, sigma)
    for shape in HC.TAIL_SHAPES:
        for kind, dtype, vk in HC.variants(shape):
            gh, ref = HC.raw_vjp(shape, kind, dtype, args)
            yard = HC.vjp_yardstick(HC.raw_vjp, shape, kind, dtype, args)
            got = twice(lambda: run_bwd(HC.image(shape, kind, dtype), vk, dtype, gh, args, general=True))
            print("yardstick", yard)
            check_vjp((shape, kind, dtype, vk, args), got["dimg"], ref, HC.vjp_bound(kind), yard)


@pytest.mark.parametrize("shape,args", [("tail-63", HC.DEFAULT), ("one-batch-plus-1", (63, HC.RBF, 0.5))])
def test_public_function_under_autograd_at_ragged_shapes(shape, args):
    """histogram.calculate_rgbuv_histogram, forward and VJP, on 3-channel images: 33 x 31 at the reference's arguments (the
    specialised kernels) and 5 x 13 with 63 RBF bins (the general ones)"""
    size, method, sigma = args
    img = HC.image(shape, "mid", 0)
    g, ref = HC.normalised_vjp(shape, "mid", 0, args)
    yard_f, yard_b = 0.0, (0.0, 0.0)                   # the reference's arguments: the suite's figures as they are
    if args != HC.DEFAULT:
        yard_f = HC.forward_yardstick(shape, "mid", 0, args)[1]
        yard_b = HC.vjp_yardstick(HC.normalised_vjp, shape, "mid", 0, args)
    x = torch.tensor(img, device=U.DEV, requires_grad=True)
    out = H.calculate_rgbuv_histogram(x, size=size, method=method, sigma=sigma)
    assert out.shape == (img.shape[0], size, size, 3) and out.requires_grad
    err = U.rel_err(out.detach().cpu().numpy(), HC.forward(shape, "mid", 0, args)[1])
    report((shape, args, "forward"), err, HC.bound(HC.FWD_BOUND, yard_f))
    assert err < HC.bound(HC.FWD_BOUND, yard_f)
    (out * torch.as_tensor(g, device=U.DEV)).sum().backward()
    got = x.grad.cpu().numpy()
    assert got.shape == img.shape and np.isfinite(got).all()
    dev = HC.deviation(got, ref)
    print("yardstick", yard_f, yard_b)
    report((shape, args, "VJP"), dev, HC.bound(HC.VJP_MID_BOUND, max(yard_b)))
    assert dev[0] < HC.bound(HC.VJP_MID_BOUND, yard_b[0]) and dev[1] < HC.bound(HC.VJP_MID_BOUND, yard_b[1])
