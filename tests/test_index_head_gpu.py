"""-m gpu: the palette-index head kernels on inputs whose argmax is known exactly (tests/index_head_cases.py): exact ties, partly
idle waves, grid-stride loops, the generic kernel at every class count it takes, saturated logits in the fused head, aliased
index views.  No argmax assertion of this file excludes a pixel: the index must be the first maximum of the exact logits.

Every output lives in a buffer pre-filled with a sentinel (the index pixels have 8 channels and a halo, the gradient pixels carry
spare channels behind the classes and a halo); after a launch everything but the view's own pixels and channels must hold the
bits it held before, and a second launch must reproduce the first bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import engine as E
from tests import gpu_util as U
from tests import index_head_cases as IC

pytestmark = pytest.mark.gpu

BF, F32 = L.BF16, L.F32
H2 = E.HALO
SENTINEL = -1536.0            # a bf16 value no index, logit or gradient of these tests takes
LAM = 0.5
LOSS_RTOL, L1_ATOL, PROBS_TOL = 1e-5, 1e-5, 1e-5          # tests/test_hist_indexed_gpu.py::test_softmax_cce_argmax_kernel
DZ_TOL = {F32: 1e-5, BF: 6e-3}


def _name(dtype):
    return "bf16" if dtype == BF else "f32"


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _halo(n, h, w, ld, dtype, fill=SENTINEL):
    hb = E.HaloBuf(n, h, w, ld, dtype, U.DEV)
    hb._flat.fill_(fill)
    return hb


def _interior(hb):
    return hb.t[:, H2:H2 + hb.h, H2:H2 + hb.w, :]


class Watched:
    """a sentinel-filled HaloBuf of which a launch may write the first nc channels of the interior pixels and nothing else"""

    def __init__(self, n, h, w, ld, nc, dtype):
        self.hb, self.nc = _halo(n, h, w, ld, dtype), nc
        self.mask = torch.ones(self.hb._flat.shape, dtype=torch.bool, device=U.DEV)
        numel = self.hb.t.numel()
        self.mask[:numel].view(self.hb.t.shape)[:, H2:H2 + h, H2:H2 + w, :nc] = False
        self.before = self.hb._flat.clone()

    def region(self):
        return _interior(self.hb)[..., :self.nc].double().cpu().numpy()

    def check_around(self, what):
        assert torch.equal(_bits(self.hb._flat[self.mask]), _bits(self.before[self.mask])), f"{what}: an element outside the view changed"

    def bits(self):
        return _bits(self.hb._flat).clone()


# ---------------------------------------------------------------------------------------------------------------- p2p_softmax_cce_argmax
def _softmax_launches(dtype, n, h, w, c, z, spare, views, images=None, with_probs=True, label=""):
    """Every form of the call on logits z [n,h,w,c] (exact in dtype), once per logits view of `views` ("dense", or the ld of a
    haloed, sentinel-filled buffer): the training call, the generate call (no dz, no probabilities, both scales 0), target and
    fake_idx the same view; each against float64, with the sentinel and relaunch checks.  spare: channels behind the classes in
    the gradient pixels.  images: the float64 reference is computed image by image and dz compared on these images
    (loss and index: always on all)."""
    tdt = U.tdt(dtype)
    M = n * h * w
    t = IC.targets(n, h, w, c)
    inv = 1.0 / M
    if images is None:
        ref = IC.softmax_ref(z.reshape(M, c), t.reshape(M), LAM * inv, want_probs=with_probs)
    else:                   # the long case: float64 in chunks of one image, dz kept for `images` only
        ref = {"idx": np.empty(M, np.int64), "cce": np.empty(M), "l1": np.empty(M), "dz": {}}
        for i in range(n):
            r = IC.softmax_ref(z[i].reshape(h * w, c), t[i].reshape(-1), LAM * inv, want_probs=False)
            for k in ("idx", "cce", "l1"):
                ref[k][i * h * w:(i + 1) * h * w] = r[k]
            if i in images:
                ref["dz"][i] = r["dz"].reshape(h, w, c)
    want_loss = IC.losses(ref, inv, c)
    z_d = U.dev(np.array(z).reshape(M, c), tdt)           # (a copy: the cases are read-only)
    zviews = {}
    for v in views:
        if v == "dense":
            zviews[v] = E.DenseBuf(n, h, w, c, tdt, U.DEV)
            zviews[v].t.copy_(z_d)
        else:
            zviews[f"haloed ld {v}"] = _halo(n, h, w, v, dtype)
            _interior(zviews[f"haloed ld {v}"])[..., :c] = z_d.view(n, h, w, c)
    tb = _halo(n, h, w, 8, dtype)
    _interior(tb)[..., 0] = U.dev(t.astype(np.float32), tdt)
    part = torch.zeros(2 * 8192, dtype=torch.float32, device=U.DEV)

    def launch(zb, tview, fake, dz, probs, loss, gs, ic):
        L.call("p2p_softmax_cce_argmax", dtype, n, h, w, c, C.byref(zb.view()), C.byref(tview), C.byref(fake.hb.view()), gs, ic,
               C.byref(dz.hb.view()) if dz else None, U.ptr(probs) if probs is not None else None, U.ptr(part), U.ptr(loss), U.stream())
        torch.cuda.synchronize()

    def check_index(fake, what):
        got = fake.region()[..., 0].reshape(M).astype(np.int64)
        bad = np.flatnonzero(got != ref["idx"])
        assert not len(bad), f"{what}: {len(bad)} of {M} indices are not the first maximum; first pixels {bad[:8]}: got {got[bad[:8]]}, want {ref['idx'][bad[:8]]}"
        fake.check_around(what)

    for zname, zb in zviews.items():
        what = f"{label} {_name(dtype)} {n}x{h}x{w}x{c} z {zname}"
        # ---- the training call: gradient, probabilities, both losses; twice
        fake, dz = Watched(n, h, w, 8, 1, dtype), Watched(n, h, w, c + spare, c, dtype)
        probs = torch.full((M * c + 64,), float("nan"), dtype=torch.float32, device=U.DEV) if with_probs else None
        if probs is not None:
            probs[M * c:] = SENTINEL
        loss = torch.full((2,), float("nan"), dtype=torch.float32, device=U.DEV)
        launch(zb, tb.view(), fake, dz, probs, loss, LAM * inv, inv)
        first = (fake.bits(), dz.bits(), loss.clone(), probs.clone() if probs is not None else None)
        check_index(fake, what)
        dz.check_around(what)
        lv = loss.cpu().numpy().astype(np.float64)
        print(f"  {what}: loss {lv[0]:.7g} (f64 {want_loss[0]:.7g}), l1 {lv[1]:.7g} (f64 {want_loss[1]:.7g})")
        assert abs(lv[0] - want_loss[0]) <= LOSS_RTOL * want_loss[0], (what, lv[0], want_loss[0])
        assert abs(lv[1] - want_loss[1]) <= L1_ATOL, (what, lv[1], want_loss[1])
        if images is None:
            got_dz = dz.region()
            assert not np.isnan(got_dz).any(), f"{what}: gradient elements not written"
            err = U.rel_err(got_dz.reshape(M, c), ref["dz"])
            assert err <= DZ_TOL[dtype], (what, "dz", err)
        else:
            for i in images:
                got_dz = _interior(dz.hb)[i, ..., :c].double().cpu().numpy()
                err = U.rel_err(got_dz, ref["dz"][i])
                assert err <= DZ_TOL[dtype], (what, "dz image", i, err)
        if probs is not None:
            assert bool((probs[M * c:] == SENTINEL).all()), f"{what}: probabilities written past the end"
            err = U.rel_err(probs[:M * c].cpu().numpy().reshape(M, c), ref["p"])
            assert err <= PROBS_TOL, (what, "probs", err)
        fake.hb._flat.copy_(fake.before)
        dz.hb._flat.copy_(dz.before)
        launch(zb, tb.view(), fake, dz, probs, loss, LAM * inv, inv)
        assert torch.equal(fake.bits(), first[0]) and torch.equal(dz.bits(), first[1]) and torch.equal(_bits(loss), _bits(first[2])), \
            f"{what}: second launch differs"
        if probs is not None:
            assert torch.equal(_bits(probs), _bits(first[3])), f"{what}: second launch differs (probabilities)"
        del dz, probs
        # ---- the generate call: no gradient, no probabilities, both scales 0
        fake = Watched(n, h, w, 8, 1, dtype)
        launch(zb, tb.view(), fake, None, None, loss, 0.0, 0.0)
        check_index(fake, what + " (generate)")
        assert not loss.cpu().numpy().any()
        # ---- target and fake_idx the same view (generate_indexed): the losses still see the targets, the view ends as the index
        both = Watched(n, h, w, 8, 1, dtype)
        _interior(both.hb)[..., 0] = U.dev(t.astype(np.float32), tdt)
        launch(zb, both.hb.view(), both, None, None, loss, LAM * inv, inv)
        check_index(both, what + " (aliased)")
        lv = loss.cpu().numpy().astype(np.float64)
        assert abs(lv[0] - want_loss[0]) <= LOSS_RTOL * want_loss[0] and abs(lv[1] - want_loss[1]) <= L1_ATOL, (what, "aliased", lv, want_loss)
        assert torch.equal(_bits(loss), _bits(first[2])), f"{what}: the aliased launch's losses differ from the plain launch's"


@pytest.mark.parametrize("dtype", [F32, BF], ids=_name)
@pytest.mark.parametrize("n,h,w", IC.SOFTMAX_SHAPES, ids=lambda v: str(v))
def test_index_head_softmax256_exact_ties(dtype, n, h, w):
    """p2p_softmax_cce_argmax, 256-way fast path (16 lanes per pixel): quarter-step logits, groups and waves partly idle"""
    print()
    _softmax_launches(dtype, n, h, w, 256, IC.quarter_logits(n, h, w, 256), spare=8, views=("dense", 264), label="fast")


GENERIC = [(F32, 1, 4), (F32, 65, 68), (F32, 100, 103), (F32, 512, 515), (BF, 100, 103), (BF, 256, 260)]


@pytest.mark.parametrize("dtype,c,ld", GENERIC, ids=[f"{_name(d)}-c{c}-ld{ld}" for d, c, ld in GENERIC])
def test_index_head_softmax_generic_kernel(dtype, c, ld):
    """the wave-per-pixel kernel: its C != 256 branch at 1, 2, 2 and 8 logits per lane, and its C == 256 branch (4 logits per
    lane, 8-byte loads) through bf16 views whose ld = 260 is no multiple of 8; every shape of the fast-path test (the ragged batch
    among them)"""
    print()
    for n, h, w in IC.SOFTMAX_SHAPES:
        # (C == 256: a dense 256-channel view would take the fast path)
        _softmax_launches(dtype, n, h, w, c, IC.quarter_logits(n, h, w, c), spare=ld - c, views=(ld,) if c == 256 else ("dense", ld),
                          label="generic")


def test_index_head_softmax_generic_grid_stride():
    """N = 5, 58 x 58: 16 820 pixels > 4096 workgroups x 4 waves, so a wave of the generic kernel takes a second pixel"""
    print()
    n, h, w, c = 5, 58, 58, 100
    assert n * h * w > 4096 * 4
    _softmax_launches(F32, n, h, w, c, IC.quarter_logits(n, h, w, c), spare=3, views=("dense",), label="generic stride")


def test_index_head_softmax256_grid_stride():
    """N = 3, 210 x 210, f32: 132 300 pixels > 8192 workgroups x 16 groups with a ragged tail (132 300 = 16 * 8268 + 12), the shape
    class the f32 engine enters at batch > 32; the last image holds the second trip of the loop and the tail.  Index, both losses
    and the gradient on every pixel; float64 in chunks of an image, no probabilities.  The one long case of this file: 1.3 s
    on an MI355X machine by the test's own clock (printed), so nothing of the host work had to go."""
    print()
    n, h, w, c = 3, 210, 210, 256
    assert n * h * w > 8192 * 16 and (n * h * w) % 16
    t0 = time.perf_counter()
    z = np.concatenate([IC.quarter_logits(1, h, w, c, seed=1 + i) for i in range(n)])
    _softmax_launches(F32, n, h, w, c, z, spare=0, views=("dense",), images=range(n), with_probs=False, label="fast stride")
    print(f"  wall time {time.perf_counter() - t0:.1f} s")


def test_index_head_softmax_refuses_bf16_above_256_classes():
    """indices travel as values of the dtype, and 257, 259, ... are no bf16 values: the call is refused before any launch"""
    n, h, w, c = 1, 1, 3, 300
    zb = _halo(n, h, w, c, BF, fill=0.0)
    tb, fb = _halo(n, h, w, 8, BF, fill=0.0), _halo(n, h, w, 8, BF)
    before = fb._flat.clone()
    part = torch.zeros(2 * 8192, dtype=torch.float32, device=U.DEV)
    loss = torch.full((2,), SENTINEL, dtype=torch.float32, device=U.DEV)
    args = (n, h, w, c, C.byref(zb.view()), C.byref(tb.view()), C.byref(fb.view()), 0.0, 0.0, None, None, U.ptr(part), U.ptr(loss), U.stream())
    rc = L.lib().p2p_softmax_cce_argmax(BF, *args)
    assert rc < 0
    msg = L.lib().p2p_last_error().decode()
    assert "bf16" in msg and "256" in msg and "indices" in msg, msg
    with pytest.raises(L.P2PError, match="not bf16 values"):
        L.call("p2p_softmax_cce_argmax", BF, *args)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fb._flat), _bits(before)) and bool((loss == SENTINEL).all())         # nothing ran
    assert L.lib().p2p_softmax_cce_argmax(BF, n, h, w, 257, *args[4:]) < 0
    # f32 keeps C <= 512 (test_index_head_softmax_generic_kernel runs 512) and refuses 513
    assert L.lib().p2p_softmax_cce_argmax(F32, n, h, w, 513, *args[4:]) < 0


# ---------------------------------------------------------------------------------------------------------------- p2p_argmax_lastdim
def test_index_head_argmax_lastdim_exact_ties():
    """quarter-step rows: one row, a partly idle workgroup, one row more than 2048 workgroups x 4 waves; class counts around the
    64 lanes of a wave"""
    for M in (1, 5, 8193):
        for c in (1, 63, 64, 65, 256, 300):
            z = IC.quarter_logits(1, 1, M, c, seed=7).reshape(M, c)
            out = torch.full((M + 16,), -7, dtype=torch.int32, device=U.DEV)
            L.call("p2p_argmax_lastdim", U.ptr(U.dev(np.array(z))), M, c, U.ptr(out), U.stream())
            got = out.cpu().numpy()
            assert (got[M:] == -7).all(), (M, c)
            bad = np.flatnonzero(got[:M] != IC.first_max(z))
            assert not len(bad), f"M {M}, C {c}: {len(bad)} rows are not the first maximum, first {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------------- p2p_head_softmax_cce
@pytest.mark.parametrize("case", IC.HEAD_CASES, ids=lambda c: c.id)
def test_index_head_fused_on_lattice_operands(case):
    """p2p_head_softmax_cce (bf16, W = 64) on lattice operands: the index is the first maximum of the exact logits on every pixel;
    losses, gradient and bias gradient at the tolerances of
    tests/test_hist_indexed_gpu.py::test_fused_indexed_head_matches_conv_softmax_cce_argmax.  H = 4: the workgroup's strip touches
    the top and the bottom halo at once; n = 3, H = 12: image boundaries between workgroups."""
    n, h, S, cin, cpad, Cn = case.n, case.h, IC.HEAD_W, IC.HEAD_CIN, IC.HEAD_CPAD, IC.HEAD_NCLS
    x, w, bias, z, t = IC.head_operands(case)
    M = n * h * S
    inv = 1.0 / M
    gs = LAM * inv
    ref = IC.softmax_ref(z.reshape(M, Cn), t.reshape(M), gs, want_probs=False)
    want_loss = IC.losses(ref, inv, Cn)
    assert L.lib().p2p_head_softmax_ok(BF, n, h, S, cpad, Cn)
    tdt = U.tdt(BF)
    xb = E.HaloBuf(n, h, S, cpad, BF, U.DEV)                            # zero halo, zero pad channels
    _interior(xb)[..., :cin] = U.dev(np.array(x), tdt)
    wt = np.zeros((16, Cn, cpad), np.float32)                            # op-G copy wt[tap][d][g]
    wt[:, :, :cin] = w.reshape(16, cin, Cn).transpose(0, 2, 1)
    wt_d, bias_d = U.dev(wt.reshape(-1), tdt), U.dev(np.array(bias))
    tb = _halo(n, h, S, 8, BF)
    _interior(tb)[..., 0] = U.dev(t.astype(np.float32), tdt)
    fake, dz = Watched(n, h, S, 8, 1, BF), Watched(n, h, S, Cn, Cn, BF)
    nws = L.lib().p2p_head_softmax_workspace_bytes(n, h) // 4
    runs = []
    for _ in range(2):
        fake.hb._flat.copy_(fake.before)
        dz.hb._flat.copy_(dz.before)
        ws = torch.full((nws + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
        loss = torch.full((2,), float("nan"), dtype=torch.float32, device=U.DEV)
        dbias = torch.full((Cn + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
        dbias[Cn:] = SENTINEL
        L.call("p2p_head_softmax_cce", BF, n, h, S, cpad, Cn, C.byref(xb.view()), U.ptr(wt_d), U.ptr(bias_d), C.byref(tb.view()),
               C.byref(fake.hb.view()), gs, inv, C.byref(dz.hb.view()), U.ptr(dbias), U.ptr(ws), U.ptr(loss), U.stream())
        torch.cuda.synchronize()
        runs.append((fake.bits(), dz.bits(), _bits(loss).clone(), _bits(dbias).clone()))
    got = fake.region()[..., 0].reshape(M).astype(np.int64)
    bad = np.flatnonzero(got != ref["idx"])
    assert not len(bad), (f"{case.id}: {len(bad)} of {M} indices are not the first maximum of the exact logits; first pixels {bad[:8]}: "
                          f"got {got[bad[:8]]}, want {ref['idx'][bad[:8]]}")
    fake.check_around(case.id + " index")               # only channel 0 of the index pixels is written
    dz.check_around(case.id + " dz")                    # the halo of the gradient is untouched
    lv = loss.cpu().numpy().astype(np.float64)
    print(f"\n  {case.id}: loss {lv[0]:.7g} (f64 {want_loss[0]:.7g}), l1 {lv[1]:.7g} (f64 {want_loss[1]:.7g})")
    assert np.isfinite(lv).all(), lv
    assert abs(lv[0] - want_loss[0]) < 2e-5 * want_loss[0], (lv[0], want_loss[0])
    assert abs(lv[1] - want_loss[1]) < 1e-5, (lv[1], want_loss[1])
    got_dz = dz.region()
    assert not np.isnan(got_dz).any()
    err = U.rel_err(got_dz.reshape(M, Cn), ref["dz"])
    print(f"  dz error {err:.3g} of the maximum")
    assert err < 6e-3                                   # the gradient is stored in bf16
    assert bool((dbias[Cn:] == SENTINEL).all())
    np.testing.assert_allclose(dbias[:Cn].cpu().numpy(), got_dz.sum(axis=(0, 1, 2)), rtol=2e-5, atol=1e-7)
    for a, b in zip(*runs):
        assert torch.equal(a, b), f"{case.id}: second launch differs"
