"""-m gpu: the contraction kernels on integer-lattice operands (tests/lattice.py), compared bit for bit, in process with the
default switches.

Operands that are small integers times a power of two make every product and every partial sum exact in f32, so a launch must
store the exact sum (f32) or its round-to-nearest-even (bf16) whatever its summation order, K split or tile shape: no tolerance,
every image compared, and a single lost, stale or foreign term changes the stored bits wherever the integer sum is within +-256
(asserted for at least 0.99 of every bf16 case's outputs, from the reference alone).  A mismatch message lists the first ten
positions with got - want in lattice steps: the delta is the wrong term's value, the position says which tap, chunk or strip.

The first test is the premise: p2p_conv_direct (plain FMAs, ops G / P / W and the bias gradient) and one p2p_wgemm launch per
dtype (mfma_f32_32x32x16_bf16 / 32x32x2f32).  The entry points with a checker in tests/test_step_launches_gpu.py run through it
(operands="lattice": NaN before the launch, sentinel around the view, a second launch bit-identical) at the smallest shapes
tests/test_kernels_gpu.py uses for them plus one case of three or more images, so that image boundaries inside a tile are compared;
the dispatch arms of p2p_igemm, brig, p2p_wgemm and p2p_wgrad_small get the same pass in the children of
tests/test_switch_routes_gpu.py.  p2p_conv_direct and p2p_inc_conv (an f32 MFMA with fixed-order sums) have no checker there and
are driven here.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import engine as E
from tests import gpu_util as U
from tests import lattice as LT
from tests import step_launches as SL
from tests import switch_routes as R
from tests import test_fid_gpu as FID
from tests import test_step_launches_gpu as T

pytestmark = pytest.mark.gpu

BF, F32 = L.BF16, L.F32
PTR = R.PTR
WHERE = ("image", "y", "x", "channel")


def _name(dtype):
    return "bf16" if dtype == BF else "f32"


def _dtype(name, dec):
    if name in ("p2p_colsum", "p2p_colsum_batched"):
        return F32
    return dec[1] if name == "p2p_conv_strip" else dec[2] if name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewin_actbwd", "p2p_conv_fewout") else dec[0]


def _run(name, dec, seed):
    """one launch through its checker in lattice mode; returns the families ({'exact ...': 0, 'insensitive share': ...})"""
    dtype = _dtype(name, dec)
    errs = T._reissue_one(name, dec, seed, {"operands": "lattice"})
    print(f"  {name[4:]:18s} " + ", ".join(f"{f} {e:.4f}" if f.endswith("share") else f"{f} {e:g}" for f, e in sorted(errs.items())))
    assert any(f.startswith("exact ") for f in errs), errs
    bad = {f: e for f, e in errs.items() if not e < T._tol(f, dtype)}
    assert not bad, f"{name}: {bad}"
    if dtype == BF and any(f == "exact out" for f in errs):
        assert errs["insensitive share"] <= 0.01 + 1e-12
    return errs


# ---------------------------------------------------------------------------------------------------------------- p2p_conv_direct
def _conv_direct(dtype, n, lh, cg, cd, stride, seed):
    """ops G (with bias), P, W and the bias gradient of one layer on lattice operands; the inputs sit at a channel offset of
    haloed buffers whose other channels hold +-64 steps, the outputs in NaN-filled views with a sentinel around them"""
    rng = np.random.default_rng(seed)
    tdt, esz = U.tdt(dtype), SL.elem_size(dtype)
    H = stride * lh
    Kg, Kp, Kw = 16 * cg, (4 if stride == 2 else 16) * cd, n * lh * lh
    out_bf16 = dtype == BF
    hi, s_hi = LT.operands(rng, (n, H, H, cg), "x", Kg, dtype, out_bf16)
    lo, s_lo = LT.operands(rng, (n, lh, lh, cd), "x", Kp, dtype, out_bf16)
    w, s_w = LT.operands(rng, (4, 4, cg, cd), "w", max(Kg, Kp), dtype, out_bf16)
    assert Kw * 9 < 2 ** 24
    bias = LT.small_ints(rng, cd, s_hi * s_w)
    keep_hi, hv = T.in_view(T._vd(H, H, cg + 5, coff=3, halo=2, align=(3 * esz) % 16), hi, dtype, rng, lambda s: LT.other_channels(rng, s, s_hi))
    keep_lo, lv = T.in_view(T._vd(lh, lh, cd + 2, coff=1, halo=2, align=esz % 16), lo, dtype, rng, lambda s: LT.other_channels(rng, s, s_lo))
    w_d, bias_d = U.dev(w.reshape(-1), tdt), U.dev(bias)
    out_g = T.OutBuf(T._vd(lh, lh, cd + 3, coff=2, halo=2, align=(2 * esz) % 16), n, lh, lh, cd, tdt, esz)
    out_p = T.OutBuf(T._vd(H, H, cg), n, H, H, cg, tdt, esz)
    dw, db = T.FlatOut(16 * cg * cd), T.FlatOut(cd)
    L.call("p2p_conv_direct", L.OP_G, stride, dtype, n, lh, lh, cg, cd, C.byref(hv), C.byref(out_g.view), U.ptr(w_d), U.ptr(bias_d),
           None, None, U.stream())
    L.call("p2p_conv_direct", L.OP_P, stride, dtype, n, lh, lh, cg, cd, C.byref(out_p.view), C.byref(lv), U.ptr(w_d), None, None, None,
           U.stream())
    L.call("p2p_conv_direct", L.OP_W, stride, dtype, n, lh, lh, cg, cd, C.byref(hv), C.byref(lv), None, None, dw.ptr(), db.ptr(),
           U.stream())
    torch.cuda.synchronize()
    for o in (out_g, out_p, dw, db):
        o.check_around("p2p_conv_direct")
    g_sum, p_sum = SL.conv_g(hi, w, stride), SL.conv_p(lo, w, stride)
    msgs = [LT.describe_mismatches(out_g.region(), LT.expected(g_sum, dtype, bias=bias), s_hi * s_w, WHERE),
            LT.describe_mismatches(out_p.region(), LT.expected(p_sum, dtype), s_lo * s_w, WHERE),
            LT.describe_mismatches(dw.values().reshape(4, 4, cg, cd), LT.expected(SL.conv_w(hi, lo, stride), F32), s_hi * s_lo, ("kh", "kw", "g", "d")),
            LT.describe_mismatches(db.values(), LT.expected(lo.astype(np.float64).sum(axis=(0, 1, 2)), F32), s_lo, ("d",))]
    shares = (LT.sensitive_share(LT.to_int(g_sum, s_hi * s_w) + LT.to_int(bias, s_hi * s_w)), LT.sensitive_share(LT.to_int(p_sum, s_lo * s_w)))
    del keep_hi, keep_lo
    return dict(zip(("op G", "op P", "op W", "dbias"), msgs)), shares


def test_premise_fma_and_mfma_accumulation_is_exact_on_the_lattice():
    """The premise of every other test of this file and of the lattice pass of the switch children: on lattice operands plain
    FMAs (p2p_conv_direct: ops G, P, W and the bias gradient) and the MFMA accumulators (one p2p_wgemm launch per dtype:
    mfma_f32_32x32x16_bf16 and mfma_f32_32x32x2f32) give the integer reference bit for bit.  (Measured on an MI355X when this
    file was written: both do, 0 mismatches.)  If the plain-FMA launches pass and an MFMA launch does not, the message says so."""
    direct = {}
    for dtype in (F32, BF):
        msgs, _ = _conv_direct(dtype, 2, 4, 4, 64, 2, seed=1)
        direct.update({f"{_name(dtype)} {k}": m for k, m in msgs.items() if m})
    mfma = {}
    for dtype in (F32, BF):
        name, dec = R.wgemm(dtype, 2, 8, 128, 128, 2)
        try:
            _run(name, dec, seed=2)
        except AssertionError as e:
            mfma[_name(dtype)] = str(e)
    assert not direct, f"plain-FMA accumulation (p2p_conv_direct) is not exact on lattice operands: {direct}"
    assert not mfma, f"p2p_conv_direct is exact on lattice operands and the MFMA launch (p2p_wgemm) is not: {mfma}"


CONV_DIRECT = [(2, 4, 4, 64, 2), (2, 5, 36, 4, 1), (2, 1, 5, 7, 2), (1, 3, 2, 2, 2), (3, 3, 5, 6, 1)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=_name)
@pytest.mark.parametrize("n,lh,cg,cd,stride", CONV_DIRECT)
def test_conv_direct_exact(dtype, n, lh, cg, cd, stride):
    msgs, shares = _conv_direct(dtype, n, lh, cg, cd, stride, seed=10 + n + lh)
    print(f"\n  conv_direct {_name(dtype)}: sensitive share op G {shares[0]:.4f}, op P {shares[1]:.4f}")
    assert not any(msgs.values()), {k: m for k, m in msgs.items() if m}
    if dtype == BF:
        assert min(shares) >= 0.99


# ---------------------------------------------------------------------------------------------------------------- entry points with a checker
def _strip(op, n, lh, lw):
    """p2p_conv_strip on up6 (32 <-> 128 channels, bf16): haloed gathered view, dense raw output, fused statistics where offered"""
    cg, cd = 32, 128
    assert L.lib().p2p_conv_strip_ok(op, BF, n, lh, lw, cg, cd)
    slots = L.lib().p2p_conv_strip_stat_slots(op, BF, n, lh, lw, cg, cd)
    halo = lambda h, w, c: ("view", T._vd(h, w, c, halo=R.HALO))
    dense = lambda h, w, c: ("view", T._vd(h, w, c))
    hi, lo = (halo(2 * lh, 2 * lw, cg), dense(lh, lw, cd)) if op == L.OP_G else (dense(2 * lh, 2 * lw, cg), halo(lh, lw, cd))
    return "p2p_conv_strip", [op, BF, n, lh, lw, cg, cd, hi, lo, PTR, PTR if slots > 0 else None, None]


@pytest.mark.parametrize("n,lh,lw", [(2, 32, 32), (5, 4, 32), (3, 64, 64)])
@pytest.mark.parametrize("op", [L.OP_G, L.OP_P], ids=["G", "P"])
def test_conv_strip_exact(op, n, lh, lw):
    print()
    _run(*_strip(op, n, lh, lw), seed=20 + n)


def _edge(entry, op, stride, dtype, n, lh, cg, cd, bias=True, act=L.ACT_LEAKY):
    """an edge launch of the layer (hi: cg channels, lo: cd channels) as test_kernels_gpu.py::test_edge_layers_on_mfma issues it:
    op G contracts pad8(cg) channels into cd columns behind 8 other channels, op P contracts pad8(cd) into the first min(cg, 32)"""
    if op == L.OP_G:
        name, dec = R.edge(op, stride, dtype, n, lh, E.pad8(cg), cd, bias=bias, act=act, wide=8)
    else:
        name, dec = R.edge(op, stride, dtype, n, lh, E.pad8(cd), min(cg, 32), bias=bias, act=act)
    return entry, dec


FEWIN = [(L.OP_G, 2, 32, 4, 64, 2), (L.OP_G, 3, 32, 8, 64, 2), (L.OP_G, 2, 16, 1, 64, 2), (L.OP_G, 5, 8, 3, 48, 1), (L.OP_G, 2, 8, 5, 20, 1),
         (L.OP_P, 2, 64, 36, 4, 1), (L.OP_P, 3, 32, 64, 1, 1)]


@pytest.mark.parametrize("op,n,lh,cg,cd,stride", FEWIN, ids=[f"{R._opn(c[0])}-n{c[1]}-{c[2]}x{c[2]}-{c[3]}-{c[4]}-s{c[5]}" for c in FEWIN])
def test_conv_fewin_exact(op, n, lh, cg, cd, stride):
    """bf16 only (weights in registers, strip in LDS, one K step = two taps), bias + LeakyReLU epilogue"""
    name, dec = _edge("p2p_conv_fewin", op, stride, BF, n, lh, cg, cd)
    assert L.lib().p2p_conv_fewin_ok(*dec[:8])
    print()
    _run(name, dec, seed=30 + n)


@pytest.mark.parametrize("n,lh,cg,cd", [(2, 64, 36, 4), (3, 32, 64, 1)])
def test_conv_fewin_actbwd_exact(n, lh, cg, cd):
    """the data gradient with the LeakyReLU backward of the layer below in its epilogue, gate view at a channel offset"""
    _, dec = _edge("p2p_conv_fewin", L.OP_P, 1, BF, n, lh, cg, cd)
    assert L.lib().p2p_conv_fewin_ok(*dec[:8]) and dec[7] % 8 == 0
    gate = R._vd(lh, lh, dec[7] + 8, coff=8, halo=R.HALO)
    print()
    _run("p2p_conv_fewin_actbwd", dec[:12] + [gate, 0.3, None], seed=40 + n)


FEWOUT = [(L.OP_G, 2, 64, 36, 4, 1), (L.OP_G, 3, 32, 64, 1, 1), (L.OP_G, 1, 128, 33, 3, 1), (L.OP_G, 5, 8, 60, 2, 1),
          (L.OP_P, 2, 32, 4, 64, 2), (L.OP_P, 2, 16, 1, 64, 2)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=_name)
@pytest.mark.parametrize("op,n,lh,cg,cd,stride", FEWOUT, ids=[f"{R._opn(c[0])}-n{c[1]}-{c[2]}x{c[2]}-{c[3]}-{c[4]}-s{c[5]}" for c in FEWOUT])
def test_conv_fewout_exact(dtype, op, n, lh, cg, cd, stride):
    """tap-major GEMM + shifted sum out of LDS; both dtypes (p2p_conv_fewout_ok offers every one of these shapes in both)"""
    name, dec = _edge("p2p_conv_fewout", op, stride, dtype, n, lh, cg, cd, bias=op == L.OP_G, act=L.ACT_LEAKY if op == L.OP_G else L.ACT_NONE)
    assert L.lib().p2p_conv_fewout_ok(*dec[:8])
    print()
    _run(name, dec, seed=50 + n)


EDGE = [(2, 8, 4, 64, 2), (3, 8, 8, 64, 2), (2, 16, 36, 4, 1), (2, 8, 64, 1, 1), (1, 4, 33, 256, 1), (2, 8, 1, 64, 2)]      # test_edge_layers_on_mfma


@pytest.mark.parametrize("dtype", [F32, BF], ids=_name)
@pytest.mark.parametrize("n,lh,cg,cd,stride", EDGE)
def test_edge_layers_exact(dtype, n, lh, cg, cd, stride):
    """p2p_igemm_edge (op G with bias + LeakyReLU into a channel slice, op P into the first columns), p2p_wgemm_edge with msplit 1
    and 2, p2p_view_colsum (the bias gradient) of the edge layers"""
    print()
    _run(*_edge("p2p_igemm_edge", L.OP_G, stride, dtype, n, lh, cg, cd), seed=60)
    _run(*_edge("p2p_igemm_edge", L.OP_P, stride, dtype, n, lh, cg, cd, bias=False, act=L.ACT_NONE), seed=61)
    for ms in (1, 2):
        _run(*R.wgemm_edge(dtype, stride, n, lh, cg, cd, ms), seed=62 + ms)
    esz = SL.elem_size(dtype)
    _run("p2p_view_colsum", [dtype, n, lh, lh, cd, R._vd(lh, lh, E.pad8(cd), halo=R.HALO, esz=esz), PTR, PTR, None], seed=65)


@pytest.mark.parametrize("n", [2, 3])
def test_head_dgrad_exact(n):
    """p2p_head_dgrad at the shape of test_hist_indexed_gpu.py::test_indexed_head_data_gradient_kernel (K = 16 * 256)"""
    S, cg, cd = 64, 33, 256
    assert L.lib().p2p_head_dgrad_ok(BF, n, S, S, cd, 32, E.up32(cg), cd, 40)
    print()
    _run("p2p_head_dgrad", [BF, n, S, S, cd, 32, R._vd(S, S, cd, halo=R.HALO), PTR, E.up32(cg), R._vd(S, S, 40), None], seed=70 + n)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h", [8, 16])
def test_head_dgrad_exact_short_images(h, n):
    """p2p_head_dgrad accepts any H % 8 == 0 at W = 64.  H = 8: the one workgroup of an image has the top and the bottom halo in
    its 11-row strip at once; H = 16: one halo each; n = 3: image boundaries between workgroups.  The output pixels have 40
    channels: the 8 behind the 32 written ones hold the checker's sentinel, which must survive (OutBuf.check_around)."""
    S, cg, cd = 64, 33, 256
    assert L.lib().p2p_head_dgrad_ok(BF, n, h, S, cd, 32, E.up32(cg), cd, 40)
    print()
    _run("p2p_head_dgrad", [BF, n, h, S, cd, 32, R._vd(h, S, cd, halo=R.HALO), PTR, E.up32(cg), R._vd(h, S, 40), None], seed=170 + h + n)


def test_column_sums_exact():
    """p2p_colsum (a power-of-two scale) and p2p_colsum_batched over ragged tasks inside a larger output buffer"""
    print()
    _run("p2p_colsum", [PTR, 37, 19, 0.5, PTR, None], seed=80)
    tasks = ((0, 5, 64, 8), (320, 3, 19, 100), (377, 130, 7, 200))
    _run("p2p_colsum_batched", [PTR, ("tasks", tasks), 3, 64, ("store", "G", 256, 0), None], seed=81)


# ---------------------------------------------------------------------------------------------------------------- p2p_inc_conv
@pytest.mark.parametrize("case", FID.CONV_CASES, ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}{c[3]}_{c[4]}to{c[5]}_n{c[8]}")
def test_inc_conv_exact(case):
    """the FID network's convolution (f32 MFMA, fixed-order sums) on lattice input and kernel, a power-of-two scale and an integer
    shift, then ReLU: the f32 result exactly, with the sentinel checks of tests/test_fid_gpu.py around the channel slice"""
    kh, kw, stride, padding, cin, cout, H, W, N = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + cin)
    K = kh * kw * cin
    x, sx = LT.operands(rng, (N, H, W, cin), "x", K, F32, False)
    k, sk = LT.operands(rng, (kh, kw, cin, cout), "w", K, F32, False)
    step = sx * sk
    scale = (2.0 ** rng.integers(-2, 3, size=cout)).astype(np.float32)
    shift = LT.small_ints(rng, cout, step * 0.25, lim=40)          # (a multiple of the smallest scaled step)
    pt, pl = ((kh - 1) // 2, (kw - 1) // 2) if padding == "same" else (0, 0)
    conv = F.conv2d(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(k.astype(np.float64)).permute(3, 2, 0, 1),
                    stride=stride, padding=(pt, pl)).permute(0, 2, 3, 1).numpy()
    LT.to_int(conv, step)                                           # (the float64 reference is on the lattice: exact)
    want = np.maximum(LT.expected(conv, F32) * scale + shift, np.float32(0))
    assert want.dtype == np.float32 and np.array_equal(want.astype(np.float64), np.maximum(conv * scale + shift, 0.0))
    OH, OW = conv.shape[1:3]
    in_off = 0 if cin % 16 else 16
    xin = torch.as_tensor(LT.other_channels(rng, (N, H, W, cin + 2 * in_off), sx)).to(U.DEV)
    xin[..., in_off:in_off + cin] = U.dev(x)
    out_off = 32
    out = torch.full((N, OH, OW, cout + 48), FID.SENTINEL, dtype=torch.float32, device=U.DEV)
    wd, sc, sh = U.dev(k.reshape(-1, cout)), U.dev(scale), U.dev(shift)
    xv, ov = FID._view(xin, in_off), FID._view(out, out_off)
    got = []
    for _ in range(2):
        L.call("p2p_inc_conv", N, H, W, cin, kh, kw, stride, pt, pl, OH, OW, cout, C.byref(xv), wd.data_ptr(), sc.data_ptr(),
               sh.data_ptr(), C.byref(ov), FID._stream())
        got.append(out.cpu().numpy())
    assert np.array_equal(got[0], got[1])
    g = got[0]
    assert np.all(g[..., :out_off] == FID.SENTINEL) and np.all(g[..., out_off + cout:] == FID.SENTINEL)
    msg = LT.describe_mismatches(g[..., out_off:out_off + cout], want, step * 0.25, WHERE)
    assert not msg, msg
