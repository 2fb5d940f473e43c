"""-m gpu: the InstanceNorm, loss, Adam and colour-point kernels on the inputs their arithmetic was designed around -- large mean /
std ratios, constant channels, variances far below eps, saturated logits and tanh, exact L1 ties, zero / underflowing / huge
gradients, colour lists at their capacity.  Cases, references and bounds: tests/numeric_edges.py (proved able to fail by
tests/test_numeric_edges_cpu.py).  Every test prints its worst figures as `EDGE ...` lines (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import engine as E
from tests import ema_oracle as EO
from tests import gpu_util as U
from tests import numeric_edges as NE
from tests import switch_routes as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
DT = {L.F32: "f32", L.BF16: "bf16"}
NORM_PARAMS = [pytest.param(c, d, id=f"{c.id}-{DT[d]}") for d in NE.DTYPES for c in NE.NORM_CASES]


def _by_regime(e, c):
    return " ".join(f"R{r} {float(e[:, [ch for ch in range(c) if NE.regime(ch) == r]].max()):.2f}" for r in range(min(6, c)))


# ---------------------------------------------------------------------------------------------------------------- A: the forms
def test_the_cases_reach_every_statistics_computing_arm():
    want_f, want_b = NE.statistics_arms()
    got = [NE.norm_routes(c, d) for d in NE.DTYPES for c in NE.NORM_CASES]
    assert want_f <= {f for f, _ in got} and want_b <= {b for _, b in got}


@pytest.mark.parametrize("case,dtype", NORM_PARAMS)
def test_norm_act_on_ill_conditioned_channels(case, dtype):
    """p2p_norm_act_fwd / _bwd in the form the case selects: stored statistics within the mu / rs bounds of the f64 moments, the
    apply pass against f64 from the kernel's own statistics, the constant channels against act(drop(beta)), the backward against the
    closed form in f64 from the kernel's statistics."""
    n, h, c, tdt = case.n, case.h, case.c, U.tdt(dtype)
    x, gamma, beta, mask = NE.norm_input(case, dtype)
    arm_f, arm_b = NE.norm_routes(case, dtype)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    mask_d = U.dev(mask.reshape(-1, c), torch.uint8) if mask is not None else None
    mp = U.ptr(mask_d) if mask is not None else None
    out = E.HaloBuf(n, h, h, c + 8, dtype, U.DEV)
    stats = torch.full((n, c, 2), float("nan"), dtype=torch.float32, device=U.DEV)
    raw = E.DenseBuf(n, h, h, c, tdt, U.DEV)
    if case.nslabs:
        src = U.dev(NE.pow2_slabs(x, case.nslabs).reshape(-1))
        raw.t.fill_(float("nan"))
        raw_args, raw_out = (U.ptr(src), 2, case.nslabs, n * h * h * c), raw.ptr()
    else:
        raw.t.copy_(U.dev(x.reshape(-1, c), tdt))
        raw_args, raw_out = (raw.ptr(), 1, 1, 0), None
    if case.slots:
        sp = NE.slot_partials(x, case.slots)
        ws, nsplit = U.dev(sp.reshape(-1)), -case.slots
    else:
        ws, nsplit = torch.empty(n * 16 * c * 2, dtype=torch.float32, device=U.DEV), case.nsplit
    L.call("p2p_norm_act_fwd", dtype, n, h, h, c, *raw_args, U.ptr(g_d), U.ptr(b_d), NE.EPS, case.act, NE.ALPHA, mp,
           C.byref(out.view(coff=8)), raw_out, U.ptr(stats), U.ptr(ws), ws.numel() * 4, nsplit, U.stream())
    if case.nslabs:
        assert np.array_equal(U.dense_to_np(raw), x)              # the slabs sum to x bit for bit, and so does the loader
    st = stats.cpu().numpy().astype(np.float64)
    mu, rs = st[..., 0], st[..., 1]
    assert np.isfinite(st).all()

    # 1. the stored statistics
    if case.slots:
        e_mu, e_rs = NE.given_stat_errors(mu, rs, *NE.pooled64(sp, h * h), x)
    else:
        e_mu, e_rs = NE.stat_errors(mu, rs, x)
    print(f"\nEDGE norm {case.id} {DT[dtype]} fwd {R.describe('norm_fwd', arm_f)}: mu/bound {_by_regime(e_mu, c)}  rs/bound {_by_regime(e_rs, c)}")
    assert e_mu.max() <= 1.0, _by_regime(e_mu, c)
    assert e_rs.max() <= 1.0, _by_regime(e_rs, c)

    # 2. the apply pass, from the kernel's own statistics
    got = U.halo_to_np(out).astype(np.float64)
    assert np.count_nonzero(got[..., :8]) == 0
    got = got[..., 8:]
    err = NE.plane_err(got, NE.apply64(x, mu, rs, gamma, beta, case.act, mask))
    const = [ch for ch in range(c) if NE.regime(ch) in NE.CONSTANT]
    cref = NE.constant_ref(x, beta, case.act, mask)
    dev = np.abs(got - cref)[..., const]
    bound = NE.constant_out_bound(x, gamma, beta, case.act, mask, dtype)[..., const]
    exact = bool((got[..., const] == U.q(cref, dtype)[..., const]).all())
    print(f"EDGE norm {case.id} {DT[dtype]} apply err/tol {err / NE.OUT_TOL[dtype]:.2f}  constant channels dev/bound {float((dev / bound).max()):.2f}"
          f" exact {exact}")
    assert err <= NE.OUT_TOL[dtype]
    assert (dev <= bound).all(), float((dev / bound).max())

    # 3. the backward pass, from the kernel's own statistics
    dy1, dy2 = NE.grad_sources(case, dtype)
    g1 = E.DenseBuf(n, h, h, c + 8, tdt, U.DEV)
    g1.t.copy_(U.dev(dy1.reshape(-1, c + 8), tdt))
    if case.gslabs:
        g2_d = U.dev(dy2.reshape(-1))
        gs2 = L.GSrc(g2_d.data_ptr(), 2, 5, n * h * h * c, c, 0)
        dy = dy1[..., 8:].astype(np.float64) + dy2.astype(np.float64).sum(0)
    else:
        g2 = E.DenseBuf(n, h, h, c, tdt, U.DEV)
        g2.t.copy_(U.dev(dy2.reshape(-1, c), tdt))
        gs2 = g2.gsrc()
        dy = dy1[..., 8:].astype(np.float64) + dy2
    draw = E.HaloBuf(n, h, h, c, dtype, U.DEV)
    part = torch.zeros((2, n, c), dtype=torch.float32, device=U.DEV)
    nws = torch.empty(n * 16 * c * 2, dtype=torch.float32, device=U.DEV)
    L.call("p2p_norm_act_bwd", dtype, n, h, h, c, raw.ptr(), U.ptr(stats), U.ptr(g_d), U.ptr(b_d), case.act, NE.ALPHA, mp,
           C.byref(g1.gsrc(coff=8)), C.byref(gs2), C.byref(draw.view()), U.ptr(part[1]), U.ptr(part[0]), U.ptr(nws), nws.numel() * 4,
           case.nsplit, U.stream())
    dx, dgamma, dbeta, kink = NE.backward64(x, mu, rs, gamma, beta, case.act, mask, dy)
    assert kink.mean() <= NE.KINK_SHARE
    got_dx = U.halo_to_np(draw).astype(np.float64)
    assert np.isfinite(got_dx).all()
    diff = np.where(kink, 0.0, np.abs(got_dx - dx))
    e_dx = diff.max() / np.abs(dx).max()
    # a constant channel behind a closed ReLU has d(raw) = 0 everywhere: then the kernel's must be 0 too
    e_const = max(float(diff[..., ch].max() / (np.abs(dx[..., ch]).max() or np.finfo(np.float64).tiny)) for ch in const)
    dgam, dbet = (torch.empty(c, dtype=torch.float32, device=U.DEV) for _ in range(2))
    L.call("p2p_colsum", U.ptr(part[1]), n, c, 1.0, U.ptr(dgam), U.stream())
    L.call("p2p_colsum", U.ptr(part[0]), n, c, 1.0, U.ptr(dbet), U.stream())
    e_g, e_b = U.rel_err(dgam.cpu().numpy(), dgamma), U.rel_err(dbet.cpu().numpy(), dbeta)
    print(f"EDGE norm {case.id} {DT[dtype]} bwd {R.describe('norm_bwd', arm_b)}: d(raw) {e_dx:.1e} constant channels {e_const:.1e} "
          f"dgamma {e_g:.1e} dbeta {e_b:.1e}  undecided gates {int(kink.sum())}")
    assert e_dx < NE.BWD_TOL[dtype] and e_const < NE.BWD_TOL[dtype]
    assert e_g < NE.PART_TOL and e_b < NE.PART_TOL


@pytest.mark.parametrize("dtype", NE.DTYPES, ids=["f32", "bf16"])
def test_norm_1x1_with_huge_constants(dtype):
    """One pixel per map: the mean is the pixel, so whatever the convolution produced -- up to 3e19, whose square overflows f32 --
    the output is act(drop(beta)) and d(raw) is 0, bit-identical between p2p_norm_act_fwd_1x1 / _bwd_1x1 and the general entry
    points at H = W = 1."""
    n, c, tdt = 3, 64, U.tdt(dtype)
    rng = np.random.default_rng(61)
    vals = np.array([5.1, -200.0, 3e19, -3e19, 1e10, 65536.0, -1e-30, 0.0])
    x = U.q(vals[rng.integers(0, len(vals), size=(n, 1, 1, c))], dtype)
    x[0, 0, 0, :8] = U.q(vals, dtype)
    gamma = rng.normal(size=c).astype(np.float32)
    beta = (0.5 * rng.normal(size=c)).astype(np.float32)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    raw = E.DenseBuf(n, 1, 1, c, tdt, U.DEV)
    raw.t.copy_(U.dev(x.reshape(-1, c), tdt))
    nws = torch.empty(n * 16 * c * 2, dtype=torch.float32, device=U.DEV)
    dy1 = U.dev(U.q(rng.normal(size=(n, c + 8)), dtype), tdt)
    dy2 = U.dev(rng.normal(size=(5, n, c)).astype(np.float32).reshape(-1))
    gs1, gs2 = L.GSrc(dy1.data_ptr(), 1, 1, n * (c + 8), c + 8, 8), L.GSrc(dy2.data_ptr(), 2, 5, n * c, c, 0)
    for act in (L.ACT_LEAKY, L.ACT_RELU):
        for use_mask in (False, True):
            mask = rng.integers(0, 2, size=(n, 1, 1, c)).astype(np.uint8) if use_mask else None
            mask_d = U.dev(mask.reshape(-1, c), torch.uint8) if use_mask else None
            mp = U.ptr(mask_d) if use_mask else None
            want, got = E.HaloBuf(n, 1, 1, c + 8, dtype, U.DEV), E.HaloBuf(n, 1, 1, c + 8, dtype, U.DEV)
            stats = torch.full((n, c, 2), float("nan"), dtype=torch.float32, device=U.DEV)
            L.call("p2p_norm_act_fwd", dtype, n, 1, 1, c, raw.ptr(), 1, 1, 0, U.ptr(g_d), U.ptr(b_d), NE.EPS, act, NE.ALPHA, mp,
                   C.byref(want.view(coff=8)), None, U.ptr(stats), U.ptr(nws), nws.numel() * 4, 1, U.stream())
            L.call("p2p_norm_act_fwd_1x1", dtype, n, c, U.ptr(g_d), U.ptr(b_d), act, NE.ALPHA, mp, C.byref(got.view(coff=8)), U.stream())
            assert torch.equal(want._flat.view(torch.int16 if dtype == L.BF16 else torch.int32),
                               got._flat.view(torch.int16 if dtype == L.BF16 else torch.int32))
            st = stats.cpu().numpy()
            assert np.array_equal(st[..., 0], x[:, 0, 0, :]) and np.isfinite(st).all()
            assert np.abs(st[..., 1] / (1.0 / math.sqrt(NE.EPS)) - 1).max() <= NE.rs_bound(0.0)
            # bit for bit: the kernel's own float32 operations, beta * keep, then alpha (as float32) * that on the negative side
            y32 = np.broadcast_to(beta, x.shape) * (mask.astype(np.float32) * np.float32(2) if use_mask else np.float32(1))
            ref = U.q(np.where(y32 > 0, y32, (np.float32(NE.ALPHA) if act == L.ACT_LEAKY else np.float32(0)) * y32), dtype)
            assert np.abs(ref - NE.constant_ref(x, beta, act, mask)).max() <= 2.0 ** -8 * np.abs(beta).max() * 2
            assert np.array_equal(U.halo_to_np(got)[..., 8:], ref)
            part_w = torch.full((2, n, c), float("nan"), dtype=torch.float32, device=U.DEV)
            part_g = torch.full((2, n, c), float("nan"), dtype=torch.float32, device=U.DEV)
            draw = E.HaloBuf(n, 1, 1, c, dtype, U.DEV)
            draw.t.fill_(float("nan"))
            L.call("p2p_norm_act_bwd", dtype, n, 1, 1, c, raw.ptr(), U.ptr(stats), U.ptr(g_d), U.ptr(b_d), act, NE.ALPHA, mp, C.byref(gs1),
                   C.byref(gs2), C.byref(draw.view()), U.ptr(part_w[1]), U.ptr(part_w[0]), U.ptr(nws), nws.numel() * 4, 1, U.stream())
            L.call("p2p_norm_act_bwd_1x1", dtype, n, c, U.ptr(g_d), U.ptr(b_d), act, NE.ALPHA, mp, C.byref(gs1), C.byref(gs2),
                   U.ptr(part_g[1]), U.ptr(part_g[0]), U.stream())
            assert torch.count_nonzero(draw.t[:, E.HALO, E.HALO, :]) == 0                  # d(raw) = 0, not NaN from 0 * inf
            assert torch.equal(part_w.view(torch.int32), part_g.view(torch.int32)) and torch.count_nonzero(part_g[1]) == 0
            assert bool(torch.isfinite(part_g).all())


# ---------------------------------------------------------------------------------------------------------------- A: conv epilogues
def _weights(w, cg, cd, dtype):
    wn = torch.empty(16 * cg * cd, dtype=U.tdt(dtype), device=U.DEV)
    wt = torch.empty(16 * cg * cd, dtype=U.tdt(dtype), device=U.DEV)
    w_d = U.dev(w.reshape(-1))
    L.call("p2p_weight_prep", dtype, U.ptr(w_d), cg, cd, U.ptr(wn), U.ptr(wt), U.stream())
    return wn, wt


def _epilogue_checks(tag, dtype, n, res_h, res_w, ncols, out, spart, slots, ratio):
    """the slot partials of a conv epilogue against the STORED output (bounds of check 1 with k = 0), then the apply-only norm pass
    over them (check 2)"""
    x = U.dense_to_np(out)
    assert np.isfinite(x).all()
    x64 = x.astype(np.float64)
    got_ratio = float(np.median(np.abs(x64.mean(axis=(1, 2))) / x64.std(axis=(1, 2))))
    sp = spart.view(n, slots, ncols, 2).cpu().numpy().astype(np.float64)
    cnt = res_h * res_w / slots
    mean = sp[..., 0].mean(axis=1)                                     # the pooling formula of tests/test_kernels_gpu.py
    m2 = sp[..., 1].sum(axis=1) + cnt * ((sp[..., 0] - mean[:, None, :]) ** 2).sum(axis=1)
    e_mu, e_rs = NE.given_stat_errors(mean, 1.0 / np.sqrt(m2 / (res_h * res_w) + NE.EPS), *NE.stats64(x)[:2], x)
    print(f"\nEDGE conv {tag} {DT[dtype]} mean/std {got_ratio:.0f} (aimed {ratio:.0f}) slots {slots}: pooled mu/bound {e_mu.max():.2f} "
          f"rs/bound {e_rs.max():.2f}")
    assert 0.5 * ratio <= got_ratio <= 2 * ratio
    assert e_mu.max() <= 1.0 and e_rs.max() <= 1.0
    rng = np.random.default_rng(7)
    gamma = (1 + 0.2 * rng.normal(size=ncols)).astype(np.float32)
    beta = (0.2 * rng.normal(size=ncols)).astype(np.float32)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    y = E.HaloBuf(n, res_h, res_w, ncols, dtype, U.DEV)
    stats = torch.full((n, ncols, 2), float("nan"), dtype=torch.float32, device=U.DEV)
    L.call("p2p_norm_act_fwd", dtype, n, res_h, res_w, ncols, out.ptr(), 1, 1, 0, U.ptr(g_d), U.ptr(b_d), NE.EPS, L.ACT_LEAKY, NE.ALPHA,
           None, C.byref(y.view()), None, U.ptr(stats), U.ptr(spart), spart.numel() * 4, -slots, U.stream())
    st = stats.cpu().numpy().astype(np.float64)
    e_mu, e_rs = NE.stat_errors(st[..., 0], st[..., 1], x)
    got = U.halo_to_np(y)
    err = NE.plane_err(got, NE.apply64(x, st[..., 0], st[..., 1], gamma, beta, L.ACT_LEAKY, None))
    print(f"EDGE conv {tag} {DT[dtype]} norm over the slots: mu/bound {e_mu.max():.2f} rs/bound {e_rs.max():.2f} apply err/tol "
          f"{err / NE.OUT_TOL[dtype]:.2f}")
    assert e_mu.max() <= 1.0 and e_rs.max() <= 1.0
    assert err <= NE.OUT_TOL[dtype]


@pytest.mark.parametrize("dtype", NE.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("op,n,lh,cg,cd", NE.IGEMM_CASES)
def test_igemm_epilogue_statistics_of_an_offset_output(dtype, op, n, lh, cg, cd):
    ratio = NE.CONV_RATIO[dtype]
    a, w, _ = NE.conv_operands(op, n, lh, lh, cg, cd, dtype, ratio)
    wn, wt = _weights(w, cg, cd, dtype)
    ab = U.halo_from(a, dtype)
    ncols, res = (cd, lh) if op == L.OP_G else (cg, 2 * lh)
    slots = L.lib().p2p_igemm_layer_stat_slots(op, dtype, n, lh, lh, cg, cd)
    assert slots > 0
    out = E.DenseBuf(n, res, res, ncols, U.tdt(dtype), U.DEV)
    out.t.fill_(float("nan"))
    spart = torch.full((n * slots * ncols * 2,), float("nan"), dtype=torch.float32, device=U.DEV)
    hv, lv = (ab.view(), out.view()) if op == L.OP_G else (out.view(), ab.view())
    L.call("p2p_igemm", op, dtype, n, lh, lh, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wt if op == L.OP_G else wn), 1, None, U.ptr(spart),
           U.stream())
    _epilogue_checks(f"igemm {'GP'[op]} {n}x{lh}x{lh} {cg}->{cd}", dtype, n, res, res, ncols, out, spart, slots, ratio)


@pytest.mark.parametrize("cbw", [1, 2])
@pytest.mark.parametrize("op,n,lh,cg,cd", NE.BRIG_CASES)
def test_block_resident_epilogue_statistics_of_an_offset_output(op, n, lh, cg, cd, cbw, monkeypatch):
    """p2p_igemm through the block-resident kernel (csrc/brig.hip), whose epilogue feeds the same slots"""
    if cbw == 2 and (cg if op == L.OP_P else cd) % (64 if op == L.OP_P else 256):
        pytest.skip("the 64-channels-per-wave form needs whole 64 / 256 channel tiles")
    dtype = L.BF16
    monkeypatch.setenv("P2P_BRIG_CBW", str(cbw))
    monkeypatch.setenv("P2P_BRIG_MIN_WG", "1")
    assert L.lib().p2p_brig_ok(op, dtype, n, lh, lh, cg, cd) == 1
    a, w, ratio = NE.conv_operands(op, n, lh, lh, cg, cd, dtype, NE.FUSED_RATIO, scale=NE.FUSED_SCALE)
    wn, wt = _weights(w, cg, cd, dtype)
    ab = U.halo_from(a, dtype)
    ncols, res = (cd, lh) if op == L.OP_G else (cg, 2 * lh)
    slots = L.lib().p2p_igemm_layer_stat_slots(op, dtype, n, lh, lh, cg, cd)
    assert slots == L.lib().p2p_brig_stat_slots(op, dtype, n, lh, lh, cg, cd) and slots >= 1
    out = E.DenseBuf(n, res, res, ncols, U.tdt(dtype), U.DEV)
    out.t.fill_(float("nan"))
    spart = torch.full((n * slots * ncols * 2,), float("nan"), dtype=torch.float32, device=U.DEV)
    hv, lv = (ab.view(), out.view()) if op == L.OP_G else (out.view(), ab.view())
    L.call("p2p_igemm", op, dtype, n, lh, lh, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wt if op == L.OP_G else wn), 1, None, U.ptr(spart),
           U.stream())
    _epilogue_checks(f"brig {'GP'[op]} {n}x{lh}x{lh} {cg},{cd} cbw{cbw}", dtype, n, res, res, ncols, out, spart, slots, NE.FUSED_RATIO)


def test_conv_strip_epilogue_statistics_of_an_offset_output():
    dtype, (op, n, lh, cg, cd) = L.BF16, NE.STRIP_CASE
    ratio = NE.CONV_RATIO[dtype]
    a, w, _ = NE.conv_operands(op, n, lh, lh, cg, cd, dtype, ratio)
    wn, _ = _weights(w, cg, cd, dtype)
    ab = U.halo_from(a, dtype)
    assert L.lib().p2p_conv_strip_ok(op, dtype, n, lh, lh, cg, cd)
    slots = L.lib().p2p_conv_strip_stat_slots(op, dtype, n, lh, lh, cg, cd)
    assert slots > 0
    out = E.DenseBuf(n, 2 * lh, 2 * lh, cg, U.tdt(dtype), U.DEV)
    out.t.fill_(float("nan"))
    spart = torch.full((n * slots * cg * 2,), float("nan"), dtype=torch.float32, device=U.DEV)
    L.call("p2p_conv_strip", op, dtype, n, lh, lh, cg, cd, C.byref(out.view()), C.byref(ab.view()), U.ptr(wn), U.ptr(spart), U.stream())
    _epilogue_checks(f"strip P {n}x{lh}x{lh} {cg}<-{cd}", dtype, n, 2 * lh, 2 * lh, cg, out, spart, slots, ratio)


@pytest.mark.parametrize("cbw", [1, 2])
@pytest.mark.parametrize("op,n,lh,cg,cd,act", NE.FUSED_CASES)
def test_fused_block_on_an_offset_output(op, n, lh, cg, cd, act, cbw, monkeypatch):
    """p2p_igemm_norm_act (convolution, statistics, normalisation and activation in one launch) on positive operands.  Against the
    f64 graph conv -> bf16 store -> InstanceNorm -> activation the bound is max(OUT_TOL, 3 x the deviation of the same graph in
    float32 on the CPU): an element of the convolution that sits on a bf16 rounding boundary falls either way with the order of the
    f32 sum, in torch as in the MFMAs.  Against its OWN stored convolution result the kernel has no such excuse: the statistics
    meet the bounds of check 1 (k = 0) and the output OUT_TOL."""
    dtype = L.BF16
    monkeypatch.setenv("P2P_BRIG_CBW", str(cbw))
    monkeypatch.setenv("P2P_BRIG_MIN_WG", "1")
    if cbw == 2 and (cg if op == L.OP_P else cd) % (64 if op == L.OP_P else 256):
        pytest.skip("the 64-channels-per-wave form needs whole 64 / 256 channel tiles")
    assert L.lib().p2p_igemm_norm_act_ok(op, dtype, n, lh, lh, cg, cd) == 1
    a, w, ratio = NE.conv_operands(op, n, lh, lh, cg, cd, dtype, NE.FUSED_RATIO, scale=NE.FUSED_SCALE)
    wn, wt = _weights(w, cg, cd, dtype)
    ab = U.halo_from(a, dtype)
    ncols, res = (cd, lh) if op == L.OP_G else (cg, 2 * lh)
    rng = np.random.default_rng(8)
    gamma = (1 + 0.2 * rng.normal(size=ncols)).astype(np.float32)
    beta = (0.2 * rng.normal(size=ncols)).astype(np.float32)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    raw = E.DenseBuf(n, res, res, ncols, U.tdt(dtype), U.DEV)
    raw.t.fill_(float("nan"))
    y = E.HaloBuf(n, res, res, ncols + 32, dtype, U.DEV)
    stats = torch.full((n, ncols, 2), float("nan"), dtype=torch.float32, device=U.DEV)
    hv, lv = (ab.view(), raw.view()) if op == L.OP_G else (raw.view(), ab.view())
    L.call("p2p_igemm_norm_act", op, dtype, n, lh, lh, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wt if op == L.OP_G else wn),
           U.ptr(g_d), U.ptr(b_d), NE.EPS, act, NE.ALPHA, C.byref(y.view(coff=32)), U.ptr(stats), U.stream())
    x = U.dense_to_np(raw)
    got = U.halo_to_np(y).astype(np.float64)
    assert np.isfinite(x).all() and not got[..., :32].any()
    got = got[..., 32:]
    st = stats.cpu().numpy().astype(np.float64)
    e_mu, e_rs = NE.given_stat_errors(st[..., 0], st[..., 1], *NE.stats64(x)[:2], x)
    err_own = NE.plane_err(got, NE.apply64(x, st[..., 0], st[..., 1], gamma, beta, act, None))
    ref64, dev32 = NE.fused_graphs(op, a, w, gamma, beta, act)
    dev_k = U.rel_err(got, ref64)
    bound = max(NE.OUT_TOL[dtype], 3 * dev32)
    print(f"\nEDGE fused {'GP'[op]} {n}x{lh}x{lh} {cg},{cd} cbw{cbw} mean/std {ratio:.0f}: mu/bound {e_mu.max():.2f} rs/bound {e_rs.max():.2f} own-statistics err/tol "
          f"{err_own / NE.OUT_TOL[dtype]:.2f}  graph deviation {dev_k:.2e} (float32 CPU graph {dev32:.2e}, bound {bound:.2e})")
    assert e_mu.max() <= 1.0 and e_rs.max() <= 1.0
    assert err_own <= NE.OUT_TOL[dtype]
    assert dev_k <= bound


# ---------------------------------------------------------------------------------------------------------------- B: losses
@pytest.mark.parametrize("pad8", [False, True], ids=["plain", "pad8"])
@pytest.mark.parametrize("dtype", NE.DTYPES, ids=["f32", "bf16"])
def test_bce_at_saturated_logits(dtype, pad8):
    """|x| > 88.7 overflows a naive exp; the stable form max(x,0) - xz + log1p(exp(-|x|)) and 1 / (1 + exp(-x)) stay finite"""
    n2, h = 6, 8
    nr = n2 // 2
    logits = NE.bce_logits(dtype, n2, h)
    lb = U.halo_from(logits, dtype)
    ch = 8 if pad8 else 1
    dld, dlg = E.HaloBuf(n2, h, h, ch, dtype, U.DEV), E.HaloBuf(n2 - nr, h, h, ch, dtype, U.DEV)
    part = torch.full((3 * 256,), float("nan"), dtype=torch.float32, device=U.DEV)
    loss = torch.zeros(4, dtype=torch.float32, device=U.DEV)
    inv = 1.0 / (nr * h * h)
    L.call("p2p_bce_logits_pad8" if pad8 else "p2p_bce_logits", dtype, n2, nr, h, h, C.byref(lb.view()), inv, C.byref(dld.view()),
           C.byref(dlg.view()), U.ptr(part), U.stream())
    L.call("p2p_loss_partials_sum", U.ptr(part), 3, U.ptr(loss), U.stream())
    x = logits.astype(np.float64)
    want = [NE.bce64(x[:nr], 1.0).mean(), NE.bce64(x[nr:], 0.0).mean(), NE.bce64(x[nr:], 1.0).mean()]
    got = loss.cpu().numpy()[:3]
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-5)
    s = NE.sigmoid64(x)
    gd = np.concatenate([(s[:nr] - 1.0), s[nr:]]) * inv
    gg = (s[nr:] - 1.0) * inv
    tol = 1e-5 if dtype == L.F32 else 6e-3
    got_d, got_g = U.halo_to_np(dld), U.halo_to_np(dlg)
    assert np.isfinite(got_d).all() and np.isfinite(got_g).all()
    assert not got_d[..., 1:].any() and not got_g[..., 1:].any()
    print(f"\nEDGE bce {DT[dtype]} pad8 {pad8}: losses rel {np.abs(got / want - 1).max():.1e} grads {U.rel_err(got_d[..., :1], gd):.1e} "
          f"{U.rel_err(got_g[..., :1], gg):.1e}")
    assert U.rel_err(got_d[..., :1], gd) < tol and U.rel_err(got_g[..., :1], gg) < tol


@pytest.mark.parametrize("form", ["fwd", "pair"])
@pytest.mark.parametrize("dtype", NE.DTYPES, ids=["f32", "bf16"])
def test_tanh_l1_at_saturation_and_exact_ties(dtype, form):
    """tanh(z) is exactly +-1 from |z| = 10 on (f32 and bf16 alike) and a sprite's background is exactly -1: fake == real there.  The
    L1 gradient at a tie is sign(0) = 0, so dz holds the other gradient sources alone, and exactly 0 where tanh saturated."""
    n, s, c = 3, 16, 4
    z, pos = NE.tanh_field(dtype, n, s, c)
    rng = np.random.default_rng(62)
    real0 = U.q(rng.uniform(-1, 1, size=(n, s, s, c)), dtype)
    src = U.q(rng.uniform(-1, 1, size=(n, s, s, 4)), dtype)
    gd_src = U.q(rng.normal(size=(n, s, s, 8)), dtype)
    gx = rng.normal(size=(n, s, s, 4)).astype(np.float32) * 0.1               # one f32 slab: the histogram gradient's source
    inv = 1.0 / (n * s * s * c)
    zb = U.halo_from(z, dtype)

    def forward(real):
        part = torch.full((256,), float("nan"), dtype=torch.float32, device=U.DEV)
        loss = torch.zeros(1, dtype=torch.float32, device=U.DEV)
        f32copy = torch.full((n, s, s, c), float("nan"), dtype=torch.float32, device=U.DEV)
        if form == "pair":
            rb = U.halo_from(np.concatenate([real, src], -1), dtype)
            fb = E.HaloBuf(n, s, s, 8, dtype, U.DEV)
            L.call("p2p_tanh_l1_fwd_pair", dtype, n, s, s, C.byref(zb.view()), C.byref(rb.view()), C.byref(fb.view()), inv, U.ptr(part),
                   U.ptr(f32copy), U.stream())
        else:
            rb = U.halo_from(real, dtype)
            fb = E.HaloBuf(n, s, s, c, dtype, U.DEV)
            L.call("p2p_tanh_l1_fwd", dtype, n, s, s, c, C.byref(zb.view()), C.byref(rb.view()), C.byref(fb.view()), inv, U.ptr(part),
                   U.ptr(f32copy), U.stream())
        L.call("p2p_loss_partials_sum", U.ptr(part), 1, U.ptr(loss), U.stream())
        return rb, fb, U.halo_to_np(fb), f32copy.cpu().numpy(), float(loss[0])

    _, _, fake, copy, l1 = forward(real0)
    assert np.isfinite(fake).all() and np.isfinite(copy).all()
    t64 = np.tanh(z.astype(np.float64))
    sat = np.abs(z) >= 10
    assert sat.sum() >= 8 * 8 and np.array_equal(fake[..., :c][sat], np.sign(z[sat])) and np.array_equal(copy[sat], np.sign(z[sat]))
    assert np.abs(copy - t64).max() < 1e-6 and U.rel_err(fake[..., :c], t64) < NE.OUT_TOL[dtype]
    if form == "pair":
        assert np.array_equal(fake[..., c:], src)
    want_l1 = np.abs(real0.astype(np.float64) - fake[..., :c]).mean()
    assert abs(l1 - want_l1) <= (1e-5 if dtype == L.F32 else 3e-3) * want_l1

    # exact ties on a quarter of the elements, the saturated ones among them
    tie = rng.random(size=z.shape) < 0.25
    tie.reshape(-1)[pos[3:].reshape(-1)[::2]] = True                       # every other copy of the |z| >= 10 edge values
    real = np.where(tie, fake[..., :c], real0).astype(np.float32)
    assert (tie & sat & (real == -1)).sum() >= 8 and (tie & sat & (real == 1)).sum() >= 8
    rb, fb, fake2, _, _ = forward(real)
    assert np.array_equal(fake2, fake if form == "fwd" else np.concatenate([fake[..., :c], src], -1))
    gsrc = E.DenseBuf(n, s, s, 8, U.tdt(dtype), U.DEV)
    gsrc.t.copy_(U.dev(gd_src.reshape(-1, 8), U.tdt(dtype)))
    gx_d = U.dev(gx.reshape(-1))
    gxs = L.GSrc(gx_d.data_ptr(), 2, 1, n * s * s * 4, 4, 0)
    lam = 100.0
    f = fake[..., :c].astype(np.float64)
    other = gd_src[..., :c].astype(np.float64) + gx
    want = (other + lam * inv * np.sign(f - real)) * (1 - f * f)
    ok = tie | (np.abs(f - real0) > 1e-2)                 # off the ties: test_losses' mask against a sign that bf16 rounding flips
    tol = 1e-5 if dtype == L.F32 else 1e-2
    for pad in (False, True):
        dzb = E.HaloBuf(n, s, s, 8 if pad else c, dtype, U.DEV)
        dzb.t.fill_(float("nan"))
        if pad:
            L.call("p2p_tanh_l1_bwd_pad8", dtype, n, s, s, C.byref(fb.view()), C.byref(rb.view()), C.byref(gsrc.gsrc()), C.byref(gxs),
                   lam * inv, C.byref(dzb.view()), U.stream())
        else:
            L.call("p2p_tanh_l1_bwd", dtype, n, s, s, c, C.byref(fb.view()), C.byref(rb.view()), C.byref(gsrc.gsrc()), C.byref(gxs),
                   lam * inv, C.byref(dzb.view()), U.stream())
        dz = U.halo_to_np(dzb).astype(np.float64)
        assert np.isfinite(dz).all() and (not pad or not dz[..., c:].any())
        dz = dz[..., :c]
        assert not dz[sat].any()                                               # 1 - t^2 = 0 exactly
        err = np.abs(dz - want)[ok].max() / np.abs(want).max()
        err_tie = np.abs(dz - other * (1 - f * f))[tie].max() / np.abs(want).max()
        print(f"\nEDGE tanh_l1 {DT[dtype]} {form} pad8 {pad}: dz {err:.1e} at the ties {err_tie:.1e} ({int(tie.sum())} ties, {int((tie & sat).sum())} saturated)")
        assert err < tol and err_tie < tol


# ---------------------------------------------------------------------------------------------------------------- C: Adam
@pytest.mark.parametrize("entry", ["p2p_adam_flat", "p2p_adam_flat_dev", "p2p_adam_flat_dev_excl", "p2p_adam_ema_flat_dev",
                                   "p2p_adam_ema_flat_dev_excl"])
def test_adam_on_degenerate_gradients(entry):
    """three steps over gradients of {0, +-1e-30, +-1e-18, +-1, +-1e15} mixed inside every 16-byte vector, n not a multiple of 4"""
    n, (lo, hi) = NE.ADAM_N, NE.ADAM_HOLE
    lr, b1, b2, eps = 2e-4, 0.5, 0.999, 1e-7
    rng = np.random.default_rng(63)
    p0 = rng.normal(size=n).astype(np.float32)
    g = NE.adam_gradients()
    excl, ema = entry.endswith("_excl"), "ema" in entry
    live = np.ones(n, bool)
    if excl:
        live[lo:hi] = False
    pd, md, vd = U.dev(p0), torch.zeros(n, device=U.DEV), torch.zeros(n, device=U.DEV)
    ed = pd.clone()
    t_dev = torch.zeros(1, dtype=torch.int32, device=U.DEV)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=U.DEV)
    ref = NE.adam_reference(p0, g, 3, lr, b1, b2, eps)
    e_ref = p0.copy()
    quiet, fading = slice(0, 64), slice(64, 128)
    prev_p = p0.copy()
    for t in (1, 2, 3):
        gd = U.dev(g[t - 1])
        L.call("p2p_adam_tick", U.ptr(t_dev), U.ptr(lr_dev), lr, b1, b2, U.stream())
        four = (U.ptr(pd), U.ptr(gd), U.ptr(md), U.ptr(vd))
        hyper = (U.ptr(lr_dev), b1, b2, eps, 1.0)
        if entry == "p2p_adam_flat":
            L.call(entry, *four, n, t, lr, b1, b2, eps, 1.0, U.stream())
        elif entry == "p2p_adam_flat_dev":
            L.call(entry, *four, n, *hyper, U.stream())
        elif entry == "p2p_adam_flat_dev_excl":
            L.call(entry, *four, n, lo, hi, *hyper, U.stream())
        elif entry == "p2p_adam_ema_flat_dev":
            L.call(entry, *four, U.ptr(ed), n, *hyper, U.ptr(t_dev), 0.999, 1, U.stream())
        else:
            L.call(entry, *four, U.ptr(ed), n, lo, hi, *hyper, U.ptr(t_dev), 0.999, 1, U.stream())
        p, m, v = (a.cpu().numpy() for a in (pd, md, vd))
        pr, mr, vr = ref[t - 1]
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
        np.testing.assert_allclose(p[live], pr[live], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(m[live], mr[live], rtol=1e-6, atol=NE.F32_TINY)
        np.testing.assert_allclose(v[live], vr[live], rtol=5e-5, atol=NE.F32_TINY)        # (1 - 0.999f) in f32, as keras does
        if excl:
            assert np.array_equal(p[~live], p0[~live]) and not m[~live].any() and not v[~live].any()
        # g = 0 on zero moments: nothing moves, bit for bit
        assert np.array_equal(p[quiet].view(np.int32), p0[quiet].view(np.int32))
        assert not m[quiet].view(np.int32).any() and not v[quiet].view(np.int32).any()
        if t > 1:       # g turned 0 after a non-zero step: the moments decay, the parameter keeps moving
            assert (np.abs(m[fading]) < np.abs(m_prev[fading])).all() and (v[fading] <= v_prev[fading]).all()
            moving = np.abs(pr[fading] - ref[t - 2][0][fading]) > 4 * np.spacing(np.abs(p0[fading]))
            assert moving.sum() >= 16 and (p[fading][moving] != prev_p[fading][moving]).all()
        m_prev, v_prev, prev_p = m.copy(), v.copy(), p.copy()
        if ema:
            e_ref = np.where(live, EO.ema_step(e_ref, p, t), e_ref)
            e = ed.cpu().numpy()
            assert np.isfinite(e).all() and np.array_equal(e.view(np.int32), e_ref.astype(np.float32).view(np.int32))
    print(f"\nEDGE adam {entry}: p max rel {np.abs(p[live] / pr[live] - 1).max():.1e}")


# ---------------------------------------------------------------------------------------------------------------- D: colour points
def _hist3(img, use_points, cap):
    N, S = img.shape[0], img.shape[1]
    t = U.dev(img)
    view = L.Tensor(t.data_ptr(), S * S, S, 4)
    raw = torch.empty(N * 3 * 64 * 64, dtype=torch.float32, device=U.DEV)
    ws = torch.empty(L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4, dtype=torch.float32, device=U.DEV)
    pts = torch.full((N, cap, 4), float("nan"), dtype=torch.float32, device=U.DEV)
    npts = torch.full((N,), -7, dtype=torch.int32, device=U.DEV)
    if use_points:
        L.call("p2p_rgbuv_points", L.F32, N, S, S, C.byref(view), cap, U.ptr(pts), U.ptr(npts), U.stream())
    L.call("p2p_rgbuv_hist_fwd3", L.F32, N, S, S, C.byref(view), U.ptr(pts) if use_points else None, U.ptr(npts) if use_points else None,
           cap, U.ptr(raw), U.ptr(ws), U.stream())
    out = torch.empty((N, 64, 64, 3), dtype=torch.float32, device=U.DEV)
    L.call("p2p_hist_normalize", U.ptr(raw), N, U.ptr(out), U.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64), npts.cpu().numpy(), pts.cpu().numpy()


@pytest.mark.parametrize("size", [32, 64])
def test_colour_lists_at_their_capacity_in_a_mixed_batch(size):
    """one batch that mixes listed and dense images, with cap = 64: exactly cap colours (listed), cap + 1 (dense), one colour, every
    pixel its own"""
    cap = 64
    img, want = NE.points_batch(size)
    ref = rg.rgbuv_histogram(torch.tensor(img, dtype=F64)).numpy()
    dense, _, _ = _hist3(img, False, cap)
    listed, npts, pts = _hist3(img, True, cap)
    assert npts.tolist() == want.tolist()
    for i in range(4):
        peak = ref[i].max()
        e_d, e_l, e_x = (np.abs(a - b).max() / peak for a, b in ((dense[i], ref[i]), (listed[i], ref[i]), (listed[i], dense[i])))
        print(f"\nEDGE points {size}x{size} image {i} npoints {npts[i]}: dense {e_d:.1e} listed {e_l:.1e} listed-dense {e_x:.1e}")
        assert e_d <= 1e-4 and e_l <= 1e-4 and e_x <= 1e-4
        if npts[i] > 0:
            k = int(npts[i])
            assert pts[i, :k, 3].sum() == size * size and (pts[i, :k, 3] >= 1).all()
            assert {tuple(r) for r in pts[i, :k, :3]} == {tuple(r) for r in img[i].reshape(-1, 4)[:, :3]}


def test_hellinger_gradient_with_saturated_channels():
    """the fused Hellinger backward for a fake batch that holds exact -1 and +1 channels (x = 0 and x = 1 after the shift: the
    log-chroma of a black channel is log(1e-6))"""
    B, size = 2, 32
    rng = np.random.default_rng(64)
    _, tgt = rg.synthetic_rgba_batch(rng, B, 64, palette_size=12)
    tgt = tgt[:, :size, :size]
    fake = np.clip(tgt + rng.normal(scale=0.05, size=tgt.shape), -1, 1).astype(np.float32)
    sel = rng.random(size=fake[..., :3].shape)
    fake[..., :3][sel < 0.15] = -1.0
    fake[..., :3][sel > 0.85] = 1.0
    fake[0, :4, :4, :3] = -1.0                   # whole black and whole white pixels too
    fake[1, :4, :4, :3] = 1.0
    ft = torch.tensor(fake, dtype=F64, requires_grad=True)
    real_h = rg.rgbuv_histogram(torch.tensor(tgt, dtype=F64))
    rg.hellinger_loss(real_h, rg.rgbuv_histogram(ft)).backward()
    ref = ft.grad.numpy()
    pad = lambda a: U.halo_from(np.concatenate([a, np.zeros_like(a)], -1), L.F32)       # noqa: E731
    rb, fb = pad(tgt), pad(fake)
    nh = B * 3 * 64 * 64
    h_r, h_f, gh = (torch.empty(nh, dtype=torch.float32, device=U.DEV) for _ in range(3))
    tot = torch.empty((2, B), dtype=torch.float32, device=U.DEV)
    sq, sqp = torch.zeros(4, dtype=torch.float32, device=U.DEV), torch.zeros(B, dtype=torch.float32, device=U.DEV)
    L.call("p2p_rgbuv_hist_fwd", L.F32, B, size, size, C.byref(rb.view()), U.ptr(h_r), U.stream())
    L.call("p2p_rgbuv_hist_fwd", L.F32, B, size, size, C.byref(fb.view()), U.ptr(h_f), U.stream())
    L.call("p2p_hellinger_fwd", U.ptr(h_r), U.ptr(h_f), B, U.ptr(tot[0]), U.ptr(tot[1]), U.ptr(sqp), U.ptr(sq), U.stream())
    one = torch.full((B * size * size * 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    L.call("p2p_rgbuv_hist_hellinger_bwd3", L.F32, B, size, size, C.byref(fb.view()), U.ptr(h_r), U.ptr(h_f), U.ptr(tot[0]),
           U.ptr(tot[1]), U.ptr(sq), 1.0 / (2.0 * math.sqrt(2.0) * B), U.ptr(gh), U.ptr(one), U.stream())
    got = one.view(B, size, size, 4).cpu().numpy()
    assert np.isfinite(got).all() and np.count_nonzero(got[..., 3]) == 0
    e_max, e_l2 = U.rel_err(got, ref), np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"\nEDGE hellinger saturated: max-norm {e_max:.1e} L2 {e_l2:.1e}")
    assert e_max < 2e-3 and e_l2 < 2e-3
