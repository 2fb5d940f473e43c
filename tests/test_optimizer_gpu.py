"""-m gpu: optimizer options.  The new entry points through the C ABI against the restatements of
tests/optimizer_oracle.py -- guard elements around every output, outputs filled with NaN, every launch twice with the second
bit-identical -- then the engine's steps (f32, B = 2, 64x64, injected dropout masks) against the restatement applied to the
step's own gradients, replayed, captured, data-parallel and class-level runs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import parallel as PAR
from palette_and_histo_gan_amd import pix2pix_model as M
from palette_and_histo_gan_amd import schedules as SCH
from tests import optimizer_oracle as OO

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4               # floats in front of and behind every device buffer (keeps 16-byte alignment)
B1, B2, EPS = 0.5, 0.999, 1e-7


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _guarded(values, fill=np.nan):
    """device tensor [guard | values | guard], the guards set to `fill`; returns (whole tensor, pointer of the payload)"""
    values = np.asarray(values)
    full = np.full(values.size + 2 * GUARD, fill, values.dtype)
    full[GUARD:GUARD + values.size] = values.reshape(-1)
    t = _dev(full)
    return t, t.data_ptr() + GUARD * t.element_size()


def _payload(t, n=None):
    a = t.cpu().numpy()
    return a[GUARD:len(a) - GUARD if n is None else GUARD + n]


def _guards_intact(t, fill_is_nan=True):
    a = t.cpu().numpy()
    g = np.concatenate([a[:GUARD], a[-GUARD:]])
    return bool(np.isnan(g).all()) if fill_is_nan else bool((g == g[0]).all())


def _bits(a):
    return np.asarray(a, F32).reshape(-1).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- p2p_adam_tick_sched
SCHEDULES = {
    "constant": (SCH.Constant(2e-4), (1, 2, 10_080)),
    "constant_warmup": (SCH.Constant(2e-4, warmup_steps=5), (1, 2, 5, 6, 7, 10_080)),
    "exponential": (SCH.ExponentialDecay(1e-3, 100, 0.5), (1, 2, 100, 101, 102, 10_080)),
    "exponential_staircase": (SCH.ExponentialDecay(1e-3, 100, 0.5, staircase=True), (1, 2, 100, 101, 102, 200, 201, 10_080)),
    "piecewise": (SCH.PiecewiseConstantDecay([10, 20, 30], [1e-3, 5e-4, 2.5e-4, 1e-4]), (1, 2, 10, 11, 12, 20, 21, 22, 30, 31, 32, 10_080)),
    "piecewise_8": (SCH.PiecewiseConstantDecay(list(range(1, 9)), [1e-3 / (k + 1) for k in range(9)]), (1, 2, 3, 8, 9, 10, 10_080)),
    "polynomial": (SCH.PolynomialDecay(1e-2, 100, end_learning_rate=1e-4, power=2.0), (1, 2, 100, 101, 102, 10_080)),
    "polynomial_cycle": (SCH.PolynomialDecay(1e-2, 100, end_learning_rate=1e-4, power=0.5, cycle=True), (1, 2, 100, 101, 102, 10_080)),
    "cosine": (SCH.CosineDecay(2e-4, 100, alpha=0.05), (1, 2, 51, 100, 101, 102, 10_080)),
    "linear": (SCH.LinearDecay(2e-4, 100, 100), (1, 2, 100, 101, 102, 200, 201, 202, 10_080)),
    "linear_warmup": (SCH.LinearDecay(2e-4, 8, 8, end=1e-5, warmup_steps=4), (1, 2, 4, 5, 8, 9, 10, 16, 17, 18, 10_080)),
}


def _tick(entry, t, *args):
    """one launch from t_dev = t - 1: (t_dev after, lr_t_dev after), guards checked"""
    td, tp = _guarded(np.array([t - 1], np.int32), fill=-7)
    ld, lp = _guarded(np.array([np.nan], F32))
    L.call(entry, tp, lp, *args, _stream())
    torch.cuda.synchronize()
    assert _guards_intact(td, False) and _guards_intact(ld)
    return int(_payload(td)[0]), _payload(ld)[0]


@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_tick_sched_follows_every_schedule_kind(kind):
    """lr_t_dev against the float64 restatement rounded to float32: at most 1 ulp apart (the device's f64 pow and cos are not
    correctly rounded); t = 1, 2, the steps around every boundary (the schedule is read at t - 1), 10 080"""
    sched, steps = SCHEDULES[kind]
    s = sched.struct()
    worst = 0
    for t in steps:
        t1, got = _tick("p2p_adam_tick_sched", t, C.byref(s), B1, B2)
        t2, again = _tick("p2p_adam_tick_sched", t, C.byref(s), B1, B2)
        want = OO.lr_t(sched, t, B1, B2)
        d = OO.ulps(got, want)
        print(f"{kind} t {t}: lr {sched(t - 1):.9g} lr_t {got!r} want {want!r} ulps {d}")
        assert t1 == t2 == t and _same(got, again)
        assert np.isfinite(got) and d <= 1, (kind, t, got, want)
        worst = max(worst, d)
    print(f"{kind}: worst {worst} ulp")


def test_constant_schedule_is_p2p_adam_tick_bit_for_bit():
    for lr, b1, b2 in ((2e-4, 0.5, 0.999), (4e-4, 0.0, 0.999), (1e-3, 0.9, 0.99)):
        s = SCH.Constant(float(F32(lr))).struct()          # the float32 rate p2p_adam_tick receives
        for t in (1, 2, 3, 17, 1000, 10_080):
            _, a = _tick("p2p_adam_tick", t, lr, b1, b2)
            _, b = _tick("p2p_adam_tick_sched", t, C.byref(s), b1, b2)
            assert _same(a, b), (lr, b1, b2, t, a, b)


# ---------------------------------------------------------------------------------------------------------------- global norm
SWEEP = 4 * 256 * L.SUMSQ_MAX_PARTS                     # elements of one sweep of the capped grid
NORM_CASES = [(1, None), (3, None), (4, None), (5, None), (255, None), (1023, None), (1025, None), (SWEEP + 4 * 256 + 3, None),
              (4099, (1001, 2050)),                     # unaligned at both ends
              (4099, (1026, 1029)),                     # cuts two vectors and holds none
              (SWEEP + 1025, (5, SWEEP - 3))]           # nearly everything, across the sweep


def _norm_launch(g, hole, clipnorm):
    n = g.size
    gd, gp = _guarded(g)
    pd, pp = _guarded(np.full(L.SUMSQ_MAX_PARTS, np.nan, F32))
    sd, sp = _guarded(np.array([np.nan, np.nan], F32))           # [scale, norm]
    nparts, parts = (C.c_int * 1)(-1), (C.c_void_p * 1)(pp)
    lo, hi = hole or (0, 0)
    L.call("p2p_sumsq_partials", gp, n, lo, hi, pp, nparts, _stream())
    L.call("p2p_clip_scale", parts, nparts, 1, clipnorm, sp, sp + 4, _stream())
    torch.cuda.synchronize()
    assert _guards_intact(gd) and _guards_intact(pd) and _guards_intact(sd)
    return nparts[0], _payload(pd), _payload(sd)


@pytest.mark.parametrize("n,hole", NORM_CASES)
def test_global_norm_and_scale_equal_the_float32_restatement(n, hole):
    rng = np.random.default_rng(n)
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 1, size=n)).astype(F32)
    if hole:
        g[hole[0]:hole[1]] = np.nan                     # the hole is never looked at: anything there must not matter
    want_parts = OO.sumsq_partials(g, *(hole or (0, 0)))
    want_norm = OO.global_norm([want_parts])
    assert np.isfinite(want_norm) and want_norm > 0
    for factor in (0.5, 2.0, 1.0):
        clip = F32(factor) * want_norm
        nb, parts, (scale, norm) = _norm_launch(g, hole, clip)
        nb2, parts2, (scale2, norm2) = _norm_launch(g, hole, clip)
        assert nb == nb2 == want_parts.size == OO.sumsq_grid(n)[1]
        assert _same(parts[:nb], want_parts) and np.isnan(parts[nb:]).all()
        assert _same(parts[:nb], parts2[:nb]) and _same(scale, scale2) and _same(norm, norm2)
        assert _same(norm, want_norm), (norm, want_norm)
        assert _same(scale, OO.clip_scale(want_norm, clip))
        if factor == 0.5:
            assert scale < 1.0
        else:
            assert scale == F32(1.0)                    # exactly 1 below AND at the threshold


def test_a_non_finite_gradient_gives_a_nan_scale_and_two_buffers_concatenate():
    rng = np.random.default_rng(0)
    g = rng.normal(size=2000).astype(F32)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[777] = bad
        _, _, (scale, norm) = _norm_launch(h, None, 1.0)
        assert np.isnan(scale) and not np.isfinite(norm)
    # two gradient buffers behind one scale: the partial lists are concatenated in argument order
    a, b = rng.normal(size=70_001).astype(F32), rng.normal(size=513).astype(F32)
    bufs = [_guarded(x) for x in (a, b)]
    outs = [_guarded(np.full(L.SUMSQ_MAX_PARTS, np.nan, F32)) for _ in bufs]
    sd, sp = _guarded(np.array([np.nan, np.nan], F32))
    counts, ptrs = (C.c_int * 2)(), (C.c_void_p * 2)(outs[0][1], outs[1][1])
    for k, x in enumerate((a, b)):
        one = (C.c_int * 1)()
        L.call("p2p_sumsq_partials", bufs[k][1], x.size, 0, 0, outs[k][1], one, _stream())
        counts[k] = one[0]
    L.call("p2p_clip_scale", ptrs, counts, 2, 1.0, sp, sp + 4, _stream())
    torch.cuda.synchronize()
    want = OO.global_norm([OO.sumsq_partials(a), OO.sumsq_partials(b)])
    scale, norm = _payload(sd)
    assert _same(norm, want) and _same(scale, OO.clip_scale(want, 1.0)) and scale < 1.0
    assert abs(float(norm) - float(np.sqrt((a.astype(np.float64) ** 2).sum() + (b.astype(np.float64) ** 2).sum()))) < 1e-3 * float(norm)


# ---------------------------------------------------------------------------------------------------------------- p2p_adam_step
def _adam_state(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=n).astype(F32)
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 0, size=n)).astype(F32)
    m = (0.1 * rng.normal(size=n)).astype(F32)
    v = (rng.uniform(0, 1e-2, size=n)).astype(F32)
    e = (p + 0.01 * rng.normal(size=n)).astype(F32)
    return p, g, m, v, e


def _run_adam(entry, state, hole, ema, t=3, lr_t=1.7e-4, gscale=None, clipvalue=0.0, decay=0.99, warmup=1):
    """one launch of `entry` ("step" or one of the four flat entry points) on fresh guarded copies: (p, m, v, e) after; `gscale`
    reaches "step" as a device scalar and a flat entry point by value"""
    p, g, m, v, e = state
    n = p.size
    bufs = [_guarded(x) for x in (p, g, m, v, e)]
    lrd, lrp = _guarded(np.array([lr_t], F32))
    td, tp = _guarded(np.array([t], np.int32), fill=-7)
    sd, sp = _guarded(np.array([1.0 if gscale is None else gscale], F32))
    ptr = [b[1] for b in bufs]
    lo, hi = hole or (0, 0)
    if entry == "step":
        h = L.AdamHyper(B1, B2, EPS, clipvalue, decay)
        a = L.AdamArgs(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4] if ema else None, n, lo, hi, lrp, sp if gscale is not None else None, tp,
                       C.pointer(h), warmup if ema else 0, 0)
        L.call("p2p_adam_step", C.byref(a), _stream())
    else:
        name = "p2p_adam" + ("_ema" if ema else "") + "_flat_dev" + ("_excl" if hole else "")
        args = ptr[:4] + ([ptr[4]] if ema else []) + [n] + ([lo, hi] if hole else []) + [lrp, B1, B2, EPS, 1.0 if gscale is None else gscale]
        args += [tp, decay, warmup] if ema else []
        L.call(name, *args, _stream())
    torch.cuda.synchronize()
    for b, _ in bufs + [(lrd, 0), (sd, 0)]:
        assert _guards_intact(b)
    assert _same(_payload(bufs[1][0]), g)            # the gradient is read only
    return [_payload(bufs[k][0]) for k in (0, 2, 3, 4)]


@pytest.mark.parametrize("n", [5, 1024, 4099])
@pytest.mark.parametrize("hole", [False, True])
@pytest.mark.parametrize("ema", [False, True])
def test_adam_step_with_options_off_is_the_entry_point_it_generalises(n, hole, ema):
    state = _adam_state(n, n)
    ex = None if not hole else {5: (1, 3), 1024: (130, 517), 4099: (1001, 2050)}[n]
    old = _run_adam("flat", state, ex, ema)
    new = _run_adam("step", state, ex, ema)
    again = _run_adam("step", state, ex, ema)
    one = _run_adam("step", state, ex, ema, gscale=1.0)           # a device scale of exactly 1 is no scale
    for k, name in enumerate("pmve"):
        assert _same(old[k], new[k]) and _same(new[k], again[k]) and _same(new[k], one[k]), name
    p, g, m, v, e = state
    assert not _same(new[0], p)
    if ex:
        for k, x in enumerate((p, m, v, e)):
            assert _same(new[k][ex[0]:ex[1]], x[ex[0]:ex[1]])
    if not ema:
        assert _same(new[3], e)
    # and both are the restatement
    wp, wm, wv = OO.adam_flat(p, g, m, v, 1.7e-4, B1, B2, EPS, hole=ex)
    assert _same(new[0], wp) and _same(new[1], wm) and _same(new[2], wv)
    if ema:
        we = OO.ema_element(e, wp, 3, 0.99, 1)
        if ex:
            we[ex[0]:ex[1]] = e[ex[0]:ex[1]]
        assert _same(new[3], we)


@pytest.mark.parametrize("n,hole", [(5, None), (1024, None), (4099, (1001, 2050))])
def test_adam_step_gradient_options_equal_the_restatement(n, hole):
    p, g, m, v, e = state = _adam_state(n, 100 + n)
    c = float(np.median(np.abs(g)))
    g[0], g[1 % n], g[n - 1] = c, -c, np.nextafter(F32(c), F32(1))          # exactly at +c and -c, one ulp above
    # clipvalue
    got = _run_adam("step", state, hole, True, clipvalue=c)
    again = _run_adam("step", state, hole, True, clipvalue=c)
    wp, wm, wv = OO.adam_flat(p, g, m, v, 1.7e-4, B1, B2, EPS, clipvalue=c, hole=hole)
    assert all(_same(a, b) for a, b in zip(got, again))
    assert _same(got[0], wp) and _same(got[1], wm) and _same(got[2], wv)
    if n > 5:           # (at n = 5 the only element beyond c is the one a single ulp above it)
        off = _run_adam("step", state, hole, True)
        assert not _same(got[0], off[0])
    # a device scale: an ordinary one, and one that takes the small gradients into the denormals (m starts at 0 there so that the
    # denormal reaches the moments alone)
    for scale, m0 in ((0.37, m), (2.0 ** -120, np.zeros_like(m))):
        st = (p, g, m0, v, e)
        got = _run_adam("step", st, hole, False, gscale=scale)
        again = _run_adam("step", st, hole, False, gscale=scale)
        wp, wm, wv = OO.adam_flat(p, g, m0, v, 1.7e-4, B1, B2, EPS, gscale=scale, hole=hole)
        assert all(_same(a, b) for a, b in zip(got, again))
        assert _same(got[0], wp) and _same(got[1], wm) and _same(got[2], wv), scale
        if scale < 1e-30:
            live = np.ones(n, bool)
            if hole:
                live[hole[0]:hole[1]] = False
            tiny = np.abs(wm[live & (wm != 0)])
            assert tiny.size and tiny.min() < np.finfo(F32).tiny       # denormal moments were really produced and kept
    # a NaN scale (non-finite norm) poisons every live element, as tf.clip_by_global_norm's does
    got = _run_adam("step", state, hole, False, gscale=np.nan)
    live = np.ones(n, bool)
    if hole:
        live[hole[0]:hole[1]] = False
    assert np.isnan(got[0][live]).all() and _same(got[0][~live], p[~live])


# One whole sweep of the capped grid (8192 workgroups of 256 lanes, one 16-byte vector each), one more workgroup's worth of vectors
# and a 3-element tail: the lanes of the first workgroup walk on to a second vector, everyone else stops after one.  The holes take
# out fewer than 256 vectors, so the grid stays capped and the second sweep is still there.
ADAM_SWEEP = 8192 * 256 * 4
ADAM_N = ADAM_SWEEP + 4 * 256 + 3
ADAM_SWEEP_HOLES = {"no_hole": None,
                    "across_the_sweep": (ADAM_SWEEP - 100, ADAM_SWEEP + 200),         # whole vectors on both sides of the boundary
                    "unaligned_ends": (1001, 1502)}                                   # cuts a vector at either end
SWEEP_SCALE = 0.37


@pytest.fixture(scope="module")
def sweep_case():
    """the state, the clip threshold and the restatement's (p, m, v) without a hole for the three gradient forms, computed once"""
    state = _adam_state(ADAM_N, 7)
    p, g, m, v, e = state
    c = float(np.median(np.abs(g)))
    want = {"plain": OO.adam_flat(p, g, m, v, 1.7e-4, B1, B2, EPS),
            "clipvalue": OO.adam_flat(p, g, m, v, 1.7e-4, B1, B2, EPS, clipvalue=c),
            "scale": OO.adam_flat(p, g, m, v, 1.7e-4, B1, B2, EPS, gscale=SWEEP_SCALE)}
    for a in state + tuple(x for w in want.values() for x in w):
        a.setflags(write=False)
    return state, c, want


@pytest.mark.parametrize("hole", list(ADAM_SWEEP_HOLES))
def test_adam_past_one_sweep_of_the_capped_grid(sweep_case, hole):
    """every flat entry point (scale 1, and a scale by value) and p2p_adam_step (clipvalue with the average, a device scale
    without) at an n the capped grid covers in two sweeps: the restatement's bits outside the hole, the hole and the guards
    untouched"""
    state, c, want = sweep_case
    ex = ADAM_SWEEP_HOLES[hole]
    live = np.ones(ADAM_N, bool)
    if ex:
        live[ex[0]:ex[1]] = False
    assert ADAM_N // 4 - (~live).sum() // 4 > ADAM_SWEEP // 4           # more live vectors than lanes in the capped grid
    runs = [("flat", "plain", False, {}), ("flat", "plain", True, {}),
            ("step", "clipvalue", True, {"clipvalue": c}), ("step", "scale", False, {"gscale": SWEEP_SCALE}),
            ("flat", "scale", False, {"gscale": SWEEP_SCALE})]
    for entry, form, ema, opts in runs:
        got = _run_adam(entry, state, ex, ema, **opts)
        wp, wm, wv = want[form]
        we = OO.ema_element(state[4], wp, 3, 0.99, 1) if ema else state[4]
        for name, new, restated, before in zip("pmve", got, (wp, wm, wv, we), (state[0], state[2], state[3], state[4])):
            assert _same(new[live], restated[live]), (entry, form, ema, name)
            assert _same(new[~live], before[~live]), (entry, form, ema, name, "the hole was written")


# ---------------------------------------------------------------------------------------------------------------- engine
S, BATCH = 64, 2


class _Case:
    """one f32 engine state and batch; the gradients of the step from that state (apply_update=False) and the parameters a
    default step leaves, computed once and shared"""

    def __init__(self):
        rng = np.random.default_rng(21)
        Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, torch.float64), rng)
        Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, torch.float64), rng)
        self.params = ({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
        self.src, self.tgt = rg.synthetic_rgba_batch(rng, BATCH, S)
        self.masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(BATCH, S)]
        eng = self.engine()
        self.p0 = {"G": eng.G.params.cpu().numpy().copy(), "D": eng.D.params.cpu().numpy().copy()}
        eng.train_step_rgba(self.src, self.tgt, 100.0, masks=self.masks, apply_update=False)
        torch.cuda.synchronize()
        self.g = {"G": eng.G.grads.cpu().numpy().copy(), "D": eng.D.grads.cpu().numpy().copy()}
        self.norm64 = {k: float(np.sqrt((g.astype(np.float64) ** 2).sum())) for k, g in self.g.items()}
        self.step(eng)
        self.default = {"G": eng.G.params.cpu().numpy().copy(), "D": eng.D.params.cpu().numpy().copy()}
        assert _same(eng.G.grads.cpu().numpy(), self.g["G"]) and _same(eng.D.grads.cpu().numpy(), self.g["D"])

    def engine(self):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
        eng.set_params(*self.params)
        return eng

    def step(self, eng):
        out = eng.train_step_rgba(self.src, self.tgt, 100.0, masks=self.masks)
        torch.cuda.synchronize()
        return out

    def restated(self, eng, sid, gscale=1.0, clipvalue=0.0, t=1):
        """the parameters of store `sid` after the first step from p0, by the restatement applied to the shared gradients with
        the step size the device holds (lr_t_dev has its own test)"""
        store = eng.G if sid == "G" else eng.D
        h = store.opt.hyper
        zeros = np.zeros_like(self.p0[sid])
        return OO.adam_flat(self.p0[sid], self.g[sid], zeros, zeros, float(store.lr_t_dev[0]), h.beta1, h.beta2, h.eps, gscale, clipvalue)


@pytest.fixture(scope="module")
def case():
    return _Case()


def _params(eng):
    return {"G": eng.G.params.cpu().numpy(), "D": eng.D.params.cpu().numpy()}


def test_engine_global_clipnorm_that_binds(case):
    eng = case.engine()
    want = {}
    for sid, store in (("G", eng.G), ("D", eng.D)):
        eng.set_optimizer(store, clipping=(None, 0.5 * case.norm64[sid]))
        norm = OO.global_norm([OO.sumsq_partials(case.g[sid])])
        want[sid] = (norm, OO.clip_scale(norm, F32(0.5 * case.norm64[sid])))
        assert abs(float(norm) - case.norm64[sid]) <= OO.sumsq_error_bound(case.g[sid].size)[2] * case.norm64[sid]
    case.step(eng)
    got = _params(eng)
    for sid, store in (("G", eng.G), ("D", eng.D)):
        norm, scale = want[sid]
        assert scale < 1.0
        assert _same(store.opt.norm_dev.cpu().numpy(), norm) and _same(store.opt.scale_dev.cpu().numpy(), scale), sid
        p, m, v = case.restated(eng, sid, gscale=scale)
        assert _same(got[sid], p) and _same(store.m.cpu().numpy(), m) and _same(store.v.cpu().numpy(), v), sid
        assert not _same(got[sid], case.default[sid])


def test_engine_global_clipnorm_that_does_not_bind_is_a_default_step(case):
    eng = case.engine()
    for sid, store in (("G", eng.G), ("D", eng.D)):
        eng.set_optimizer(store, clipping=(None, 2.0 * case.norm64[sid]))
    case.step(eng)
    got = _params(eng)
    for sid, store in (("G", eng.G), ("D", eng.D)):
        assert float(store.opt.scale_dev[0]) == 1.0
        assert _same(store.opt.norm_dev.cpu().numpy(), OO.global_norm([OO.sumsq_partials(case.g[sid])]))
        assert _same(got[sid], case.default[sid]), sid


def test_engine_clipvalue_at_the_median(case):
    eng = case.engine()
    c = {sid: float(np.median(np.abs(case.g[sid]))) for sid in "GD"}
    for sid, store in (("G", eng.G), ("D", eng.D)):
        eng.set_optimizer(store, clipping=(c[sid], None))
    case.step(eng)
    got = _params(eng)
    for sid in "GD":
        assert c[sid] > 0
        p, _, _ = case.restated(eng, sid, clipvalue=c[sid])
        assert _same(got[sid], p), sid
        assert not _same(got[sid], case.default[sid])


def test_engine_discriminator_with_its_own_rate_and_beta(case):
    eng = case.engine()
    eng.set_optimizer(eng.D, learning_rate=4e-4, beta1=0.0)
    case.step(eng)
    got = _params(eng)
    assert _same(got["G"], case.default["G"])                           # the generator's optimizer is untouched
    assert OO.ulps(float(eng.D.lr_t_dev[0]), OO.lr_t(4e-4, 1, 0.0, B2)) <= 1 and OO.ulps(float(eng.G.lr_t_dev[0]), OO.lr_t(2e-4, 1, B1, B2)) <= 1
    p, _, _ = case.restated(eng, "D")
    assert eng.D.opt.hyper.beta1 == 0.0 and _same(got["D"], p) and not _same(got["D"], case.default["D"])
    # and the default step itself is the restatement with both options off
    ref = case.engine()
    case.step(ref)
    for sid in "GD":
        assert _same(case.default[sid], case.restated(ref, sid)[0]), sid


def test_engine_linear_decay_on_the_generator(case):
    eng = case.engine()
    sched = SCH.LinearDecay(2e-4, 2, 2)
    eng.set_optimizer(eng.G, learning_rate=sched)
    for t in range(1, 5):
        case.step(eng)
        got, want = F32(float(eng.G.lr_t_dev[0])), OO.lr_t(sched, t, B1, B2)
        print(f"t {t}: rate {sched(t - 1):.6g} lr_t {got!r} want {want!r} ulps {OO.ulps(got, want)}")
        assert _same(got, want), (t, got, want)
        assert eng.lr == sched(t)                                       # the rate of the step that follows
        assert OO.ulps(float(eng.D.lr_t_dev[0]), OO.lr_t(2e-4, t, B1, B2)) <= 1
    assert [sched(t) for t in range(5)] == [2e-4, 2e-4, 2e-4, 1e-4, 0.0]  # what the four steps ran at, and what a fifth would


# ---------------------------------------------------------------------------------------------------------------- replay, graph
def test_replayed_steps_with_a_schedule_and_clipping_equal_steps_issued_from_python():
    Bt = 4
    batches = list(DU.synthetic_rgba_ds(5 * Bt, batch_size=Bt, palette_size=24, seed=4))
    runs = []
    for replay in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=5)
        eng.replay_enabled = replay
        for store in (eng.G, eng.D):
            eng.set_optimizer(store, learning_rate=SCH.ExponentialDecay(2e-4, 2, 0.5), clipping=(None, 0.05))
        losses, norms, recorded = [], [], None
        for t, b in enumerate(batches):
            if t == 3:          # another schedule object and threshold: slots, no new recording
                recorded = len(eng._replays)
                eng.set_optimizer(eng.G, learning_rate=SCH.CosineDecay(3e-4, 10), clipping=(None, 0.02))
            losses.append(eng.train_step_rgba(b[0], b[1], 100.0))
            norms.append(torch.stack([eng.G.opt.norm_dev[0], eng.G.opt.scale_dev[0], eng.G.lr_t_dev[0], eng.D.lr_t_dev[0]]).clone())
        torch.cuda.synchronize()
        if replay:
            assert recorded == 1 and len(eng._replays) == 1
            names = [n for n, _ in next(iter(eng._replays.values()))[1] if n is not None]
            assert names.count("p2p_adam_tick_sched") == 2 and names.count("p2p_clip_scale") == 2 and "p2p_adam_tick" not in names
        else:
            assert len(eng._replays) == 0
        runs.append((torch.stack(losses).cpu(), torch.stack(norms).cpu(), eng))
    (la, na, a), (lb, nb, b) = runs
    assert torch.equal(la, lb) and torch.equal(na, nb), (la - lb).abs().max()
    assert float(na[:, 1].max()) < 1.0                                  # the clipping was binding
    for t in range(5):
        sched = SCH.ExponentialDecay(2e-4, 2, 0.5) if t < 3 else SCH.CosineDecay(3e-4, 10)
        assert OO.ulps(float(na[t, 2]), OO.lr_t(sched, t + 1, B1, B2)) <= 1, t
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf


def test_a_captured_graph_follows_the_schedule():
    eng = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=12)
    sched = SCH.LinearDecay(2e-4, 0, 2, end=2e-5)
    eng.set_optimizer(eng.G, learning_rate=sched)
    src, tgt = next(iter(DU.synthetic_rgba_ds(BATCH, batch_size=BATCH, palette_size=24, seed=11)))
    step = eng.graphed_rgba_step(BATCH, 100.0)
    assert eng.G.t == 0 and int(eng.G.t_dev[0]) == 0
    rates = []
    for t in range(1, 4):
        step(torch.as_tensor(src).cuda(), torch.as_tensor(tgt).cuda())
        torch.cuda.synchronize()
        assert int(eng.G.t_dev[0]) == t == eng.G.t
        rates.append(float(eng.G.lr_t_dev[0]))
        assert OO.ulps(rates[-1], OO.lr_t(sched, t, B1, B2)) <= 1, (t, rates)
    assert len({sched(t) for t in range(3)}) == 3                      # three different rates


# ---------------------------------------------------------------------------------------------------------------- data parallel
def _dp_worker(rank, world, port, q, tmp):
    import faulthandler
    import sys
    faulthandler.dump_traceback_later(int(os.environ.get("P2P_TEST_DUMP_AFTER", "240")), exit=True, file=sys.stderr)
    os.chdir(tmp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    try:
        comm = PAR.DataParallel("cuda:0", backend="gloo")
        batches = list(DU.synthetic_rgba_ds(8, batch_size=4, palette_size=24, seed=9))          # global batch 4: 2 per rank
        m = M.Pix2PixModel(None, None, "front2right", "dp-clip-test", 100.0, dtype="f32", data_parallel=comm, seed=5,
                           generator_optimizer=M.Adam(2e-4, beta_1=0.5, global_clipnorm=0.05),
                           discriminator_optimizer=M.Adam(2e-4, beta_1=0.5, global_clipnorm=1e-3))
        norms = []
        for k, b in enumerate(batches):
            m.train_step(b, k, 1)
            norms.append([float(m.generator_optimizer.last_global_norm), float(m.discriminator_optimizer.last_global_norm),
                          float(m.engine.G.opt.scale_dev[0]), float(m.engine.D.opt.scale_dev[0])])
        torch.cuda.synchronize()
        q.put(("ok", rank, m.engine.G.params.cpu().numpy().copy(), m.engine.D.params.cpu().numpy().copy(), np.array(norms, F32)))
        comm.barrier()
        comm.destroy()
    except BaseException:
        import traceback
        q.put(("error", rank, traceback.format_exc()))
        q.close()
        q.join_thread()
        os._exit(1)
    q.close()
    q.join_thread()
    os._exit(0)


@pytest.mark.timeout(600)
def test_two_ranks_clip_by_the_same_norm(tmp_path, monkeypatch):
    """each rank takes the norm of the all-reduced gradient: the same values in the same order, the same scale, no collective"""
    monkeypatch.chdir(tmp_path)
    world, port = 2, 29691
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        item = q.get(timeout=300)
        if item[0] == "error":
            for p in procs:
                p.kill()
            pytest.fail(f"rank {item[1]} failed:\n{item[2]}")
        got[item[1]] = item[2:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    (g0, d0, n0), (g1, d1, n1) = got[0], got[1]
    assert _same(g0, g1) and _same(d0, d1) and _same(n0, n1)
    assert n0.shape == (2, 4) and (n0[:, 2:] < 1.0).all() and np.isfinite(n0).all()          # both norms were binding in both steps


# ---------------------------------------------------------------------------------------------------------------- classes
def _model(train, name, **kw):
    return M.Pix2PixModel(train, train, "front2right", name, lambda_l1=100.0, dtype="f32", seed=47,
                          discriminator_optimizer=M.Adam(4e-4, beta_1=0.5),
                          generator_optimizer=M.Adam(SCH.LinearDecay(2e-4, 2, 2), beta_1=0.5, global_clipnorm=1.0), **kw)


def test_model_classes_take_optimizers_log_them_and_resume(tmp_path, monkeypatch):
    import json
    monkeypatch.chdir(tmp_path)
    train = DU.synthetic_rgba_ds(4, batch_size=2)
    a = _model(train, "optim-a")
    assert a.engine.D.opt.lr.value == F32(4e-4) and a.engine.G.opt.scheduled and a.engine.G.opt.clipnorm.value == 1.0
    a.fit(4, 2)
    rows = [json.loads(x) for x in open(a.summary_writer.path)]
    names = {r["name"] for r in rows}
    assert {"generator/learning_rate", "generator/gradient_norm"} <= names
    assert "discriminator/learning_rate" not in names and "discriminator/gradient_norm" not in names      # a plain rate, no clipping
    rates = [r["value"] for r in rows if r["name"] == "generator/learning_rate"]
    assert rates[:4] == [2e-4, 2e-4, 2e-4, 1e-4][:len(rates)] and all(r["value"] > 0 for r in rows if r["name"] == "generator/gradient_norm")
    st = a.checkpoint.state()
    assert st["optimizer"]["generator"]["global_clipnorm"] == 1.0 and st["optimizer"]["discriminator"]["learning_rate"] == 4e-4
    assert st["optimizer"]["generator"]["learning_rate"].startswith("LinearDecay(")
    assert {k for k in st if k != "optimizer"} == {"G", "G.m", "G.v", "G.t", "D", "D.m", "D.v", "D.t", "mask_counter", "step_count"}

    # a checkpoint at step 2, resumed in a fresh model, ends where the uninterrupted run ends
    batches = list(iter(train)) * 2
    b, c = _model(train, "optim-b"), _model(train, "optim-c")
    for k in range(4):
        b.train_step(batches[k], k, 1)
        if k == 1:
            path = b.checkpoint.save(str(tmp_path / "mid.pt"))
    c.checkpoint.restore(path)
    assert c.generator_optimizer.iterations == 2
    for k in range(2, 4):
        c.train_step(batches[k], k, 1)
    torch.cuda.synchronize()
    for sb, sc in ((b.engine.G, c.engine.G), (b.engine.D, c.engine.D)):
        for buf in ("params", "m", "v", "lr_t_dev"):
            assert torch.equal(getattr(sb, buf), getattr(sc, buf)), buf
    # restoring into a model built with other settings is accepted and warns once
    d = M.Pix2PixModel(train, train, "front2right", "optim-d", lambda_l1=100.0, dtype="f32", seed=47)
    with pytest.warns(UserWarning, match="other optimizer settings"):
        d.checkpoint.restore(path)
    assert "optimizer" not in d.checkpoint.state() and d.generator_optimizer.last_global_norm is None

    # attributes of a bound optimizer write through: the next step runs at the new rate, with no new recording
    before = float(c.engine.D.lr_t_dev[0])
    recorded = len(c.engine._replays)
    c.discriminator_optimizer.learning_rate = 8e-4
    assert c.discriminator_optimizer.learning_rate == 8e-4 and c.engine.D.opt.lr.value == F32(8e-4)
    c.train_step(batches[0], 4, 1)
    torch.cuda.synchronize()
    after = float(c.engine.D.lr_t_dev[0])
    assert OO.ulps(after, OO.lr_t(8e-4, 5, B1, B2)) <= 1 and after > 1.9 * before and len(c.engine._replays) == recorded
    c.generator_optimizer.learning_rate = SCH.Constant(1e-4, warmup_steps=100)
    c.train_step(batches[1], 5, 1)
    assert OO.ulps(float(c.engine.G.lr_t_dev[0]), OO.lr_t(SCH.Constant(1e-4, warmup_steps=100), 6, B1, B2)) <= 1
    with pytest.raises(ValueError):
        c.generator_optimizer.clipvalue = 0.1          # beside global_clipnorm
    assert c.generator_optimizer.clipvalue is None and not c.engine.G.opt.clipvalue_on
