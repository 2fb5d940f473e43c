"""-m gpu: Pix2PixEngine.elide_dead_bottleneck.  The encoder block that normalises a 1x1 map puts out
act(beta) and passes no gradient to its kernel, its gamma or the block above, exactly; the fused train steps leave that work out.
The argument is exact, so every comparison here is bit for bit: the 1x1 normalisation kernels and Adam with a hole against the
entry points they stand in for, and whole train steps with the switch on against the switch off."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import keras_weights as KW
from palette_and_histo_gan_amd import networks as NW
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
DTYPES = [L.F32, L.BF16]
SENTINEL = -1234.5          # exact in bf16 and f32


def _bits(t):
    """the tensor as integers: +0 and -0, and NaN payloads, compare as the bits they are"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1x1 normalisation
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n,c", [(1, 8), (3, 8), (1, 520), (3, 520)])
def test_norm_1x1_entry_points_equal_the_general_ones_bit_for_bit(dtype, n, c):
    """p2p_norm_act_fwd_1x1 / p2p_norm_act_bwd_1x1 against p2p_norm_act_fwd / p2p_norm_act_bwd at H = W = 1: one vector of channels
    and a ragged multiple of 8, with and without mask, both activations, dense and four-slab f32 gradient sources, the convolution
    result dense or in f32 split-K slabs (the new forward reads neither).  gamma has both signs and beta holds +0 and -0: the sign
    of 0 * gamma decides the sign of a zero output."""
    rng = np.random.default_rng(1000 * n + c)
    tdt = U.tdt(dtype)
    gamma = rng.normal(size=c).astype(np.float32)
    beta = (0.5 * rng.normal(size=c)).astype(np.float32)
    beta[::5], beta[1::5] = 0.0, -0.0
    g_d, b_d = U.dev(gamma), U.dev(beta)
    x = U.q(rng.normal(size=(n, 1, 1, c)) * 2 + 0.3, dtype)
    slabs = (rng.normal(size=(4, n, c)) * 0.8).astype(np.float32)
    raw = E.DenseBuf(n, 1, 1, c, tdt, U.DEV)
    raw.t.copy_(U.dev(x.reshape(-1, c), tdt))
    slabs_d = U.dev(slabs.reshape(-1))
    nws = torch.empty(max(n, 2) * 16 * c * 2, dtype=torch.float32, device=U.DEV)
    dy1 = U.dev(U.q(rng.normal(size=(n, c + 8)), dtype), tdt)                  # dense source behind a channel offset
    dy2 = U.dev(rng.normal(size=(4, n, c)).astype(np.float32).reshape(-1))      # four f32 slabs: one trip of the slab loader
    g_dense = L.GSrc(dy1.data_ptr(), 1, 1, n * (c + 8), c + 8, 8)
    g_slabs = L.GSrc(dy2.data_ptr(), 2, 4, n * c, c, 0)
    for use_mask in (False, True):
        mask_d = U.dev(rng.integers(0, 2, size=(n, c)).astype(np.uint8), torch.uint8) if use_mask else None
        mp = U.ptr(mask_d) if use_mask else None
        for act in (L.ACT_LEAKY, L.ACT_RELU):
            for raw_kind in (1, 2):
                want, got = E.HaloBuf(n, 1, 1, c + 8, dtype, U.DEV), E.HaloBuf(n, 1, 1, c + 8, dtype, U.DEV)
                for hb in (want, got):
                    hb._flat.fill_(SENTINEL)        # halo, channel padding and guard band: a stray store shows
                stats = torch.empty((n, c, 2), dtype=torch.float32, device=U.DEV)
                raw_out = E.DenseBuf(n, 1, 1, c, tdt, U.DEV)
                L.call("p2p_norm_act_fwd", dtype, n, 1, 1, c, raw.ptr() if raw_kind == 1 else U.ptr(slabs_d), raw_kind,
                       1 if raw_kind == 1 else 4, n * c, U.ptr(g_d), U.ptr(b_d), 1e-3, act, 0.3, mp, C.byref(want.view(coff=8)),
                       None if raw_kind == 1 else raw_out.ptr(), U.ptr(stats), U.ptr(nws), nws.numel() * 4, 1, U.stream())
                L.call("p2p_norm_act_fwd_1x1", dtype, n, c, U.ptr(g_d), U.ptr(b_d), act, 0.3, mp, C.byref(got.view(coff=8)), U.stream())
                assert _same(want._flat, got._flat), f"forward differs (mask {use_mask}, act {act}, raw kind {raw_kind})"
                raw_b = raw if raw_kind == 1 else raw_out
                for g1, g2, what in ((g_dense, None, "dense"), (g_slabs, None, "slabs"), (g_dense, g_slabs, "dense + slabs")):
                    part_w = torch.full((2, n, c), float("nan"), dtype=torch.float32, device=U.DEV)
                    part_g = torch.full((2, n, c), float("nan"), dtype=torch.float32, device=U.DEV)
                    draw = E.HaloBuf(n, 1, 1, c, dtype, U.DEV)
                    L.call("p2p_norm_act_bwd", dtype, n, 1, 1, c, raw_b.ptr(), U.ptr(stats), U.ptr(g_d), U.ptr(b_d), act, 0.3, mp,
                           C.byref(g1), C.byref(g2) if g2 is not None else None, C.byref(draw.view()), U.ptr(part_w[1]),
                           U.ptr(part_w[0]), U.ptr(nws), nws.numel() * 4, 1, U.stream())
                    L.call("p2p_norm_act_bwd_1x1", dtype, n, c, U.ptr(g_d), U.ptr(b_d), act, 0.3, mp, C.byref(g1),
                           C.byref(g2) if g2 is not None else None, U.ptr(part_g[1]), U.ptr(part_g[0]), U.stream())
                    where = f"(mask {use_mask}, act {act}, raw kind {raw_kind}, sources {what})"
                    assert _same(part_w[0], part_g[0]), f"dbeta partials differ {where}"
                    assert _same(part_g[1], torch.zeros_like(part_g[1])), f"dgamma partials are not +0 {where}"
                    assert _same(part_w[1], part_g[1]) and torch.count_nonzero(draw.t) == 0, f"the premise fails {where}"
                    if act == L.ACT_LEAKY and not use_mask:       # (no gate can close: every channel carries its gradient)
                        assert torch.count_nonzero(part_g[0]) == n * c, f"dbeta is dead too {where}"
    # a pixel that is no whole number of 16-byte vectors is refused, not served by something else
    with pytest.raises(L.P2PError):
        L.call("p2p_norm_act_fwd_1x1", dtype, n, 12, U.ptr(g_d), U.ptr(b_d), L.ACT_RELU, 0.3, None, C.byref(got.view(coff=8)), U.stream())


# ---------------------------------------------------------------------------------------------------------------- Adam with a hole
def test_adam_with_an_excluded_range_equals_the_flat_adam_outside_and_writes_nothing_inside():
    """p2p_adam_flat_dev_excl against p2p_adam_flat_dev on 4099 elements with g = 0 on the excluded range [1027, 3001) -- unaligned
    at both ends, so a 16-byte vector straddles each -- for t = 1 and 2.  Inside the range params, m and v hold a sentinel."""
    n, lo, hi = 4099, 1027, 3001
    rng = np.random.default_rng(77)
    inside = torch.zeros(n, dtype=torch.bool, device=U.DEV)
    inside[lo:hi] = True

    def buf(a):
        return U.dev(a.astype(np.float32))
    p_ref = buf(rng.normal(size=n) * 0.02)
    m_ref, v_ref = buf(np.zeros(n)), buf(np.zeros(n))
    p_new, m_new, v_new = p_ref.clone(), m_ref.clone(), v_ref.clone()
    p_start = p_ref.clone()
    for t in (p_new, m_new, v_new):
        t[inside] = SENTINEL
    t_dev = torch.zeros(1, dtype=torch.int32, device=U.DEV)
    lr_t = torch.zeros(1, dtype=torch.float32, device=U.DEV)
    b1, b2, eps = 0.5, 0.999, 1e-7
    for step in (1, 2):
        g = buf(rng.normal(size=n) * 1e-3)
        g[inside] = 0.0
        L.call("p2p_adam_tick", U.ptr(t_dev), U.ptr(lr_t), 2e-4, b1, b2, U.stream())
        assert int(t_dev[0]) == step
        L.call("p2p_adam_flat_dev", U.ptr(p_ref), U.ptr(g), U.ptr(m_ref), U.ptr(v_ref), n, U.ptr(lr_t), b1, b2, eps, 1.0, U.stream())
        L.call("p2p_adam_flat_dev_excl", U.ptr(p_new), U.ptr(g), U.ptr(m_new), U.ptr(v_new), n, lo, hi, U.ptr(lr_t), b1, b2, eps, 1.0,
               U.stream())
        for what, ref, new in (("params", p_ref, p_new), ("m", m_ref, m_new), ("v", v_ref, v_new)):
            assert _same(ref[~inside], new[~inside]), f"t = {step}: {what} differs outside the excluded range"
            assert bool((new[inside] == SENTINEL).all()), f"t = {step}: {what} was written inside the excluded range"
        assert not bool((p_ref[~inside] == p_start[~inside]).any()), "the flat Adam left an element alone: the test shows less"
        p_start = p_ref.clone()
    # with g = 0 and zero moments the flat Adam leaves the range alone as well: the hole changes no result
    assert torch.count_nonzero(m_ref[inside]) == 0 and torch.count_nonzero(v_ref[inside]) == 0
    with pytest.raises(L.P2PError):
        L.call("p2p_adam_flat_dev_excl", U.ptr(p_new), U.ptr(g), U.ptr(m_new), U.ptr(v_new), n, lo, n + 1, U.ptr(lr_t), b1, b2, eps, 1.0,
               U.stream())


# ---------------------------------------------------------------------------------------------------------------- whole steps
B = 3
STEP_MODELS = ("baseline-bf16", "baseline-f32", "indexed-bf16")
ONE_BY_ONE = (1, 1, 512, 512)       # LH, LW, Cg, Cd of the dead block's GEMMs (and of the first decoder block's, which stay)


def _engine(model, level, replay=True, S=64):
    kind, dtype_name = model.split("-")
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    if kind == "indexed":
        eng = E.Pix2PixEngine(1, 256, "softmax", S, dtype, device=U.DEV, seed=47)
        src, tgt, _ = DU.synthetic_indexed_batch(np.random.default_rng([47, 0]), B if S == 64 else 1, S, 24)
        src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
        step = lambda: eng.train_step_indexed(src_d, tgt_d, 0.01)        # noqa: E731
    else:
        eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, device=U.DEV, seed=47)
        src, tgt = rg.synthetic_rgba_batch(np.random.default_rng(48), B if S == 64 else 1, S)
        src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
        step = lambda: eng.train_step_rgba(src_d, tgt_d, 100.0)          # noqa: E731
    # f32 is the parity mode by default (batch_invariant), which keeps every launch: off here, so that the f32 kernels are elided too
    eng.batch_invariant = False
    eng.elide_dead_bottleneck = level
    eng.replay_enabled = replay
    return eng, step


def _state(eng):
    """every parameter, m, v and both operand copies of every layer"""
    out = {}
    for sid, st in (("G", eng.G), ("D", eng.D)):
        out.update({f"{sid}.params": st.params.clone(), f"{sid}.m": st.m.clone(), f"{sid}.v": st.v.clone()})
    for (sid, name), lw in eng.W.items():
        for tag in ("wn", "wt", "wd"):
            if getattr(lw, tag) is not None:
                out[f"{sid}.{name}.{tag}"] = getattr(lw, tag).clone()
    return out


def _gemm_calls(rec):
    """(name, (LH, LW, Cg, Cd)) of the GEMM launches of a recorded step"""
    out = []
    for name, args in rec:
        if name in ("p2p_igemm", "p2p_igemm_norm_act"):
            out.append((name, tuple(int(v) for v in args[3:7])))
        elif name == "p2p_wgemm":
            out.append((name, tuple(int(v) for v in args[2:6])))
    return out


def _run(model, level, replay, S=64):
    eng, step = _engine(model, level, replay, S)
    try:
        losses = [step().clone() for _ in range(3)]          # eager, recorded, replayed (or three eager steps)
        torch.cuda.synchronize()
        recs = [rec for _, rec in eng._replays.values()]
        assert len(recs) == (1 if replay else 0)
        return losses, _state(eng), [(n, a) for n, a in recs[0] if n is not None] if replay else None
    finally:
        del eng, step
        gc.collect()
        torch.cuda.empty_cache()


_REFERENCE = {}


def _reference(model, replay):
    if (model, replay) not in _REFERENCE:
        _REFERENCE[(model, replay)] = _run(model, 0, replay)
    return _REFERENCE[(model, replay)]


@pytest.mark.parametrize("replay", [True, False], ids=["replayed", "eager"])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("model", STEP_MODELS)
def test_three_steps_are_bit_identical_with_the_switch_on_and_off(model, level, replay):
    want_losses, want, rec_off = _reference(model, replay)
    got_losses, got, rec_on = _run(model, level, replay)
    for k, (a, b) in enumerate(zip(want_losses, got_losses)):
        assert torch.equal(a, b), f"losses of step {k + 1}: {a.tolist()} with the switch off, {b.tolist()} with it on"
    assert sorted(want) == sorted(got)
    differ = [k for k in want if not torch.equal(want[k], got[k])]
    assert not differ, f"differ after three steps: {differ}"
    if replay:
        off, on = _gemm_calls(rec_off), _gemm_calls(rec_on)
        count = lambda calls, name: sum(1 for n, s in calls if n == name and s == ONE_BY_ONE)        # noqa: E731
        # off: the dead block's forward and data-gradient GEMMs and the first decoder block's two; on: the decoder's alone
        assert (count(off, "p2p_igemm"), count(on, "p2p_igemm")) == (4, 2), (off, on)
        assert (count(off, "p2p_wgemm"), count(on, "p2p_wgemm")) == (2, 1), (off, on)
        assert len(on) == len(off) - 3
        names_on = {n for n, _ in rec_on}
        new = {"p2p_norm_act_fwd_1x1", "p2p_norm_act_bwd_1x1", "p2p_adam_flat_dev_excl"}
        assert (new <= names_on) if level == 2 else not (new & names_on), sorted(new & names_on)


def test_a_128x128_engine_issues_the_same_calls_with_the_switch_on_and_off():
    """the bottleneck is 2x2 from 128x128 on: nothing is dead, nothing is elided"""
    calls = {}
    for level in (0, 1, 2):
        _, _, rec = _run("baseline-bf16", level, True, S=128)
        calls[level] = [(n, tuple(int(v) for t, v in zip(L.SIGNATURES[n], a) if t is C.c_int and isinstance(v, int))) for n, a in rec]
    assert calls[0] == calls[1] == calls[2] and len(calls[0]) > 100


# ---------------------------------------------------------------------------------------------------------------- outside writers
def _fresh_copies(eng, lw, master):
    wn = torch.zeros_like(lw.wn) if lw.wn is not None else None
    wt = torch.zeros_like(lw.wt)
    L.call("p2p_weight_prep_pad", eng.dtype, U.ptr(master), lw.cg, lw.cd, U.ptr(wn) if wn is not None else None, E.up32(lw.cg), lw.lo_pad,
           U.ptr(wt), E.up32(lw.cd), lw.hi_pad, U.stream())
    return wn, wt


@pytest.mark.parametrize("how", ["set_params", "set_weights", "npz"])
def test_weights_written_from_outside_reach_the_frozen_copies(how, tmp_path):
    """The elided steps never refresh the dead kernel's operand copies; everything that writes the masters from outside does.  After
    such a write the copies equal a fresh p2p_weight_prep of the new kernel, the next steps leave kernel and copies alone, and
    generate() (which runs the block's convolution) equals an engine that never elided anything."""
    eng, step = _engine("baseline-bf16", 1)
    ref, _ = _engine("baseline-bf16", 0)
    try:
        name = f"down{eng._dead}"
        for _ in range(3):
            step()
        assert eng._frozen_ok is True
        vals = eng.G.export()
        new = np.random.default_rng(5).normal(0.0, 0.05, size=vals[name + ".kernel"].shape).astype(np.float32)
        vals[name + ".kernel"] = new
        if how == "set_params":
            eng.set_params(g_values=vals)
        elif how == "set_weights":
            NW.UnetGenerator(4, 4, "tanh").bind(eng, eng.G).set_weights(list(vals.values()))
        else:
            path = str(tmp_path / "g.npz")
            np.savez(path, format=np.array(KW.FORMAT), **{f"generator/{i:03d}:{k}": v for i, (k, v) in enumerate(vals.items())})
            KW.import_model(eng, path, with_optimizer=False, which=("generator",))
        lw = eng.W[("G", name)]
        master = eng.G.view(eng.G.params, name + ".kernel")
        assert torch.equal(master.cpu(), torch.as_tensor(new))
        for k in range(2):
            wn, wt = _fresh_copies(eng, lw, master)
            assert _same(lw.wt, wt) and (lw.wn is None or _same(lw.wn, wn)), f"stale copies of the frozen kernel ({how}, after {k} steps)"
            step()
        assert eng._frozen_ok is True and torch.equal(master.cpu(), torch.as_tensor(new)), "the frozen kernel moved"
        src = rg.synthetic_rgba_batch(np.random.default_rng(9), 2, 64)[0]
        masks = [np.ones(s, np.uint8) for s in rg.dropout_mask_shapes(2, 64)]
        ref.G.params.copy_(eng.G.params)
        ref.refresh_weight_copies()
        assert torch.equal(eng.generate(src, masks=masks), ref.generate(src, masks=masks))
    finally:
        del eng, ref, step
        gc.collect()
        torch.cuda.empty_cache()


def test_live_moments_on_the_dead_kernel_switch_the_elision_off():
    """A checkpoint of a 128x128 run has the same shapes and live Adam moments on that kernel: Adam then moves it although its
    gradient is 0, and the step issues everything."""
    eng, step = _engine("baseline-bf16", 1)
    ref, ref_step = _engine("baseline-bf16", 0)
    try:
        lo, hi = eng._frozen
        for e in (eng, ref):
            e.G.m[lo:hi] = 1e-3
            e.G.v[lo:hi] = 1e-6
            e.refresh_weight_copies()
        before = eng.G.params[lo:hi].clone()
        a, b = [step() for _ in range(2)], [ref_step() for _ in range(2)]
        assert eng._frozen_ok is False and eng._elision() == 0
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(eng.G.params, ref.G.params)
        assert not torch.equal(eng.G.params[lo:hi], before), "Adam did not move the kernel: the test shows nothing"
    finally:
        del eng, ref, step, ref_step
        gc.collect()
        torch.cuda.empty_cache()
