"""-m gpu: every launch a benchmarked train step makes, re-issued on test-owned buffers and compared with float64.

The kernels pick their variant from the launch size (256-row im2col tiles, the block-resident kernel, K splits, register-resident
norm forms ...), so small-shape tests do not reach what bench.py runs.  For each bench.CONFIGS entry the engine is built as bench.py
builds it, the recorded step's call list (the list p2p_replay re-issues) is reduced to unique launch signatures, and every launch of
an entry point with a checker below is re-issued with the recorded integer / float arguments and view geometry on seeded operands:
- per-image outputs are compared in full for a set of images (tests/step_launches.image_set), per image (per image and channel for
  normalised outputs); weight gradients over the whole batch, per tap;
- every output element of the view is NaN before and finite after; everything around the view (halo ring, other channels up to ld,
  the tail of the buffer) holds a sentinel that must be bit-for-bit unchanged;
- fused InstanceNorm statistics (slot partials) equal the f64 moments of the stored output;
- a second launch on the same inputs is bit-identical.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bench
from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from tests import gpu_util as U
from tests import step_launches as SL

pytestmark = pytest.mark.gpu

OUT_TOL = {L.F32: 2e-5, L.BF16: 6e-3}      # test_kernels_gpu.py: activation-dtype outputs
F32_TOL = 2e-5                              # f32 slabs / statistics of short contractions (test_kernels_gpu.py)
SENTINEL = -1234.5                          # exact in bf16 and f32
TAIL = 256                                  # elements of sentinel behind every output buffer

CONFIGS = [("c1", "bf16"), ("c2", "bf16"), ("c3", "bf16"), ("c4", "bf16"), ("c5", "bf16"), ("c2", "f32")]

# entry points of a recorded step that this file does not re-issue, with the reason.  A call that is neither here nor in
# CHECKERS fails the test: a new entry point cannot slip past.
OUT_OF_SCOPE = {
    "p2p_adam_flat": "optimizer", "p2p_adam_flat_dev": "optimizer", "p2p_adam_tick": "optimizer",
    "p2p_adam_prep_batched": "optimizer", "p2p_weight_prep": "packing (weight copies)",
    "p2p_weight_prep_pad": "packing (weight copies)", "p2p_weight_prep_batched": "packing (weight copies)",
    "p2p_pack_input": "packing", "p2p_pack_input_multi": "packing", "p2p_pack_pair": "packing", "p2p_pack_pair_idx": "packing",
    "p2p_unpack": "packing",
    "p2p_bce_logits": "loss", "p2p_bce_logits_pad8": "loss", "p2p_loss_partials_sum": "loss", "p2p_tanh_l1_fwd": "loss",
    "p2p_tanh_l1_fwd_pair": "loss", "p2p_tanh_l1_bwd": "loss", "p2p_tanh_l1_bwd_pad8": "loss", "p2p_finish_losses": "loss",
    "p2p_hellinger_fwd": "loss", "p2p_hellinger_finish": "loss", "p2p_hist_normalize": "loss",
    "p2p_colsum": "loss / parameter-gradient reduction", "p2p_colsum_batched": "parameter-gradient reduction",
    "p2p_view_colsum": "bias-gradient reduction",
    "p2p_dropout_mask": "dropout RNG", "p2p_dropout_mask_dev": "dropout RNG", "p2p_counter_add": "dropout RNG",
    "p2p_event_record": "stream operation", "p2p_stream_wait_event": "stream operation", "p2p_arm_stop_event": "stream operation",
    "p2p_event_create": "stream operation",
}


def _val(v):
    """a recorded ctypes argument as a Python value (structures for byref arguments)"""
    if v is None:
        return None
    obj = getattr(v, "_obj", None)
    if obj is not None:
        return obj
    if isinstance(v, C._SimpleCData):
        return v.value
    return v


def _blocks():
    """(address, size) of every allocated block of torch's caching allocator on the device"""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            if b["state"] == "active_allocated":
                out.append((addr, b["size"]))
            addr += b["size"]
    return out


def _coff(ptr, ld, esz, blocks):
    """(channel offset, pixel index inside its image) of a view pointer, counted from the start of the allocation it points into.
    The caller checks that the pixel index is the view's first interior pixel: the allocation then starts on the pixel grid of
    the view and the channel offset is the one the engine used."""
    for a, s in blocks:
        if a <= ptr < a + s:
            assert (ptr - a) % esz == 0, f"view pointer {ptr:#x} is not on an element boundary"
            e = (ptr - a) // esz
            return e % ld, e // ld
    raise AssertionError(f"view pointer {ptr:#x} is in no allocation")


# ---------------------------------------------------------------------------------------------------------------- harvest
def _build(cfg, dtype_name):
    model, B, S, lam_l1, lam_hist, palette = bench.CONFIGS[cfg]
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    if model == "indexed":
        eng = E.Pix2PixEngine(1, 256, "softmax", S, dtype, device=U.DEV, seed=47)
        src, tgt, _ = DU.synthetic_indexed_batch(np.random.default_rng([47, 0]), B, S, palette)
        src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
        return eng, lambda: eng.train_step_indexed(src_d, tgt_d, lam_l1, global_batch=B)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, device=U.DEV, seed=47)
    src, tgt = bench.synthetic_batch(0, B, S, palette)
    src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
    return eng, lambda: eng.train_step_rgba(src_d, tgt_d, lam_l1, lam_hist, global_batch=B)


def _esz(dtype):
    return 2 if dtype == L.BF16 else 4


def _view_desc(t, ld_esz, blocks):
    esz = ld_esz
    coff, pix = _coff(t.ptr, t.ld, esz, blocks)
    return {"ptr": t.ptr, "img_stride": int(t.img_stride), "row_stride": int(t.row_stride), "ld": int(t.ld),
            "align": t.ptr % 16, "coff": coff, "pix": pix % int(t.img_stride)}


def _gsrc_desc(g, dtype, blocks):
    esz = 4 if g.kind == 2 else _esz(dtype)
    return {"kind": int(g.kind), "nslabs": int(g.nslabs), "slab_stride": int(g.slab_stride), "ld": int(g.ld),
            "coff": int(g.coff), "align": g.ptr % 16 if g.ptr else 0}


def _decode(name, args, blocks):
    """(name, args) -> list of plain values: ints / floats, view and gsrc descriptions, 'null' / 'ptr' for pointers"""
    types = L.SIGNATURES[name]
    assert len(types) == len(args), name
    vals = [_val(a) for a in args]
    dtype = None
    if name in ("p2p_igemm", "p2p_igemm_norm_act", "p2p_conv_strip"):
        dtype = vals[1]
    elif name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewin_actbwd", "p2p_conv_fewout"):
        dtype = vals[2]
    elif name in ("p2p_wgemm", "p2p_wgemm_edge", "p2p_wgrad_small", "p2p_norm_act_fwd", "p2p_norm_act_fwd_tail",
                  "p2p_norm_act_bwd", "p2p_act_bwd", "p2p_rgbuv_points", "p2p_rgbuv_hist_fwd3", "p2p_rgbuv_hist_hellinger_bwd3",
                  "p2p_head_dgrad", "p2p_head_softmax_cce"):
        dtype = vals[0]
    out = []
    for t, v in zip(types, vals):
        if t is L._TP:
            out.append(None if v is None else ("view", _view_desc(v, _esz(dtype), blocks)))
        elif t is L._GP:
            out.append(None if v is None else ("gsrc", _gsrc_desc(v, dtype, blocks)))
        elif t is C.c_void_p:
            p = v.value if isinstance(v, C.c_void_p) else v
            out.append(None if not p else ("ptr", p % 16))
        elif t is C.c_float:
            out.append(float(v))
        else:
            out.append(int(v))
    return out


def _signature(name, dec):
    key = []
    for d in dec:
        if isinstance(d, tuple) and d[0] != "ptr":
            key.append((d[0],) + tuple(sorted((k, v) for k, v in d[1].items() if k != "ptr")))
        else:
            key.append(d)
    return (name,) + tuple(key[:-1])           # the last argument is the stream


def harvest(cfg, dtype_name):
    """unique launch signatures of the recorded step of one bench config: {signature: (name, decoded args)}, and the raw count"""
    eng, step = _build(cfg, dtype_name)
    try:
        for _ in range(2):         # the first step of a kind is eager, the second one is recorded (_begin_record)
            step()
        torch.cuda.synchronize()
        assert len(eng._replays) == 1, f"{cfg}: the step was not recorded"
        rec = next(iter(eng._replays.values()))[1]
        assert rec, f"{cfg}: empty recording"
        blocks = _blocks()
        uniq, names = {}, []
        for name, args in rec:
            assert name is not None, "single-GPU step with a collective segment"
            names.append(name)
            if name not in CHECKERS:
                continue
            dec = _decode(name, args, blocks)
            uniq.setdefault(_signature(name, dec), (name, dec))
        return uniq, names
    finally:
        del eng
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- buffers
class OutBuf:
    """A test-owned buffer laid out like a recorded output view: same pixel strides, ld, channel offset and 16-byte alignment.
    The nc channels of the view's pixels start as NaN, everything else (halo ring, the other channels, TAIL elements) as SENTINEL."""

    def __init__(self, desc, n, h, w, nc, tdt, esz):
        ld, coff = desc["ld"], desc["coff"]
        rs, ist = desc["row_stride"], desc["img_stride"]
        halo = (rs - w) // 2
        assert rs == w + 2 * halo and ist == (h + 2 * halo) * rs, f"view geometry {desc} does not fit {h}x{w} with a halo"
        assert coff + nc <= ld, (desc, nc)
        _check_grid(desc, h, w)
        hp, wp = h + 2 * halo, w + 2 * halo
        numel = n * hp * wp * ld
        off0 = (halo * wp + halo) * ld + coff
        self.flat_all = torch.empty(numel + TAIL + 16, dtype=tdt, device=U.DEV)
        base = self.flat_all.data_ptr()
        s = next(s for s in range(16) if (base + (s + off0) * esz) % 16 == desc["align"])
        self.flat = self.flat_all[s:s + numel + TAIL]
        self.t = self.flat[:numel].view(n, hp, wp, ld)
        self.sl = (slice(None), slice(halo, halo + h), slice(halo, halo + w), slice(coff, coff + nc))
        self.view = L.Tensor(base + (s + off0) * esz, ist, rs, ld)
        self.mask = torch.ones(self.flat.shape, dtype=torch.bool, device=U.DEV)
        self.mask[:numel].view(n, hp, wp, ld)[self.sl] = False
        self.reset()

    def reset(self):
        self.flat.fill_(SENTINEL)
        self.t[self.sl] = float("nan")
        self._before = self.flat.clone()

    def region(self):
        return self.t[self.sl].double().cpu().numpy()

    def check_around(self, what):
        got, want = self.flat[self.mask], self._before[self.mask]
        assert torch.equal(got.view(torch.int16) if got.element_size() == 2 else got.view(torch.int32),
                           want.view(torch.int16) if want.element_size() == 2 else want.view(torch.int32)), \
            f"{what}: an element outside the view changed"
        r = self.t[self.sl]
        assert not bool(torch.isnan(r).any()), f"{what}: {int(torch.isnan(r).sum())} elements of the view were not written"


class FlatOut:
    """f32 output of a given length (slabs, statistics, weight gradients): NaN, then TAIL sentinel elements"""

    def __init__(self, numel, align=0):
        self.numel = numel
        self.all = torch.empty(numel + TAIL + 4, dtype=torch.float32, device=U.DEV)
        s = next(s for s in range(4) if (self.all.data_ptr() + 4 * s) % 16 == align)
        self.flat = self.all[s:s + numel + TAIL]
        self.reset()

    def reset(self):
        self.flat[:self.numel] = float("nan")
        self.flat[self.numel:] = SENTINEL

    def ptr(self):
        return C.c_void_p(self.flat.data_ptr())

    def values(self):
        return self.flat[:self.numel].double().cpu().numpy()

    def check_around(self, what):
        assert bool((self.flat[self.numel:] == SENTINEL).all()), f"{what}: written past the end"
        assert not bool(torch.isnan(self.flat[:self.numel]).any()), f"{what}: elements not written"


def _check_grid(desc, h, w):
    """the recorded view starts at the first interior pixel of an image of its buffer (halo = (row_stride - w) / 2)"""
    halo = (desc["row_stride"] - w) // 2
    if "pix" in desc:
        assert desc["pix"] == halo * desc["row_stride"] + halo, f"view {desc} is not at the first interior pixel of a {h}x{w} image"


def in_view(desc, x, dtype, fill_rng):
    """input view with the recorded geometry holding x [n,h,w,c] at the recorded channel offset.  The other channels of the pixels
    hold random values (a kernel must not use them), the halo ring and the tail are zero (the gathering kernels read the halo as
    the convolution's zero padding, include/p2pgan.h Conventions).  Returns (keep-alive tensor, p2p_tensor)."""
    n, h, w, c = x.shape
    ld, coff, rs, ist = desc["ld"], desc["coff"], desc["row_stride"], desc["img_stride"]
    halo = (rs - w) // 2
    assert rs == w + 2 * halo and ist == (h + 2 * halo) * rs and coff + c <= ld, (desc, x.shape)
    _check_grid(desc, h, w)
    esz = _esz(dtype)
    hp, wp = h + 2 * halo, w + 2 * halo
    numel = n * hp * wp * ld
    off0 = (halo * wp + halo) * ld + coff
    flat_all = torch.zeros(numel + TAIL + 16, dtype=U.tdt(dtype), device=U.DEV)
    base = flat_all.data_ptr()
    s = next(s for s in range(16) if (base + (s + off0) * esz) % 16 == desc["align"])
    t = flat_all[s:s + numel].view(n, hp, wp, ld)
    other = torch.as_tensor(U.q(fill_rng.normal(size=(n, h, w, ld)), dtype)).to(U.DEV)
    t[:, halo:halo + h, halo:halo + w, :] = other.to(t.dtype)
    t[:, halo:halo + h, halo:halo + w, coff:coff + c] = torch.as_tensor(x).to(U.DEV).to(t.dtype)
    return flat_all, L.Tensor(base + (s + off0) * esz, ist, rs, ld)


def gsrc_in(desc, n, h, w, c, dtype, rng, live=None):
    """gradient source with the recorded kind / slabs / ld / offset: returns (keep-alive, p2p_gsrc, summed f64 values [n,h,w,c]).
    live [n*h*w, c] (bool): the source is zero where it is False"""
    pix = n * h * w
    ld, coff, ns, ss = desc["ld"], desc["coff"], max(desc["nslabs"], 1), desc["slab_stride"]
    if desc["kind"] == 2:
        assert ss >= pix * ld, desc
        data = rng.normal(size=(ns, ss)).astype(np.float32)
        if live is not None:
            for k in range(ns):
                data[k, :pix * ld].reshape(pix, ld)[:, coff:coff + c] *= live
        t = torch.as_tensor(data.reshape(-1)).to(U.DEV)
        vals = np.zeros((pix, c), np.float32)
        for k in range(ns):
            vals = vals + data[k, :pix * ld].reshape(pix, ld)[:, coff:coff + c]       # f32, slab order
        ref = vals.astype(np.float64)
    else:
        data = U.q(rng.normal(size=(pix, ld)), dtype)
        if live is not None:
            data[:, coff:coff + c] *= live
        t = torch.as_tensor(data).to(U.DEV).to(U.tdt(dtype)).contiguous()
        ref = data[:, coff:coff + c].astype(np.float64)
    g = L.GSrc(t.data_ptr(), desc["kind"], desc["nslabs"], ss, ld, coff)
    return t, g, ref.reshape(n, h, w, c)


def _prep(dtype, w, cg, cd, wn_shape=None, wt_shape=None):
    """p2p_weight_prep_pad: wn [16][rows][cols] and / or wt [16][rows][cols] in the activation dtype"""
    w_d = U.dev(w.reshape(-1))
    wn = torch.zeros(16 * wn_shape[0] * wn_shape[1], dtype=U.tdt(dtype), device=U.DEV) if wn_shape else None
    wt = torch.zeros(16 * wt_shape[0] * wt_shape[1], dtype=U.tdt(dtype), device=U.DEV) if wt_shape else None
    L.call("p2p_weight_prep_pad", dtype, U.ptr(w_d), cg, cd, U.ptr(wn) if wn is not None else None, *(wn_shape or (0, 0)),
           U.ptr(wt) if wt is not None else None, *(wt_shape or (0, 0)), U.stream())
    return wn if wn is not None else wt


# ---------------------------------------------------------------------------------------------------------------- checkers
class Launch:
    """one re-issued launch: outputs (OutBuf / FlatOut), the launch closure and the evaluation (returns {family: worst error})"""

    def __init__(self, outs, go, evaluate):
        self.outs, self.go, self.evaluate = outs, go, evaluate


def _conv_family(name, a, rng):
    """p2p_igemm, p2p_conv_strip, p2p_igemm_norm_act (stride 2, full channel counts) and the edge forms p2p_igemm_edge,
    p2p_conv_fewin, p2p_conv_fewout, p2p_conv_fewin_actbwd (cin_pad contracted channels, ncols outputs, stride 1 or 2)"""
    edge = name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewout", "p2p_conv_fewin_actbwd")
    if edge:
        op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows = a[:9]
        in_d, out_d = a[9][1], a[10][1]
        if op == L.OP_G:
            cg, cd, in_shape, out_shape = cin_pad, ncols, (stride * LH, stride * LW, cin_pad), (LH, LW, ncols)
        else:
            cg, cd, in_shape, out_shape = ncols, cin_pad, (LH, LW, cin_pad), (stride * LH, stride * LW, ncols)
    else:
        op, dtype, N, LH, LW, cg, cd = a[:7]
        stride = 2
        hi_d, lo_d = a[7][1], a[8][1]
        in_d, out_d = (hi_d, lo_d) if op == L.OP_G else (lo_d, hi_d)
        in_shape = (2 * LH, 2 * LW, cg) if op == L.OP_G else (LH, LW, cd)
        out_shape = (LH, LW, cd) if op == L.OP_G else (2 * LH, 2 * LW, cg)
    tdt, esz = U.tdt(dtype), _esz(dtype)
    x = U.q(rng.normal(size=(N,) + in_shape), dtype)
    w = U.q(rng.normal(scale=1.0 / np.sqrt(16 * in_shape[2]), size=(4, 4, cg, cd)), dtype)
    keep_in, in_v = in_view(in_d, x, dtype, rng)
    if edge:
        if op == L.OP_G:
            wbuf = _prep(dtype, w, cg, cd, wt_shape=(w_rows, cin_pad))
        else:
            wbuf = _prep(dtype, w, cg, cd, wn_shape=(w_rows, cin_pad))
    else:
        wbuf = _prep(dtype, w, cg, cd, wn_shape=(cg, cd)) if op == L.OP_P else _prep(dtype, w, cg, cd, wt_shape=(cd, cg))
    nout = out_shape[2]
    res_h, res_w = out_shape[0], out_shape[1]
    outs, extra = [], {}
    sk = a[7 + 3] if name == "p2p_igemm" else 1
    slabs = None
    out = OutBuf(out_d, N, res_h, res_w, nout, tdt, esz)      # (not written with split-K slabs)
    if name == "p2p_igemm" and sk > 1:
        slabs = FlatOut(sk * N * res_h * res_w * nout, a[11][1] if a[11] else 0)
        outs.append(slabs)
    else:
        outs.append(out)
    hv, lv = (in_v, out.view) if op == L.OP_G else (out.view, in_v)
    spart = None
    stat_idx = {"p2p_igemm": 12, "p2p_conv_strip": 10}.get(name)
    if stat_idx is not None and a[stat_idx] is not None:
        slots = (L.lib().p2p_igemm_layer_stat_slots(op, dtype, N, LH, LW, cg, cd) if name == "p2p_igemm"
                 else L.lib().p2p_conv_strip_stat_slots(op, dtype, N, LH, LW, cg, cd))
        assert slots > 0, (name, a)
        spart = FlatOut(N * slots * nout * 2, a[stat_idx][1])
        outs.append(spart)
        extra["slots"] = slots
    bias = gate = gamma = beta = None
    if name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewout") and a[12] is not None:
        bias = rng.normal(size=ncols).astype(np.float32)
    bias_d = U.dev(bias) if bias is not None else None
    if name == "p2p_conv_fewin_actbwd":
        gate = U.q(rng.normal(size=(N, res_h, res_w, nout)), dtype)
        keep_gate, gate_v = in_view(a[12][1], gate, dtype, rng)
    if name == "p2p_igemm_norm_act":
        gamma = (1 + 0.2 * rng.normal(size=nout)).astype(np.float32)
        beta = (0.2 * rng.normal(size=nout)).astype(np.float32)
        g_d, b_d = U.dev(gamma), U.dev(beta)
        y = OutBuf(a[15][1], N, res_h, res_w, nout, tdt, esz)
        stats = FlatOut(N * nout * 2, a[16][1])
        outs += [y, stats]

    def go():
        st = U.stream()
        if name == "p2p_igemm":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), sk,
                   slabs.ptr() if slabs else None, spart.ptr() if spart else None, st)
        elif name == "p2p_conv_strip":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), spart.ptr() if spart else None, st)
        elif name == "p2p_igemm_norm_act":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), U.ptr(g_d), U.ptr(b_d), a[12], a[13],
                   a[14], C.byref(y.view), stats.ptr(), st)
        elif name == "p2p_conv_fewin_actbwd":
            L.call(name, op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows, C.byref(in_v), C.byref(out.view), U.ptr(wbuf),
                   C.byref(gate_v), a[13], st)
        else:
            L.call(name, op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows, C.byref(in_v), C.byref(out.view), U.ptr(wbuf),
                   U.ptr(bias_d) if bias_d is not None else None, a[13], a[14], st)

    def evaluate():
        errs = {}
        imgs = SL.image_set(N, seed=N * 7 + LH)
        conv = (SL.conv_g(x[imgs], w, stride) if op == L.OP_G else SL.conv_p(x[imgs], w, stride))
        if slabs is not None:
            got = slabs.values().reshape(sk, N, res_h, res_w, nout).sum(0)[imgs]
            errs["f32 slabs"] = SL.per_image_err(got, conv)
            return errs
        full = out.region()
        got = full[imgs]
        if name == "p2p_conv_fewin_actbwd":
            ref = conv * np.where(gate[imgs] > 0, 1.0, a[13])
        elif name == "p2p_igemm_norm_act":
            ref = conv
        else:
            ref = conv + (bias if bias is not None else 0.0)
            ref = SL.act(ref, a[13], a[14]) if edge else ref
        errs["out " + ("bf16" if dtype == L.BF16 else "f32")] = SL.per_image_err(got, ref)
        if spart is not None:
            mean, var = SL.pooled_moments(spart.values().reshape(N, extra["slots"], nout, 2), res_h * res_w / extra["slots"])
            errs["stats"] = SL.moment_err(mean, var, full)                       # every image: the stored output's moments
            errs["stats f64"] = SL.moment_err(mean[imgs], var[imgs], conv)       # the compared images: the f64 convolution's
        if name == "p2p_igemm_norm_act":
            st_v = stats.values().reshape(N, nout, 2)
            var = 1.0 / st_v[..., 1].astype(np.float64) ** 2 - a[12]
            errs["stats"] = SL.moment_err(st_v[..., 0], var, full, eps=a[12])
            errs["stats f64"] = SL.moment_err(st_v[imgs][..., 0], var[imgs], conv, eps=a[12])
            want = SL.norm_act(got, gamma, beta, a[12], a[13], a[14])
            pre = SL.norm_act(got, gamma, beta, a[12], 0, 0.0)
            errs["norm out"] = SL.per_image_channel_err(y.region()[imgs], want, np.maximum(np.abs(want), np.abs(pre)))
        return errs

    keep = (keep_in, wbuf, bias_d) + ((keep_gate,) if gate is not None else ()) + ((g_d, b_d) if gamma is not None else ())
    launch = Launch(outs, go, evaluate)
    launch.keep = keep
    return launch


def _wgrad_family(name, a, rng):
    """p2p_wgemm (stride 2), p2p_wgemm_edge, p2p_wgrad_small: dW over the whole batch"""
    if name == "p2p_wgemm":
        dtype, N, LH, LW, cg, cd = a[:6]
        stride, hi_d, lo_d, ms = 2, a[6][1], a[7][1], a[9]
    else:
        dtype, stride, N, LH, LW, cg, cd = a[:7]
        hi_d, lo_d = a[7][1], a[8][1]
        ms = a[10] if name == "p2p_wgemm_edge" else None
    hi = U.q(rng.normal(size=(N, stride * LH, stride * LW, cg)), dtype)
    lo = U.q(rng.normal(size=(N, LH, LW, cd)), dtype)
    keep_hi, hv = in_view(hi_d, hi, dtype, rng)
    keep_lo, lv = in_view(lo_d, lo, dtype, rng)
    dw = FlatOut(16 * cg * cd, a[8 if name == "p2p_wgemm" else 9][1])
    if name == "p2p_wgrad_small":
        nb = L.lib().p2p_wgrad_small_blocks(dtype, stride, N, LH, LW, cg, cd, hv.ld, lv.ld)
        assert nb > 0, a
        ws_n = nb * 16 * cg * cd
    else:
        ws_n = L.lib().p2p_wgemm_workspace_bytes(N, LH, LW, cg, cd, ms) // 4
    ws = torch.full((max(ws_n, 4),), float("nan"), dtype=torch.float32, device=U.DEV)

    def go():
        st = U.stream()
        if name == "p2p_wgemm":
            L.call(name, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), ms, U.ptr(ws) if a[10] else None, st)
        elif name == "p2p_wgemm_edge":
            L.call(name, dtype, stride, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), ms, U.ptr(ws) if a[11] else None, st)
        else:
            L.call(name, dtype, stride, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), U.ptr(ws), st)

    def evaluate():
        ref = SL.conv_w(hi, lo, stride)
        k = N * LH * LW
        # K = N*LH*LW products of activation-dtype values (exact in f32), summed in f32 in a fixed blocked order.  The rounding
        # error of a sum of K random-sign terms grows like sqrt(K) * 2^-24 relative to the result; 4 * sqrt(K) * 2^-24 is 2e-5
        # at K = 2^12 and 2.4e-4 at K = 2^20 (c5: 256 images of 64x64), far below one missing K block (~6 %).
        tol = max(F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24)
        return {"dW f32": SL.per_tap_err(dw.values().reshape(4, 4, cg, cd), ref) * F32_TOL / tol}

    launch = Launch([dw], go, evaluate)
    launch.keep = (keep_hi, keep_lo, ws)
    return launch


def _norm_fwd(name, a, rng):
    """p2p_norm_act_fwd / p2p_norm_act_fwd_tail"""
    dtype, N, H, W, Cc = a[:5]
    raw_kind, nslabs, slab_stride = a[6], a[7], a[8]
    has_norm = a[9] is not None
    eps, act, alpha = a[11], a[12], a[13]
    nsplit = a[20]
    tdt, esz = U.tdt(dtype), _esz(dtype)
    pix = N * H * W
    if raw_kind == 2:
        sl = (rng.normal(size=(nslabs, slab_stride)) * 0.8 + 0.1).astype(np.float32)
        acc = np.zeros((pix, Cc), np.float32)
        for k in range(nslabs):
            acc = acc + sl[k, :pix * Cc].reshape(pix, Cc)
        x = U.q(acc, dtype).reshape(N, H, W, Cc)
        raw_t = torch.as_tensor(sl.reshape(-1)).to(U.DEV)
    else:
        x = U.q(rng.normal(size=(N, H, W, Cc)) * 2 + 0.3, dtype)
        raw_t = torch.as_tensor(x.reshape(-1)).to(U.DEV).to(tdt)
    gamma = (1 + 0.2 * rng.normal(size=Cc)).astype(np.float32)
    beta = (0.2 * rng.normal(size=Cc)).astype(np.float32)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    mask = rng.integers(0, 2, size=(N, H, W, Cc)).astype(np.uint8) if a[14] is not None else None
    mask_d = U.dev(mask.reshape(-1), torch.uint8) if mask is not None else None
    tail_ch = a[22] if name == "p2p_norm_act_fwd_tail" else 0
    out = OutBuf(a[15][1], N, H, W, Cc + tail_ch, tdt, esz)     # the tail channels follow this layer's channels in the view
    outs = [out]
    raw_out = None
    if a[16] is not None:
        raw_out = OutBuf({"ld": Cc, "coff": 0, "row_stride": W, "img_stride": H * W, "align": a[16][1]}, N, H, W, Cc, tdt, esz)
        outs.append(raw_out)
    stats = None
    if a[17] is not None:
        stats = FlatOut(N * Cc * 2, a[17][1])
        outs.append(stats)
    ws_bytes = a[19]
    ws = torch.full((max(ws_bytes // 4, 4),), float("nan"), dtype=torch.float32, device=U.DEV)
    if nsplit < 0:
        # apply-only pass over statistics slots written by a convolution epilogue: slot k holds the mean and the centred sum of
        # squares of the k-th run of H*W/slots pixels of the image -- disjoint groups with different moments, so the kernel must
        # pool them (parallel-variance rule) to reach the image's mean and variance
        slots = -nsplit
        assert (H * W) % slots == 0, (H, W, slots)
        grp = x.astype(np.float64).reshape(N, slots, H * W // slots, Cc)
        mom = np.stack([grp.mean(axis=2), ((grp - grp.mean(axis=2, keepdims=True)) ** 2).sum(axis=2)], axis=-1)   # [N][slots][C][2]
        ws[:N * slots * Cc * 2] = torch.as_tensor(mom.reshape(-1).astype(np.float32)).to(U.DEV)
    tail = None
    if tail_ch:
        tail = U.q(rng.normal(size=(N, H, W, tail_ch)), dtype)
        keep_tail, tail_v = in_view(a[21][1], tail, dtype, rng)

    def go():
        args = (dtype, N, H, W, Cc, U.ptr(raw_t), raw_kind, nslabs, slab_stride, U.ptr(g_d) if has_norm else None,
                U.ptr(b_d) if has_norm else None, eps, act, alpha, U.ptr(mask_d) if mask is not None else None, C.byref(out.view),
                C.c_void_p(raw_out.view.ptr) if raw_out else None, stats.ptr() if stats else None, U.ptr(ws), ws_bytes, nsplit)
        if name == "p2p_norm_act_fwd_tail":
            L.call(name, *args, C.byref(tail_v), a[22], U.stream())
        else:
            L.call(name, *args, U.stream())

    def evaluate():
        errs = {}
        imgs = SL.image_set(N, seed=N * 5 + H)
        want = SL.norm_act(x[imgs], gamma if has_norm else None, beta if has_norm else None, eps, act, alpha,
                           mask[imgs] if mask is not None else None)
        pre = SL.norm_act(x[imgs], gamma if has_norm else None, beta if has_norm else None, eps, 0, 0.0) * (2.0 if mask is not None else 1.0)
        reg = out.region()
        errs["norm out"] = SL.per_image_channel_err(reg[imgs][..., :Cc], want, np.maximum(np.abs(want), np.abs(pre)))
        if tail is not None:
            assert np.array_equal(reg[..., Cc:], tail.astype(np.float64)), "tail channels"
        if raw_out is not None:
            assert np.array_equal(raw_out.region(), x.astype(np.float64)), "raw_out is not the rounded slab sum"
        if stats is not None and has_norm:
            st_v = stats.values().reshape(N, Cc, 2)
            errs["stats"] = SL.moment_err(st_v[..., 0], 1.0 / st_v[..., 1].astype(np.float64) ** 2 - eps, x, eps=eps)
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (raw_t, g_d, b_d, mask_d, ws) + ((keep_tail,) if tail is not None else ())
    return launch


def _act_bwd(name, a, rng):
    """p2p_act_bwd: draw = (g1 + g2) * (act_out > 0 ? 1 : alpha)"""
    dtype, N, H, W, Cc = a[:5]
    alpha = a[8]
    gate = U.q(rng.normal(size=(N, H, W, Cc)), dtype)
    keep_gate, gate_v = in_view(a[5][1], gate, dtype, rng)
    k1, g1, r1 = gsrc_in(a[6][1], N, H, W, Cc, dtype, rng)
    k2, g2, r2 = gsrc_in(a[7][1], N, H, W, Cc, dtype, rng) if a[7] is not None else (None, None, 0.0)
    out = OutBuf(a[9][1], N, H, W, Cc, U.tdt(dtype), _esz(dtype))

    def go():
        L.call(name, dtype, N, H, W, Cc, C.byref(gate_v), C.byref(g1), C.byref(g2) if g2 is not None else None, alpha,
               C.byref(out.view), U.stream())

    def evaluate():
        want = (r1 + r2) * np.where(gate > 0, 1.0, alpha)
        return {"out " + ("bf16" if dtype == L.BF16 else "f32"): SL.per_image_err(out.region(), want)}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep_gate, k1, k2)
    return launch


def _norm_bwd(name, a, rng):
    """p2p_norm_act_bwd: d(raw) of y = act(drop(InstanceNorm(raw))) for dy = g1 + g2, and the per-image dgamma / dbeta partials"""
    dtype, N, H, W, Cc = a[:5]
    act, alpha = a[9], a[10]
    assert a[6] is not None and a[7] is not None, "the backward pass of a block without normalisation"
    tdt, esz = U.tdt(dtype), _esz(dtype)
    eps = rg.IN_EPS                # (the backward pass reads mean / rstd from stats; eps is not an argument)
    x = U.q(rng.normal(size=(N, H, W, Cc)) * 2 + 0.3, dtype)
    xd = x.astype(np.float64)
    mean, var = xd.mean(axis=(1, 2)), xd.var(axis=(1, 2))
    stats = np.stack([mean, 1.0 / np.sqrt(var + eps)], axis=-1).astype(np.float32)       # what the forward pass leaves
    gamma = (1 + 0.2 * rng.normal(size=Cc)).astype(np.float32)
    beta = (0.2 * rng.normal(size=Cc)).astype(np.float32)
    mask = rng.integers(0, 2, size=(N, H, W, Cc)).astype(np.uint8) if a[11] is not None else None
    # the gradient sources are zero where the activation's input is within 1e-3 of 0: an f32 gate that rounds to the other side
    # of 0 than the f64 one then changes nothing (at batch 256 the compared planes hold ~10^7 elements)
    pre = SL.norm_act(xd, gamma, beta, eps, 0, 0.0)
    live = (np.abs(pre) > 1e-3).reshape(N * H * W, Cc)
    k1, g1, r1 = gsrc_in(a[12][1], N, H, W, Cc, dtype, rng, live)
    k2, g2, r2 = gsrc_in(a[13][1], N, H, W, Cc, dtype, rng, live) if a[13] is not None else (None, None, 0.0)
    raw_t = torch.as_tensor(x.reshape(-1)).to(U.DEV).to(tdt)
    st_d, g_d, b_d = U.dev(stats.reshape(-1)), U.dev(gamma), U.dev(beta)
    mask_d = U.dev(mask.reshape(-1), torch.uint8) if mask is not None else None
    draw = OutBuf(a[14][1], N, H, W, Cc, tdt, esz)
    dgam, dbet = FlatOut(N * Cc, a[15][1]), FlatOut(N * Cc, a[16][1])
    ws_bytes, nsplit = a[18], a[19]
    ws = torch.full((max(ws_bytes // 4, 4),), float("nan"), dtype=torch.float32, device=U.DEV)

    def go():
        L.call(name, dtype, N, H, W, Cc, U.ptr(raw_t), U.ptr(st_d), U.ptr(g_d), U.ptr(b_d), act, alpha,
               U.ptr(mask_d) if mask is not None else None, C.byref(g1), C.byref(g2) if g2 is not None else None, C.byref(draw.view),
               dgam.ptr(), dbet.ptr(), U.ptr(ws), ws_bytes, nsplit, U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=N * 3 + H)
        xt = torch.tensor(xd[imgs], requires_grad=True)
        gt = torch.tensor(gamma, dtype=torch.float64)
        bt = torch.tensor(beta, dtype=torch.float64)
        y = (xt - xt.mean(dim=(1, 2), keepdim=True)) * torch.rsqrt(xt.var(dim=(1, 2), unbiased=False, keepdim=True) + eps) * gt + bt
        if mask is not None:
            y = y * torch.tensor(mask[imgs], dtype=torch.float64) * 2.0
        y = torch.where(y > 0, y, alpha * y) if act == L.ACT_LEAKY else (torch.relu(y) if act == L.ACT_RELU else y)
        dy = torch.as_tensor((r1 + r2)[imgs] if a[13] is not None else r1[imgs])
        (y * dy).sum().backward()
        # per-image partials in closed form: dgamma_n = sum dz * xhat, dbeta_n = sum dz, dz = d(loss)/d(gamma * xhat + beta)
        xh = (xd[imgs] - mean[imgs][:, None, None]) / np.sqrt(var[imgs][:, None, None] + eps)
        z = xh * gamma + beta
        drop = mask[imgs] * 2.0 if mask is not None else 1.0
        zm = z * drop
        slope = np.where(zm > 0, 1.0, alpha if act == L.ACT_LEAKY else (0.0 if act == L.ACT_RELU else 1.0))
        dz = dy.numpy() * slope * drop
        fam = "d(raw) " + ("bf16" if dtype == L.BF16 else "f32")
        errs = {fam: SL.per_image_err(draw.region()[imgs], xt.grad.numpy())}
        want_g, want_b = (dz * xh).sum(axis=(1, 2)), dz.sum(axis=(1, 2))
        got_g, got_b = dgam.values().reshape(N, Cc)[imgs], dbet.values().reshape(N, Cc)[imgs]
        errs["dgamma/dbeta"] = max(SL.per_image_err(got_g, want_g), SL.per_image_err(got_b, want_b))
        return errs

    launch = Launch([draw, dgam, dbet], go, evaluate)
    launch.keep = (k1, k2, raw_t, st_d, g_d, b_d, mask_d, ws)
    return launch


def _sprites(rng, N, S):
    """real sprites and a noisy 'fake' of them (f32 NHWC in [-1, 1], alpha channel included)"""
    _, real = DU.synthetic_rgba_batch(rng, N, S, palette_size=24)
    fake = np.clip(real + rng.normal(scale=0.05, size=real.shape), -1, 1).astype(np.float32)
    return np.asarray(real, np.float32), fake


def _hist_ref(img):
    """normalised histograms [n,64,64,3] of f32 images, float64, a few images at a time"""
    return np.concatenate([rg.rgbuv_histogram(torch.tensor(img[i:i + 4], dtype=torch.float64)).numpy()
                           for i in range(0, len(img), 4)])


def _raw_to_norm(raw, N):
    """raw histograms [N][3][64][64] -> [N][64][64][3] divided by the per-image total (p2p_hist_normalize)"""
    r = np.asarray(raw, np.float64).reshape(N, 3, 64, 64).transpose(0, 2, 3, 1)
    return r / r.sum(axis=(1, 2, 3), keepdims=True)


def _points(name, a, rng):
    """p2p_rgbuv_points: the distinct colours of every tile of 1024 pixels with their pixel counts"""
    dtype, N, H, W, _, cap = a[:6]
    real, _ = _sprites(rng, N, H)
    keep, view = in_view(a[4][1], real, dtype, rng)
    pts = FlatOut(N * cap * 4, a[6][1])
    npts = torch.full((N + 64,), -7, dtype=torch.int32, device=U.DEV)

    def go():
        pts.flat[:pts.numel] = 0.0           # entries past npoints[n] are not written
        L.call(name, dtype, N, H, W, C.byref(view), cap, pts.ptr(), U.ptr(npts), U.stream())

    def evaluate():
        assert bool((pts.flat[pts.numel:] == SENTINEL).all()), "points written past N * cap entries"
        got_n = npts[:N].cpu().numpy()
        assert (npts[N:] == -7).all(), "npoints written past N"
        p = pts.values().reshape(N, cap, 4)
        tiles = (H * W + 1023) // 1024
        for n in SL.image_set(N, seed=N):
            rgb = real[n].reshape(-1, 4)[:, :3]
            colours = np.unique(rgb, axis=0)
            k = int(got_n[n])
            if k < 0:
                assert len(colours) > cap // tiles, (n, len(colours))
                continue
            want = {}
            for t in range(tiles):
                u, c = np.unique(rgb[t * 1024:(t + 1) * 1024], axis=0, return_counts=True)
                for col, cnt in zip(map(tuple, u), c):
                    want.setdefault(col, []).append(int(cnt))
            got = {}
            for r in p[n, :k]:
                got.setdefault(tuple(np.float32(r[:3])), []).append(int(r[3]))
            assert sorted(got) == sorted(want) and all(sorted(got[c]) == sorted(want[c]) for c in want), f"image {n}: colour list"
        return {"points": 0.0}

    launch = Launch([], go, evaluate)
    launch.keep = (keep, pts, npts)
    launch.fixed = (pts.flat, npts)
    return launch


def _hist_fwd3(name, a, rng):
    """p2p_rgbuv_hist_fwd3 (with the colour list of p2p_rgbuv_points where the step passes one): raw histograms [N][3][64][64]"""
    dtype, N, H, W = a[:4]
    cap = a[7]
    real, _ = _sprites(rng, N, H)
    keep, view = in_view(a[4][1], real, dtype, rng)
    hist = FlatOut(N * 3 * 64 * 64, a[8][1])
    ws = torch.full((L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4 + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    pts = npts = None
    if a[5] is not None:
        pts = torch.zeros(N * cap * 4 + 4, dtype=torch.float32, device=U.DEV)
        npts = torch.zeros(N, dtype=torch.int32, device=U.DEV)
        L.call("p2p_rgbuv_points", dtype, N, H, W, C.byref(view), cap, U.ptr(pts), U.ptr(npts), U.stream())

    def go():
        L.call(name, dtype, N, H, W, C.byref(view), U.ptr(pts) if pts is not None else None,
               U.ptr(npts) if npts is not None else None, cap, hist.ptr(), U.ptr(ws), U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=N + H)
        got = _raw_to_norm(hist.values(), N)[imgs]
        return {"histogram": SL.per_image_err(got, _hist_ref(real[imgs]))}

    launch = Launch([hist], go, evaluate)
    launch.keep = (keep, ws, pts, npts)
    return launch


def _hist_bwd3(name, a, rng):
    """p2p_rgbuv_hist_hellinger_bwd3: coef * d(sum_n s_n)/d(fake) / sqrt(sq_sum), s_n = sum (sqrt(p_n) - sqrt(t_n))^2 of the
    normalised histograms (histogram.py:84-89; coef = lambda / (2 sqrt(2) B)).  The histogram inputs are produced by
    p2p_rgbuv_hist_fwd3 (checked against f64 by its own re-issue); the gradient is compared with f64 autograd of the oracle."""
    dtype, N, H, W = a[:4]
    coef = a[10]
    real, fake = _sprites(rng, N, H)
    keep_f, fview = in_view(a[4][1], fake, dtype, rng)
    rt = torch.as_tensor(real).to(U.DEV).contiguous()
    rview = L.Tensor(rt.data_ptr(), H * W, W, 4)
    ws = torch.empty(L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4 + 4, dtype=torch.float32, device=U.DEV)
    h_r, h_f = (torch.empty(N * 3 * 64 * 64, dtype=torch.float32, device=U.DEV) for _ in range(2))
    for v, out in ((rview, h_r), (fview, h_f)):
        L.call("p2p_rgbuv_hist_fwd3", dtype, N, H, W, C.byref(v), None, None, 1024, U.ptr(out), U.ptr(ws), U.stream())
    hr, hf = h_r.double().cpu().numpy().reshape(N, -1), h_f.double().cpu().numpy().reshape(N, -1)
    tot_r, tot_f = hr.sum(axis=1), hf.sum(axis=1)
    sq = float(((np.sqrt(hf / tot_f[:, None]) - np.sqrt(hr / tot_r[:, None])) ** 2).sum())
    tot = U.dev(np.stack([tot_r, tot_f]).astype(np.float32))
    sq_d = U.dev(np.array([sq, 0, 0, 0], np.float32))
    gh = torch.full((N * 3 * 64 * 64,), float("nan"), dtype=torch.float32, device=U.DEV)
    dimg = FlatOut(N * H * W * 4, a[12][1])

    def go():
        L.call(name, dtype, N, H, W, C.byref(fview), U.ptr(h_r), U.ptr(h_f), U.ptr(tot[0]), U.ptr(tot[1]), U.ptr(sq_d), coef, U.ptr(gh),
               dimg.ptr(), U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=2 * N + H)
        got = dimg.values().reshape(N, H, W, 4)[imgs]
        assert not got[..., 3].any(), "alpha gradient"
        t_ref = _hist_ref(real[imgs])
        ref = np.zeros_like(got)
        for j in range(0, len(imgs), 4):
            ft = torch.tensor(fake[imgs[j:j + 4]], dtype=torch.float64, requires_grad=True)
            s = ((torch.sqrt(rg.rgbuv_histogram(ft)) - torch.sqrt(torch.tensor(t_ref[j:j + 4]))) ** 2).sum()
            s.backward()
            ref[j:j + 4] = ft.grad.numpy() * coef / np.sqrt(sq)
        return {"hist grad": SL.per_image_err(got, ref)}

    launch = Launch([dimg], go, evaluate)
    launch.keep = (keep_f, rt, ws, h_r, h_f, tot, sq_d, gh)
    return launch


def _head_dgrad(name, a, rng):
    """p2p_head_dgrad: op P, stride 1, of the indexed head into the first `cout` channels of the output view"""
    dtype, N, H, W, ncls, cout = a[:6]
    w_rows = a[8]
    dz = U.q(rng.normal(size=(N, H, W, ncls)), dtype)
    keep, dzv = in_view(a[6][1], dz, dtype, rng)
    w = U.q(rng.normal(scale=1.0 / np.sqrt(16 * ncls), size=(4, 4, cout, ncls)), dtype)
    wn = _prep(dtype, w, cout, ncls, wn_shape=(w_rows, ncls))
    out = OutBuf(a[9][1], N, H, W, cout, U.tdt(dtype), _esz(dtype))

    def go():
        L.call(name, dtype, N, H, W, ncls, cout, C.byref(dzv), U.ptr(wn), w_rows, C.byref(out.view), U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=N + 11)
        return {"out bf16": SL.per_image_err(out.region()[imgs], SL.conv_p(dz[imgs], w, 1))}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep, wn)
    return launch


def _head_softmax(name, a, rng):
    """p2p_head_softmax_cce: Conv2D(ncls, 4, stride 1, SAME, bias) + softmax + CCE + argmax + gradient + bias gradient"""
    dtype, N, H, W, cin_pad, ncls = a[:6]
    gscale, inv = a[11], a[12]
    x = U.q(rng.normal(size=(N, H, W, cin_pad)), dtype)
    keep_x, xv = in_view(a[6][1], x, dtype, rng)
    w = U.q(rng.normal(scale=2.0 / np.sqrt(16 * cin_pad), size=(4, 4, cin_pad, ncls)), dtype)
    wt = _prep(dtype, w, cin_pad, ncls, wt_shape=(ncls, cin_pad))
    bias = (0.1 * rng.normal(size=ncls)).astype(np.float32)
    bias_d = U.dev(bias)
    tgt = rng.integers(0, ncls, size=(N, H, W, 1)).astype(np.float32)
    keep_t, tv = in_view(a[9][1], tgt, dtype, rng)
    fidx = OutBuf(a[10][1], N, H, W, 1, U.tdt(dtype), _esz(dtype))
    dz = OutBuf(a[13][1], N, H, W, ncls, U.tdt(dtype), _esz(dtype))
    outs = [fidx, dz]
    dbias = None
    if a[14] is not None:
        dbias = FlatOut(ncls, a[14][1])
        outs.append(dbias)
    ws = torch.full((L.lib().p2p_head_softmax_workspace_bytes(N, H) // 4 + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    loss = FlatOut(2, a[16][1])
    outs.append(loss)

    def go():
        L.call(name, dtype, N, H, W, cin_pad, ncls, C.byref(xv), U.ptr(wt), U.ptr(bias_d), C.byref(tv), C.byref(fidx.view), gscale, inv,
               C.byref(dz.view), dbias.ptr() if dbias else None, U.ptr(ws), loss.ptr(), U.stream())

    def evaluate():
        imgs = set(SL.image_set(N, seed=N + 13))
        got_dz, got_idx = dz.region(), fidx.region()[..., 0]
        onehot_err = cce = 0.0
        worst_dz, argmax_bad, argmax_n = 0.0, 0, 0
        for j in range(0, N, 8):            # whole batch: the losses are batch sums
            z = SL.conv_g(x[j:j + 8], w, 1) + bias
            zt = torch.tensor(z)
            logp = torch.log_softmax(zt, -1)
            p = logp.exp().numpy()
            ti = tgt[j:j + 8, ..., 0].astype(np.int64)
            cce += float(-np.take_along_axis(logp.numpy(), ti[..., None], -1).sum())
            oh = np.eye(ncls)[ti]
            onehot_err += float(np.abs(oh - p).sum())
            sel = [i - j for i in range(j, min(j + 8, N)) if i in imgs]
            if sel:
                worst_dz = max(worst_dz, SL.per_image_err(got_dz[j:j + 8][sel], gscale * (p - oh)[sel]))
                top2 = np.sort(p[sel], -1)[..., -2:]
                clear = (top2[..., 1] - top2[..., 0]) > 1e-6 * top2[..., 1]
                argmax_bad += int(((got_idx[j:j + 8][sel] != p[sel].argmax(-1)) & clear).sum())
                argmax_n += int(clear.size)
        assert argmax_bad == 0, f"{argmax_bad} of {argmax_n} argmax indices differ from f64"
        lv = loss.values()
        errs = {"out bf16": worst_dz}
        k = N * H * W
        long_k = max(F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24) / F32_TOL       # long-K f32 sums: see _wgrad_family
        errs["loss f32"] = max(abs(lv[0] - inv * cce) / (inv * cce), abs(lv[1] - inv / ncls * onehot_err) / (inv / ncls * onehot_err)) / long_k
        if dbias is not None:       # column sums of the stored (rounded) gradient
            want = got_dz.sum(axis=(0, 1, 2))
            errs["dbias f32"] = float(np.abs(dbias.values() - want).max() / np.abs(want).max()) / long_k
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (keep_x, wt, bias_d, keep_t, ws)
    return launch


CHECKERS = {n: _conv_family for n in ("p2p_igemm", "p2p_igemm_norm_act", "p2p_conv_strip", "p2p_igemm_edge", "p2p_conv_fewin",
                                      "p2p_conv_fewin_actbwd", "p2p_conv_fewout")}
CHECKERS.update({n: _wgrad_family for n in ("p2p_wgemm", "p2p_wgemm_edge", "p2p_wgrad_small")})
CHECKERS.update({"p2p_norm_act_fwd": _norm_fwd, "p2p_norm_act_fwd_tail": _norm_fwd, "p2p_act_bwd": _act_bwd,
                 "p2p_norm_act_bwd": _norm_bwd, "p2p_rgbuv_points": _points, "p2p_rgbuv_hist_fwd3": _hist_fwd3,
                 "p2p_rgbuv_hist_hellinger_bwd3": _hist_bwd3, "p2p_head_dgrad": _head_dgrad, "p2p_head_softmax_cce": _head_softmax})


def _tol(family, dtype):
    if family.startswith("out") or family == "stats f64":
        return OUT_TOL[dtype]
    if family.startswith("d(raw)"):
        return 1e-2 if dtype == L.BF16 else 1e-4       # test_kernels_gpu.py::test_norm_act_fwd_bwd
    if family == "histogram":
        return 1e-4                                     # test_hist_indexed_gpu.py: f32 logf / division against f64
    if family == "hist grad":
        return 2e-3                                     # test_hist_indexed_gpu.py: gradient spanning ~6 decades (1/(x+1e-6))
    if family in ("loss f32", "dbias f32", "points"):
        return F32_TOL          # (loss / bias sums already scaled by the long-K bound; points: exact)
    if family == "norm out":
        return OUT_TOL[dtype]
    if family == "dW f32":
        return F32_TOL          # (already scaled by the long-K bound in _wgrad_family)
    if family == "f32 slabs":
        return F32_TOL
    # statistics (per image and channel: mean error / standard deviation, relative variance error / 5) and the dgamma / dbeta
    # partials (test_kernels_gpu.py: 1e-4)
    return 1e-4


def _reissue(name, dec, seed):
    rng = np.random.default_rng(seed)
    launch = CHECKERS[name](name, dec, rng)
    launch.go()
    torch.cuda.synchronize()
    for o in launch.outs:
        o.check_around(name)
    first = [o.flat.clone() for o in launch.outs]
    fixed = [t.clone() for t in getattr(launch, "fixed", ())]
    for o in launch.outs:
        o.reset()
    launch.go()
    torch.cuda.synchronize()
    for t, f in zip(getattr(launch, "fixed", ()), fixed):
        assert torch.equal(t, f), f"{name}: second launch differs"
    for o, f in zip(launch.outs, first):
        assert torch.equal(o.flat.view(torch.int16) if o.flat.element_size() == 2 else o.flat.view(torch.int32),
                           f.view(torch.int16) if f.element_size() == 2 else f.view(torch.int32)), f"{name}: second launch differs"
    errs = launch.evaluate()
    del launch
    return errs


@pytest.mark.parametrize("cfg,dtype_name", CONFIGS, ids=[f"{c}-{d}" for c, d in CONFIGS])
def test_every_launch_of_the_benchmarked_step_against_f64(cfg, dtype_name):
    uniq, names = harvest(cfg, dtype_name)
    unknown = sorted({n for n in names if n not in CHECKERS and n not in OUT_OF_SCOPE})
    assert not unknown, f"{cfg}: entry points neither re-issued nor listed as out of scope: {unknown}"
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    table, failures = {}, []
    for k, (sig, (name, dec)) in enumerate(sorted(uniq.items(), key=lambda kv: repr(kv[0]))):
        row = table.setdefault(name, {"launches": 0, "worst": {}})
        row["launches"] += 1
        try:
            errs = _reissue(name, dec, seed=1000 + k)
        except AssertionError as e:
            failures.append(f"{name} {dec[:10]}: {e}")
            continue
        for fam, e in errs.items():
            row["worst"][fam] = max(row["worst"].get(fam, 0.0), e)
            if not e < _tol(fam, dtype):
                failures.append(f"{name} {[d for d in dec if not isinstance(d, tuple)][:12]}: {fam} error {e:.3g} >= {_tol(fam, dtype):.3g}")
        torch.cuda.empty_cache()
    print(f"\n[{cfg} {dtype_name}] {len(names)} calls per step, {len(uniq)} unique re-issued launch signatures")
    print(f"  {'entry point':28s} {'launches':>8s}  worst error per family (tolerance)")
    for name in sorted(table):
        r = table[name]
        fams = ", ".join(f"{f} {e:.2e} ({_tol(f, dtype):.0e})" for f, e in sorted(r["worst"].items()))
        print(f"  {name:28s} {r['launches']:8d}  {fams}")
    assert not failures, "\n".join(failures)
    assert table, f"{cfg}: no launch re-issued"


# ---------------------------------------------------------------------------------------------------------------- replay key
def _calls_of(rec):
    return [(n, tuple(int(_val(v)) for t, v in zip(L.SIGNATURES[n], args) if t is C.c_int))
            for n, args in rec if n is not None and n not in ("p2p_event_record", "p2p_stream_wait_event", "p2p_arm_stop_event")]


@pytest.mark.parametrize("attr,dtype,B", [("batch_invariant", L.F32, 8), ("wgemm_pipe", L.BF16, 64)])
def test_recorded_step_issues_what_the_eager_step_issues(attr, dtype, B):
    """batch_invariant and wgemm_pipe choose kernels and K splits when the step is recorded: a recording must not be replayed after
    one of them has changed (engine._replay_key).  Both start off and are switched on: the buffers of the step are sized when it
    first runs, and the switched-off settings need the larger split-K / weight-gradient workspaces."""
    S = 64
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, device=U.DEV, seed=47)
    setattr(eng, attr, False)
    src, tgt = bench.synthetic_batch(0, B, S, None)
    src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)

    def step():
        return eng.train_step_rgba(src_d, tgt_d, 100.0, global_batch=B)

    def eager_calls():
        log = []
        orig = L.call

        def logger(name, *args):
            orig(name, *args)
            log.append((name, args))
        L.call = logger
        try:
            step()
        finally:
            L.call = orig
        return _calls_of(log)

    try:
        step()
        step()                                    # recorded
        assert len(eng._replays) == 1
        before = eager_calls()
        setattr(eng, attr, True)
        after = eager_calls()
        assert after != before, f"flipping {attr} changes no launch at batch {B}: the test shows nothing"
        step()
        step()                                    # eager + recorded under the new setting, or a stale replay
        torch.cuda.synchronize()
        last = next(reversed(eng._replays.values()))[1]
        assert _calls_of(last) == after, f"the step replayed after flipping {attr} is not what an eager step issues"
    finally:
        del eng
        gc.collect()
        torch.cuda.empty_cache()
