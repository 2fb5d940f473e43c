"""The A/B switches (README "Tuning / A-B switches") that send a layer through a different kernel, each run against float64.

The library caches its switches per process, so a setting needs a process of its own:

    python -m tests.switch_routes --setting NAME --mode {query,gpu}

prints one JSON document.  `query` needs no GPU: it asks the library's route queries (include/p2pgan.h "route queries": the
launchers' own decision functions) which instantiation every launch of the setting's cases takes -- tests/test_switch_routes_cpu.py
proves from that, before anything touches a GPU, that a setting moves its cases to another kernel and that every dispatch arm of the
launchers is reached by some case.  `gpu` runs the cases: each direct case through the checker of its entry point in
tests/test_step_launches_gpu.py (seeded operands on test-owned buffers laid out like the described views, NaN in every output
element before the launch, a sentinel in the halo ring / the other channels of the pixels / behind the buffer that must survive,
float64 reference, fused statistics against the f64 moments, a second launch bit-identical) plus a SHA-256 of the output bytes,
and -- the convolutions and weight gradients -- a second time with that checker's operands="lattice" (tests/lattice.py: the
result is exact, every image is compared, the row's "exact" families count the elements that differ from the reference);
the step case through that file's _check_step on an engine with the setting's attribute overrides.
tests/test_switch_routes_gpu.py starts one child per setting.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys

from palette_and_histo_gan_amd import _lib as L
from tests import step_launches as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F = L.BF16, L.F32
G, P_ = L.OP_G, L.OP_P
HALO = 2                    # buffers.HALO: the ring of the engine's haloed buffers
PTR = ("ptr", 0)
_FAKE = 1 << 20             # address of every pointer a query is handed (16-byte aligned; the queries dereference none)


# ---------------------------------------------------------------------------------------------------------------- codes of the header
def header_arms():
    """{launcher: set of codes} from the P2P_*_ARMS lists of include/p2pgan.h, composed with the header's own P2P_*_ROUTE macros
    (evaluated as Python expressions)"""
    text = open(os.path.join(ROOT, "include", "p2pgan.h")).read()
    text = text.replace("\\\n", " ")
    macros = {}
    for m in re.finditer(r"^#define (P2P_\w+)\(([^)]*)\)\s+(.*)$", text, flags=re.M):
        name, params, body = m.group(1), [p.strip() for p in m.group(2).split(",")], m.group(3)
        body = re.sub(r"/\*.*?\*/", "", body)
        macros[name] = (params, body)

    def call(name, args):
        params, body = macros[name]
        return int(eval(body, {"__builtins__": {}}, dict(zip(params, args))))

    def arms(list_name):
        body = macros[list_name][1]
        return [tuple(int(x) for x in m.group(1).split(",")) for m in re.finditer(r"X\(([^)]*)\)", body)]

    out = {
        "igemm": {call("P2P_IGEMM_ROUTE", a + (wm,)) for a in arms("P2P_IGEMM_ARMS") for wm in (0, 1)},
        "brig": {call("P2P_BRIG_ROUTE", a) for a in arms("P2P_BRIG_ARMS")},
        "wgemm": {a[0] for a in arms("P2P_WGEMM_ARMS")},
        "ws": {call("P2P_WS_ROUTE", a) for a in arms("P2P_WS_ARMS")},
        "norm_fwd": {call("P2P_NORM_ROUTE", a + (0,)) for a in arms("P2P_NORM_FWD_ARMS")},
        "norm_bwd": {call("P2P_NORM_ROUTE", a + (0,)) for a in arms("P2P_NORM_BWD_ARMS")},
    }
    out["_compose"] = call
    return out


def arm_of(launcher, code):
    """the dispatch arm of a code: the normalisation codes also carry the channel group, a launch argument (P2P_NORM_ROUTE_ARM)"""
    return code & 0xff if launcher in ("norm_fwd", "norm_bwd") else code


def describe(launcher, code):
    """a route code in words"""
    if code < 0:
        return "refused"
    if launcher == "igemm":
        if code == 0:
            return "-> brig"
        fam = {1: "igemm_kernel", 2: "igemm_kernel<GEN>", 3: "igemm_pipe<G>", 4: "igemm_pipe<P>"}[code & 7]
        tile = ("128x128", "256x128", "128x64", "256x64", "128x32", "256x32")[(code >> 3) & 7]
        return f"{fam} {tile} kg{((code >> 6) & 1) + 1} nst{((code >> 7) & 3) + 2}" + (" w_major" if code >> 9 else "")
    if launcher == "brig":
        if code == 0:
            return "not offered"
        return (f"brig op {'P' if code & 2 else 'G'} cbw{((code >> 2) & 1) + 1}" + ("" if code & 8 else " no-stagger") +
                (" fused-norm" if code & 16 else ""))
    if launcher == "wgemm":
        return ("wgemm_pipe", "128x128", "64x128", "32x128", "64x64", "32x64", "64x32", "32x32")[code]
    if launcher == "ws":
        return (f"ws s{(code & 1) + 1} {('1x1', '1x2', '1x4', '2x1', '2x2')[(code >> 1) & 7]} {16 if code & 16 else 8} waves"
                f" pack{(code >> 5) & 3}" + (" swizzle" if code & 128 else ""))
    form = ("scalar", "small", "reg", "vec0", "vec1+2", "vec3")[code & 7]
    return f"{form} ppl{(code >> 3) & 15}" + (" slabs" if code & 128 else "") + (f" CG{1 << (code >> 8)}" if code >> 8 else "")


# ---------------------------------------------------------------------------------------------------------------- routes of a launch
def _view(d):
    d = d[1]
    return L.Tensor(_FAKE + d.get("align", 0), d["img_stride"], d["row_stride"], d["ld"])


def _gs(d):
    if d is None:
        return None
    d = d[1]
    return C.byref(L.GSrc(_FAKE + d.get("align", 0), d["kind"], d["nslabs"], d["slab_stride"], d["ld"], d["coff"]))


def _p(d):
    return None if d is None else C.c_void_p(_FAKE + d[1])


def routes(name, dec):
    """[(launcher, code)] of a decoded launch (tests/step_launches.decode, or a hand-written one): what the launcher of the entry
    point would start.  Entry points without a route query give []."""
    lib = L.lib()
    if name == "p2p_igemm":
        op, dtype, N, LH, LW, cg, cd = dec[:7]
        hi, lo = _view(dec[7]), _view(dec[8])
        code = lib.p2p_igemm_route(op, dtype, N, LH, LW, cg, cd, C.byref(hi), C.byref(lo), dec[10], int(dec[12] is not None))
        if code == 0:
            return [("igemm", 0), ("brig", lib.p2p_brig_route(op, dtype, N, LH, LW, cg, cd, 0))]
        return [("igemm", code)]
    if name == "p2p_igemm_norm_act":
        return [("brig", lib.p2p_brig_route(*dec[:7], 1))]
    if name == "p2p_igemm_edge":
        i, o = _view(dec[9]), _view(dec[10])
        return [("igemm", lib.p2p_igemm_edge_route(*dec[:9], C.byref(i), C.byref(o), int(dec[12] is not None), dec[13]))]
    if name in ("p2p_wgemm", "p2p_wgemm_edge"):
        if name == "p2p_wgemm":
            dtype, stride, shape, hi, lo, ms = dec[0], 2, dec[1:6], _view(dec[6]), _view(dec[7]), dec[9]
        else:
            dtype, stride, shape, hi, lo, ms = dec[0], dec[1], dec[2:7], _view(dec[7]), _view(dec[8]), dec[10]
        return [("wgemm", lib.p2p_wgemm_route(dtype, stride, *shape, C.byref(hi), C.byref(lo), ms))]
    if name == "p2p_wgrad_small":
        return [("ws", lib.p2p_wgrad_small_route(*dec[:7], dec[7][1]["ld"], dec[8][1]["ld"]))]
    if name in ("p2p_norm_act_fwd", "p2p_norm_act_fwd_tail"):
        out = _view(dec[15])
        tail = _view(dec[21]) if name == "p2p_norm_act_fwd_tail" else None
        code = lib.p2p_norm_act_fwd_route(*dec[:5], _p(dec[5]), dec[6], dec[7], dec[8], _p(dec[9]), _p(dec[10]), C.byref(out), _p(dec[16]),
                                          _p(dec[17]), _p(dec[18]), dec[19], dec[20], C.byref(tail) if tail is not None else None,
                                          dec[22] if tail is not None else 0)
        return [("norm_fwd", code)]
    if name == "p2p_norm_act_bwd":
        draw = _view(dec[14])
        code = lib.p2p_norm_act_bwd_route(*dec[:5], _p(dec[5]), _p(dec[6]), _p(dec[7]), _p(dec[8]), _gs(dec[12]), _gs(dec[13]), C.byref(draw),
                                          _p(dec[15]), _p(dec[16]), _p(dec[17]), dec[18], dec[19])
        return [("norm_bwd", code)]
    return []


# ---------------------------------------------------------------------------------------------------------------- direct cases
def _vd(h, w, ld, coff=0, halo=0, esz=2):
    rs = w + 2 * halo
    return ("view", {"img_stride": (h + 2 * halo) * rs, "row_stride": rs, "ld": ld, "align": (coff * esz) % 16, "coff": coff,
                     "pix": halo * rs + halo})


def _esz(dtype):
    return 2 if dtype == BF else 4


def igemm(op, dtype, n, lh, cg, cd, sk=1, stats=False, wide=0):
    """p2p_igemm on lh x lh lo maps: the gathered view haloed, the output dense (what a raw convolution result is) or, with wide,
    a channel slice behind `wide` other channels of a haloed buffer (concat by slice)"""
    e = _esz(dtype)
    hi_c, lo_c = cg, cd
    if op == G:
        hi, lo = _vd(2 * lh, 2 * lh, hi_c, halo=HALO, esz=e), (_vd(lh, lh, cd + wide, coff=wide, halo=HALO, esz=e) if wide else _vd(lh, lh, lo_c, esz=e))
    else:
        hi = _vd(2 * lh, 2 * lh, cg + wide, coff=wide, halo=HALO, esz=e) if wide else _vd(2 * lh, 2 * lh, hi_c, esz=e)
        lo = _vd(lh, lh, lo_c, halo=HALO, esz=e)
    return ("p2p_igemm", [op, dtype, n, lh, lh, cg, cd, hi, lo, PTR, sk, PTR if sk > 1 else None, "auto" if stats == "auto" else (PTR if stats else None), None])


def igemm_block(op, dtype, n, lh, cg, cd, act):
    """p2p_igemm_norm_act: raw result dense, activated output into a channel slice of a wider haloed buffer"""
    e = _esz(dtype)
    res, nout = (lh, cd) if op == G else (2 * lh, cg)
    hi = _vd(2 * lh, 2 * lh, cg, halo=HALO, esz=e) if op == G else _vd(2 * lh, 2 * lh, cg, esz=e)
    lo = _vd(lh, lh, cd, esz=e) if op == G else _vd(lh, lh, cd, halo=HALO, esz=e)
    return ("p2p_igemm_norm_act", [op, dtype, n, lh, lh, cg, cd, hi, lo, PTR, PTR, PTR, 1e-3, act, 0.3,
                                   _vd(res, res, nout + 32, coff=32, halo=HALO, esz=e), PTR, None])


def edge(op, stride, dtype, n, lh, cin_pad, ncols, bias=False, act=L.ACT_NONE, wide=0):
    """p2p_igemm_edge: haloed input of cin_pad channels, output a channel slice (behind `wide` channels) of a haloed buffer"""
    e = _esz(dtype)
    s_in, s_out = (stride, 1) if op == G else (1, stride)
    out_ld = (ncols + wide + 7) // 8 * 8
    return ("p2p_igemm_edge", [op, stride, dtype, n, lh, lh, cin_pad, ncols, (ncols + 31) // 32 * 32,
                               _vd(s_in * lh, s_in * lh, cin_pad, halo=HALO, esz=e), _vd(s_out * lh, s_out * lh, out_ld, coff=wide, halo=HALO, esz=e),
                               PTR, PTR if bias else None, act, 0.3, None])


def wgemm(dtype, n, lh, cg, cd, ms):
    e = _esz(dtype)
    return ("p2p_wgemm", [dtype, n, lh, lh, cg, cd, _vd(2 * lh, 2 * lh, cg, halo=HALO, esz=e), _vd(lh, lh, cd, halo=HALO, esz=e), PTR, ms,
                          PTR if ms > 1 else None, None])


def wgemm_edge(dtype, stride, n, lh, cg, cd, ms):
    e = _esz(dtype)
    pad = lambda c: (c + 7) // 8 * 8
    return ("p2p_wgemm_edge", [dtype, stride, n, lh, lh, cg, cd, _vd(stride * lh, stride * lh, pad(cg), halo=HALO, esz=e),
                               _vd(lh, lh, pad(cd), halo=HALO, esz=e), PTR, ms, PTR if ms > 1 else None, None])


def wsmall(dtype, stride, n, lh, cg, cd):
    e = _esz(dtype)
    pad = lambda c: (c + 7) // 8 * 8
    return ("p2p_wgrad_small", [dtype, stride, n, lh, lh, cg, cd, _vd(stride * lh, stride * lh, pad(cg), halo=HALO, esz=e),
                                _vd(lh, lh, pad(cd), halo=HALO, esz=e), PTR, PTR, None])


def norm_fwd(dtype, n, h, c, nslabs=0, mask=False, nsplit=1, act=L.ACT_LEAKY, pad=8, norm=True):
    """p2p_norm_act_fwd: dense input (nslabs 0) or split-K slabs, output into channels [pad, pad + c) of a haloed buffer"""
    e = _esz(dtype)
    kind = 2 if nslabs else 1
    ws_bytes = n * 16 * c * 2 * 4
    return ("p2p_norm_act_fwd", [dtype, n, h, h, c, PTR, kind, max(nslabs, 1), n * h * h * c if nslabs else 0, PTR if norm else None,
                                 PTR if norm else None, 1e-3, act, 0.3, PTR if mask else None, _vd(h, h, c + pad, coff=pad, halo=HALO, esz=e),
                                 PTR if nslabs else None, PTR if norm else None, PTR, ws_bytes, nsplit, None])


def norm_bwd(dtype, n, h, c, slabs=False, mask=False, nsplit=1, act=L.ACT_LEAKY):
    """p2p_norm_act_bwd: first gradient source dense at a channel offset, the second (optional) f32 slabs; d(raw) haloed"""
    e = _esz(dtype)
    g1 = ("gsrc", {"kind": 1, "nslabs": 0, "slab_stride": 0, "ld": c + 8, "coff": 8, "align": 0})
    g2 = ("gsrc", {"kind": 2, "nslabs": 5, "slab_stride": n * h * h * c, "ld": c, "coff": 0, "align": 0}) if slabs else None
    ws_bytes = n * 16 * c * 2 * 4
    return ("p2p_norm_act_bwd", [dtype, n, h, h, c, PTR, PTR, PTR, PTR, act, 0.3, PTR if mask else None, g1, g2,
                                 _vd(h, h, c, halo=HALO, esz=e), PTR, PTR, PTR, ws_bytes, nsplit, None])


def block(op, dtype, n, lh, cg, cd, act):
    """conv + InstanceNorm + activation of one block as the engine issues it: the fused launch where p2p_igemm_norm_act_ok offers
    it, else p2p_igemm with fused statistics (where the layer has slots) + p2p_norm_act_fwd over them"""
    return ("block", [op, dtype, n, lh, cg, cd, act])


def resolve(case):
    """a case -> the [(name, dec)] launches it makes under the switches of this process"""
    name, dec = case
    lib = L.lib()
    if name == "p2p_igemm" and dec[12] == "auto":         # fused statistics where the layer's kernel has slots for them (as the engine asks)
        dec = list(dec)
        dec[12] = PTR if dec[10] == 1 and lib.p2p_igemm_layer_stat_slots(*dec[:7]) > 0 else None
        return [(name, dec)]
    if name != "block":
        return [(name, dec)]
    op, dtype, n, lh, cg, cd, act = dec
    if lib.p2p_igemm_norm_act_ok(op, dtype, n, lh, lh, cg, cd):
        return [igemm_block(op, dtype, n, lh, cg, cd, act)]
    res, nout = (lh, cd) if op == G else (2 * lh, cg)
    conv = resolve(igemm(op, dtype, n, lh, cg, cd, stats="auto"))[0]
    slots = lib.p2p_igemm_layer_stat_slots(op, dtype, n, lh, lh, cg, cd) if conv[1][12] is not None else 0
    nf = norm_fwd(dtype, n, res, nout, nsplit=-slots if slots else 1, act=act, pad=32)
    if slots:
        nf[1][19] = n * slots * nout * 2 * 4          # ws = the statistics slots of the convolution
    return [conv, nf]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _igemm_small(dtypes=(BF, F)):
    """the smallest stride-2 launches the pipelined kernel takes by default: K bytes per tap 128 (bf16; f32 256), 128 columns"""
    out = []
    for dt in dtypes:
        t = "bf16" if dt == BF else "f32"
        for n, lh in ((2, 4), (3, 8)):
            for sk in (1, 4):
                out.append((f"igemm G 64->128 {lh}x{lh} n{n} sk{sk} {t}", igemm(G, dt, n, lh, 64, 128, sk)))
                out.append((f"igemm P 128<-64 {lh}x{lh} n{n} sk{sk} {t}", igemm(P_, dt, n, lh, 128, 64, sk)))
        # fused statistics: whole 128-row AND whole 256-row tiles (M = 256), so that P2P_IGEMM_BIG=1 keeps them
        out.append((f"igemm G 64->128 8x8 n4 stats {t}", igemm(G, dt, 4, 8, 64, 128, 1, stats="auto")))
        out.append((f"igemm P 128<-64 4x4 n16 stats {t}", igemm(P_, dt, 16, 4, 128, 64, 1, stats="auto")))
        out.append((f"igemm G 128->256 4x4 n3 slice {t}", igemm(G, dt, 3, 4, 128, 256, 1, wide=64)))
        out.append((f"igemm P 256<-128 4x4 n2 slice {t}", igemm(P_, dt, 2, 4, 256, 128, 1, wide=64)))
    return out


WS_PACKED = [(f"ws {cg}->{cd} s{s} {lh}x{lh} n{n} bf16", wsmall(BF, s, n, lh, cg, cd))
             for cg, cd, s in ((4, 64, 2), (8, 64, 2), (36, 4, 1), (64, 1, 1)) for n, lh in ((2, 32), (3, 64))]
WS_UNPACKED = [(f"ws {cg}->{cd} s{s} {lh}x{lh} n{n} {'bf16' if dt == BF else 'f32'}", wsmall(dt, s, n, lh, cg, cd))
               for dt, cg, cd, s, n, lh in ((BF, 32, 64, 2, 2, 32), (BF, 64, 32, 2, 3, 32), (BF, 64, 64, 2, 2, 32), (BF, 32, 128, 2, 2, 16),
                                            (BF, 32, 32, 2, 3, 32), (BF, 64, 64, 1, 2, 32), (BF, 32, 64, 1, 3, 16), (BF, 64, 32, 1, 2, 32),
                                            (BF, 32, 128, 1, 2, 32))]
# (32 -> 32 at stride 1: 64-byte pixels on both sides, which the swizzle leaves in natural order; 8 -> 64 at stride 1: packed)
WS_PLAIN = [("ws 32->32 s1 64x64 n2 bf16", wsmall(BF, 1, 2, 64, 32, 32))]
WS_PACKED_S1 = [("ws 8->64 s1 32x32 n2 bf16", wsmall(BF, 1, 2, 32, 8, 64))]
WS_F32 = [(f"ws {cg}->{cd} s{s} {lh}x{lh} n{n} f32", wsmall(F, s, n, lh, cg, cd))
          for cg, cd, s, n, lh in ((32, 64, 2, 2, 32), (64, 32, 2, 3, 32), (64, 64, 2, 2, 32), (32, 128, 2, 2, 16), (32, 32, 2, 3, 32),
                                   (64, 64, 1, 2, 32), (32, 64, 1, 3, 16), (64, 32, 1, 2, 32), (32, 128, 1, 2, 32), (32, 32, 1, 2, 64))]
WGEMM_PIPE = [(f"wgemm {cg}x{cd} 8x8 n2 msplit {ms} bf16", wgemm(BF, 2, 8, cg, cd, ms)) for cg, cd in ((128, 128), (128, 256)) for ms in (1, 2)]

_NORM_SHAPES = [(c, h) for c in (32, 64, 256) for h in (8, 16, 32)]       # (64x64 maps never take the register forms: nothing to move)
NORM_FWD = ([(f"norm fwd C{c} {h}x{h} n3 dense bf16", norm_fwd(BF, 3, h, c)) for c, h in _NORM_SHAPES] +
            [(f"norm fwd C{c} {h}x{h} n9 slabs mask bf16", norm_fwd(BF, 9, h, c, nslabs=3, mask=True, act=L.ACT_RELU, nsplit=4)) for c, h in _NORM_SHAPES] +
            [("norm fwd C64 16x16 n3 dense mask f32", norm_fwd(F, 3, 16, 64, mask=True, nsplit=2)), ("norm fwd C32 8x8 n9 slabs f32", norm_fwd(F, 9, 8, 32, nslabs=5))])
NORM_BWD = ([(f"norm bwd C{c} {h}x{h} n3 bf16", norm_bwd(BF, 3, h, c)) for c, h in _NORM_SHAPES] +
            [(f"norm bwd C{c} {h}x{h} n9 slabs mask bf16", norm_bwd(BF, 9, h, c, slabs=True, mask=True, act=L.ACT_RELU, nsplit=4)) for c, h in _NORM_SHAPES] +
            [("norm bwd C64 16x16 n3 mask f32", norm_bwd(F, 3, 16, 64, mask=True, nsplit=2)), ("norm bwd C32 8x8 n9 slabs f32", norm_bwd(F, 9, 8, 32, slabs=True))])

# the shapes of test_kernels_gpu.py::test_igemm_block_resident_wide_maps / test_fused_block_conv_instance_norm_activation
_BRIG_SHAPES = [(P_, 3, 8, 64, 64), (P_, 5, 8, 128, 32), (P_, 9, 8, 64, 96), (P_, 2, 16, 64, 96), (P_, 1, 16, 128, 64), (P_, 2, 32, 64, 32),
                (P_, 1, 64, 64, 32), (G, 3, 8, 32, 256), (G, 5, 8, 64, 256), (G, 2, 16, 64, 256), (G, 1, 16, 96, 512), (G, 2, 32, 32, 256),
                (G, 1, 64, 32, 256), (G, 2, 16, 64, 128)]
_BLOCK_SHAPES = [(P_, 5, 8, 128, 64, L.ACT_RELU), (P_, 2, 16, 64, 96, L.ACT_RELU), (G, 3, 8, 64, 256, L.ACT_LEAKY), (G, 2, 16, 32, 256, L.ACT_LEAKY)]


def _opn(op):
    return "G" if op == G else "P"


BRIG_G = [(f"brig G {cg}->{cd} {lh}x{lh} n{n}", igemm(op, BF, n, lh, cg, cd, stats="auto")) for op, n, lh, cg, cd in _BRIG_SHAPES if op == G]
BRIG_P = [(f"brig P {cg}<-{cd} {lh}x{lh} n{n}", igemm(op, BF, n, lh, cg, cd, stats="auto")) for op, n, lh, cg, cd in _BRIG_SHAPES if op == P_]
BRIG_SLICE = [(f"brig {_opn(op)} {cg}/{cd} {lh}x{lh} n{n} slice", igemm(op, BF, n, lh, cg, cd, wide=64)) for op, n, lh, cg, cd in _BRIG_SHAPES[2:4] + _BRIG_SHAPES[8:10]]
BRIG_CBW2 = [(f"brig {_opn(op)} {cg}/{cd} {lh}x{lh} n{n}", igemm(op, BF, n, lh, cg, cd, stats="auto"))
             for op, n, lh, cg, cd in _BRIG_SHAPES if (cg if op == P_ else cd) % (64 if op == P_ else 256) == 0]
BLOCKS = [(f"block {_opn(op)} {cg}/{cd} {lh}x{lh} n{n}", block(op, BF, n, lh, cg, cd, act)) for op, n, lh, cg, cd, act in _BLOCK_SHAPES]
BLOCKS_CBW2 = [(i, c) for (i, c), s in zip(BLOCKS, _BLOCK_SHAPES) if (s[3] if s[0] == P_ else s[4]) % (64 if s[0] == P_ else 256) == 0]

# launches that fill 256-row tiles / lose the second K group by the launcher's default thresholds
IGEMM_BIG = [("igemm G 64->128 8x8 n256 sk4 bf16", igemm(G, BF, 256, 8, 64, 128, 4)), ("igemm P 128<-64 4x4 n256 sk4 bf16", igemm(P_, BF, 256, 4, 128, 64, 4))]
IGEMM_KG1 = [("igemm G 64->128 16x16 n49 sk4 bf16", igemm(G, BF, 49, 16, 64, 128, 4)), ("igemm P 128<-64 8x8 n49 sk4 bf16", igemm(P_, BF, 49, 8, 128, 64, 4))]
IGEMM_F32_WIDE = [("igemm G 64->128 8x8 n256 sk4 f32", igemm(G, F, 256, 8, 64, 128, 4)), ("igemm G 64->128 16x16 n49 sk4 f32", igemm(G, F, 49, 16, 64, 128, 4))]

# arms of igemm_kernel that neither the suite's default tests nor a switch reach: the generic kernel on 128-column tiles with a
# short K (two LDS stages) in both block orders, the 256 x 64 tile of the power-of-two kernel (>= 131072 rows), its 128 x 32 tile
# with two stages in weight-major order
IGEMM_MORE = [("edge G 8->128 s2 8x8 n2 bf16", edge(G, 2, BF, 2, 8, 8, 128, bias=True, act=L.ACT_LEAKY, wide=8)),
              ("edge G 8->128 s2 16x16 n16 bf16", edge(G, 2, BF, 16, 16, 8, 128)),
              ("edge G 40->256 s1 4x4 n1 bf16", edge(G, 1, BF, 1, 4, 40, 256, bias=True, act=L.ACT_LEAKY, wide=8)),
              ("igemm G 32->32 4x4 n2 sk8 bf16", igemm(G, BF, 2, 4, 32, 32, 8)),
              ("igemm G 32->64 32x32 n128 bf16", igemm(G, BF, 128, 32, 32, 64, 1))]
WGEMM_MORE = [(f"wgemm {c}x{c} 8x8 n3 {'bf16' if dt == BF else 'f32'}", wgemm(dt, 3, 8, c, c, 1)) for dt in (BF, F) for c in (64, 32)]
NORM_MORE = [("norm fwd C64 32x32 n2 slabs wide groups bf16", norm_fwd(BF, 2, 32, 64, nslabs=2, nsplit=0x204))]

GROUPS = {"igemm_more": IGEMM_MORE, "igemm_gen": IGEMM_MORE[:3], "wgemm_more": WGEMM_MORE, "norm_more": NORM_MORE, "ws_plain": WS_PLAIN, "ws_packed_s1": WS_PACKED_S1,
          "igemm_small": _igemm_small(), "igemm_small_bf16": _igemm_small((BF,)), "igemm_big": IGEMM_BIG, "igemm_kg1": IGEMM_KG1,
          "igemm_f32_wide": IGEMM_F32_WIDE, "ws_packed": WS_PACKED, "ws_unpacked": WS_UNPACKED, "ws_f32": WS_F32, "wgemm_pipe": WGEMM_PIPE,
          "norm_fwd": NORM_FWD, "norm_bwd": NORM_BWD, "brig_g": BRIG_G, "brig_p": BRIG_P, "brig_slice": BRIG_SLICE, "brig_cbw2": BRIG_CBW2,
          "blocks": BLOCKS, "blocks_cbw2": BLOCKS_CBW2}


# ---------------------------------------------------------------------------------------------------------------- the settings
# name: (environment, engine attribute overrides, baseline row, direct case groups, step case (model, S, dtype name, B) or None)
# The baseline row is the setting a case's route and output hash are compared with: `default`, or -- for the block-resident kernel,
# which the product keeps for launches of >= 160 workgroups -- `brig_min_wg` / `brig_cbw2`, the default with P2P_BRIG_MIN_WG=1 (and
# P2P_BRIG_CBW=2) as tests/test_kernels_gpu.py sets them to reach that kernel at small batches.
_MW = {"P2P_BRIG_MIN_WG": "1"}
_BASE64 = ("baseline", 64, "bf16")
SETTINGS = {
    "default": ({}, {}, None, ["igemm_small", "igemm_big", "igemm_kg1", "igemm_f32_wide", "ws_packed", "ws_unpacked", "ws_f32", "wgemm_pipe",
                               "norm_fwd", "norm_bwd", "igemm_more", "wgemm_more", "norm_more", "ws_plain", "ws_packed_s1"], None),
    "brig_min_wg": (_MW, {}, None, ["brig_g", "brig_p", "brig_slice", "blocks"], None),
    "brig_cbw2": (dict(_MW, P2P_BRIG_CBW="2"), {}, None, ["brig_cbw2", "blocks_cbw2"], None),
    # ---- library
    "P2P_IGEMM_PIPE=0": ({"P2P_IGEMM_PIPE": "0"}, {}, "default", ["igemm_small", "igemm_big", "igemm_kg1"], _BASE64 + (1,)),
    "P2P_IGEMM_PIPE=2": ({"P2P_IGEMM_PIPE": "2"}, {}, "default", ["igemm_kg1"], _BASE64 + (49,)),
    "P2P_IGEMM_PIPE=3": ({"P2P_IGEMM_PIPE": "3"}, {}, "default", ["igemm_small_bf16"], _BASE64 + (1,)),
    # (4 differs from the automatic choice in f32 without fused statistics only, where 1 pins one variant: engine.batch_invariant)
    "P2P_IGEMM_PIPE=4": ({"P2P_IGEMM_PIPE": "4"}, {}, "default", ["igemm_f32_wide"], None),
    "P2P_IGEMM_BIG=0": ({"P2P_IGEMM_BIG": "0"}, {}, "default", ["igemm_big"], _BASE64 + (49,)),
    "P2P_IGEMM_BIG=1": ({"P2P_IGEMM_BIG": "1"}, {}, "default", ["igemm_small_bf16", "igemm_gen"], _BASE64 + (1,)),
    "P2P_IGEMM_PIPE=0+BIG=1": ({"P2P_IGEMM_PIPE": "0", "P2P_IGEMM_BIG": "1"}, {}, "default", ["igemm_small"], _BASE64 + (1,)),
    "P2P_IGEMM_WMAJOR=0": ({"P2P_IGEMM_WMAJOR": "0"}, {}, "default", ["igemm_small"], _BASE64 + (1,)),
    "P2P_WS_PACK=0": ({"P2P_WS_PACK": "0"}, {}, "default", ["ws_packed", "ws_packed_s1"], _BASE64 + (1,)),
    "P2P_WS_W16=0": ({"P2P_WS_W16": "0"}, {}, "default", ["ws_unpacked", "ws_plain", "ws_f32"], _BASE64 + (1,)),
    "P2P_WS_SWIZZLE=0": ({"P2P_WS_SWIZZLE": "0"}, {}, "default", ["ws_unpacked"], _BASE64 + (1,)),
    "P2P_WS_W16=0+SWIZZLE=0": ({"P2P_WS_W16": "0", "P2P_WS_SWIZZLE": "0"}, {}, "default", ["ws_unpacked"], None),
    "P2P_WGEMM_PIPE=0": ({"P2P_WGEMM_PIPE": "0"}, {}, "default", ["wgemm_pipe"], _BASE64 + (16,)),
    "P2P_NORM_FWD_REG=0": ({"P2P_NORM_FWD_REG": "0"}, {}, "default", ["norm_fwd"], _BASE64 + (1,)),
    "P2P_NORM_BWD_REG=0": ({"P2P_NORM_BWD_REG": "0"}, {}, "default", ["norm_bwd"], _BASE64 + (1,)),
    "P2P_BRIG=0": (dict(_MW, P2P_BRIG="0"), {}, "brig_min_wg", ["brig_g", "brig_p", "brig_slice", "blocks"], _BASE64 + (16,)),
    "P2P_BRIG=1": (dict(_MW, P2P_BRIG="1"), {}, "brig_min_wg", ["brig_p"], _BASE64 + (16,)),
    "P2P_BRIG=2": (dict(_MW, P2P_BRIG="2"), {}, "brig_min_wg", ["brig_g"], _BASE64 + (16,)),
    "P2P_BRIG_STAGGER=0": (dict(_MW, P2P_BRIG_STAGGER="0"), {}, "brig_min_wg", ["brig_g", "brig_p", "brig_slice", "blocks"], _BASE64 + (16,)),
    "P2P_BRIG_STAGGER=0+CBW=2": (dict(_MW, P2P_BRIG_STAGGER="0", P2P_BRIG_CBW="2"), {}, "brig_cbw2", ["brig_cbw2", "blocks_cbw2"], None),
    "P2P_BRIG_FUSE_NORM=0": (dict(_MW, P2P_BRIG_FUSE_NORM="0"), {}, "brig_min_wg", ["blocks"], _BASE64 + (16,)),
    # ---- engine (attribute overrides; the step case is the whole check)
    "use_conv_strip=False": ({}, {"use_conv_strip": False}, "default", [], _BASE64 + (1,)),
    "use_conv_fewin=False": ({}, {"use_conv_fewin": False}, "default", [], _BASE64 + (1,)),
    "use_conv_fewout=False": ({}, {"use_conv_fewout": False}, "default", [], _BASE64 + (1,)),
    "use_head_fused=False": ({}, {"use_head_fused": False}, "default", [], ("indexed", 64, "bf16", 1)),
    "fuse_act_bwd=0": ({}, {"fuse_act_bwd": 0}, "default", [], _BASE64 + (1,)),
    "split_prep=0": ({}, {"split_prep": 0}, "default", [], _BASE64 + (1,)),
    "wgemm_pipe=False": ({}, {"wgemm_pipe": False}, "default", [], _BASE64 + (32,)),
    "splitk_target=64": ({}, {"splitk_target": 64}, "default", [], _BASE64 + (17,)),
    "splitk_target=512": ({}, {"splitk_target": 512}, "default", [], _BASE64 + (1,)),
}
BASELINES = ("default", "brig_min_wg", "brig_cbw2")

# Switches that are no setting here, with the reason
LEFT_OUT = {
    "P2P_WS_ABL": "diagnostic: computes wrong results on purpose (staging only / contraction only)",
    "P2P_WS_WANT, P2P_WS_WANT_PACK, P2P_WGEMM_WANT, P2P_WGEMM_WANT_PIPE": "grid size (workgroups wanted per launch) only: the same kernel",
    "P2P_NORM_REG_WGS": "grid size only: which channel group width the register forms take, a launch argument of the same kernels",
    "P2P_BRIG_MIN_WG": "grid-size threshold of the block-resident kernel; no setting of its own, part of every P2P_BRIG* row",
    "P2P_WGEMM_PIPE_MAXWG": "grid-size cap of the pipelined weight-gradient kernel: picks no kernel the P2P_WGEMM_PIPE rows do not",
    "P2P_WS_TH_PACK": "strip height of the packed layers: a launch argument of the same kernel",
}

# Switches whose kernels compute every sum in the same order as the default's and must therefore give BIT-IDENTICAL outputs (the
# case hashes equal the baseline child's), with what was read to decide so
BIT_IDENTICAL = {
    "P2P_IGEMM_WMAJOR=0": "igemm.hip: w_major only maps blockIdx to (row tile, column tile, z); a tile's K loop and epilogue do not depend on it",
    "P2P_BRIG_STAGGER=0": "brig.hip: a.stagger only delays the weight-ring DMA issue of waves 4-7 behind their first MFMA group",
    "P2P_BRIG_STAGGER=0+CBW=2": "as P2P_BRIG_STAGGER=0, on the 64-channels-per-wave form",
    "P2P_WS_SWIZZLE=0": "wgrad_small.hip: mh / ml only permute where a 64-byte chunk of a pixel sits in the LDS strip (ws_swz); every "
                        "MFMA gets the same operands in the same order",
}
# ... and the engine switches that only move work between launches: the STEP's results (losses and every parameter after two
# steps) must be bit-identical to the default engine's
STEP_BIT_IDENTICAL = {
    "fuse_act_bwd=0": "p2p_conv_fewin_actbwd is bit-identical to p2p_conv_fewin + p2p_act_bwd (include/p2pgan.h; "
                      "test_kernels_gpu.py::test_conv_fewin_actbwd_equals_conv_then_act_bwd)",
    "split_prep=0": "the same weight-copy launches over the same masters, issued at another point of the step",
}


# Settings whose step the meta-device census cannot tell from the default's, with the reason: for these the recorded steps of the GPU
# children are compared instead (tests/test_switch_routes_gpu.py)
CENSUS_BLIND = {
    "use_head_fused=False": "p2p_head_softmax_ok asks the device for its LDS limit: without a GPU the census takes the generic head anyway",
    "split_prep=0": "the early Adam part (engine._adam_head) waits for an event of the weight-gradient stream, which a meta-device step has not",
}


def cases_of(setting):
    return [c for g in SETTINGS[setting][3] for c in GROUPS[g]]


# ---------------------------------------------------------------------------------------------------------------- the default tests' shapes
def kernel_test_cases():
    """the launches of tests/test_kernels_gpu.py's parametrisations that go through a launcher with a route query, as cases (for the
    routes only: what the default settings already run against f64)"""
    out = []
    for dt in (F, BF):
        e = _esz(dt)
        for n, lh, cg, cd, splitk in [(2, 4, 64, 128, 1), (3, 8, 32, 64, 1), (2, 2, 128, 256, 2), (1, 1, 512, 512, 4), (7, 1, 64, 128, 1),
                                      (130, 1, 128, 64, 2), (5, 16, 32, 128, 1), (2, 4, 256, 32, 1), (2, 8, 64, 64, 2)]:
            for op in (G, P_):
                ntaps = (16 if op == G else 4) if lh > 1 else (4 if op == G else 1)
                cc, sk = (cg if op == G else cd), splitk
                while sk > 1 and (ntaps % sk or ((ntaps // sk) * cc * e) % 128):
                    sk //= 2
                out.append(igemm(op, dt, n, lh, cg, cd, sk))
        for op, n, lh, cg, cd in [(G, 8, 8, 64, 128), (P_, 8, 8, 64, 128), (G, 4, 16, 32, 64), (P_, 64, 4, 128, 256), (P_, 128, 32, 32, 128)]:
            out.append(igemm(op, dt, n, lh, cg, cd, 1, stats=True))
        for n, lh, cg, cd, ms in [(2, 4, 32, 128, 1), (2, 8, 64, 128, 2), (3, 4, 128, 256, 1), (1, 1, 128, 128, 1), (2, 16, 32, 128, 4),
                                  (5, 2, 64, 256, 1), (4, 4, 128, 256, 1), (8, 8, 128, 128, 2), (64, 1, 128, 128, 1), (16, 2, 256, 128, 2),
                                  (2, 16, 128, 128, 1), (1, 32, 128, 128, 4), (20, 4, 128, 128, 3)]:
            out.append(wgemm(dt, n, lh, cg, cd, ms))
        for n, lh, cg, cd, stride in [(2, 8, 4, 64, 2), (3, 8, 8, 64, 2), (2, 16, 36, 4, 1), (2, 8, 64, 1, 1), (1, 4, 33, 256, 1), (2, 8, 1, 64, 2)]:
            pad = lambda c: (c + 7) // 8 * 8
            out.append(edge(G, stride, dt, n, lh, pad(cg), cd, bias=True, act=L.ACT_LEAKY, wide=8))
            out.append(edge(P_, stride, dt, n, lh, pad(cd), min(cg, 32)))
            out += [wgemm_edge(dt, stride, n, lh, cg, cd, ms) for ms in (1, 2)]
        for n, lh, cg, cd, stride in [(3, 32, 4, 64, 2), (2, 32, 8, 64, 2), (2, 64, 36, 4, 1), (3, 32, 64, 1, 1), (2, 16, 1, 64, 2), (20, 64, 33, 8, 1),
                                      (3, 32, 32, 128, 2), (2, 16, 64, 128, 2), (2, 16, 64, 256, 2), (2, 32, 64, 64, 2), (2, 128, 36, 4, 1),
                                      (2, 128, 64, 1, 1)]:
            out.append(wsmall(dt, stride, n, lh, cg, cd))
        for n, h, c, nslabs in [(2, 4, 64, 16), (3, 2, 512, 7), (2, 8, 256, 5), (3, 16, 128, 4), (2, 32, 64, 2), (2, 64, 32, 3)]:
            out.append(norm_fwd(dt, n, h, c, nslabs=nslabs))
        for n, h, c, nsplit in [(3, 8, 32, 1), (2, 32, 32, 4), (2, 16, 64, 1), (2, 8, 128, 1), (2, 64, 32, 4)]:
            nm, dec = norm_fwd(dt, n, h, c, nsplit=nsplit, act=L.ACT_RELU, pad=0)
            dec[15] = _vd(h, h, c + 8, halo=HALO, esz=e)
            out.append(("p2p_norm_act_fwd_tail", dec[:-1] + [_vd(h, h, 8, halo=HALO, esz=e), 8, None]))
    for dt, pad in ((F, 4), (BF, 4), (BF, 8)):
        for n, h, c, mask, norm, nsplit in [(2, 4, 64, False, True, 1), (3, 8, 32, True, True, 1), (2, 1, 512, False, True, 4), (2, 4, 36, True, True, 1),
                                            (2, 8, 64, False, False, 2), (2, 32, 32, False, True, 4), (3, 16, 128, True, True, 8), (5, 2, 64, True, True, 1),
                                            (3, 3, 16, False, True, 1), (2, 2, 8, False, False, 1), (256, 8, 128, True, True, 4),
                                            (2, 16, 128, False, True, 2), (2, 32, 64, False, True, 4), (3, 8, 256, True, True, 1),
                                            (2, 16, 128, False, True, 0x202), (2, 32, 64, False, True, 0x204), (3, 8, 256, True, True, 0x201),
                                            (3, 16, 64, True, True, 0x201), (2, 32, 32, False, True, 0x201), (2, 16, 128, False, True, 0x102),
                                            (3, 8, 256, True, True, 0x101)]:
            out.append(norm_fwd(dt, n, h, c, mask=mask, nsplit=nsplit, pad=pad, norm=norm))
            if norm:        # (the backward launch of a block without normalisation is refused by nothing, but it takes the scalar kernel)
                out.append(norm_bwd(dt, n, h, c, slabs=True, mask=mask, nsplit=nsplit))
    return out


def brig_test_cases(cbw):
    """test_igemm_block_resident_wide_maps / test_fused_block_conv_instance_norm_activation at one P2P_BRIG_CBW (the tests set it,
    with P2P_BRIG_MIN_WG=1, through the environment: brig_plan reads both at every call)"""
    ok = lambda op, cg, cd: cbw == 1 or (cg if op == P_ else cd) % (64 if op == P_ else 256) == 0
    out = [igemm(op, BF, n, lh, cg, cd, stats=True) for op, n, lh, cg, cd in _BRIG_SHAPES if ok(op, cg, cd)]
    out += [igemm(op, BF, n, lh, cg, cd, wide=64) for op, n, lh, cg, cd in _BRIG_SHAPES if ok(op, cg, cd)]
    return out + [igemm_block(op, BF, n, lh, cg, cd, act) for op, n, lh, cg, cd, act in _BLOCK_SHAPES]


def _all_routes(cases):
    out = set()
    for case in cases:
        for name, dec in resolve(case):
            out.update(routes(name, dec))
    return out


def existing_default_routes():
    """{(launcher, code)} the suite's default-setting tests run: tests/test_kernels_gpu.py and every launch of the benchmarked and
    off-benchmark steps of tests/test_step_launches_gpu.py (meta-device census at the batches those tests run)"""
    import bench
    got = _all_routes(kernel_test_cases())
    saved = {k: os.environ.get(k) for k in ("P2P_BRIG_CBW", "P2P_BRIG_MIN_WG")}
    try:
        os.environ["P2P_BRIG_MIN_WG"] = "1"
        for cbw in (1, 2):
            os.environ["P2P_BRIG_CBW"] = str(cbw)
            got |= _all_routes(brig_test_cases(cbw))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    batches = {case: set(bs) for case, bs in SL.OFF_BENCH_BATCHES.items()}
    for cfg, dtype_name in [("c1", "bf16"), ("c2", "bf16"), ("c3", "bf16"), ("c4", "bf16"), ("c5", "bf16"), ("c2", "f32")]:   # test_step_launches_gpu.CONFIGS
        model, B, S = bench.CONFIGS[cfg][:3]
        batches.setdefault((model, S, dtype_name), set()).add(B)
    for case, bs in batches.items():
        census = SL.Census(*case)
        for B in sorted(bs):
            for name, dec in census.launches(B):
                got.update(routes(name, dec))
    return got


# ---------------------------------------------------------------------------------------------------------------- the child
def steps_based_on(baseline):
    """the step cases of the settings that compare with this baseline row"""
    return sorted({st[4] for st in SETTINGS.values() if st[2] == baseline and st[4] is not None})


def step_keys(step, attrs):
    """the variant keys of the meta-device census of the step under this process's switches and the attribute overrides, each
    extended with the routes of its launch; as sorted strings"""
    from palette_and_histo_gan_amd import engine as E
    model, S, dtype_name, B = step
    census = SL.Census(model, S, dtype_name)
    for attr, value in attrs.items():
        holder, name = E._switch_holder(census.eng, attr)
        assert hasattr(holder, name), attr
        setattr(holder, name, value)
    keys, codes = set(), set()
    for name, dec in census.launches(B):
        r = tuple(routes(name, dec))
        keys.add(repr(SL.variant_key(name, dec) + (("route",) + r,)))
        codes.update(r)
    # ... and how often the step calls each entry point, with the integer arguments of the batched weight copies (switches that
    # move work between launches without touching a modelled one)
    calls = {}
    for name, args in census.log:
        k = (name,) + (tuple(int(SL.val(a)) for a in args[2:4]) if name == "p2p_weight_prep_batched" else ())
        calls[k] = calls.get(k, 0) + 1
    keys.update(repr(("calls",) + k + (n,)) for k, n in calls.items())
    return sorted(keys), codes


def _dtype_of(name, dec):
    return dec[1] if name in ("p2p_igemm", "p2p_igemm_norm_act") else (dec[2] if name == "p2p_igemm_edge" else dec[0])


def _seed(cid, k):
    return int.from_bytes(hashlib.sha256(f"{cid}#{k}".encode()).digest()[:4], "little")


def run_launch(T, name, dec, seed, **kw):
    """test_step_launches_gpu._reissue_one, plus the SHA-256 of every output buffer's bytes after the first launch"""
    import numpy as np
    import torch
    launch = T.CHECKERS[name](name, dec, np.random.default_rng(seed), **kw)
    launch.go()
    torch.cuda.synchronize()
    for o in launch.outs:
        o.check_around(name)
    first = [o.flat.clone() for o in launch.outs]
    h = hashlib.sha256()
    for f in first:
        h.update(T._bits(f).cpu().numpy().tobytes())
    for o in launch.outs:
        o.reset()
    launch.go()
    torch.cuda.synchronize()
    for o, f in zip(launch.outs, first):
        assert torch.equal(T._bits(o.flat), T._bits(f)), f"{name}: second launch differs"
    errs = launch.evaluate()
    del launch
    return errs, h.hexdigest()


def probed_steps(baseline):
    """the steps of a baseline row that its GPU child records (signatures) and runs (result hash): those of the settings whose
    recorded step or step results are compared with the baseline's"""
    return sorted({SETTINGS[s][4] for s in list(CENSUS_BLIND) + list(STEP_BIT_IDENTICAL) if SETTINGS[s][2] == baseline})


def step_result_hash(T, step, attrs):
    """SHA-256 of the loss vectors of two train steps and of every parameter after them (a fresh engine as
    test_step_launches_gpu._build makes it, with the attribute overrides)"""
    import gc
    import torch
    from palette_and_histo_gan_amd import engine as E
    model, S, dtype_name, B = step
    eng, go = T._build(SL.step_desc(model, B, S), dtype_name)
    for attr, value in attrs.items():
        holder, name = E._switch_holder(eng, attr)
        setattr(holder, name, value)
    h = hashlib.sha256()
    try:
        for _ in range(2):
            h.update(T._bits(go().float().contiguous()).cpu().numpy().tobytes())
        torch.cuda.synchronize()
        for store in (eng.G, eng.D):
            h.update(T._bits(store.params).cpu().numpy().tobytes())
    finally:
        del eng, go
        gc.collect()
        torch.cuda.empty_cache()
    return h.hexdigest()


def run_gpu(setting):
    import torch
    from tests import test_step_launches_gpu as T
    env, attrs, _, _, step = SETTINGS[setting]
    doc = {"setting": setting, "mode": "gpu", "cases": {}, "failures": []}
    if setting in BASELINES:
        doc["probes"] = {}
        for st in probed_steps(setting):
            uniq, _ = T.harvest(SL.step_desc(st[0], st[3], st[1]), st[2], {})
            doc["probes"][repr(tuple(st))] = {"signatures": sorted(repr(k) for k in uniq), "hash": step_result_hash(T, st, {})}
    for cid, case in cases_of(setting):
        row = doc["cases"][cid] = {"routes": [], "errors": {}, "exact": {}, "sha256": []}
        for k, (name, dec) in enumerate(resolve(case)):
            row["routes"] += [[l, c] for l, c in routes(name, dec)]
            dtype = _dtype_of(name, dec)
            try:
                errs, digest = run_launch(T, name, dec, _seed(cid, k))
            except (AssertionError, L.P2PError) as e:       # (a refused launch is a failure of the case; a device fault ends the child)
                if "illegal" in str(e):
                    raise
                doc["failures"].append(f"{cid}: {name}: {e}")
                continue
            row["sha256"].append(digest)
            for fam, err in errs.items():
                row["errors"][f"{name[4:]} {fam}"] = [err, T._tol(fam, dtype)]
                if not err < T._tol(fam, dtype):
                    doc["failures"].append(f"{cid}: {name}: {fam} error {err:.3g} >= {T._tol(fam, dtype):.3g}")
            torch.cuda.empty_cache()
            if T.CHECKERS[name] not in T.LATTICE_CHECKERS:
                continue
            # the same launch on integer-lattice operands (tests/lattice.py): the same route, every image, no tolerance.  Two
            # routes of one case are then equal to each other because both equal the reference.
            try:
                errs, _ = run_launch(T, name, dec, _seed(cid + " lattice", k), operands="lattice")
            except (AssertionError, L.P2PError) as e:
                if "illegal" in str(e):
                    raise
                doc["failures"].append(f"{cid}: {name} (lattice): {e}")
                continue
            for fam, err in errs.items():
                if fam.startswith("exact ") or fam == "insensitive share":
                    row["exact"][f"{name[4:]} {fam}"] = err
                else:           # (statistics and the normalised output keep their tolerances in this mode)
                    row["errors"][f"{name[4:]} {fam} (lattice)"] = [err, T._tol(fam, dtype)]
                if not err < T._tol(fam, dtype):
                    doc["failures"].append(f"{cid}: {name} (lattice): {fam} {err:.3g} >= {T._tol(fam, dtype):.3g}")
            torch.cuda.empty_cache()
    if step is not None:
        model, S, dtype_name, B = step
        label = f"{setting}: {model} {S}x{S} batch {B}"
        try:
            uniq = T._check_step(SL.step_desc(model, B, S), dtype_name, dict(attrs), label)
            keys = set()
            for name, dec in uniq.values():
                if name in SL.MODELLED:
                    keys.add(repr(SL.variant_key(name, dec) + (("route",) + tuple(routes(name, dec)),)))
            doc["step"] = {"desc": list(step), "keys": sorted(keys), "signatures": sorted(repr(k) for k in uniq)}
            if setting in STEP_BIT_IDENTICAL:
                doc["step"]["hash"] = step_result_hash(T, step, attrs)
        except AssertionError as e:
            doc["failures"].append(f"step {label}: {e}")
    return doc


def run_query(setting):
    env, attrs, _, _, step = SETTINGS[setting]
    doc = {"setting": setting, "mode": "query", "cases": {}}
    for cid, case in cases_of(setting):
        doc["cases"][cid] = {"routes": [[l, c] for name, dec in resolve(case) for l, c in routes(name, dec)]}
    if step is not None:
        keys, codes = step_keys(step, attrs)
        doc["step"] = {"desc": list(step), "keys": keys, "routes": sorted([l, c] for l, c in codes)}
    if setting in BASELINES:       # the census every setting based on this row compares with
        doc["steps"] = {repr(tuple(st)): step_keys(st, {})[0] for st in steps_based_on(setting)}
    if setting == "default":
        doc["existing"] = sorted([l, c] for l, c in existing_default_routes())
    return doc


def child_env(setting):
    """the environment of a setting's child: the parent's without any P2P_* switch, plus the setting's own"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("P2P_") or k == "P2P_LIB"}
    env.update(SETTINGS[setting][0])
    return env


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--setting", required=True, choices=sorted(SETTINGS))
    ap.add_argument("--mode", required=True, choices=("query", "gpu"))
    a = ap.parse_args(argv)
    for k, v in SETTINGS[a.setting][0].items():
        assert os.environ.get(k) == v, f"{a.setting} needs {k}={v} in the environment of this process (the library reads it once)"
    real_stdout = sys.stdout
    sys.stdout = sys.stderr                  # the checkers print their tables: the JSON document alone goes to stdout
    try:
        doc = run_query(a.setting) if a.mode == "query" else run_gpu(a.setting)
    finally:
        sys.stdout = real_stdout
    json.dump(doc, sys.stdout)
    sys.stdout.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
