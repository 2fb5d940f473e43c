"""Cases, geometry, inputs and float64 references for the tests of the histogram kernels (csrc/hist.hip) at ragged pixel counts and
odd bin counts: no GPU.

    constants         B3_PB, H3_PB, H3_PS, GB_PB, PT_TILE, the `constexpr int PB` of the three kernels that have one, MAXB and the
                      two numbers of launch_hist_bwd3's nsplit loop are READ from the text of hist.hip: when a batch size changes,
                      tests/test_hist_cases_cpu.py fails instead of the shapes below silently losing their tails
    geometry          every kernel walks the image in batches of pixels; `ranges` restates the split of rgbuv_hist_bwd3_kernel
                      (nsplit ranges) and rgbuv_hist_fwd3_kernel (H3_PS ranges over the pixels or the colour list): chunk, q0, q1,
                      nb (C division, <= 0 for an empty range) and the length of the partial last batch; `batches` the plain
                      loops; `general_fwd_geometry` / `general_bwd_geometry` the bins per thread, the clamped duplicate bins, Sp
                      and the row blocks of each wave
    SHAPES            the smallest (N, H, W) that reach each class of tests/test_hist_cases_cpu.py
    BIN_CASES         size x method x sigma for the general kernels; sigma follows the bin spacing so that every raw total is
                      far from 0 (RBF with sigma 0.02 on two bins is exp(-2500): reference and kernel would both return 0 / 0)
                      and so that the last bin row carries weight (the padded float4 contraction can then be seen to fail)
    inputs            `mid` (every channel in [-0.8, 0.8]: the tight bounds), `sprite` (palette sprites with exact-black pixels:
                      the loose bound; the last pixel is opaque, so that a lost last pixel moves the histogram), `rich` (a palette
                      of 200 colours: colour lists of several batches); all rounded through the view's dtype
    references        oracle.reference_graph.rgbuv_histogram in float64; `raw_histogram`, the same expression before the
                      normalisation in the kernels' [N][3][S][S] layout (equal to the oracle after normalising: CPU test); the
                      VJPs under torch.autograd on a float64 leaf; the Hellinger loss and its gradient; and each of them in
                      float32 as the YARDSTICK of DESIGN.md section 2 (`deviation` from the float64 result)
"""
import collections
import functools
import os
import re

import numpy as np
import torch

from oracle import reference_graph as rg
from tests import gpu_util as U

F64, F32 = torch.float64, torch.float32
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "palette_and_histo_gan_amd", "csrc", "hist.hip")
with open(HIP) as _f:
    TEXT = _f.read()


# ---- constants read from hist.hip ----------------------------------------------------------------------------------------------

def _define(name):
    m = re.search(rf"^#define {name} (\d+)\b", TEXT, re.M)
    assert m, f"hist.hip no longer defines {name}"
    return int(m.group(1))


def _kernel_constant(kernel, name):
    """`name = <int>` of a constexpr int declaration inside the body of `kernel`"""
    at = TEXT.index(f"void {kernel}(")
    end = TEXT.find("__global__", at)
    body = TEXT[at:end if end > 0 else len(TEXT)]
    m = re.search(rf"constexpr int [^;]*\b{name} = (\d+)", body)
    assert m, f"{kernel} no longer declares constexpr int {name}"
    return int(m.group(1))


def _nsplit_loop():
    m = re.search(r"while \(N \* nsplit < (\d+) && \(H \* W\) / \(nsplit \* 2\) >= (\d+) \* B3_PB\) nsplit \*= 2;", TEXT)
    assert m, "launch_hist_bwd3's nsplit loop changed: restate it in tests/hist_cases.py"
    return int(m.group(1)), int(m.group(2))


def _general_lds():
    m = re.search(r"shm = \(size_t\)\(2 \* (\d+) \* size \+ (\d+)\) \* sizeof\(float\)", TEXT)
    assert m, "p2p_rgbuv_hist_general's LDS size changed: restate it in tests/hist_cases.py"
    return int(m.group(1)), int(m.group(2))


HB = _define("HB")
B3_PB, H3_PB, H3_PS, GB_PB, PT_TILE = (_define(k) for k in ("B3_PB", "H3_PB", "H3_PS", "GB_PB", "PT_TILE"))
FWD_PB = _kernel_constant("rgbuv_hist_fwd_kernel", "PB")
BWD_PB = _kernel_constant("rgbuv_hist_bwd_kernel", "PB")
GEN_PB = _kernel_constant("rgbuv_hist_general_kernel", "PB")
MAXB = _kernel_constant("rgbuv_hist_general_kernel", "MAXB")
NSPLIT_WORKGROUPS, NSPLIT_MIN_BATCHES = _nsplit_loop()
GEN_LDS_PB = _general_lds()
THREADS = 256                     # the general kernels' workgroup: 4 waves


# ---- geometry --------------------------------------------------------------------------------------------------------------------

Range = collections.namedtuple("Range", "q0 q1 nb tail")      # nb <= 0: the range is empty; tail: pixels of a partial last batch


def _cdiv(a, b):
    """C's integer division (towards zero)"""
    return abs(a) // b if a >= 0 else -(abs(a) // b)


def ranges(total, nsplit, pb):
    """the kernels' `chunk`, `q0`, `q1`, `nb` for each of the nsplit ranges over `total` pixels (or colour points)"""
    chunk = (total + nsplit - 1) // nsplit
    chunk = (chunk + pb - 1) // pb * pb
    out = []
    for ps in range(nsplit):
        q0 = ps * chunk
        q1 = min(total, q0 + chunk)
        nb = _cdiv(q1 - q0 + pb - 1, pb)
        out.append(Range(q0, q1, nb, (q1 - q0) % pb if nb > 0 else 0))
    return chunk, out


def bwd3_nsplit(N, HW):
    """launch_hist_bwd3"""
    nsplit = 1
    while N * nsplit < NSPLIT_WORKGROUPS and HW // (nsplit * 2) >= NSPLIT_MIN_BATCHES * B3_PB:
        nsplit *= 2
    return nsplit


def bwd3_ranges(N, HW):
    return ranges(HW, bwd3_nsplit(N, HW), B3_PB)[1]


def fwd3_ranges(total):
    """rgbuv_hist_fwd3_kernel: total = H W (dense) or the image's number of colour points (listed)"""
    return ranges(total, H3_PS, H3_PB)[1]


def batches(HW, pb):
    """a plain loop `for p0 in 0, pb, ...`: (number of batches, pixels of the partial last one or 0)"""
    return (HW + pb - 1) // pb, HW % pb


def point_tiles(HW):
    """pixels of each PT_TILE tile of rgbuv_points_kernel"""
    return [min(PT_TILE, HW - t0) for t0 in range(0, HW, PT_TILE)]


def general_fwd_geometry(S):
    """rgbuv_hist_general_kernel: bins per thread, and how many (thread, k) slots hold the clamped duplicate bin S S - 1"""
    nb = (S * S + THREADS - 1) // THREADS
    assert nb <= MAXB
    return dict(bins_per_thread=nb, duplicates=nb * THREADS - S * S)


def general_bwd_geometry(S):
    """rgbuv_hist_general_bwd_kernel: Sp and the first rows of the four-row blocks that each wave contracts"""
    Sp = (S + 3) & ~3
    return dict(Sp=Sp, pad=Sp - S, wave_blocks=[list(range(4 * w, Sp, 16)) for w in range(THREADS // 64)])


# ---- cases -------------------------------------------------------------------------------------------------------------------------

SHAPES = collections.OrderedDict([
    ("one-pixel", (1, 1, 1)),                   # nb 1, tail 1 everywhere
    ("one-batch-plus-1", (3, 5, 13)),           # HW 65: bwd3 nb 2 tail 1; fwd3 ranges (1, 0) (1, 1) (empty)
    ("two-batches", (2, 8, 16)),                # HW 128: nb 2, no tail
    ("three-batches-tail-56", (2, 8, 23)),      # HW 184: bwd3 nb 3 tail 56; mod 96 = 88, mod 32 = 24; fwd3 last range tail 56
    ("fwd3-two-batches", (1, 17, 19)),          # HW 323: fwd3 ranges of 2, 2 and 2 batches, the last with a tail of 3
    ("fwd3-three-batches", (1, 19, 23)),        # HW 437: fwd3 ranges of 3, 3 and 1 batches, tail 53
    ("tail-63", (3, 33, 31)),                   # HW 1023: mod 64 = 63, mod 32 = 31, mod 96 = 63; one point tile of 1023
    ("tile-plus-8", (2, 24, 43)),               # HW 1032: bwd3 nsplit 2, splits (9, 0) and (8, tail 8); points: a full tile, then 8
    ("splits-tail-63", (2, 65, 63)),            # HW 4095: bwd3 nsplit 4, last split tail 63; fwd3 last range tail 63
    ("empty-split", (1, 82, 100)),              # HW 8200: bwd3 nsplit 16, split 14 = 3 batches with tail 8, split 15 empty
    ("anchor-8x8", (2, 8, 8)),                  # the suite's earlier shapes: no tail in the 64-pixel kernels
    ("anchor-64x64", (2, 64, 64)),
])
TAIL_SHAPES = ("three-batches-tail-56", "tail-63")
GENERAL_SHAPES = TAIL_SHAPES + ("two-batches",)
EARLIER_SHAPES = ((8, 8), (64, 64), (128, 128), (40, 24))      # what the suite launched the histogram kernels at before

IQ, RBF, NONE = "inverse-quadratic", "RBF", "thresholding"      # method codes 0, 1, 2 ("thresholding": no kernel function)
METHOD_CODE = {IQ: 0, RBF: 1, NONE: 2}
SIZES = (2, 3, 5, 15, 63, 127, 128)
# sigma per size: about the bin spacing or wider for the small grids, so that bins at the rim of the grid (d = +-3, where mid-range
# pixels with |u| <= 2.2 are 0.8 away) keep weight; the reference's sharp 0.02 at the maximum size
_SIGMA = {2: {IQ: 2.0, RBF: 2.0}, 3: {IQ: 1.5, RBF: 1.5}, 5: {IQ: 1.0, RBF: 1.0}, 15: {IQ: 0.5, RBF: 0.5},
          63: {IQ: 0.3, RBF: 0.5}, 127: {IQ: 0.3, RBF: 0.5}, 128: {IQ: 0.02, RBF: 0.05}}
BIN_CASES = tuple((s, m, _SIGMA[s][IQ if m == NONE else m]) for s in SIZES for m in (IQ, RBF, NONE))
NORMALIZE_BWD_SIZES = (2, 5, 63, 64, 127)
TOTAL_FLOOR = 1e-3            # raw total per pixel: a thousandth of one unit-weight pixel falling on a bin centre
DTYPES = (0, 1)               # _lib.F32, _lib.BF16
DEFAULT = (64, IQ, 0.02)

FWD_BOUND, VJP_MID_BOUND, VJP_SPRITE_BOUND = 1e-4, 1e-4, 2e-3      # the figures of test_hist_indexed_gpu / test_hist_autograd_gpu
YARDSTICK_MARGIN = 1.5


def bound(existing, yardstick):
    """max(the project's figure, 1.5 x the deviation of the oracle evaluated in float32 from float64)"""
    return max(existing, YARDSTICK_MARGIN * yardstick)


def has_sprite(shape):
    N, H, W = SHAPES[shape]
    return H * W >= 65


def kinds(shape):
    return ("mid", "sprite") if has_sprite(shape) else ("mid",)


def variants(shape):
    """(image kind, dtype, view kind): the mid-range image through every view in both dtypes, the sprite once per dtype"""
    out = [("mid", dt, vk) for dt in DTYPES for vk in ("dense4", "dense3", "strided")]
    if has_sprite(shape):
        out += [("sprite", 0, "dense4"), ("sprite", 1, "strided")]
    return out


def vjp_bound(kind):
    return VJP_MID_BOUND if kind == "mid" else VJP_SPRITE_BOUND


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def _seed(shape, salt):
    return 1000 * (list(SHAPES).index(shape) + 1) + salt


@functools.lru_cache(maxsize=None)
def image(shape, kind, dtype, salt=0):
    """float32 (N, H, W, 3), every value representable in the view's dtype; read-only"""
    N, H, W = SHAPES[shape]
    rng = np.random.default_rng(_seed(shape, salt + {"mid": 1, "sprite": 2, "rich": 3}[kind]))
    if kind == "mid":
        img = rng.uniform(-0.8, 0.8, size=(N, H, W, 3)).astype(np.float32)
    else:
        _, tgt = rg.synthetic_rgba_batch(rng, N, 128 if max(H, W) > 64 else 64, palette_size=24 if kind == "sprite" else 200)
        img = tgt[:, :H, :W, :3].copy()
        for n in range(N):                     # an opaque last pixel: losing it must move the histogram
            img[n, -1, -1] = np.array([200, 90 + 20 * n, 40], np.float32) / 127.5 - 1.0
    img = U.q(img, dtype)
    if kind == "mid":
        img = np.clip(img, -0.796875, 0.796875)          # bf16 rounds 0.7999 up to 0.8008; 51 / 64 is representable in both dtypes
    img.setflags(write=False)
    return img


def upstream(seed, shape):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def colour_points(img):
    """rgbuv_points_kernel restated: per image the (r, g, b, count) rows, tile by tile, each tile's distinct colours in the order
    of their first pixel"""
    out = []
    for im in np.asarray(img, np.float32).reshape(img.shape[0], -1, 3):
        rows = []
        for t0 in range(0, len(im), PT_TILE):
            tile = im[t0:t0 + PT_TILE]
            uniq, first, count = np.unique(tile, axis=0, return_index=True, return_counts=True)
            order = np.argsort(first)
            rows.append(np.concatenate([uniq[order], count[order, None].astype(np.float32)], axis=1))
        out.append(np.concatenate(rows))
    return out


# ---- references ----------------------------------------------------------------------------------------------------------------------

def raw_histogram(image_t, size=64, sigma=0.02, method=IQ, weight=None):
    """rg.rgbuv_histogram before its normalisation, as (N, 3, size, size) -- the kernels' raw layout; `weight` (N, HW) scales each
    pixel's contribution (0 removes the pixel)"""
    eps = 1e-6
    dom = torch.linspace(-3.0, 3.0, size, dtype=image_t.dtype)
    I = (image_t * 0.5 + 0.5)[..., :3].reshape(image_t.shape[0], -1, 3)
    Iy = torch.sqrt((I ** 2).sum(-1) + eps)
    if weight is not None:
        Iy = Iy * weight
    Iy = Iy.unsqueeze(-1)

    def component(comp, p1, p2):
        Iu = (torch.log(comp + eps) - torch.log(p1 + eps)).unsqueeze(-1)
        Iv = (torch.log(comp + eps) - torch.log(p2 + eps)).unsqueeze(-1)
        du, dv = (Iu - dom) ** 2 / sigma ** 2, (Iv - dom) ** 2 / sigma ** 2
        if method == RBF:
            du, dv = torch.exp(-du), torch.exp(-dv)
        elif method == IQ:
            du, dv = 1.0 / (1.0 + du), 1.0 / (1.0 + dv)
        return (Iy * du).transpose(1, 2) @ dv

    r, g, b = I[..., 0], I[..., 1], I[..., 2]
    return torch.stack([component(r, g, b), component(g, r, b), component(b, r, g)], dim=1)


def normalise(raw):
    """(N, 3, S, S) raw -> the reference's (N, S, S, 3) normalised tensor (histogram.py:75-79)"""
    return raw.permute(0, 2, 3, 1) / raw.sum(dim=(1, 2, 3), keepdim=True)


def oracle(image_t, size, method, sigma):
    return rg.rgbuv_histogram(image_t, size=size, sigma=sigma, method=method)


def deviation(got, ref):
    """(max-norm relative error, relative L2 error) against the float64 reference"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return U.rel_err(got, ref), float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300))


def _np(t):
    return t.detach().double().numpy()


@functools.lru_cache(maxsize=None)
def forward(shape, kind, dtype, args=DEFAULT, precision=F64):
    """(raw (N, 3, S, S), normalised (N, S, S, 3) by the oracle) of the case's image, evaluated in `precision`"""
    size, method, sigma = args
    x = torch.tensor(image(shape, kind, dtype), dtype=precision)
    return _np(raw_histogram(x, size, sigma, method)), _np(oracle(x, size, method, sigma))


def forward_yardstick(shape, kind, dtype, args):
    """max-norm deviations of the float32 evaluation: (raw, normalised)"""
    ref, low = forward(shape, kind, dtype, args), forward(shape, kind, dtype, args, F32)
    return deviation(low[0], ref[0])[0], deviation(low[1], ref[1])[0]


def _vjp(fn, img, g, precision):
    x = torch.tensor(img, dtype=precision, requires_grad=True)
    (fn(x) * torch.as_tensor(g, dtype=precision)).sum().backward()
    return _np(x.grad)


@functools.lru_cache(maxsize=None)
def raw_vjp(shape, kind, dtype, args=DEFAULT, precision=F64):
    """(gh (N, 3, S, S) float32, d <gh, raw histogram> / d img (N, H, W, 3))"""
    size, method, sigma = args
    N = SHAPES[shape][0]
    gh = upstream(_seed(shape, 11), (N, 3, size, size))
    return gh, _vjp(lambda x: raw_histogram(x, size, sigma, method), image(shape, kind, dtype), gh, precision)


@functools.lru_cache(maxsize=None)
def normalised_vjp(shape, kind, dtype, args=DEFAULT, precision=F64):
    """(g (N, S, S, 3) float32, d <g, oracle histogram> / d img (N, H, W, 3))"""
    size, method, sigma = args
    N = SHAPES[shape][0]
    g = upstream(_seed(shape, 12), (N, size, size, 3))
    return g, _vjp(lambda x: oracle(x, size, method, sigma), image(shape, kind, dtype), g, precision)


def vjp_yardstick(which, shape, kind, dtype, args):
    """(max-norm, L2) deviation of the float32 evaluation of raw_vjp / normalised_vjp"""
    return deviation(which(shape, kind, dtype, args, F32)[1], which(shape, kind, dtype, args)[1])


@functools.lru_cache(maxsize=None)
def hellinger(shape, kind, dtype):
    """the closed-form case of test_hist_indexed_gpu.py: (real image, fake image, loss, d loss / d fake) in float64"""
    real, fake = image(shape, kind, dtype, salt=50), image(shape, kind, dtype)
    ft = torch.tensor(fake, dtype=F64, requires_grad=True)
    loss = rg.hellinger_loss(rg.rgbuv_histogram(torch.tensor(real, dtype=F64)), rg.rgbuv_histogram(ft))
    loss.backward()
    return real, fake, float(loss.detach()), _np(ft.grad)


@functools.lru_cache(maxsize=None)
def normalize_bwd(size, precision=F64):
    """p2p_hist_normalize_bwd: (raw (N, 3, S, S) float32 positive, g (N, S, S, 3) float32, d <g, raw^T / sum raw> / d raw)"""
    N = 3
    rng = np.random.default_rng(7000 + size)
    raw = rng.uniform(0.05, 4.0, size=(N, 3, size, size)).astype(np.float32)
    g = rng.normal(size=(N, size, size, 3)).astype(np.float32)
    return raw, g, _vjp(normalise, raw, g, precision)
