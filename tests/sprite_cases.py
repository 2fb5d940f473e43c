"""Inputs and numpy references for the tests of the sprite batch kernels (csrc/sprites.hip): no torch, no GPU.

    colour cube       the 2^24 RGB colours as 4096 sprites of 64 x 64 pixels, each colour once, alpha 255: colour n = 65536 R +
                      256 G + B sits in sprite n >> 12 at pixel n & 4095 (4096 = 2^24 / 64^2: nothing smaller holds the cube)
    hue_rotate_f32    the kernel's hue rotation restated in numpy float32, step for step and without FMA contraction; its
                      largest deviation from the float64 oracle (oracle/input_pipeline.adjust_hue) is the YARDSTICK for the
                      device result: HUE_MARGIN yardsticks are allowed, because hipcc may contract h6 + 6 delta and
                      c (1 - |f - 1|) into FMAs and each contraction can move the hue angle by an ulp
    position code     sprites whose pixel names its own position (R = G = B = x, A = 1 + y; the target bank transposed): grey,
                      so hue leaves it alone; alpha never 0, so nothing is blackened; the translated batch is then compared
                      with oracle.input_pipeline.translate_nearest bit for bit
    gather / relabel  numpy fancy indexing for p2p_gather_rows_i32, the two formulas of p2p_palette_relabel_batch
    png_unfilter_reference   PNG 1.2 section 6 un-filtering, written apart from the library's and the fixtures' code
"""
import numpy as np

from oracle import input_pipeline as ip

F32 = np.float32
CUBE_SPRITES, CUBE_S = 4096, 64
CUBE_CHUNK = 256                                  # images per host comparison: 1 Mpixel, f64 temporaries of 25 MB
HUE_MARGIN = 4.0                                  # device bound = HUE_MARGIN x yardstick of the same delta ...
HUE_BOUND_CAP_NORMALISED = 2e-5                   # ... and never more than the bound the suite had before
# The largest yardstick over the whole cube at ANY delta the loader can draw, [-0.5, 0.5]: about one ulp of the hue angle
# (2^-22 for h6 in [4, 8)) times a chroma of 255 = 6e-5 per rounding, two to three roundings.  Recorded here for batches of
# real sprites (few colours, arbitrary deltas, so a yardstick of their own would be a sample of a few hundred points);
# tests/test_sprite_cases_cpu.py asserts that no cube case measures more.
CUBE_YARDSTICK_RAW, CUBE_YARDSTICK_NORMALISED = 1.4e-4, 1.15e-6
GUARD = 64


def f32_normalise(u8):
    """dataset_utils.normalize as the kernel computes it: two f32 operations"""
    return np.asarray(u8).astype(F32) / F32(127.5) - F32(1.0)


def f32_plain(u8):
    return np.asarray(u8).astype(F32)


def output_format(normalise):
    return f32_normalise if normalise else f32_plain


# ---- the colour cube ---------------------------------------------------------------------------------------------------------

def cube_sprites(lo=0, hi=CUBE_SPRITES):
    """uint8 [hi - lo][64][64][4]: sprites lo .. hi - 1 of the cube"""
    n = np.arange(lo * 4096, hi * 4096, dtype=np.uint32)
    out = np.empty((len(n), 4), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = n >> 16, (n >> 8) & 255, n & 255, 255
    return out.reshape(hi - lo, CUBE_S, CUBE_S, 4)


HUE_DELTAS = {"+half": F32(0.5), "-half": F32(-0.5), "below-half": np.nextafter(F32(0.5), F32(0)), "third": F32(1.0 / 3.0),
              "per-image": np.linspace(-0.5, 0.5, CUBE_SPRITES).astype(F32)}


def cube_deltas(case):
    """f32 [4096]: the hue delta of every image of the batch"""
    return np.broadcast_to(HUE_DELTAS[case], (CUBE_SPRITES,)).astype(F32)


def hue_rotate_f32(rgb, delta):
    """hue_rotate of csrc/sprites.hip in numpy float32: rgb f32 [..., 3] (0..255), delta f32 broadcastable to rgb[..., 0]"""
    rgb = np.asarray(rgb, F32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    delta = np.broadcast_to(np.asarray(delta, F32), r.shape)
    vmax, vmin = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    c = vmax - vmin
    safe = np.where(c > 0, c, F32(1))
    h6 = np.where(vmax == r, (g - b) / safe, np.where(vmax == g, F32(2) + (b - r) / safe, F32(4) + (r - g) / safe))
    h6 = h6 + F32(6) * delta
    h6 = h6 - F32(6) * np.floor(h6 * (F32(1) / F32(6)))
    h6 = np.where(h6 >= F32(6), h6 - F32(6), h6)
    h6 = np.where(h6 < F32(0), F32(0), h6)
    sector = np.minimum(5, h6.astype(np.int32))
    f = h6 - (sector & ~1).astype(F32)
    x = c * (F32(1) - np.abs(f - F32(1)))
    zero = np.zeros_like(c)
    table = [(c, x, zero), (x, c, zero), (zero, c, x), (zero, x, c), (x, zero, c), (c, zero, x)]
    out = np.empty_like(rgb)
    for k in range(3):
        out[..., k] = np.choose(sector, [t[k] for t in table]) + vmin
    assert out.dtype == F32 and h6.dtype == F32 and x.dtype == F32
    return np.where((c > 0)[..., None], out, rgb)


class HueFigures:
    """largest deviations from the f64 oracle, in 0..255 units and after x / 127.5 - 1"""

    def __init__(self):
        self.yard_raw = self.yard_norm = 0.0

    def merge(self, other):
        self.yard_raw, self.yard_norm = max(self.yard_raw, other.yard_raw), max(self.yard_norm, other.yard_norm)
        return self


def hue_reference(rgb_u8, delta):
    """(oracle f64 [..., 3] in 0..255, the f32 restatement, HueFigures of the restatement against the oracle) for uint8 colours
    and f32 deltas broadcastable to rgb_u8[..., 0]"""
    delta = np.asarray(delta, F32)
    want = ip.adjust_hue(rgb_u8.astype(np.float64), delta.astype(np.float64))
    mine = hue_rotate_f32(rgb_u8.astype(F32), delta)
    fig = HueFigures()
    fig.yard_raw = float(np.abs(mine - want).max())
    fig.yard_norm = float(np.abs((mine / F32(127.5) - F32(1.0)) - ip.normalize(want)).max())
    return want, mine, fig


def cube_chunk_reference(case, lo, reverse=False):
    """hue_reference of cube images lo .. lo + CUBE_CHUNK - 1 of the batch; reverse: the batch holds sprite 4095 - b at image b
    (the target side of the cube launch), still with delta[b]"""
    hi = lo + CUBE_CHUNK
    delta = cube_deltas(case)[lo:hi].reshape(-1, 1, 1)
    sprites = cube_sprites(CUBE_SPRITES - hi, CUBE_SPRITES - lo)[::-1] if reverse else cube_sprites(lo, hi)
    return (sprites,) + hue_reference(sprites[..., :3], delta)


def hue_exact_mismatches(got, sprites_u8, normalise):
    """the tolerance-free properties of a hue-rotated batch (got f32 [n, S, S, 4] of opaque sprites_u8): numbers of pixels whose
    largest / smallest channel is not the input's bit for bit (c = vmax - vmin, c + vmin and 0 + vmin are exact on integers),
    whose channels leave [min, max], whose grey colour moved, whose alpha is not the un-augmented formula's"""
    fmt = output_format(normalise)
    rgb_in = sprites_u8[..., :3]
    lo, hi = fmt(rgb_in.min(-1)), fmt(rgb_in.max(-1))
    rgb = got[..., :3]
    grey = (rgb_in[..., 0] == rgb_in[..., 1]) & (rgb_in[..., 1] == rgb_in[..., 2])
    with np.errstate(invalid="ignore"):
        inside = ((rgb >= lo[..., None]) & (rgb <= hi[..., None])).all(-1)
    return {"max": int((rgb.max(-1).view(np.int32) != hi.view(np.int32)).sum()),
            "min": int((rgb.min(-1).view(np.int32) != lo.view(np.int32)).sum()),
            "range": int((~inside).sum()),
            "grey": int((rgb[grey].view(np.int32) != fmt(rgb_in[grey]).view(np.int32)).sum()),
            "alpha": int((got[..., 3].view(np.int32) != fmt(sprites_u8[..., 3]).view(np.int32)).sum())}


# ---- every alpha on a handful of colours ---------------------------------------------------------------------------------------

ALPHA_COLOURS = np.array([[255, 255, 255], [90, 90, 90], [255, 0, 0], [1, 2, 3], [200, 31, 117], [0, 77, 77]], np.uint8)


def alpha_sprites():
    """uint8 [6][16][16][4]: sprite k is ALPHA_COLOURS[k] everywhere (non-black under alpha 0 too), pixel i has alpha i"""
    out = np.empty((len(ALPHA_COLOURS), 16, 16, 4), np.uint8)
    out[..., :3] = ALPHA_COLOURS[:, None, None, :]
    out[..., 3] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return out


# ---- geometry ----------------------------------------------------------------------------------------------------------------

GEOMETRY_SIZES = (4, 32, 64, 128)
SWEEP_FIXED_DX, SWEEP_FIXED_DY = 0.3, -0.4        # non-integer, rounding to "no move"
TRANSLATE_HEIGHT, TRANSLATE_WIDTH = (-0.15, 0.075), (-0.125, 0.125)     # dataset_utils.py:89, as fractions of S


def position_sprites(S):
    """uint8 [2][S][S][4]: sprite 0 (the source bank) R = G = B = x, A = 1 + y; sprite 1 (the target bank) transposed"""
    y, x = np.mgrid[0:S, 0:S]
    src = np.stack([x, x, x, 1 + y], -1)
    tgt = np.stack([y, y, y, 1 + x], -1)
    return np.stack([src, tgt]).astype(np.uint8)


def geometry_rows(S):
    """f32 [B][4] augmentation rows (apply, hue delta, dy, dx) of the geometry batch of size S"""
    sweep = np.arange(-(S + 1), S + 1 + 0.125, 0.25)
    rows = [(1, 0.0, dy, SWEEP_FIXED_DX) for dy in sweep] + [(1, 0.0, SWEEP_FIXED_DY, dx) for dx in sweep]
    ends_y = [F32(F32(v) * F32(S)) for v in TRANSLATE_HEIGHT]
    ends_x = [F32(F32(v) * F32(S)) for v in TRANSLATE_WIDTH]
    for dy in ends_y:
        for dx in ends_x:                         # what uniform(lo, hi) * S can return at the ends, and one ulp inside
            rows += [(1, 0.0, dy, dx), (1, 0.0, np.nextafter(dy, F32(0)), np.nextafter(dx, F32(0)))]
    rng = np.random.default_rng(100 + S)
    for _ in range(8):                            # not representable in f32, both axes moving, a hue rotation on top
        rows.append((1, rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3) * S, rng.uniform(-0.3, 0.3) * S))
    rows += [(0, 0.3, 5.0, 5.0), (0, -0.2, -(S + 1.0), 0.5), (0, 0.0, 0.5, S + 1.0)]          # apply = 0: the shift is ignored
    return np.array(rows, np.float64).astype(F32)


_geometry = {}


def geometry_reference(S):
    """(rows f32 [B][4], uint8 [2][B][S][S][4]): what translate_nearest makes of the two position-coded sprites per row.
    Computed once per size and shared: do not modify.  (One oracle call per row, on an image that carries both codes.)"""
    if S not in _geometry:
        from concurrent.futures import ThreadPoolExecutor
        rows, bank = geometry_rows(S), position_sprites(S)
        both = np.concatenate([bank[0][..., 2:], bank[1][..., 2:]], -1)          # (x, 1 + y, y, 1 + x)
        want = np.empty((2, len(rows), S, S, 4), np.uint8)

        def one(b):
            on, _, dy, dx = rows[b]
            t = ip.translate_nearest(both, dy, dx) if on else both
            want[0, b], want[1, b] = t[..., [0, 0, 0, 1]], t[..., [2, 2, 2, 3]]

        with ThreadPoolExecutor(8) as pool:
            list(pool.map(one, range(len(rows))))
        want.setflags(write=False)
        _geometry[S] = (rows, want)
    return _geometry[S]


def shift_classes(rows, S):
    """which classes of shift the applied rows reach, from the f32 coordinates the transform computes"""
    seen = set()
    grid = np.arange(S, dtype=F32)
    for on, _, dy, dx in rows:
        if not on:
            continue
        fy, fx = (grid - F32(dy)).astype(np.float64), (grid - F32(dx)).astype(np.float64)
        sy, sx = ip._round_half_away(fy), ip._round_half_away(fx)
        iy, ix = (sy >= 0) & (sy < S), (sx >= 0) & (sx < S)
        for f in (fy, fx):
            half = np.abs(f) % 1.0 == 0.5
            seen |= {"tie-positive"} if (half & (f > 0)).any() else set()
            seen |= {"tie-negative"} if (half & (f < 0)).any() else set()
        if not iy.any() or not ix.any():
            seen.add("wholly-out")
            continue
        if iy.all() and ix.all():
            seen.add("untouched" if (sy == np.arange(S)).all() and (sx == np.arange(S)).all() else "moved-inside")
        seen |= {"out-top"} if not iy[0] else set()             # the first output rows sample above the frame
        seen |= {"out-bottom"} if not iy[-1] else set()
        seen |= {"out-left"} if not ix[0] else set()
        seen |= {"out-right"} if not ix[-1] else set()
    return seen


SHIFT_CLASSES = {"untouched", "out-top", "out-bottom", "out-left", "out-right", "wholly-out", "tie-positive", "tie-negative"}


# ---- gather and relabel ------------------------------------------------------------------------------------------------------

GATHER_ROW_INTS = (4, 1024, 4096, 16384, 16388, 20480)       # 16 workgroups x 256 threads x 4 ints = 16384: the last two cross it
GATHER_BATCHES = (1, 5, 300)
GATHER_ROWS = 7


def gather_case(row_ints, B):
    """(table int32 [7][row_ints], selectors int32 [B]): distinct values everywhere, repeated selectors, first and last row"""
    table = (np.arange(GATHER_ROWS * row_ints, dtype=np.int64) * 2654435761 % (1 << 31)).astype(np.int32).reshape(GATHER_ROWS, row_ints)
    sel = np.random.default_rng(row_ints + B).integers(0, GATHER_ROWS, size=B).astype(np.int32)
    sel[0] = GATHER_ROWS - 1
    if B >= 5:
        sel[1:5] = [0, 3, 3, GATHER_ROWS - 1]
    return table, sel


RELABEL_N = (1, 100, 4096, 16384, 16389)                      # 16 workgroups x 256 threads = 4096 indices per row of the grid
RELABEL_P, RELABEL_C, RELABEL_B = (1, 7, 256), (1, 4), (1, 5)
RELABEL_PERMS = ("identity", "reversal", "random")


def relabel_case(n, P, C, B, kind, seed=0):
    """(src, tgt int32 [B][n], pal int32 [B][P][C], perm, inv int32 [B][P]) with a valid permutation per sample"""
    rng = np.random.default_rng([n, P, C, B, seed])
    src, tgt = (rng.integers(0, P, size=(B, n)).astype(np.int32) for _ in range(2))
    pal = rng.integers(0, 256, size=(B, P, C)).astype(np.int32)
    if kind == "identity":
        perm = np.tile(np.arange(P), (B, 1))
    elif kind == "reversal":
        perm = np.tile(np.arange(P)[::-1], (B, 1))
    else:
        perm = np.stack([rng.permutation(P) for _ in range(B)])
    inv = np.empty_like(perm)
    np.put_along_axis(inv, perm, np.tile(np.arange(P), (B, 1)), axis=1)
    return src, tgt, pal, perm.astype(np.int32), inv.astype(np.int32)


def relabel_reference(src, tgt, pal, perm, inv):
    """idx_out[b][i] = inv[b][clamp(idx_in[b][i])], pal_out[b][j] = pal_in[b][clamp(perm[b][j])]; clamp to [0, P)"""
    P = pal.shape[1]
    rows = np.arange(len(pal))[:, None]
    return (inv[rows, np.clip(src, 0, P - 1)], inv[rows, np.clip(tgt, 0, P - 1)], pal[rows, np.clip(perm, 0, P - 1)])


def decode_indexed(idx, pal):
    """io_utils.indexed_to_rgba for a batch: [B][n] indices, [B][P][C] palettes -> [B][n][C]"""
    return pal[np.arange(len(pal))[:, None], idx]


# ---- PNG scanlines -----------------------------------------------------------------------------------------------------------

def png_unfilter_reference(filtered, height, row_bytes, bpp):
    """PNG 1.2 section 6.6 on bytes: height rows of (filter type, row_bytes filtered bytes) -> uint8 [height][row_bytes]"""
    data = bytes(filtered)
    out = [[0] * row_bytes for _ in range(height)]
    for y in range(height):
        line = data[y * (row_bytes + 1):(y + 1) * (row_bytes + 1)]
        kind, prior = line[0], out[y - 1] if y else [0] * row_bytes
        for i in range(row_bytes):
            left = out[y][i - bpp] if i >= bpp else 0
            above = prior[i]
            corner = prior[i - bpp] if i >= bpp else 0
            if kind == 0:
                pred = 0
            elif kind == 1:
                pred = left
            elif kind == 2:
                pred = above
            elif kind == 3:
                pred = (left + above) // 2
            elif kind == 4:
                est = left + above - corner
                dist = [abs(est - left), abs(est - above), abs(est - corner)]
                pred = (left, above, corner)[dist.index(min(dist))]          # ties: left, then above, then the corner
            else:
                raise ValueError(f"filter type {kind}")
            out[y][i] = (line[1 + i] + pred) & 255
    return np.array(out, np.uint8).reshape(height, row_bytes)


def real_sprites(count=64):
    """uint8 [count][64][64][4]: the first PNGs of tests/golden/reference_sprites.npz, decoded by the library's reader"""
    import os
    import tempfile
    from palette_and_histo_gan_amd import png
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_sprites.npz"))
    offs, data = z["offsets"], z["data"]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(count):
            path = os.path.join(tmp, f"{i}.png")
            with open(path, "wb") as f:
                f.write(data[offs[i]:offs[i + 1]].tobytes())
            out.append(png.read_png(path))
    return np.stack(out)
