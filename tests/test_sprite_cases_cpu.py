"""CPU proof of tests/sprite_cases.py, the builders and numpy references that tests/test_sprite_kernels_gpu.py holds the sprite
batch kernels against -- and p2p_png_unfilter, the one function of csrc/sprites.hip that runs on the host.

The yardstick of the hue tolerance is measured here: the largest deviation of the float32 restatement of the kernel's hue
rotation from the float64 oracle over all 2^24 colours, per delta (printed; 0..255 units / after x / 127.5 - 1):

    +half 9.16e-5 / 7.77e-7    -half 9.16e-5 / 7.77e-7    below-half 1.39e-4 / 1.14e-6    third 1.06e-4 / 8.30e-7
    per-image (linspace(-0.5, 0.5, 4096)) 1.37e-4 / 1.11e-6
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import input_pipeline as ip
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import io_utils
from tests import sprite_cases as SC


def test_the_cube_holds_every_colour_once():
    cube = SC.cube_sprites()
    assert cube.shape == (4096, 64, 64, 4) and cube.dtype == np.uint8 and (cube[..., 3] == 255).all()
    flat = cube.reshape(-1, 4).astype(np.uint32)
    key = (flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2]
    assert np.array_equal(key, np.arange(1 << 24, dtype=np.uint32))          # every colour, once, in order
    assert np.array_equal(SC.cube_sprites(700, 702), cube[700:702])
    # the reversed chunk is what the target side of the launch (tgt_idx = 4095 .. 0) holds at images lo .. lo + 255
    sprites = SC.cube_chunk_reference("+half", 256, reverse=True)[0]
    assert np.array_equal(sprites, cube[4095 - np.arange(256, 512)])
    d = SC.cube_deltas("per-image")
    assert d.dtype == np.float32 and d[0] == -0.5 and d[-1] == 0.5 and (np.diff(d) > 0).all()
    assert SC.HUE_DELTAS["below-half"] < 0.5 and np.nextafter(SC.HUE_DELTAS["below-half"], np.float32(1)) == np.float32(0.5)


def _chunk_figures(args):
    case, lo = args
    sprites, want, mine, fig = SC.cube_chunk_reference(case, lo)
    # the restatement has the tolerance-free properties the kernel is asked for
    got = np.concatenate([mine, np.full(mine.shape[:-1] + (1,), 255, np.float32)], -1)
    return fig, SC.hue_exact_mismatches(got, sprites, 0)


@pytest.mark.parametrize("case", list(SC.HUE_DELTAS))
def test_f32_hue_restatement_against_the_f64_oracle_over_the_whole_cube(case):
    """the yardstick of the device tolerance: what float32 costs WITHOUT FMA contraction"""
    with ThreadPoolExecutor(8) as pool:
        res = list(pool.map(_chunk_figures, [(case, lo) for lo in range(0, SC.CUBE_SPRITES, SC.CUBE_CHUNK)]))
    fig = SC.HueFigures()
    for f, exact in res:
        fig.merge(f)
        assert not any(exact.values()), exact
    print(f"hue yardstick {case}: f32 restatement vs f64 oracle over 2^24 colours {fig.yard_raw:.3e} (0..255), "
          f"{fig.yard_norm:.3e} (normalised)")
    assert 0 < fig.yard_raw <= SC.CUBE_YARDSTICK_RAW and 0 < fig.yard_norm <= SC.CUBE_YARDSTICK_NORMALISED
    assert SC.HUE_MARGIN * SC.CUBE_YARDSTICK_NORMALISED <= SC.HUE_BOUND_CAP_NORMALISED          # the old bound is never exceeded


def test_f32_hue_restatement_known_answers_and_the_checks_that_watch_it():
    red = np.array([[255, 0, 0]], np.float32)
    assert np.array_equal(SC.hue_rotate_f32(red, np.float32(0.5)), [[0, 255, 255]])
    assert np.array_equal(SC.hue_rotate_f32(red, np.float32(0.0)), red)
    assert np.abs(SC.hue_rotate_f32(red, np.float32(1 / 3)) - [[0, 255, 0]]).max() < 1e-4
    grey = np.array([[90, 90, 90], [0, 0, 0]], np.float32)
    assert np.array_equal(SC.hue_rotate_f32(grey, np.float32(0.37)), grey)
    # a swapped pair of sector rows, an unwritten pixel and a moved alpha are all seen
    sprites = SC.cube_sprites(2000, 2001)
    good = np.concatenate([SC.hue_rotate_f32(sprites[..., :3].astype(np.float32), np.float32(0.2)), np.full((1, 64, 64, 1), 255, np.float32)], -1)
    assert not any(SC.hue_exact_mismatches(good, sprites, 0).values())
    norm = good / np.float32(127.5) - np.float32(1.0)
    assert not any(SC.hue_exact_mismatches(norm, sprites, 1).values())
    bad = good.copy()
    bad[0, 5, 5] = np.nan
    assert SC.hue_exact_mismatches(bad, sprites, 0)["max"] == 1 and SC.hue_exact_mismatches(bad, sprites, 0)["alpha"] == 1
    swapped = good[..., [1, 0, 2, 3]]
    want = SC.hue_reference(sprites[..., :3], np.float32(0.2))[0]
    assert np.abs(swapped[..., :3] - want).max() > 1.0 and np.abs(good[..., :3] - want).max() < 2e-4


def test_alpha_sprites_hold_every_alpha_over_non_black_colours():
    a = SC.alpha_sprites()
    assert a.shape == (6, 16, 16, 4)
    for k in range(6):
        assert sorted(a[k, ..., 3].ravel()) == list(range(256)) and (a[k, ..., :3] == SC.ALPHA_COLOURS[k]).all()
        assert a[k, 0, 0, 3] == 0 and a[k, 0, 0, :3].any()
    black = ip.blacken_transparent_pixels(a)
    assert not black[:, 0, 0].any() and np.array_equal(black.reshape(6, 256, 4)[:, 1:], a.reshape(6, 256, 4)[:, 1:])


@pytest.mark.parametrize("S", SC.GEOMETRY_SIZES)
def test_shift_sweep_reaches_every_class(S):
    rows, want = SC.geometry_reference(S)
    bank = SC.position_sprites(S)
    assert rows.dtype == np.float32 and len(rows) == 2 * (8 * (S + 1) + 1) + 8 + 8 + 3
    assert (bank[0, ..., 3] >= 1).all() and (bank[0, ..., 0] == np.arange(S)).all() and (bank[0, ..., 3] == 1 + np.arange(S)[:, None]).all()
    assert np.array_equal(bank[1, ..., 0], bank[0, ..., 0].T) and np.array_equal(bank[1, ..., 3], bank[0, ..., 3].T)
    seen = SC.shift_classes(rows, S)
    print(f"S = {S}: {len(rows)} rows reach {sorted(seen)}")
    assert SC.SHIFT_CLASSES <= seen, SC.SHIFT_CLASSES - seen
    on = rows[:, 0] != 0
    assert (~on).sum() == 3 and (np.abs(rows[~on, 2:]).max(1) >= 5).all()
    for b in np.flatnonzero(~on):                     # apply = 0: the shift is ignored
        assert np.array_equal(want[0, b], bank[0]) and np.array_equal(want[1, b], bank[1])
    # every class shows in the reference images themselves: all fill, fill on one side only, no fill
    fill = want[0, :, :, :, 3][on] == 0                # alpha is 1 + y, never 0, inside the frame
    assert fill.all((1, 2)).any() and (~fill).all((1, 2)).any()
    for side in (fill[:, 0, :], fill[:, -1, :], fill[:, :, 0], fill[:, :, -1]):
        assert (side.all(1) & ~fill.all((1, 2))).any()
    # every output pixel names the pixel it sampled: source code (x, 1 + y), target code (y, 1 + x) at the same place
    a, b = want[0, ::5], want[1, ::5]                 # (every fifth row is enough for the builder; the kernel gets them all)
    inside = a[..., 3] != 0
    assert np.array_equal(inside, b[..., 3] != 0) and not a[~inside].any() and not b[~inside].any()
    assert np.array_equal(a[..., 0][inside], b[..., 3][inside] - 1) and np.array_equal(a[..., 3][inside] - 1, b[..., 0][inside])
    # the random rows carry a hue rotation, and the host's extreme draws are there
    assert (rows[on, 1] != 0).sum() == 8
    assert np.float32(np.float32(-0.15) * S) in rows[:, 2] and np.float32(np.float32(0.125) * S) in rows[:, 3]


def test_round_half_away_ties_of_the_oracle():
    img = SC.position_sprites(4)[0]
    down = ip.translate_nearest(img, 0.5, SC.SWEEP_FIXED_DX)           # y - 0.5 = -0.5, 0.5, 1.5, 2.5 -> -1, 1, 2, 3
    assert not down[0].any() and np.array_equal(down[1:], img[1:])
    up = ip.translate_nearest(img, -0.5, SC.SWEEP_FIXED_DX)            # y + 0.5 -> 1, 2, 3, 4
    assert np.array_equal(up[:3], img[1:]) and not up[3].any()


def test_gather_cases():
    assert 16 * 256 * 4 == 16384 and sum(r > 16384 for r in SC.GATHER_ROW_INTS) == 2
    for row_ints in SC.GATHER_ROW_INTS:
        for B in SC.GATHER_BATCHES:
            table, sel = SC.gather_case(row_ints, B)
            assert table.shape == (SC.GATHER_ROWS, row_ints) and table.dtype == np.int32 and sel.dtype == np.int32 and len(sel) == B
            assert len(np.unique(table)) == table.size          # a row read from the wrong place or offset is seen
            assert SC.GATHER_ROWS - 1 in sel and (B < 5 or (0 in sel and len(set(sel.tolist())) < B))


@pytest.mark.parametrize("P", SC.RELABEL_P)
def test_relabel_reference_keeps_the_decoded_image(P):
    for kind in SC.RELABEL_PERMS:
        for C_ in SC.RELABEL_C:
            src, tgt, pal, perm, inv = SC.relabel_case(100, P, C_, 5, kind)
            assert all(sorted(p) == list(range(P)) for p in perm.tolist())
            assert np.array_equal(np.take_along_axis(inv, perm, 1), np.tile(np.arange(P), (5, 1)))          # inv[perm[j]] = j
            s2, t2, p2 = SC.relabel_reference(src, tgt, pal, perm, inv)
            assert np.array_equal(SC.decode_indexed(s2, p2), SC.decode_indexed(src, pal))
            assert np.array_equal(SC.decode_indexed(t2, p2), SC.decode_indexed(tgt, pal))
            for b in range(5):                     # the batch decoder is io_utils.indexed_to_rgba per sample
                assert np.array_equal(SC.decode_indexed(s2, p2)[b].reshape(10, 10, C_), io_utils.indexed_to_rgba(s2[b].reshape(10, 10, 1), p2[b]))
            if kind == "identity":
                assert np.array_equal(s2, src) and np.array_equal(t2, tgt) and np.array_equal(p2, pal)
            elif P > 1:
                assert not np.array_equal(p2, pal)
    # through perm in place of inv the image is lost (a random permutation is not its own inverse)
    src, tgt, pal, perm, inv = SC.relabel_case(100, 7, 4, 5, "random")
    s2, _, p2 = SC.relabel_reference(src, tgt, pal, perm, perm)
    assert not np.array_equal(SC.decode_indexed(s2, p2), SC.decode_indexed(src, pal))
    # values outside [0, P) are clamped
    src[0, :3], perm[1, :2] = [-5, 7, 300], [-1, 9]
    s2, _, p2 = SC.relabel_reference(src, tgt, pal, perm, inv)
    assert s2[0, :3].tolist() == [inv[0, 0], inv[0, 6], inv[0, 6]] and np.array_equal(p2[1, :2], pal[1, [0, 6]])


# ---- p2p_png_unfilter (host) -------------------------------------------------------------------------------------------------

def _unfilter(filtered, height, row_bytes, bpp):
    buf = np.frombuffer(bytes(filtered), np.uint8).copy()
    guard = 16
    out = np.full(height * row_bytes + 2 * guard, 0xA5, np.uint8)
    L.call("p2p_png_unfilter", C.c_void_p(buf.ctypes.data), height, row_bytes, bpp, C.c_void_p(out.ctypes.data + guard))
    assert (out[:guard] == 0xA5).all() and (out[-guard:] == 0xA5).all()
    return out[guard:-guard].reshape(height, row_bytes)


@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 8])
def test_png_unfilter_equals_an_independent_unfilter(bpp):
    rng = np.random.default_rng(bpp)
    shapes = [(1, 5 * bpp), (1, bpp - 1 or 1), (7, 3 * bpp + 1), (11, bpp), (6, max(1, bpp - 1)), (23, 16 * bpp)]
    for height, row_bytes in shapes:                   # height 1, rows shorter than a pixel, rows that end inside a pixel
        orders = [[f] * height for f in range(5)] + [[(y + k) % 5 for y in range(height)] for k in range(5)] + \
                 [rng.integers(0, 5, size=height).tolist()]
        for order in orders:
            raw = rng.integers(0, 256, size=(height, row_bytes + 1), dtype=np.uint8)
            raw[:, 0] = order
            if rng.random() < 0.3:                     # near-constant bytes: the Paeth ties
                raw[:, 1:] = rng.integers(0, 3, size=(height, row_bytes))
            want = SC.png_unfilter_reference(raw.tobytes(), height, row_bytes, bpp)
            assert np.array_equal(_unfilter(raw.tobytes(), height, row_bytes, bpp), want), (bpp, height, row_bytes, order)


def test_png_unfilter_refuses_what_it_cannot_do():
    raw = np.zeros((3, 9), np.uint8)
    out = np.zeros(24, np.uint8)
    raw[2, 0] = 5
    with pytest.raises(RuntimeError, match="filter type 5 in row 2"):
        L.call("p2p_png_unfilter", C.c_void_p(raw.ctypes.data), 3, 8, 4, C.c_void_p(out.ctypes.data))
    raw[2, 0] = 255
    with pytest.raises(RuntimeError, match="filter type 255"):
        L.call("p2p_png_unfilter", C.c_void_p(raw.ctypes.data), 3, 8, 4, C.c_void_p(out.ctypes.data))
    raw[2, 0] = 4
    for height, row_bytes, bpp in [(0, 8, 4), (3, 0, 4), (3, 8, 0), (3, 8, 9), (-1, 8, 4)]:
        with pytest.raises(RuntimeError, match="bad args"):
            L.call("p2p_png_unfilter", C.c_void_p(raw.ctypes.data), height, row_bytes, bpp, C.c_void_p(out.ctypes.data))
    with pytest.raises(RuntimeError, match="bad args"):
        L.call("p2p_png_unfilter", None, 3, 8, 4, C.c_void_p(out.ctypes.data))
    with pytest.raises(ValueError, match="filter type 5"):
        SC.png_unfilter_reference(bytes([5, 1, 2]), 1, 2, 1)


def test_the_real_sprites_fit_the_pipeline():
    """the first 64 sprites of the fixture: none has partial alpha, a non-black colour under alpha 0 or a pair palette beyond
    256 colours, so the indexed loader takes every pair (extract_palette raises above 256) and blackening changes nothing"""
    s = SC.real_sprites(64)
    assert s.shape == (64, 64, 64, 4) and s.dtype == np.uint8
    assert set(np.unique(s[..., 3]).tolist()) == {0, 255}
    assert not s[s[..., 3] == 0].any()
    counts = [len(io_utils._unique_rows_first_appearance(np.concatenate([s[i], s[i + 32]]).reshape(-1, 4).astype(np.int32))[0]) for i in range(32)]
    print(f"real sprite pairs: {min(counts)} .. {max(counts)} colours")
    assert 2 <= min(counts) and max(counts) <= 256
    big = np.zeros((64, 64, 4), np.uint8)
    big[..., 0], big[..., 1], big[..., 3] = np.arange(64)[:, None], np.arange(64)[None, :], 255       # 4096 colours
    with pytest.raises(ValueError, match="more than MAX_PALETTE_SIZE"):
        io_utils.extract_palette(big, "grayness")
