"""The cases of tests/hist_cases.py, without a GPU: the batch sizes restated there are the ones hist.hip has, every class of
partial batch, split and bin padding is reached by a case of each kernel it applies to, the references are finite, and -- from
the references alone -- every case can fail: a kernel that lost the last pixels, or the last padded bin row, would miss the bound
that tests/test_hist_shapes_gpu.py applies by a factor of ten."""
import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from tests import hist_cases as HC

F64 = torch.float64


def hw(shape):
    N, H, W = HC.SHAPES[shape]
    return H * W


def test_constants_are_read_from_the_kernel_source():
    """the restatement uses the constants of hist.hip, and they are today's: a changed batch size fails HERE, with the shapes
    of SHAPES to be chosen again, rather than leaving the GPU test without tails"""
    assert (HC.HB, HC.B3_PB, HC.H3_PB, HC.H3_PS, HC.GB_PB, HC.PT_TILE) == (64, 64, 64, 3, 64, 1024)
    assert (HC.FWD_PB, HC.BWD_PB, HC.GEN_PB, HC.MAXB) == (96, 64, 32, 64)
    assert (HC.NSPLIT_WORKGROUPS, HC.NSPLIT_MIN_BATCHES) == (256, 8)
    assert HC.GEN_LDS_PB == (HC.GEN_PB, HC.GEN_PB)             # the launcher's LDS size is written with the kernel's PB
    assert HC.MAXB * HC.THREADS == 128 * 128                    # size <= 128
    for name in ("B3_PB", "H3_PB", "H3_PS", "GB_PB", "PT_TILE"):
        assert f"#define {name} {getattr(HC, name)}" in HC.TEXT
    # the geometry functions take them from the module, not from literals
    assert HC.ranges(200, 2, HC.B3_PB)[0] == 2 * HC.B3_PB and HC.batches(200, HC.FWD_PB) == (3, 200 - 2 * HC.FWD_PB)
    assert HC._cdiv(-313, 64) == -4 and HC._cdiv(53, 64) == 0 and HC._cdiv(-10 + 63, 64) == 0


def test_geometry_of_the_issue_table():
    """the figures the case table was chosen by"""
    R = HC.Range
    assert HC.bwd3_ranges(1, 1) == [R(0, 1, 1, 1)]
    assert HC.bwd3_ranges(3, 65) == [R(0, 65, 2, 1)]
    assert HC.fwd3_ranges(65) == [R(0, 64, 1, 0), R(64, 65, 1, 1), R(128, 65, 0, 0)]
    assert HC.bwd3_ranges(2, 128) == [R(0, 128, 2, 0)]
    assert HC.bwd3_ranges(2, 184) == [R(0, 184, 3, 56)] and HC.fwd3_ranges(184)[-1] == R(128, 184, 1, 56)
    assert (184 % 96, 184 % 32, 1023 % 64, 1023 % 32, 1023 % 96) == (88, 24, 63, 31, 63)
    assert HC.bwd3_nsplit(2, 1032) == 2 and HC.bwd3_ranges(2, 1032) == [R(0, 576, 9, 0), R(576, 1032, 8, 8)]
    assert HC.point_tiles(1032) == [1024, 8] and HC.point_tiles(1023) == [1023]
    assert HC.bwd3_nsplit(2, 4095) == 4 and HC.bwd3_ranges(2, 4095)[-1].tail == 63 and HC.fwd3_ranges(4095)[-1].tail == 63
    r = HC.bwd3_ranges(1, 8200)
    assert len(r) == 16 and r[14] == R(8064, 8200, 3, 8) and r[15].nb <= 0 and r[15].q0 > 8200
    assert [x.nb for x in HC.fwd3_ranges(323)] == [2, 2, 2] and HC.fwd3_ranges(323)[-1].tail == 3
    assert [x.nb for x in HC.fwd3_ranges(437)] == [3, 3, 1] and HC.fwd3_ranges(437)[-1].tail == 53


def _classes(all_ranges):
    live = [r for rs in all_ranges for r in rs if r.nb > 0]
    return dict(nb={min(r.nb, 4) for r in live}, tail={r.tail for r in live}, empty=any(r.nb <= 0 for rs in all_ranges for r in rs))


def test_every_class_is_reached_by_a_case_of_each_kernel():
    shapes = list(HC.SHAPES.values())
    # rgbuv_hist_bwd3_kernel (p2p_rgbuv_hist_bwd, p2p_rgbuv_hist_hellinger_bwd3): every shape case
    b3 = _classes([HC.bwd3_ranges(N, H * W) for N, H, W in shapes])
    assert b3["nb"] == {1, 2, 3, 4}                                       # 4 stands for >= 4
    assert {0, 1, 8, 63} <= b3["tail"] and 56 in b3["tail"] and b3["empty"]
    nsplits = {HC.bwd3_nsplit(N, H * W) for N, H, W in shapes}
    assert {1, 2, 16} <= nsplits and any(4 <= s < 16 for s in nsplits)
    # rgbuv_hist_fwd3_kernel, dense mode: every shape case
    f3 = _classes([HC.fwd3_ranges(H * W) for N, H, W in shapes])
    assert f3["nb"] == {1, 2, 3, 4} and {0, 1, 8, 56, 63} <= f3["tail"] and f3["empty"]
    # ... listed mode: the colour lists of the sprite and rich images (a list is never a whole number of batches by luck alone:
    # asserted), with ranges of one batch and of several, and partial last batches
    counts = [len(p) for s in HC.SHAPES if HC.has_sprite(s) for k in ("sprite", "rich") for dt in HC.DTYPES
              for p in HC.colour_points(HC.image(s, k, dt))]
    l3 = _classes([HC.fwd3_ranges(c) for c in counts])
    assert any(c % HC.H3_PB for c in counts) and {1, 2, 3} <= l3["nb"] and any(t for t in l3["tail"]) and max(counts) < 2048
    # rgbuv_points_kernel: a partial tile alone, and after one and after several full ones
    tiles = [HC.point_tiles(H * W) for N, H, W in shapes]
    assert [1024, 8] in tiles and [1023] in tiles and any(len(t) > 2 and t[-1] < 1024 for t in tiles) and [1024] * 4 in tiles
    # the plain loops: rgbuv_hist_fwd_kernel (96) on every shape; rgbuv_hist_bwd_kernel (64) on the tail shapes; the general
    # kernels (32 forward, 64 backward) on theirs -- partial batches alone, after full ones, and none
    for pb, names in ((HC.FWD_PB, list(HC.SHAPES)), (HC.BWD_PB, HC.TAIL_SHAPES), (HC.GEN_PB, HC.GENERAL_SHAPES),
                      (HC.GB_PB, HC.TAIL_SHAPES)):
        got = [HC.batches(hw(s), pb) for s in names]
        assert any(n >= 2 and t for n, t in got), (pb, got)
        if pb != HC.FWD_PB:
            assert any(n >= 4 and t == pb - 1 for n, t in got), (pb, got)     # the longest tail: 63 of 64, 31 of 32 (1023 pixels)
    assert any(t == 0 for n, t in (HC.batches(hw(s), HC.GEN_PB) for s in HC.GENERAL_SHAPES))
    assert HC.batches(1, HC.FWD_PB) == (1, 1) and HC.batches(hw("one-batch-plus-1"), HC.BWD_PB) == (2, 1)
    # bin counts of the general kernels
    sizes = {s for s, _, _ in HC.BIN_CASES}
    assert {s % 4 for s in sizes} == {0, 1, 2, 3} and 128 in sizes
    assert {m for _, m, _ in HC.BIN_CASES} == {HC.IQ, HC.RBF, HC.NONE} and len(HC.BIN_CASES) == 3 * len(sizes)
    fwd = {s: HC.general_fwd_geometry(s) for s in sizes}
    bwd = {s: HC.general_bwd_geometry(s) for s in sizes}
    assert any(s * s < 256 and fwd[s]["duplicates"] > 0 and fwd[s]["bins_per_thread"] == 1 for s in sizes)
    assert any(s * s > 256 and s * s % 256 and fwd[s]["duplicates"] > 0 for s in sizes)
    assert fwd[128] == dict(bins_per_thread=HC.MAXB, duplicates=0)
    assert {bwd[s]["pad"] for s in sizes} == {0, 1, 2, 3}
    idle = {s: sum(1 for blocks in bwd[s]["wave_blocks"] if not blocks) for s in sizes}
    assert {idle[s] for s in sizes if s < 16} >= {3, 2, 0} and all(idle[s] == 0 for s in sizes if s >= 16)
    assert set(HC.NORMALIZE_BWD_SIZES) == {2, 5, 63, 64, 127}
    for s in HC.NORMALIZE_BWD_SIZES:
        assert 3 * s * s % 256 or s == 64                                 # elements per image: ragged against the 256 threads


def test_the_earlier_histogram_shapes_had_no_tail_in_the_64_pixel_kernels():
    """why this file exists: 8x8, 64x64, 128x128 and 40x24 are whole numbers of 64-pixel batches in every split (40x24 = 15 x 64
    = 10 x 96 = 30 x 32 has no tail in ANY kernel), and the general kernels saw multiples of 16 bins only"""
    for H, W in HC.EARLIER_SHAPES:
        HW = H * W
        assert HW % 64 == 0
        for N in (1, 2, 3, 4, 8, 64, 256):
            assert all(r.tail == 0 and r.nb > 0 for r in HC.bwd3_ranges(N, HW))
        assert all(r.tail == 0 for r in HC.fwd3_ranges(HW))
        tiles = HC.point_tiles(HW)
        assert len(tiles) == 1 or tiles[-1] == HC.PT_TILE
    assert (40 * 24) % 96 == 0 and (40 * 24) % 32 == 0
    assert (40 * 25) % 96 == 40 and (40 * 25) % 64 == 40 and (40 * 25) % 32 == 8          # the shape test_hist_autograd_gpu adds


def test_inputs_are_what_the_bounds_assume():
    for s in HC.SHAPES:
        for dt in HC.DTYPES:
            mid = HC.image(s, "mid", dt)
            assert mid.shape == HC.SHAPES[s] + (3,) and np.abs(mid).max() <= 0.8 and mid.dtype == np.float32
            assert np.array_equal(mid, HC.U.q(mid.copy(), dt))                   # representable in the view's dtype
            if HC.has_sprite(s):
                sp = HC.image(s, "sprite", dt)
                assert (sp == -1.0).all(-1).any() and (sp[:, -1, -1] > -1.0).all()      # exact-black pixels, an opaque last one
                assert all(len(p) % HC.H3_PB for p in HC.colour_points(sp))
    # the restated point list: counts cover every pixel once, tile by tile
    img = HC.image("tile-plus-8", "sprite", 0)
    for n, pts in enumerate(HC.colour_points(img)):
        assert pts[:, 3].sum() == 1032 and len(np.unique(pts[:, :3], axis=0)) == len(np.unique(img[n].reshape(-1, 3), axis=0))


def test_raw_restatement_is_the_oracle_before_its_normalisation():
    for s, args in (("tail-63", HC.DEFAULT), ("three-batches-tail-56", (5, HC.RBF, 1.0)), ("two-batches", (127, HC.NONE, 0.3))):
        size, method, sigma = args
        x = torch.tensor(HC.image(s, "mid", 0), dtype=F64)
        raw = HC.raw_histogram(x, size, sigma, method)
        want = rg.rgbuv_histogram(x, size=size, sigma=sigma, method=method)
        assert raw.shape == (x.shape[0], 3, size, size) and torch.allclose(HC.normalise(raw), want, rtol=1e-12, atol=0)
        ones = torch.ones(x.shape[0], x.shape[1] * x.shape[2], dtype=F64)
        assert torch.equal(HC.raw_histogram(x, size, sigma, method, weight=ones), raw)


def _without_last(shape, kind, dt, args, count):
    """raw float64 histogram of the case's image with its last `count` pixels removed"""
    size, method, sigma = args
    x = torch.tensor(HC.image(shape, kind, dt), dtype=F64)
    w = torch.ones(x.shape[0], x.shape[1] * x.shape[2], dtype=F64)
    w[:, w.shape[1] - count:] = 0
    return HC.raw_histogram(x, size, sigma, method, weight=w).numpy()


def _forward_can_fail(shape, kind, dt, args, limit, pbs):
    raw, _ = HC.forward(shape, kind, dt, args)
    HW = hw(shape)
    assert np.isfinite(raw).all() and (raw.sum(axis=(1, 2, 3)) > HC.TOTAL_FLOOR * HW).all(), (shape, kind, args)
    if HW == 1:
        return                                        # nothing left to compare with: the only pixel IS the histogram
    drops = {1} | {HW % pb for pb in pbs if HW % pb}
    for count in drops:
        if count == 1 and len(drops) > 1:
            continue      # a broad kernel on 1023 pixels: one pixel is a thousandth of every bin; the lost BATCH is what must show
        moved = HC.U.rel_err(_without_last(shape, kind, dt, args, count), raw)
        assert moved >= 10 * limit, (shape, kind, dt, args, count, moved, limit)


def test_every_default_forward_case_can_fail():
    """removing the last pixel (shapes without a tail) or the last partial batch of any of the kernels' batch sizes moves the raw
    float64 histogram by >= 10 x the 1e-4 of the GPU test"""
    for s in HC.SHAPES:
        for kind in HC.kinds(s):
            for dt in HC.DTYPES:
                _forward_can_fail(s, kind, dt, HC.DEFAULT, HC.FWD_BOUND, (HC.FWD_PB, HC.H3_PB))
                raw, out = HC.forward(s, kind, dt)
                assert np.isfinite(out).all() and np.isfinite(HC.raw_vjp(s, kind, dt)[1]).all()
                assert np.isfinite(HC.normalised_vjp(s, kind, dt)[1]).all() if s in ("tail-63", "one-batch-plus-1") else True
                h = HC.hellinger(s, kind, dt)
                assert np.isfinite(h[2]) and h[2] > 0 and np.isfinite(h[3]).all() and np.abs(h[3]).max() > 0


@pytest.mark.parametrize("size,method,sigma", HC.BIN_CASES)
def test_every_general_case_can_fail(size, method, sigma):
    """forward: as above, against the bound the GPU test derives (max(1e-4, 1.5 x yardstick)); backward with size % 4 != 0: zeroing
    the last bin row of gh -- what a padded float4 contraction that stopped at the last whole vector would do -- moves the VJP of
    the mid-range image (the tight bound) by >= 10 x its bound in both measures.  Every raw total is above the floor, every reference finite"""
    args = (size, method, sigma)
    for s in HC.GENERAL_SHAPES:
        for kind in HC.kinds(s):
            for dt in HC.DTYPES:
                limit = HC.bound(HC.FWD_BOUND, HC.forward_yardstick(s, kind, dt, args)[0])
                assert limit < 1e-3, (s, kind, dt, limit)               # the yardstick itself stays small
                _forward_can_fail(s, kind, dt, args, limit, (HC.GEN_PB,))
                if s not in HC.TAIL_SHAPES:
                    continue
                gh, ref = HC.raw_vjp(s, kind, dt, args)
                assert np.isfinite(ref).all() and np.abs(ref).max() > 0
                if size % 4 and kind == "mid":       # the sprite's 2e-3 is 20 x looser and its L2 norm sits in the black pixels
                    cut = gh.copy()
                    cut[:, :, size - 1, :] = 0
                    x = HC.image(s, kind, dt)
                    moved = HC.deviation(HC._vjp(lambda t: HC.raw_histogram(t, size, sigma, method), x, cut, F64), ref)
                    yard = HC.vjp_yardstick(HC.raw_vjp, s, kind, dt, args)
                    for m, y in zip(moved, yard):
                        assert m >= 10 * HC.bound(HC.vjp_bound(kind), y), (s, kind, dt, args, moved, yard)


def test_normalize_bwd_references_are_finite_and_ragged():
    for size in HC.NORMALIZE_BWD_SIZES:
        raw, g, ref = HC.normalize_bwd(size)
        assert np.isfinite(ref).all() and ref.shape == raw.shape
        # the closed form of hist.hip's comment: gh = (g^T - sum(g Hn)) / T
        T = raw.astype(np.float64).sum(axis=(1, 2, 3), keepdims=True)
        gt = g.astype(np.float64).transpose(0, 3, 1, 2)
        want = (gt - (gt * raw / T).sum(axis=(1, 2, 3), keepdims=True)) / T
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
