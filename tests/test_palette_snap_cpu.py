"""The palette-snap oracle (tests/palette_snap_oracle.py) against hand-worked answers, the 256-value round trip that makes snapping
idempotent, and the packed key the kernel minimises against brute force.  No GPU."""
import numpy as np

from tests import palette_snap_oracle as O


def _one_pixel(q, pal, sizes=None):
    img = O.normalise(np.asarray(q)).reshape(1, 1, 1, 4)
    return O.snap(img, np.asarray(pal, np.int32)[None], sizes)


def test_round_trip_of_all_256_values():
    c = np.arange(256)
    assert np.array_equal(O.quantise(O.normalise(c)), c)


def test_an_equidistant_pixel_goes_to_the_lower_slot_in_both_orders():
    a, b = [100, 50, 50, 255], [104, 50, 50, 255]
    for pal in ([a, b], [b, a]):
        s = _one_pixel([102, 50, 50, 255], pal)
        assert s.index.item() == 0 and s.distance.item() == 4
        assert np.array_equal(s.image.reshape(4), O.normalise(pal[0]))
        assert s.counts.tolist() == [[1, 0]] and s.off_palette.tolist() == [1] and s.distance_sum.tolist() == [4]


def test_duplicate_rows_have_one_answer():
    c = [7, 8, 9, 255]
    s = _one_pixel(c, [[0, 0, 0, 0], c, c, c])
    assert s.index.item() == 1 and s.distance.item() == 0 and s.counts.tolist() == [[0, 1, 0, 0]]
    assert s.off_palette.tolist() == [0] and s.distance_sum.tolist() == [0]


def test_the_largest_distance_is_260100():
    s = _one_pixel([255, 255, 255, 255], [[0, 0, 0, 0]])
    assert s.index.item() == 0 and s.distance.item() == 260100 == 4 * 255 * 255
    assert np.array_equal(s.image.reshape(4), np.full(4, -1.0, np.float32))


def test_a_palette_of_one_and_sizes_that_cut_or_exceed_the_rows():
    pal = [[10, 10, 10, 10], [200, 200, 200, 200], [201, 200, 200, 200]]
    img = O.normalise(np.array([[200, 200, 200, 200], [10, 10, 10, 10], [12, 10, 10, 10]])).reshape(1, 1, 3, 4)
    s = O.snap(img, np.asarray(pal, np.int32)[None], [1])
    assert s.index.tolist() == [[[0, 0, 0]]] and s.distance.tolist() == [[[4 * 190 * 190, 0, 4]]]
    assert s.counts.tolist() == [[3, 0, 0]] and s.off_palette.tolist() == [2] and s.distance_sum.tolist() == [4 * 190 * 190 + 4]
    full, over = O.snap(img, np.asarray(pal, np.int32)[None], None), O.snap(img, np.asarray(pal, np.int32)[None], [7])
    assert full.index.tolist() == [[[1, 0, 0]]] and full.counts.tolist() == [[2, 1, 0]]
    assert all(np.array_equal(x, y) for x, y in zip(full, over))          # a size above K counts as K


def test_an_image_without_a_palette_passes_through():
    rng = np.random.default_rng(1)
    img = rng.uniform(-1, 1, size=(2, 3, 5, 4)).astype(np.float32)
    img[0, 0, 0, 0] = np.nan
    pal = rng.integers(0, 256, size=(2, 6, 4)).astype(np.int32)
    for n in (-1, 0):
        s = O.snap(img, pal, [n, 6])
        assert (s.index[0] == -1).all() and not s.distance[0].any() and not s.counts[0].any()
        assert s.image[0].tobytes() == img[0].tobytes()                    # bit for bit, the NaN included
        assert s.off_palette[0] == 0 and s.distance_sum[0] == 0
        assert (s.index[1] >= 0).all() and s.counts[1].sum() == 15 and s.off_palette[1] > 0


def test_the_engineered_case_holds_what_it_promises():
    img, pal, sizes = O.engineered_case()
    s = O.snap(img, pal, sizes)
    idx, d = s.index.reshape(-1), s.distance.reshape(-1)
    assert idx[:3].tolist() == [10, 20, 30] and d[:3].tolist() == [4, 4, 2]          # ties: the lowest slot
    assert (idx[3], d[3]) == (0, 0) and (idx[4], d[4]) == (1, 0) and (idx[5], d[5]) == (0, 0)      # 0, 255, NaN
    assert O.quantise(img).reshape(-1, 4)[7].tolist() == [255, 0, 255, 0]
    assert idx[230] == 3 and d[230] == 0                                           # the duplicate at slot 5 never wins
    assert s.counts[0, 5] == 0 and s.counts[0, 200] == 0 and s.counts[0, 255] == 0
    assert 0 < s.off_palette[0] < 33 * 7 and s.counts.sum() == 33 * 7 and s.distance_sum[0] == d.sum()


def test_the_packed_key_decodes_to_the_brute_force_answer():
    """key_k = ((|c_k|^2 + 520200) << 8 | k) - (q.c_k << 9): its unsigned 32-bit minimum holds argmin (lowest index on ties) and
    the distance.  10^4 random draws of (q, palette) with palette sizes 1..256, duplicates, near ties and the extremes."""
    rng = np.random.default_rng(2)
    ext = np.array([[0, 0, 0, 0], [255, 255, 255, 255]])
    for t in range(10000):
        n = int(rng.integers(1, 257)) if t % 4 else 256
        pal = rng.integers(0, 256, size=(n, 4))
        q = rng.integers(0, 256, size=4)
        kind = t % 5
        if kind == 1:                                       # extremes on both sides
            q = ext[t // 5 % 2]
            pal[rng.integers(0, n)] = ext[1 - t // 5 % 2]
            if t % 3 == 0:
                pal[:] = ext[1 - t // 5 % 2]                # every slot at the largest distance, all tied
        elif kind == 2:                                     # duplicates and exact hits
            pal[rng.integers(0, n, size=3)] = q
        elif kind == 3:                                     # a cloud of near ties around q
            near = np.clip(q + rng.integers(-2, 3, size=(n, 4)), 0, 255)
            pick = rng.random(n) < 0.5
            pal[pick] = near[pick]
        D = ((pal.astype(np.int64) - q.astype(np.int64)) ** 2).sum(-1)
        want = (int(D.argmin()), int(D.min()))
        assert O.packed_key_snap(q, pal) == want, (t, q, want)
    assert O.packed_key_snap(ext[1], ext[:1]) == (0, 260100) and O.packed_key_snap(ext[0], ext[1:]) == (0, 260100)
    # the widths: the largest score, |c|^2 = 260100 with q.c = 0, still leaves the index byte alone and fits 32 bits
    assert ((260100 + O.BIAS) << 8 | 255) < 2 ** 32 and O.BIAS == 2 * 4 * 255 * 255
