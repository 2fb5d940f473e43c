"""Not gpu: the palette quantiser's definition (tests/palette_quantize_oracle.py) against hand-worked answers and its
invariances, the argument checks of palette.quantize_palette / quantize, the C ABI of the new entry point, and the promise that the
cases tests/test_palette_quantize_gpu.py runs meet what they are there for -- each property read from the oracle's trace."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import palette as P
from tests import palette_quantize_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
norm = O.SO.normalise


def _rows(r):
    return r.palette[:r.size].tolist()


# ------------------------------------------------------------------------------------------------------ hand-worked answers
def test_one_pixel_is_its_own_palette():
    r = O.quantize_image(norm([[[7, 200, 31, 255]]]), 1, 8)
    assert (_rows(r), r.size, r.iters) == ([[7, 200, 31, 255]], 1, 0) and not r.palette[1:].any()


def test_two_colours_into_one_give_the_mean_rounded_half_up():
    # 3 pixels of (10, 0, 0, 255) and 1 of (13, 1, 0, 255): sums 43, 1, 0, 1020 over 4: 10.75 -> 11, 0.25 -> 0, 0, 255
    img = norm([[[10, 0, 0, 255]] * 3 + [[13, 1, 0, 255]]])
    r = O.quantize_image(img, 1, 8)
    assert _rows(r) == [[11, 0, 0, 255]] and r.iters == 2 and r.trace["passes"][0]["counts"] == [4]
    # one pixel each of (10, ...) and (13, ...): the odd sum 23 over 2 is 11.5 and rounds UP to 12; (2 * 23 + 2) // 4 = 12
    r = O.quantize_image(norm([[[10, 0, 0, 255], [13, 1, 0, 255]]]), 1, 8)
    assert _rows(r) == [[12, 1, 0, 255]]          # 0.5 -> 1 as well
    # without a pass the starting slot stands: the lowest key
    r = O.quantize_image(norm([[[10, 0, 0, 255], [13, 1, 0, 255]]]), 1, 0)
    assert (_rows(r), r.iters) == ([[10, 0, 0, 255]], 0)


def test_an_image_with_few_colours_returns_them_sorted_whatever_else_is_asked():
    colours = np.array([[255, 255, 255, 255], [0, 0, 0, 0], [0, 10, 0, 255], [10, 0, 0, 255]])
    img = norm(colours[np.random.default_rng(1).integers(0, 4, size=(5, 6))])
    want = [[0, 0, 0, 0], [10, 0, 0, 255], [0, 10, 0, 255], [255, 255, 255, 255]]          # ascending r + 256 g + 65536 b + 2^24 a
    inits = [None, (np.array([[1, 2, 3, 4]] * 6), 6), (np.random.default_rng(2).integers(0, 256, size=(4, 4)), 4), (np.zeros((4, 4)), -1)]
    for colours_asked in (4, 5, 256):
        for iterations in (0, 1, 8, 64):
            for init in inits:
                r = O.quantize_image(img, colours_asked, iterations, init)
                assert (_rows(r), r.size, r.iters, r.trace["exact"]) == (want, 4, 0, True)
    assert not O.quantize_image(img, 3, 8).trace["exact"]


# ------------------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("colours,init", [(5, None), (16, None), (4, (O.EMPTY_SLOT_INIT, 4))])
def test_the_result_depends_on_the_multiset_of_colours_only(colours, init):
    img = O.noise_image(8, 12, 10)
    img[:6] = np.round(img[:6] * 4) / 4          # repeated colours among the noise
    want = O.quantize_image(img, colours, 8, init)
    flat = img.reshape(-1, 4)
    shuffled = flat[np.random.default_rng(3).permutation(len(flat))]
    for other in (shuffled.reshape(12, 10, 4), img.reshape(10, 12, 4), shuffled.reshape(1, 120, 4), flat.reshape(120, 1, 4)):
        got = O.quantize_image(other, colours, 8, init)
        assert np.array_equal(got.palette, want.palette) and (got.size, got.iters) == (want.size, want.iters)


# ----------------------------------------------------------------------------------------------- arguments and the C ABI
def test_argument_errors_come_before_anything_touches_a_device():
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"          # the checks are host code
    img = torch.zeros(2, 4, 4, 4)
    for fn in (P.quantize_palette, P.quantize):
        for colours in (True, False, 0, 257, -1, 16.0, "16", None):
            with pytest.raises(ValueError, match="colours"):
                fn(img, colours=colours, device=dev)
        for iterations in (True, -1, 65, 8.0, None):
            with pytest.raises(ValueError, match="iterations"):
                fn(img, iterations=iterations, device=dev)
        with pytest.raises(ValueError, match="2\\^14|16384"):
            fn(torch.zeros(1, 129, 128, 4), device=dev)
        with pytest.raises(ValueError, match="RGBA"):
            fn(torch.zeros(2, 4, 4, 3), device=dev)
        with pytest.raises(ValueError, match="palette for a batch of 2"):
            fn(img, init=(np.zeros((3, 8, 4), np.int32), None), device=dev)
        with pytest.raises(ValueError, match="palette for a batch of 2"):
            fn(img, init=(np.zeros((2, 257, 4), np.int32), None), device=dev)
        with pytest.raises(ValueError, match="palette sizes"):
            fn(img, init=(np.zeros((2, 8, 4), np.int32), [1, 2, 3]), device=dev)
        with pytest.raises(ValueError, match="pair"):
            fn(img, init=np.zeros((2, 8, 4), np.int32)[0, 0, :3], device=dev)


def test_library_exports_the_entry_point_with_the_bound_signature():
    name, nargs = "p2p_palette_quantize", 13
    if not os.path.exists(L.LIB_PATH):
        from palette_and_histo_gan_amd import build
        build.build_library(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pgan.h")).read(), flags=re.S)
    m = re.search(name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/p2pgan.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(L.SIGNATURES[name]) == nargs, args
    for a, t in zip(args, L.SIGNATURES[name]):
        assert t is (L._vp if "*" in a else (L._f if a.startswith("float") else L._i)), (a, t)
    assert L.lib().p2p_replay_fn_nargs(L.lib().p2p_replay_fn_index(name.encode())) == nargs
    # host-side argument checks: refused before any launch, with a message
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(ctypes.byref(buf, (-ctypes.addressof(buf)) % 16), ctypes.c_void_p)
    fn = L.lib().p2p_palette_quantize
    for change, word in (({4: 0}, b"colours"), ({4: 9}, b"colours"), ({5: 65}, b"iterations"), ({5: -1}, b"iterations"), ({8: 257}, b"K = 257"),
                         ({1: 129, 2: 128}, b"2^14"), ({6: p}, b"together"), ({7: p}, b"together"), ({3: None}, b"null"), ({9: None}, b"null"),
                         ({10: None}, b"null"), ({0: 0}, b"bad shape")):
        args = [1, 2, 2, p, 4, 8, None, None, 8, p, p, None, None]
        for at, value in change.items():
            args[at] = value
        assert fn(*args) < 0 and word in L.lib().p2p_last_error(), (change, L.lib().p2p_last_error())


# ---------------------------------------------------------------------------------- the shared cases promise what they claim
def test_a_tie_between_farthest_point_maxima_goes_to_the_lower_key():
    img = O.lattice_image(0, 4, 5)
    r = O.quantize_image(img, 6, 0)          # no pass: the result is the starting slots
    assert r.trace["farthest_tie"] == [False, False, False, False, True] and r.size == 6
    # the step by hand: the five slots before it, every pixel's distance to the nearest, the candidates at the maximum
    q = O.SO.quantise(img.reshape(-1, 4))
    five = O.quantize_image(img, 5, 0).palette[:5].astype(np.int64)
    m = ((q[:, None] - five[None]) ** 2).sum(-1).min(1)
    cands = np.unique(O.pack(q[m == m.max()]))
    assert len(cands) > 1
    added = set(O.pack(r.palette[:6]).tolist()) - set(O.pack(five).tolist())
    assert added == {int(cands[0])} and cands[0] < cands[1]
    assert any(t for t in O.quantize_image(O.lattice_image(960, 3, 1), 3, 0).trace["farthest_tie"])


def test_a_pixel_equidistant_from_two_slots():
    for colours in (3, 4):
        r = O.quantize_image(O.lattice_image(0, 4, 5), colours, 8)
        assert r.trace["passes"][0]["pixel_tie"]


def test_an_empty_slot_keeps_its_colour_and_is_populated_later():
    r = O.quantize_image(O.small_values_image(1), 4, 8, (O.EMPTY_SLOT_INIT, 4))
    counts = [p["counts"] for p in r.trace["passes"]]
    assert counts[0] == [0, 16, 0, 0] and counts[1] == [0, 10, 6, 0]          # the duplicate of slot 1 is empty once, then takes 6 pixels
    assert r.size == 4 and _rows(r)[0] == [0, 0, 0, 0] and _rows(r)[-1] == [255, 255, 255, 255]          # never populated, kept
    r = O.quantize_image(O.small_values_image(3), 4, 8, (O.EMPTY_SLOT_INIT, 4))
    assert [p["counts"] for p in r.trace["passes"]][:2] == [[0, 16, 0, 0], [0, 10, 6, 0]]
    # with iterations = 0 the duplicates given in init stay duplicates: three distinct rows
    assert O.quantize_image(O.small_values_image(1), 4, 0, (O.EMPTY_SLOT_INIT, 4)).size == 3


def test_coinciding_centroids_give_fewer_colours_than_asked():
    r = O.quantize_image(O.lattice_image(2243, 3, 1), 3, 8)
    assert not r.trace["exact"] and r.size == 2 and not r.palette[2:].any()
    assert O.quantize_image(O.lattice_image(2243, 3, 1), 3, 0).size == 3          # the starting slots were distinct


def test_the_number_of_passes_matters_and_a_fixed_point_stops_them():
    img = O.noise_image(0, 33, 7)
    r1, r8, r50, r64 = (O.quantize_image(img, 16, i) for i in (1, 8, 50, 64))
    assert (r1.iters, r8.iters, r50.iters, r64.iters) == (1, 8, 10, 10)          # ten passes are needed; the tenth finds C' = C
    assert not np.array_equal(r1.palette, r8.palette) and not np.array_equal(r8.palette, r50.palette)
    assert not np.array_equal(r1.palette, r50.palette) and np.array_equal(r50.palette, r64.palette)
    assert np.array_equal(O.quantize_image(img, 16, 10).palette, r50.palette) and O.quantize_image(img, 16, 10).iters == 10
    early = O.quantize_image(O.lattice_image(0, 4, 5), 4, 8)
    assert early.iters == 2 < 8          # reaches its fixed point before the cap


def test_the_gpu_batches_hold_what_their_names_say():
    img, init, sizes = O.edge_batch()
    assert img.shape == (3, 7, 9, 4) and np.isnan(img[0]).all() and np.isinf(img[2]).any() and sizes.tolist() == [0, 5, -1]
    pal, n, iters, trace = O.quantize(img, 5, 8, init, sizes, 5)
    assert [t["exact"] for t in trace] == [True, False, False] and n[0] == 1 and not pal[0].any()          # NaN quantises to 0
    free = O.quantize(img, 5, 8, None, None, 5)
    assert not np.array_equal(free[0][1], pal[1]) and np.array_equal(free[0][2], pal[2])          # init reaches image 1 alone
    sprite, true = O.sprite_like_image(1)
    keys = O.pack(O.SO.quantise(sprite.reshape(-1, 4)))
    assert len(np.unique(keys)) > 256 and 0.75 < (O.SO.quantise(sprite)[..., 3] < 64).mean() < 0.85 and len(true) == 12
