"""Not gpu: the palette lookup's definitions (tests/palette_lookup_oracle.py) -- hand-worked answers, the closed-form VJP the
backward kernel implements against float64 autograd of the restatement, the premises of the GPU test's cases (ties, filler slots)
and its yardsticks -- the C ABI of the two entry points, and the argument refusals of palette.palette_lookup and
Pix2PixIndexedColourModel, which come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import palette as P
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import palette_lookup_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------- hand-worked answers
def _one_pixel(slots):
    probs = np.zeros((1, 1, 1, O.K), np.float32)
    for k, v in slots.items():
        probs[0, 0, 0, k] = v
    return probs


PAL = np.tile(np.array(O.FILLER, np.int32), (1, O.K, 1))
PAL[0, :4] = [[0, 0, 0, 0], [10, 200, 31, 255], [90, 40, 250, 0], [255, 128, 1, 255]]


def test_a_one_hot_row_returns_the_slots_colour_bit_for_bit():
    t = O.colours(PAL, False)
    assert t.dtype == np.float32 and t[0, 1].tolist() == [np.float32(10) / np.float32(127.5) - np.float32(1), np.float32(200) / np.float32(127.5)
                                                          - np.float32(1), np.float32(31) / np.float32(127.5) - np.float32(1), 1.0]
    for k in (0, 1, 3, 4, 255):
        for f in (O.lookup32, O.lookup32_butterfly):
            assert f(_one_pixel({k: 1.0}), PAL, False).tobytes() == t[0, k].tobytes(), (k, f.__name__)
        assert O.hard_lookup(_one_pixel({k: 1.0}), PAL, False)[0].tobytes() == t[0, k].tobytes()
        assert np.array_equal(O.lookup64(_one_pixel({k: 1.0}), PAL, False)[0, 0, 0], O.colours(PAL, False, np.float64)[0, k])
    assert t[0, 4].tolist() == [1.0, -1.0, np.float32(220) / np.float32(127.5) - np.float32(1), 1.0]          # the hot-pink filler


def test_half_and_half_on_two_slots_is_their_midpoint_and_nothing_assumes_a_sum_of_one():
    t = O.colours(PAL, False, np.float64)
    y = O.lookup64(_one_pixel({1: 0.5, 3: 0.5}), PAL, False)[0, 0, 0]
    assert np.abs(y - (t[0, 1] + t[0, 3]) / 2).max() < 1e-15
    assert np.abs(O.lookup32(_one_pixel({1: 0.5, 3: 0.5}), PAL, False)[0, 0, 0] - y).max() < 2e-7
    # linear, no offset: twice the row gives twice the image, the zero row gives 0 (not -1)
    assert np.abs(O.lookup64(_one_pixel({1: 1.0, 3: 1.0}), PAL, False)[0, 0, 0] - 2 * y).max() < 1e-15
    assert not O.lookup64(_one_pixel({}), PAL, False).any() and not O.lookup32(_one_pixel({}), PAL, False).any()


def test_blacken_turns_a_transparent_slot_with_colour_into_minus_one():
    plain, black = O.colours(PAL, False), O.colours(PAL, True)
    assert plain[0, 2, 3] == -1.0 and (plain[0, 2, :3] != -1.0).all()           # alpha 0, RGB (90, 40, 250)
    assert black[0, 2].tolist() == [-1.0] * 4 and black[0, 0].tolist() == [-1.0] * 4
    keep = np.ones(O.K, bool)
    keep[2] = False
    assert np.array_equal(plain[0, keep], black[0, keep])                       # opaque slots and the filler are untouched
    assert PAL[0, 2].tolist() == [90, 40, 250, 0]                               # the palette itself is not modified
    for f in (O.lookup32, O.lookup64):
        assert f(_one_pixel({2: 1.0}), PAL, True)[0, 0, 0].tolist() == [-1.0] * 4
    assert O.hard_lookup(_one_pixel({2: 1.0}), PAL, True)[0][0, 0, 0].tolist() == [-1.0] * 4
    g = np.array([[[[1.0, 2.0, 4.0, 8.0]]]], np.float32)
    assert O.vjp32(g, PAL, True)[0, 0, 0, 2] == -15.0 and O.vjp32(g, PAL, False)[0, 0, 0, 2] != -15.0


# ---------------------------------------------------------------------------------------------------- the VJP
@pytest.mark.parametrize("blacken", [False, True])
@pytest.mark.parametrize("name", list(O.CASES))
def test_closed_form_vjp_equals_float64_autograd_of_the_restatement(name, blacken):
    probs, pal, g, _ = O.case(name, 4)
    t = torch.tensor(O.colours(pal, blacken, np.float64))
    x = torch.tensor(probs, dtype=F64, requires_grad=True)
    y = torch.einsum("nhwk,nkc->nhwc", x, t)
    assert np.abs(y.detach().numpy() - O.lookup64(probs, pal, blacken)).max() < 1e-14          # two float64 summation orders
    y.backward(torch.tensor(g, dtype=F64))
    want = x.grad.numpy()
    got = O.vjp64(g, pal, blacken)
    rel = np.abs(got - want).max() / np.abs(want).max()
    got32 = np.abs(O.vjp32(g, pal, blacken).astype(np.float64) - want).max() / np.abs(want).max()
    print(f"lookup {name} blacken {blacken}: closed form vs autograd {rel:.2e}, float32 restatement {got32:.2e} of max-norm {np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0 and rel <= 1e-10
    assert got32 <= 4 * 2.0 ** -23          # three sums and four products, each within half an ulp of a value <= the max-norm


# ---------------------------------------------------------------------------------------------------- the cases' premises
@pytest.mark.parametrize("name", list(O.CASES))
def test_the_hard_cases_hold_a_tie_and_a_filler_argmax(name):
    probs, pal, sizes = O.hard_case(name)
    _, idx = O.hard_lookup(probs, pal, False)
    top = probs.max(-1, keepdims=True)
    ties = (probs == top).sum(-1) > 1
    filler = idx >= sizes[:, None, None]
    print(f"hard {name}: {int(ties.sum())} pixels with a tie, {int(filler.sum())} with a filler argmax, of {idx.size}")
    assert ties.any() and filler.any()          # otherwise the case proves nothing
    first = probs.reshape(probs.shape[0], -1, O.K)[:, 0]
    assert (first[:, 130] == first[:, 201]).all() and (idx.reshape(len(sizes), -1)[:, 0] == 130).all()          # lowest of two equal maxima
    if idx[0].size >= 5:
        assert idx.reshape(len(sizes), -1)[:, :5].tolist() == [[130, 0, 255, 9, 1]] * len(sizes)


@pytest.mark.parametrize("name", list(O.CASES))
def test_the_soft_cases_hold_one_hot_rows_filler_mass_and_coloured_transparent_slots(name):
    for s in O.SPREADS:
        probs, pal, g, sizes = O.case(name, s)
        assert probs.dtype == np.float32 and pal.dtype == np.int32 and pal.shape == (probs.shape[0], O.K, 4)
        assert (5 <= sizes).all() and (sizes <= 40).all()
        for n, m in enumerate(sizes):
            assert (pal[n, m:] == np.array(O.FILLER)).all() and (pal[n, :m] != np.array(O.FILLER)).any(-1).all()
            clear = pal[n, :m, 3] == 0
            assert clear.sum() == 3 and (pal[n, :m][clear][:, :3] != 0).any()
        assert np.abs(probs.sum(-1) - 1).max() < 1e-5
        filler_mass = np.stack([probs[n, ..., m:].sum(-1) for n, m in enumerate(sizes)])
        one_hot = (probs == 1.0).any(-1) & ((probs != 0).sum(-1) == 1)
        if probs[0].size > O.K:
            assert one_hot.any() and (filler_mass > 0.9).any()
        assert (filler_mass > 0.5).any()          # N(0, s^2) logits over all 256 slots: most of the mass is on the filler anyway
        # three different palettes in the batch: a kernel that indexes the wrong image's palette is caught
        assert len({pal[n].tobytes() for n in range(len(sizes))}) == len(sizes)


def test_yardsticks_of_the_gpu_test():
    """prints what tests/test_palette_lookup_gpu.py compares the soft forward with: max |float32 sequential - float64| per case, and
    where the kernel's own order (four FMAs per lane, 64-lane butterfly) sits -- well inside 8 x the yardstick"""
    for name in O.CASES:
        for s in O.SPREADS:
            probs, pal, _, _ = O.case(name, s)
            y64, yard = O.reference(name, s, True)
            fly = float(np.abs(O.lookup32_butterfly(probs, pal, True).astype(np.float64) - y64).max())
            print(f"lookup {name} s {s}: yardstick (sequential f32) {yard:.2e}, butterfly order {fly:.2e}, max-norm {np.abs(y64).max():.3f}")
            assert np.abs(y64).max() <= 1.0 + 1e-6 and fly <= max(8 * yard, 2.0 ** -23 * np.abs(y64).max())
    big = [O.reference("2x64x64", s, True)[1] for s in O.SPREADS]
    assert all(1e-7 <= y <= 2e-6 for y in big), big          # a sum of 256 terms of size <= 1/256 .. 1: a few f32 ulps of 1


# ---------------------------------------------------------------------------------------------------- C ABI
NEW = {"p2p_palette_lookup_fwd": 10, "p2p_palette_lookup_bwd": 9}


def test_library_exports_the_lookup_entry_points_with_the_bound_signatures():
    if not os.path.exists(L.LIB_PATH):
        from palette_and_histo_gan_amd import build
        build.build_library(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pgan.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/p2pgan.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(L.SIGNATURES[name]) == nargs, (name, args)
        for a, t in zip(args, L.SIGNATURES[name]):
            want = L._vp if "*" in a else (L._f if a.startswith("float") else L._i)
            assert t is want, (name, a, t)
        assert L.lib().p2p_replay_fn_nargs(L.lib().p2p_replay_fn_index(name.encode())) == nargs


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(ctypes.byref(buf, (-ctypes.addressof(buf)) % 16), ctypes.c_void_p)          # host memory: never dereferenced
    off = ctypes.c_void_p(p.value + 4)
    fwd, bwd, err = L.lib().p2p_palette_lookup_fwd, L.lib().p2p_palette_lookup_bwd, L.lib().p2p_last_error
    good_f = [1, 2, 2, 256, p, p, 0, 0, p, None]
    good_b = [1, 2, 2, 256, p, p, 0, p, None]
    bad_f = [(3, 128, b"K = 128"), (3, 255, b"K = 255"), (3, 512, b"K = 512"), (4, None, b"null"), (5, None, b"null"), (8, None, b"null"),
             (4, off, b"aligned"), (5, off, b"aligned"), (8, off, b"aligned"), (0, 0, b"bad shape"), (1, 0, b"bad shape"), (2, -1, b"bad shape"),
             (0, 65536, b"bad shape"), (6, 2, b"hard = 2"), (6, -1, b"hard = -1"), (7, 2, b"blacken = 2"), (7, -1, b"blacken = -1")]
    bad_b = [(3, 128, b"K = 128"), (4, None, b"null"), (5, None, b"null"), (7, None, b"null"), (4, off, b"aligned"), (5, off, b"aligned"),
             (7, off, b"aligned"), (0, 0, b"bad shape"), (6, 2, b"blacken = 2")]
    for fn, good, bad, who in ((fwd, good_f, bad_f, b"p2p_palette_lookup_fwd"), (bwd, good_b, bad_b, b"p2p_palette_lookup_bwd")):
        for at, value, word in bad:
            args = list(good)
            args[at] = value
            assert fn(*args) < 0, (who, at, value)
            assert who in err() and word in err(), (at, value, err())


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_palette_lookup_checks_its_arguments_before_any_library_call(monkeypatch):
    import palette_and_histo_gan_amd as pkg
    assert pkg.Pix2PixIndexedColourModel is M.Pix2PixIndexedColourModel and issubclass(M.Pix2PixIndexedColourModel, M.Pix2PixIndexedModel)
    assert M.Pix2PixIndexedColourModel.differentiable_loss_hooks is True and issubclass(P.PaletteLookup, torch.autograd.Function)
    called = []
    monkeypatch.setattr(L, "call", lambda name, *a: called.append(name))
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    probs, pal = torch.zeros(2, 3, 3, 256, device=dev), np.zeros((2, 256, 4), np.int32)
    with pytest.raises(ValueError, match="palette"):
        P.palette_lookup(probs, np.zeros((3, 256, 4), np.int32), device=dev)          # batch mismatch
    with pytest.raises(ValueError, match="palette"):
        P.palette_lookup(probs, np.zeros((2, 40, 4), np.int32), device=dev)           # a short palette
    with pytest.raises(ValueError, match="palette"):
        P.palette_lookup(probs, np.zeros((2, 256, 3), np.int32), device=dev)
    with pytest.raises(ValueError, match="probabilities"):
        P.palette_lookup(torch.zeros(2, 3, 3, 128, device=dev), pal, device=dev)
    with pytest.raises(ValueError, match="indexed_to_rgba"):
        P.palette_lookup(torch.zeros(2, 3, 3, 1, dtype=torch.int32, device=dev), pal, device=dev)          # indices are not probabilities
    with pytest.raises(ValueError, match="probabilities"):
        P.palette_lookup(torch.zeros(0, 3, 3, 256, device=dev), np.zeros((0, 256, 4), np.int32), device=dev)
    for kw in ({"lambda_colour": -1.0}, {"lambda_histogram": -0.5}, {"lambda_colour": float("nan")}):
        with pytest.raises(ValueError, match=next(iter(kw))):          # before the model builds anything
            M.Pix2PixIndexedColourModel(None, None, "front2right", "indexed-colour-test", **kw)
    assert called == []
