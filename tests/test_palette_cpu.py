"""Not gpu: the palette definitions (tests/palette_oracle.py) -- the closed-form VJP the backward kernel implements against autograd
of the float64 restatement, known answers of histogram, conformance and loss -- and the C ABI of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import palette as P
from tests import palette_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@pytest.mark.parametrize("shape,sizes", [((3, 6, 10, 40), [1, 37, 40]), ((2, 16, 16, 256), [2, 256]), ((2, 5, 7, 12), [-1, 12])])
@pytest.mark.parametrize("tau", [1e-3, 5e-2])
def test_closed_form_vjp_equals_autograd_in_float64(shape, sizes, tau):
    B, H, W, K = shape
    img, pal, sz, gh, gm = O.noisy_palette_case(7 + K, B, H, W, K, sizes)
    _, _, want = O.evaluate(img, pal, sz, tau, gh, gm, F64)
    got = O.closed_form_vjp(img, pal, sz, tau, gh, gm).numpy()
    assert np.abs(want).max() > 0
    # float64 rounding (2.2e-16) of a_k - abar where one colour dominates, times 2 / tau = 2000, relative to a gradient whose
    # largest entry can be ~100 times smaller than |a| c / tau: 5e-11 at most; a wrong term would show at 1e-2
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    if sizes[0] <= 0:
        assert not got[0].any() and not want[0].any()


def test_pixels_on_palette_colours_give_the_colour_frequencies():
    rng = np.random.default_rng(3)
    B, H, W, K = 2, 9, 11, 17
    pal = np.stack([rng.permutation(256)[:K] for _ in range(4 * B)]).reshape(B, 4, K).transpose(0, 2, 1).astype(np.int32)   # distinct rows
    idx = rng.integers(0, K, size=(B, H, W))
    img = np.stack([pal[b][idx[b]] for b in range(B)]).astype(np.float32) / 127.5 - 1.0
    h, m = O.soft_palette(img, pal, None, 1e-4)
    freq = np.stack([np.bincount(idx[b].ravel(), minlength=K) / (H * W) for b in range(B)])
    assert np.abs(h.numpy() - freq).max() < 1e-9            # f32 images are not exactly u/255: the nearest other colour is >= 1.5e-5 away in d
    assert float(m.max()) < 1e-9
    assert np.abs(h.sum(-1).numpy() - 1).max() < 1e-12


def test_a_single_slot_takes_all_the_mass_and_no_histogram_gradient():
    img, pal, sz, gh, gm = O.noisy_palette_case(5, 2, 6, 10, 8, [1, 1])
    x = torch.tensor(img).to(F64).requires_grad_(True)
    h, m = O.soft_palette(x, pal, sz, 1e-3)
    e0 = np.zeros((2, 8))
    e0[:, 0] = 1
    assert np.array_equal(h.detach().numpy(), e0)
    d = (((x.detach() * 0.5 + 0.5) - (torch.tensor(pal[:, :1]).to(F64) / 255).reshape(2, 1, 1, 4)) ** 2).sum(-1)
    assert np.allclose(m.detach().numpy(), d.mean(dim=(1, 2)).numpy(), rtol=1e-14)
    (h * torch.tensor(gh).to(F64)).sum().backward()
    assert not x.grad.numpy().any()
    assert not O.closed_form_vjp(img, pal, sz, 1e-3, gh, np.zeros(2)).numpy().any()


@pytest.mark.parametrize("tau", [1e-3, 5e-2, 1.0])
def test_rows_sum_to_one_and_far_pixels_keep_their_weights(tau):
    img, pal, sz, _, _ = O.noisy_palette_case(11, 3, 6, 10, 40, [1, 37, 40])
    pal[1, :37] = pal[1, :37] // 8                  # every colour far from most pixels: exp(-d / tau) alone would underflow at 1e-3
    h, m = O.soft_palette(img, pal, sz, tau)
    assert np.abs(h.sum(-1).numpy() - 1).max() < 1e-12 and bool(torch.isfinite(m).all())
    assert not h[0, 1:].any() and not h[1, 37:].any()
    h32, _ = O.soft_palette(img, pal, sz, tau, torch.float32)
    assert np.abs(h32.sum(-1).numpy() - 1).max() < 1e-5


def test_palette_histogram_loss_known_answers():
    h = torch.rand(4, 9, dtype=F64)
    h = h / h.sum(-1, keepdim=True)
    assert float(P.palette_histogram_loss(h, h)) == 0.0
    a, b = torch.zeros(3, 5), torch.zeros(3, 5)
    a[:, 1] = 1
    b[:, 3] = 1
    assert float(P.palette_histogram_loss(a, b)) == 1.0
    assert abs(float(P.palette_histogram_loss(h, h.roll(1, 0))) - float(O.palette_histogram_loss(h, h.roll(1, 0)))) < 1e-15
    hp = h.clone().requires_grad_(True)          # finite gradient at empty slots
    z = torch.zeros(4, 9, dtype=F64)
    P.palette_histogram_loss(z, hp * 0).backward()
    assert bool(torch.isfinite(hp.grad).all())


def test_extraction_oracle_orders_keys_and_flags_overflow():
    img = np.zeros((2, 4, 5, 4), np.float32) - 1.0                     # transparent black
    img[0, 0, 0] = 1.0                                                  # opaque white: key 0xFFFFFFFF
    img[0, 1, 1] = np.array([10, 0, 0, 255], np.float32) / 127.5 - 1.0
    img[0, 1, 2] = np.array([0, 10, 0, 255], np.float32) / 127.5 - 1.0
    pal, sizes = O.extract_palette(img)
    assert sizes.tolist() == [4, 1]
    assert pal[0, :4].tolist() == [[0, 0, 0, 0], [10, 0, 0, 255], [0, 10, 0, 255], [255, 255, 255, 255]] and not pal[0, 4:].any()
    noise = np.random.default_rng(0).uniform(-1, 1, size=(1, 32, 32, 4)).astype(np.float32)
    pal, sizes = O.extract_palette(noise)
    assert sizes.tolist() == [-1] and not pal.any()


def test_argument_checks_come_before_any_launch():
    pal = np.zeros((2, 8, 4), np.int32)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"          # the checks are host code and come before any launch
    with pytest.raises(ValueError, match="temperature"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 4, device=dev), pal, temperature=0.0, device=dev)
    with pytest.raises(ValueError, match="temperature"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 4, device=dev), pal, temperature=-1.0, device=dev)
    with pytest.raises(ValueError, match="palette"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 4, device=dev), np.zeros((2, 257, 4), np.int32), device=dev)
    with pytest.raises(ValueError, match="palette"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 4, device=dev), np.zeros((3, 8, 4), np.int32), device=dev)
    with pytest.raises(ValueError, match="RGBA"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 3, device=dev), pal, device=dev)
    with pytest.raises(ValueError, match="sizes"):
        P.soft_palette_histogram(torch.zeros(2, 4, 4, 4, device=dev), pal, sizes=[1, 2, 3], device=dev)
    with pytest.raises(ValueError, match="RGBA"):
        P.extract_palette_batch(torch.zeros(4, 4, 4, device=dev), device=dev)


NEW = {"p2p_palette_extract": 8, "p2p_soft_palette_fwd": 12, "p2p_soft_palette_bwd": 12}


def test_library_exports_the_palette_entry_points_with_the_bound_signatures():
    if not os.path.exists(L.LIB_PATH):
        from palette_and_histo_gan_amd import build
        build.build_library(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pgan.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/p2pgan.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(L.SIGNATURES[name]) == nargs, (name, args)
        for a, t in zip(args, L.SIGNATURES[name]):
            want = L._vp if "*" in a else (L._f if a.startswith("float") else L._i)
            assert t is want, (name, a, t)
        assert L.lib().p2p_replay_fn_nargs(L.lib().p2p_replay_fn_index(name.encode())) == nargs
    assert hasattr(lib, "p2p_soft_palette_workspace_bytes")
    args, res = L.SPECIAL["p2p_soft_palette_workspace_bytes"]
    assert args == [L._i, L._i, L._i] and res is ctypes.c_longlong
    wb = L.lib().p2p_soft_palette_workspace_bytes
    assert wb(1, 1, 1) > 0 and wb(4, 64, 64) == 4 * wb(1, 64, 64) and wb(1, 128, 128) > wb(1, 64, 64) and wb(0, 64, 64) == 0
    # host-side argument checks of the C ABI: refused before any launch, with a message
    assert L.lib().p2p_soft_palette_fwd(1, 4, 4, None, None, None, 8, 1e-3, None, None, None, None) < 0
    assert b"null" in L.lib().p2p_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(ctypes.byref(buf, (-ctypes.addressof(buf)) % 16), ctypes.c_void_p)
    assert L.lib().p2p_soft_palette_fwd(1, 2, 2, p, p, p, 257, 1e-3, p, p, p, None) < 0 and b"257" in L.lib().p2p_last_error()
    assert L.lib().p2p_soft_palette_bwd(1, 2, 2, p, p, p, 8, 0.0, p, p, p, None) < 0 and b"temperature" in L.lib().p2p_last_error()
    assert L.lib().p2p_palette_extract(1, 2, 2, p, 300, p, p, None) < 0 and b"cap" in L.lib().p2p_last_error()
