"""-m gpu: p2p_palette_quantize (csrc/palette.hip) behind palette.quantize_palette / palette.quantize, Pix2PixModel.generate(snap=K)
and S2SModel.report_quantized / the "evaluate_quantized" callback.

The quantiser is integer arithmetic, so every comparison is equality with tests/palette_quantize_oracle.py (brute force in numpy);
tests/test_palette_quantize_cpu.py shows from the oracle's trace that the shared cases meet the ties, empty slots and coinciding
centroids they are here for.  The shapes are the smallest at which each part of the kernel can go wrong: fewer pixels than a wave,
H * W no multiple of 64, the exact-palette path beside the Lloyd path in one launch, K = 256 on a mostly-one-colour image (the
contended slot), and 128 x 128, the LDS limit."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import palette as P
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import gpu_util as U
from tests import palette_quantize_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements in front of and behind every output
SENTINEL = 0x7F7F7F7F
TAGS = ["quantized-l1/test", "quantized-l1/train", "quantized-rms/test", "quantized-rms/train"]
_inputs, _refs = {}, {}


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


def _two_colour_image():
    img = np.full((4, 4, 4), -1.0, np.float32)
    img[1:3, 1:3] = O.SO.normalise([200, 10, 30, 255])
    return img


def _case(name):
    """(img (B, H, W, 4), init_palette or None, init_sizes or None, K): built once, shared, never modified"""
    if name not in _inputs:
        if name == "1x1x1":
            v = (O.noise_image(3, 1, 1)[None], None, None, 2)
        elif name == "2x4x4-lattice":          # image 1 has two colours: the exact-palette path beside the Lloyd path
            v = (np.stack([O.lattice_image(0, 4, 5), _two_colour_image()]), None, None, 8)
        elif name == "2x4x4-coincide":
            v = (np.stack([O.lattice_image(2243, 3, 1), O.lattice_image(960, 3, 1)]), None, None, 3)
        elif name == "2x4x4-init":
            v = (np.stack([O.small_values_image(1), O.small_values_image(3)]), np.stack([O.EMPTY_SLOT_INIT] * 2), np.array([4, 4], np.int32), 4)
        elif name == "3x7x9":
            img, init, sizes = O.edge_batch()
            v = (img, init, sizes, 5)
        elif name == "1x33x7":
            v = (O.noise_image(0, 33, 7)[None], None, None, 256)
        elif name == "2x64x64":
            v = (np.stack([O.sprite_like_image(1)[0], O.noise_image(2, 64, 64)]), None, None, 256)
        elif name == "1x128x128":
            v = (O.noise_image(6, 128, 128)[None], None, None, 256)
        _inputs[name] = v
    return _inputs[name]


def _reference(name, colours, iterations):
    key = (name, colours, iterations)
    if key not in _refs:
        img, init, sizes, K = _case(name)
        _refs[key] = O.quantize(img, colours, iterations, init, sizes, K)
    return _refs[key]


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=U.DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _raw(img, colours, iterations, init, sizes, K, with_iters=True):
    """p2p_palette_quantize through the C ABI on sentinel-filled outputs between guard elements: (palette, sizes, iters or None)"""
    B, H, W, _ = img.shape
    x = U.dev(img)
    ip = isz = C.c_void_p(0)
    if init is not None:
        held = U.dev(init, torch.int32), U.dev(sizes, torch.int32)          # alive until the synchronize below
        ip, isz = U.ptr(held[0]), U.ptr(held[1])
    bufs = [_guarded((B, K, 4)), _guarded((B,)), _guarded((B,))]
    ptrs = [U.ptr(v) for _, v in bufs]
    if not with_iters:
        ptrs[2] = C.c_void_p(0)
    L.call("p2p_palette_quantize", B, H, W, U.ptr(x), colours, iterations, ip, isz, K, *ptrs, U.stream())
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    pal, sz, it = (v.cpu().numpy() for _, v in bufs)
    assert not (pal == SENTINEL).any() and not (sz == SENTINEL).any()          # every element is written
    if not with_iters:
        assert (it == SENTINEL).all()
        return pal, sz, None
    assert not (it == SENTINEL).any()
    return pal, sz, it


RUNS = [("1x1x1", 2, 8), ("1x1x1", 1, 0)] + [("2x4x4-lattice", c, 8) for c in (3, 4, 5, 6)] + [("2x4x4-coincide", 3, 8), ("2x4x4-init", 4, 8)] + \
    [("3x7x9", 5, i) for i in (0, 1, 8)] + [("1x33x7", 16, i) for i in (1, 8, 50, 64)] + [("2x64x64", c, 8) for c in (1, 16, 256)] + \
    [("1x128x128", 256, 2)]


@pytest.mark.parametrize("name,colours,iterations", RUNS, ids=[f"{n}-c{c}-i{i}" for n, c, i in RUNS])
def test_kernel_equals_the_oracle_bit_for_bit(name, colours, iterations):
    img, init, sizes, K = _case(name)
    want_pal, want_n, want_it, trace = _reference(name, colours, iterations)
    print(f"quantize {name} colours {colours} iterations {iterations}: oracle sizes {want_n.tolist()} iters {want_it.tolist()} "
          f"exact {[t['exact'] for t in trace]}")
    got = _raw(img, colours, iterations, init, sizes, K)
    assert np.array_equal(got[1], want_n) and np.array_equal(got[2], want_it)
    assert np.array_equal(got[0], want_pal)
    again = _raw(img, colours, iterations, init, sizes, K)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))          # a second launch: identical bits
    without = _raw(img, colours, iterations, init, sizes, K, with_iters=False)
    assert np.array_equal(without[0], want_pal) and np.array_equal(without[1], want_n)


def test_the_launch_mixes_the_exact_and_the_lloyd_path_and_the_exact_rows_are_the_extraction():
    img, _, _, K = _case("2x4x4-lattice")
    trace = _reference("2x4x4-lattice", 4, 8)[3]
    assert [t["exact"] for t in trace] == [False, True]
    pal, n, it = _raw(img, 4, 8, None, None, K)
    e_pal, e_n = (t.cpu().numpy() for t in P.extract_palette_batch(img[1:]))
    assert n[1] == e_n[0] == 2 and it[1] == 0 and np.array_equal(pal[1], e_pal[0, :K])


def test_an_image_alone_gives_its_rows_of_the_batched_call():
    img, init, sizes, K = _case("3x7x9")
    pal, n, it = _raw(img, 5, 8, init, sizes, K)
    for b in range(3):
        one = _raw(img[b:b + 1], 5, 8, init[b:b + 1], sizes[b:b + 1], K)
        assert np.array_equal(one[0][0], pal[b]) and one[1][0] == n[b] and one[2][0] == it[b], b


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing():
    img, init, sizes, K = _case("3x7x9")
    B, H, W, _ = img.shape
    x, ip, isz = U.dev(img), U.dev(init, torch.int32), U.dev(sizes, torch.int32)
    big = torch.zeros((1, 1, (1 << 14) + 1, 4), dtype=torch.float32, device=U.DEV)
    outs = [_guarded((B, K, 4)), _guarded((B,)), _guarded((B,))]
    good = [B, H, W, U.ptr(x), 5, 8, U.ptr(ip), U.ptr(isz), K] + [U.ptr(v) for _, v in outs] + [U.stream()]
    fn = L.lib().p2p_palette_quantize
    null = C.c_void_p(0)
    bad = {"colours = 0": ({4: 0}, "colours"), "colours > K": ({4: K + 1}, "colours"), "iterations = 65": ({5: 65}, "iterations"),
           "H * W = 2^14 + 1": ({0: 1, 1: 1, 2: (1 << 14) + 1, 3: U.ptr(big)}, "2^14"), "init_sizes alone": ({6: null}, "together"),
           "init_palette alone": ({7: null}, "together"), "K = 257": ({8: 257}, "K = 257"), "null img": ({3: null}, "null"),
           "unaligned palette_out": ({9: C.c_void_p(outs[0][1].data_ptr() + 4)}, "aligned")}
    for name, (change, word) in bad.items():
        args = list(good)
        for at, value in change.items():
            args[at] = value
        assert fn(*args) < 0, name
        msg = L.lib().p2p_last_error().decode()
        assert "p2p_palette_quantize" in msg and word in msg, (name, msg)
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b, _ in outs)          # nothing ran
    assert fn(*good) == 0
    torch.cuda.synchronize()


def test_the_wrappers_return_the_kernels_bits_and_an_image_of_at_most_k_colours():
    img, _, _, K = _case("2x64x64")
    want = _raw(img, 16, 8, None, None, K)
    pal, n = P.quantize_palette(img, colours=16)
    assert (pal.dtype, n.dtype, tuple(pal.shape), tuple(n.shape)) == (torch.int32, torch.int32, (2, 256, 4), (2,))
    assert pal.is_cuda and n.is_cuda and not pal.requires_grad
    assert np.array_equal(pal.cpu().numpy(), want[0]) and np.array_equal(n.cpu().numpy(), want[1])
    snap, pal2, n2 = P.quantize(img, colours=16)
    assert torch.equal(pal2, pal) and torch.equal(n2, n)
    direct = P.snap_to_palette(img, pal, n)
    assert all(torch.equal(a, b) for a, b in zip(snap, direct))
    again = P.snap_to_palette(snap.image, pal, n)
    assert torch.equal(again.image, snap.image) and not bool(again.distance.any())
    # starting slots through the wrapper: padded to 256 rows on the device, the sizes as given
    e_img, e_init, e_sizes, _ = _case("3x7x9")
    w_pal, w_n, _, _ = O.quantize(e_img, 5, 8, e_init, e_sizes, 256)
    g_pal, g_n = P.quantize_palette(e_img, colours=5, init=(e_init, e_sizes))
    assert np.array_equal(g_pal.cpu().numpy(), w_pal) and np.array_equal(g_n.cpu().numpy(), w_n)
    # at most k colours per image; an image that had no more keeps exactly its own
    small = np.stack([O.lattice_image(0, 4, 5), _two_colour_image()])
    for k in (1, 2, 5):
        out = P.quantize(small, colours=k)[0].image
        o_pal, o_n = (t.cpu().numpy() for t in P.extract_palette_batch(out))
        assert (0 < o_n).all() and (o_n <= k).all(), (k, o_n)
        if k >= 2:
            own_pal, own_n = (t.cpu().numpy() for t in P.extract_palette_batch(small[1:]))
            assert o_n[1] == own_n[0] == 2 and np.array_equal(o_pal[1], own_pal[0])


# ---------------------------------------------------------------------------------------------------- through the stack
def _model(cls=M.Pix2PixModel):
    if cls is M.Pix2PixIndexedModel:
        train, test = D.synthetic_indexed_ds(6, batch_size=2), D.synthetic_indexed_ds(4, batch_size=2, seed=3)
        return cls(train, test, "front2right", "quant-idx-test", lambda_segmentation=0.01, seed=5)
    train, test = D.synthetic_rgba_ds(6, batch_size=2), D.synthetic_rgba_ds(4, batch_size=2, seed=3)
    return cls(train, test, "front2right", "quant-test", lambda_l1=100.0, dtype="f32", seed=5)


def _rows(model):
    model.summary_writer.flush()
    return [r for r in map(json.loads, open(model.summary_writer.path)) if r["name"].startswith("quantized-")]


def test_generate_with_a_number_of_colours_is_the_quantised_output():
    m = _model()
    batch = next(iter(m.train_ds))

    def same_dropout(call, *a, **kw):          # generate() keeps dropout on: rewind the device's draw so that calls can be compared
        m.engine.mask_counter_dev.zero_()
        return call(*a, **kw).clone()

    raw = same_dropout(m.generate, batch)
    out = same_dropout(m.generate, batch, snap=8)
    assert out.dtype == torch.float32 and out.shape == raw.shape and not out.requires_grad
    assert torch.equal(out, P.quantize(raw, 8)[0].image) and not torch.equal(out, raw)
    _, o_n = P.extract_palette_batch(out)
    assert bool((o_n > 0).all()) and bool((o_n <= 8).all())
    with pytest.raises(TypeError, match="snap is None"):
        m.generate(batch, snap=True)
    with pytest.raises(ValueError, match="colours"):
        m.generate(batch, snap=0)


def test_report_quantized_and_the_fit_callback(capsys):
    m = _model()

    def rewound(call, *a, **kw):
        m.engine.mask_counter_dev.zero_()
        return call(*a, **kw)

    l1_train, l1_test = rewound(m.report_l1, 4)
    train, test = rewound(m.report_quantized, 4, colours=8)
    print("report_quantized", train, test)
    for d, l1 in ((train, l1_train), (test, l1_test)):
        assert set(d) == {"l1", "l1_quantized", "rms_distance", "colours"}
        assert all(isinstance(v, float) and np.isfinite(v) for v in d.values())
        assert 1.0 <= d["colours"] <= 8.0 and d["rms_distance"] > 0.0 and d["l1"] == float(l1)
    m.fit(1, 1, callbacks=["evaluate_quantized"])
    out = capsys.readouterr().out
    rows = _rows(m)
    assert sorted({r["name"] for r in rows}) == TAGS and all(np.isfinite(r["value"]) for r in rows)
    assert out.count(" Quantized: L1 ") >= 1 and "(train/test)" in out
    tr, te = m.report_quantized(4, colours=8, step=9)
    logged = {r["name"]: r["value"] for r in _rows(m) if r["step"] == 9}
    assert logged == {"quantized-l1/train": tr["l1_quantized"], "quantized-l1/test": te["l1_quantized"],
                      "quantized-rms/train": tr["rms_distance"], "quantized-rms/test": te["rms_distance"]}


def test_the_indexed_model_skips_the_callback_and_report_quantized_raises(capsys):
    m = _model(M.Pix2PixIndexedModel)
    with pytest.raises(NotImplementedError, match="on-palette by construction"):
        m.report_quantized(4)
    m.fit(1, 1, callbacks=["evaluate_quantized"])
    out = capsys.readouterr().out
    assert " Quantized: skipped (the indexed model is on-palette by construction)" in out and "Quantized: L1" not in out
    assert _rows(m) == []
