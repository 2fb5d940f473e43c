"""-m gpu: p2p_palette_snap (csrc/palette.hip) behind palette.snap_to_palette, palette.palette_metrics, Pix2PixModel.generate(snap=)
and S2SModel.report_palette / the "evaluate_palette" callback.

The snap is integer arithmetic, so everything is compared with tests/palette_snap_oracle.py (brute force in numpy) for equality.
The kernel cases are the shapes of tests/test_palette_gpu.py (fewer pixels than a wave; K = 256; several workgroups per image;
an image without a palette) on its noisy inputs -- half the pixels off-palette -- plus an engineered case of duplicates, ties,
channel extremes and a NaN."""
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
from tests import palette_oracle as PO
from tests import palette_snap_oracle as O

pytestmark = pytest.mark.gpu

CASES = {"3x6x10x40": ((3, 6, 10, 40), [1, 37, 40]), "2x16x16x256": ((2, 16, 16, 256), [2, 256]),
         "2x64x64x40": ((2, 64, 64, 40), [40, 33]), "3x6x10x40-skip": ((3, 6, 10, 40), [37, -1, 40]),
         "1x33x7x256-engineered": ((1, 33, 7, 256), [256])}
_refs = {}
GUARD = 64                      # elements in front of and behind every output
I32_SENTINEL, I64_SENTINEL = 0x7F7F7F7F, 0x7F7F7F7F7F7F7F7F
TAGS = ["palette-off/test", "palette-off/train", "palette-tv/test", "palette-tv/train"]


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


def _reference(case):
    """inputs and the oracle's answer: computed once, shared, never modified"""
    if case not in _refs:
        (B, H, W, K), sizes = CASES[case]
        if case.endswith("engineered"):
            img, pal, sizes = O.engineered_case()
        else:
            img, pal, sizes = PO.noisy_palette_case(100 + len(case) + K, B, H, W, K, sizes)[:3]
        _refs[case] = (img, pal, sizes, O.snap(img, pal, sizes))
    return _refs[case]


def _guarded(shape, dtype, sentinel):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=U.DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, sentinel):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if sentinel != sentinel else bool((g == sentinel).all())


def _raw_snap(img, pal, sizes, with_image=True, with_dist=True):
    """p2p_palette_snap through the C ABI on sentinel-filled outputs with guard elements around them; checks the guards and
    returns (index, image, dist, counts, stats) as numpy arrays (image / dist: None when not asked for)"""
    B, H, W, _ = img.shape
    K = pal.shape[1]
    x, p, s = U.dev(img), U.dev(pal, torch.int32), U.dev(sizes, torch.int32)
    nan = float("nan")
    spec = [((B, H, W), torch.int32, I32_SENTINEL), ((B, H, W, 4), torch.float32, nan), ((B, H, W), torch.int32, I32_SENTINEL),
            ((B, K), torch.int32, I32_SENTINEL), ((B, 2), torch.int64, I64_SENTINEL)]
    bufs = [_guarded(*sp) for sp in spec]
    ptr = [U.ptr(v) for _, v in bufs]
    if not with_image:
        ptr[1] = C.c_void_p(0)
    if not with_dist:
        ptr[2] = C.c_void_p(0)
    L.call("p2p_palette_snap", B, H, W, U.ptr(x), U.ptr(p), U.ptr(s), K, *ptr, U.stream())
    torch.cuda.synchronize()
    for (buf, _), sp in zip(bufs, spec):
        assert _guards_intact(buf, sp[2]), sp
    out = [v.cpu().numpy() for _, v in bufs]
    if not with_image:
        assert np.isnan(out[1]).all()
        out[1] = None
    if not with_dist:
        assert (out[2] == I32_SENTINEL).all()
        out[2] = None
    return out


def _assert_equals_oracle(got, want, img):
    index, image, dist, counts, stats = got
    assert np.array_equal(index, want.index)
    assert np.array_equal(counts, want.counts)                                   # no sentinel survives: the oracle holds none
    assert np.array_equal(stats[:, 0], want.off_palette) and np.array_equal(stats[:, 1], want.distance_sum)
    if dist is not None:
        assert np.array_equal(dist, want.distance)
    if image is not None:
        assert image.tobytes() == want.image.tobytes()                           # bit for bit (a passed-through NaN included)


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_the_oracle_bit_for_bit(case):
    img, pal, sizes, want = _reference(case)
    HW = img.shape[1] * img.shape[2]
    print(f"snap {case}: oracle off-palette {want.off_palette.tolist()} of {HW}, distance sums {want.distance_sum.tolist()}")
    assert any(0 < o < HW for o in want.off_palette)          # otherwise the case proves nothing about dist
    got = _raw_snap(img, pal, sizes)
    _assert_equals_oracle(got, want, img)
    again = _raw_snap(img, pal, sizes)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))          # a second launch: identical bits
    _assert_equals_oracle(_raw_snap(img, pal, sizes, with_image=False, with_dist=False), want, img)
    # the public wrapper: the same answer, typed and shaped as documented
    s = P.snap_to_palette(img, pal, sizes)
    assert (s.index.dtype, s.image.dtype, s.distance.dtype, s.counts.dtype, s.off_palette.dtype, s.distance_sum.dtype) == \
        (torch.int32, torch.float32, torch.int32, torch.int32, torch.int64, torch.int64)
    assert not any(t.requires_grad for t in s) and all(t.is_cuda for t in s)
    _assert_equals_oracle([s.index.cpu().numpy(), s.image.cpu().numpy(), s.distance.cpu().numpy(), s.counts.cpu().numpy(),
                           torch.stack([s.off_palette, s.distance_sum], 1).cpu().numpy()], want, img)


def test_sizes_none_means_every_slot():
    img, pal, _, _ = _reference("2x16x16x256")
    pal = pal[:, ::-1].copy()          # image 0 is painted with the case's first two colours: now the LAST two slots
    none, full = P.snap_to_palette(img, pal), P.snap_to_palette(img, pal, [256, 256])
    assert all(torch.equal(a, b) for a, b in zip(none, full))
    want = O.snap(img, pal, None)
    assert np.array_equal(none.index.cpu().numpy(), want.index) and np.array_equal(none.counts.cpu().numpy(), want.counts)
    assert int(none.counts[0, 254:].sum()) > 128          # reached only if None means all 256 slots


@pytest.mark.parametrize("case", ["2x64x64x40", "1x33x7x256-engineered", "3x6x10x40-skip"])
def test_snapping_is_idempotent_and_stays_inside_the_palette(case):
    img, pal, sizes, _ = _reference(case)
    first = P.snap_to_palette(img, pal, sizes)
    second = P.snap_to_palette(first.image, pal, sizes)
    assert torch.equal(second.index, first.index) and not bool(second.distance.any())
    assert torch.equal(second.image, first.image) and not bool(second.off_palette.any())
    keep = [b for b, n in enumerate(sizes) if n > 0]          # an image without a palette was passed through, noise and all
    got_pal, got_n = P.extract_palette_batch(first.image[keep])
    for row, n, b in zip(got_pal.cpu().numpy(), got_n.cpu().numpy(), keep):
        allowed = {tuple(c) for c in pal[b][:min(int(sizes[b]), pal.shape[1])].tolist()}
        assert 0 < n and all(tuple(c) in allowed for c in row[:n].tolist())


def test_counts_of_an_on_palette_image_are_the_soft_histogram():
    """pixels that are palette colours, colours on a grid of 40 (any two are >= 40 / 255 apart, d >= 0.0246): at tau = 1e-3 a
    foreign slot weighs <= exp(-24.6) = 2e-11, so the soft histogram is the colour frequency to 1e-6 (tests/test_palette_cpu.py
    establishes the soft side) and the hard counts must equal it"""
    rng = np.random.default_rng(3)
    B, H, W, K = 2, 9, 11, 17
    digits = np.stack([rng.permutation(7 ** 4)[:K] for _ in range(B)])
    pal = (np.stack([digits // 7 ** c % 7 for c in range(4)], axis=-1) * 40).astype(np.int32)
    idx = rng.integers(0, K, size=(B, H, W))
    img = O.normalise(np.stack([pal[b][idx[b]] for b in range(B)]))
    s = P.snap_to_palette(img, pal)
    h, m = P.soft_palette_histogram(img, pal, None, 1e-3)
    freq = np.stack([np.bincount(idx[b].ravel(), minlength=K) for b in range(B)])
    assert np.array_equal(s.counts.cpu().numpy(), freq) and not bool(s.distance.any())
    assert float((s.counts.to(torch.float32) / (H * W) - h).abs().max()) <= 1e-6


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing():
    img, pal, sizes, _ = _reference("3x6x10x40")
    B, H, W, _ = img.shape
    x, p, s = U.dev(img), U.dev(pal, torch.int32), U.dev(sizes, torch.int32)
    outs = [_guarded((B, H, W), torch.int32, I32_SENTINEL), _guarded((B, H, W, 4), torch.float32, float("nan")),
            _guarded((B, H, W), torch.int32, I32_SENTINEL), _guarded((B, 40), torch.int32, I32_SENTINEL),
            _guarded((B, 2), torch.int64, I64_SENTINEL)]
    good = [B, H, W, U.ptr(x), U.ptr(p), U.ptr(s), 40] + [U.ptr(v) for _, v in outs] + [U.stream()]
    fn = L.lib().p2p_palette_snap
    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)          # noqa: E731
    bad = {"K = 0": (6, 0, "K = 0"), "K = 257": (6, 257, "K = 257"), "null img": (3, C.c_void_p(0), "null"),
           "null index": (7, C.c_void_p(0), "null"), "null counts": (10, C.c_void_p(0), "null"),
           "null stats": (11, C.c_void_p(0), "null"), "unaligned img": (3, off4(x), "aligned"),
           "unaligned palette": (4, off4(p), "aligned"), "unaligned image_out": (8, off4(outs[1][1]), "aligned"),
           "H = 0": (1, 0, "bad shape")}
    for name, (at, value, word) in bad.items():
        args = list(good)
        args[at] = value
        assert fn(*args) == -1, name
        msg = L.lib().p2p_last_error().decode()
        assert "p2p_palette_snap" in msg and word in msg, (name, msg)
    torch.cuda.synchronize()
    assert all(bool((b == I32_SENTINEL).all()) for b, _ in (outs[0], outs[2], outs[3]))          # nothing ran
    assert bool(torch.isnan(outs[1][0]).all()) and bool((outs[4][0] == I64_SENTINEL).all())
    assert fn(*good) == 0
    with pytest.raises(ValueError, match="palette for a batch of 3"):
        P.snap_to_palette(img, pal[:2])
    with pytest.raises(ValueError, match="expected 3 palette sizes"):
        P.snap_to_palette(img, pal, [1, 2])
    with pytest.raises(ValueError, match=r"\(B, H, W, 4\) RGBA batch"):
        P.snap_to_palette(img[..., :3], pal)


# ---------------------------------------------------------------------------------------------------- through the stack
def _model(cls=M.Pix2PixModel, **kw):
    if cls is M.Pix2PixIndexedModel:
        train, test = D.synthetic_indexed_ds(6, batch_size=2), D.synthetic_indexed_ds(4, batch_size=2, seed=3)
        return cls(train, test, "front2right", "snap-idx-test", lambda_segmentation=0.01, seed=5)
    train, test = D.synthetic_rgba_ds(6, batch_size=2), D.synthetic_rgba_ds(4, batch_size=2, seed=3)
    return cls(train, test, "front2right", "snap-test", lambda_l1=100.0, dtype="f32", seed=5, **kw)


def _colours(palette, size):
    return {tuple(c) for c in palette[:size].tolist()}


def test_generate_with_snap_returns_only_palette_colours():
    m = _model()
    batch = next(iter(m.train_ds))
    src, tgt = batch

    def same_dropout(call, *a, **kw):          # generate() keeps dropout on: rewind the device's draw so that calls can be compared
        m.engine.mask_counter_dev.zero_()
        return call(*a, **kw).clone()

    raw = same_dropout(m.generate, batch)
    assert torch.equal(raw, same_dropout(m.generator, src, training=True)) and torch.equal(raw, same_dropout(m.generate, batch, snap=None))
    t_pal, t_n = (t.cpu().numpy() for t in P.extract_palette_batch(tgt))
    s_pal, s_n = (t.cpu().numpy() for t in P.extract_palette_batch(src))
    raw_snap = P.snap_to_palette(raw, t_pal, t_n)
    assert int(raw_snap.off_palette.sum()) > 0          # the raw tanh output IS off the palette: the checks below show something
    for snap, pal, n in (("target", t_pal, t_n), ("source", s_pal, s_n), ((t_pal, t_n), t_pal, t_n), ((t_pal[:, :8], None), t_pal, [8, 8])):
        out = m.generate(batch, snap=snap)
        assert out.dtype == torch.float32 and out.shape == raw.shape and not out.requires_grad
        o_pal, o_n = (t.cpu().numpy() for t in P.extract_palette_batch(out))
        for b in range(2):
            assert 0 < o_n[b] and _colours(o_pal[b], o_n[b]) <= _colours(pal[b], n[b]), (snap if isinstance(snap, str) else "pair", b)
    assert torch.equal(same_dropout(m.generate, batch, snap="target"), raw_snap.image)
    with pytest.raises(ValueError, match="snap is None"):
        m.generate(batch, snap="nearest")


def test_palette_metrics_of_a_batch_against_itself_are_zero_and_count_what_strays():
    _, real = next(iter(D.synthetic_rgba_ds(2, batch_size=2, seed=9)))
    same = P.palette_metrics(real, real)
    assert set(same) == {"off_palette", "rms_distance", "histogram_tv", "valid"}
    assert same["valid"].tolist() == [True, True]
    for k in ("off_palette", "rms_distance", "histogram_tv"):
        assert same[k].shape == (2,) and same[k].is_cuda and not bool(same[k].any()), k
    # move 5 pixels of image 0 to one target colour +1 in red (off-palette, distance 1 each, histogram unchanged when the pixel
    # already had that colour); replace image 1 by noise: more than 256 colours in the REAL image make it invalid
    real = np.array(real, np.float32)
    fake = real.copy()
    px = fake[0].reshape(-1, 4)
    colour = O.quantise(px[0]).copy()
    colour[0] += 1 if colour[0] < 255 else -1
    rows = np.flatnonzero((O.quantise(px) == O.quantise(px[0])).all(-1))[:5]
    px[rows] = O.normalise(colour)
    noise = real.copy()
    noise[1] = np.random.default_rng(1).uniform(-1, 1, size=real[1].shape)
    m = P.palette_metrics(np.stack([fake[0], real[1]]), noise)
    HW = real.shape[1] * real.shape[2]
    assert m["valid"].tolist() == [True, False]
    assert m["off_palette"].tolist() == [np.float32(len(rows)) / np.float32(HW), 0.0]
    # rms_distance is evaluated in float64 and rounded to float32 once: half a float32 ulp, 2^-24 relative, plus float64 rounding
    want_rms = np.sqrt(len(rows) / (HW * 4.0)) / 255.0
    print("rms_distance", float(m["rms_distance"][0]), "exact", want_rms, "relative", abs(float(m["rms_distance"][0]) - want_rms) / want_rms)
    assert abs(float(m["rms_distance"][0]) - want_rms) <= (2.0 ** -24 + 1e-14) * want_rms and float(m["rms_distance"][1]) == 0.0
    assert m["histogram_tv"].tolist() == [0.0, 0.0] and len(rows) == 5


def _palette_rows(model):
    model.summary_writer.flush()
    return [r for r in map(json.loads, open(model.summary_writer.path)) if r["name"].startswith("palette-")]


def test_report_palette_and_the_fit_callback(capsys):
    m = _model()
    train, test = m.report_palette(4)
    print("report_palette", train, test)
    for d in (train, test):
        assert set(d) == {"off_palette", "rms_distance", "histogram_tv"}
        assert all(isinstance(v, float) and np.isfinite(v) and 0.0 <= v <= 1.0 for v in d.values())
    assert train["off_palette"] > 0          # an untrained generator does not paint palette colours
    m.fit(4, 2, callbacks=["evaluate_palette"])
    out = capsys.readouterr().out
    rows = _palette_rows(m)
    assert sorted({r["name"] for r in rows}) == TAGS
    assert sorted((r["step"], r["name"]) for r in rows) == sorted((s, t) for s in (0, 1, 2) for t in TAGS)
    assert all(np.isfinite(r["value"]) and 0.0 <= r["value"] <= 1.0 for r in rows)
    assert out.count(" Palette: off ") == 3 and "(train/test)" in out
    tr, te = m.report_palette(4, step=9)
    logged = {r["name"]: r["value"] for r in _palette_rows(m) if r["step"] == 9}
    assert logged == {"palette-off/train": tr["off_palette"], "palette-off/test": te["off_palette"],
                      "palette-tv/train": tr["histogram_tv"], "palette-tv/test": te["histogram_tv"]}


def test_a_fit_without_the_callback_writes_no_palette_tags(capsys):
    m = _model()
    m.fit(4, 2, callbacks=["evaluate_l1"])
    out = capsys.readouterr().out
    assert _palette_rows(m) == [] and "Palette:" not in out and " L1: " in out
    assert any(r["name"] == "l1-evaluation/test" for r in map(json.loads, open(m.summary_writer.path)))


def test_the_indexed_model_skips_the_callback_and_report_palette_raises(capsys):
    m = _model(M.Pix2PixIndexedModel)
    with pytest.raises(NotImplementedError, match="on-palette by construction"):
        m.report_palette(4)
    m.fit(2, 2, callbacks=["evaluate_palette"])
    out = capsys.readouterr().out
    assert out.count(" Palette: skipped (the indexed model is on-palette by construction)") == 2 and "Palette: off" not in out
    assert _palette_rows(m) == [] and m.engine.G.t == 2
