"""-m gpu: the FID evaluation on the MI355X.  csrc/inception.hip's four entry points against f64 (one convolution per shape class
of InceptionV3, written into a channel slice of a sentinel-filled buffer), the whole feature extractor against the CPU oracle
(tests/inception_oracle.py) with calibrated synthetic weights, compare() against the oracle's FID, and report_fid /
fit(..., ["evaluate_fid"]) of both model families."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import frechet_inception_distance as FID
from palette_and_histo_gan_amd import inception as INC
from palette_and_histo_gan_amd import pix2pix_model as M
from palette_and_histo_gan_amd import png
from palette_and_histo_gan_amd import tb_events
from tests import gpu_util as U
from tests import inception_oracle as O

pytestmark = pytest.mark.gpu
DEV = U.DEV
SENTINEL = -12345.0


def _view(t, coff=0):
    """p2p_tensor of channels [coff, ...) of a dense (N, H, W, ld) tensor"""
    n, h, w, ld = t.shape
    return L.Tensor(t.data_ptr() + 4 * coff, h * w, w, ld)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def convs():
    return O.synthetic_weights()


@pytest.fixture(scope="module")
def weights_file(convs, tmp_path_factory):
    return INC.save_weights(str(tmp_path_factory.mktemp("fid") / "synthetic.inception.npz"), convs)


@pytest.fixture(scope="module")
def net(weights_file):
    return FID.network(weights_file, DEV)


# (kh, kw, stride, padding, Cin, Cout, H, W, N): the first layer (Cin = 3) and one case of every other shape class
CONV_CASES = [
    (3, 3, 2, "valid", 3, 32, 31, 29, 3),
    (1, 1, 1, "same", 64, 48, 17, 17, 1),
    (3, 3, 1, "same", 32, 64, 19, 21, 3),
    (3, 3, 1, "valid", 80, 192, 15, 15, 1),
    (3, 3, 2, "valid", 96, 96, 17, 17, 3),
    (5, 5, 1, "same", 48, 64, 13, 11, 1),
    (1, 3, 1, "same", 64, 128, 8, 8, 3),
    (3, 1, 1, "same", 64, 80, 8, 8, 1),
    (1, 7, 1, "same", 128, 160, 17, 17, 3),
    (7, 1, 1, "same", 160, 192, 17, 17, 1),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}x{c[1]}s{c[2]}{c[3]}_{c[4]}to{c[5]}_n{c[8]}")
def test_inc_conv_against_f64(case):
    kh, kw, stride, padding, cin, cout, H, W, N = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + cin)
    x = rng.uniform(-1, 1, (N, H, W, cin))
    k = rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * cin))
    scale = rng.uniform(0.5, 1.5, cout)
    shift = rng.uniform(-0.2, 0.2, cout)
    pt, pl = ((kh - 1) // 2, (kw - 1) // 2) if padding == "same" else (0, 0)
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(k).permute(3, 2, 0, 1), stride=stride, padding=(pt, pl))
    ref = torch.relu(ref * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1))
    ref = ref.permute(0, 2, 3, 1).numpy()
    OH, OW = ref.shape[1:3]
    # the input a slice of a wider buffer too (16-channel offset) for the vector path; the first layer reads a dense 3-channel map
    in_off = 0 if cin % 16 else 16
    xin = torch.full((N, H, W, cin + 2 * in_off), SENTINEL, dtype=torch.float32, device=DEV)
    xin[..., in_off:in_off + cin] = U.dev(x)
    out_off = 32
    out = torch.full((N, OH, OW, cout + 48), SENTINEL, dtype=torch.float32, device=DEV)
    w = U.dev(k.reshape(-1, cout))
    sc, sh = U.dev(scale), U.dev(shift)
    xv, ov = _view(xin, in_off), _view(out, out_off)
    got = []
    for _ in range(2):
        L.call("p2p_inc_conv", N, H, W, cin, kh, kw, stride, pt, pl, OH, OW, cout, C.byref(xv), w.data_ptr(), sc.data_ptr(),
               sh.data_ptr(), C.byref(ov), _stream())
        got.append(out.cpu().numpy())
    assert np.array_equal(got[0], got[1])                     # fixed-order sums: bit-identical relaunch
    g = got[0]
    assert np.all(g[..., :out_off] == SENTINEL) and np.all(g[..., out_off + cout:] == SENTINEL)
    err = np.abs(g[..., out_off:out_off + cout] - ref).max()
    assert err <= 1e-5 * np.abs(ref).max(), (err, np.abs(ref).max())


@pytest.mark.parametrize("kind", [0, 1])
def test_inc_pool_against_f64(kind):
    N, H, W, Cc = 3, 17, 15, 40
    x = np.random.default_rng(kind).standard_normal((N, H, W, Cc))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    ref = F.max_pool2d(xt, 3, 2) if kind == 0 else F.avg_pool2d(xt, 3, 1, padding=1, count_include_pad=False)
    ref = ref.permute(0, 2, 3, 1).numpy()
    xin = torch.full((N, H, W, Cc + 8), SENTINEL, dtype=torch.float32, device=DEV)
    xin[..., 4:4 + Cc] = U.dev(x)
    out = torch.full((N,) + ref.shape[1:3] + (Cc + 24,), SENTINEL, dtype=torch.float32, device=DEV)
    xv, ov = _view(xin, 4), _view(out, 16)
    L.call("p2p_inc_pool", kind, N, H, W, Cc, C.byref(xv), C.byref(ov), _stream())
    g = out.cpu().numpy()
    assert np.all(g[..., :16] == SENTINEL) and np.all(g[..., 16 + Cc:] == SENTINEL)
    g = g[..., 16:16 + Cc]
    if kind == 0:
        assert np.array_equal(g, ref.astype(np.float32))
    else:
        assert np.abs(g - ref).max() <= 1e-6 * np.abs(ref).max()


def test_inc_gap_against_f64():
    N, H, W, Cc = 3, 8, 8, 2048
    x = np.random.default_rng(5).uniform(0, 2, (N, H, W, Cc))
    xin = U.dev(x)
    out = torch.empty((N, Cc), dtype=torch.float32, device=DEV)
    xv = _view(xin)
    L.call("p2p_inc_gap", N, H, W, Cc, C.byref(xv), out.data_ptr(), _stream())
    ref = x.mean(axis=(1, 2))
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-6 * np.abs(ref).max()


def _prep_gpu(images):
    N, H, W, Cc = images.shape
    x = U.dev(images)
    rows, cols, chans = (U.dev(FID.index_table(a, b), torch.int32) for a, b in ((H, 299), (W, 299), (Cc, 3)))
    filt = FID.channel_filter_weights(Cc)
    w0, w1 = filt if filt else (0.0, 0.0)
    out = torch.full((N, 299, 299, 3), SENTINEL, dtype=torch.float32, device=DEV)
    mm = torch.empty(2 * N, dtype=torch.float32, device=DEV)
    ov = _view(out)
    L.call("p2p_inc_prep", N, H, W, Cc, x.data_ptr(), rows.data_ptr(), cols.data_ptr(), chans.data_ptr(), 299, 299, w0, w1,
           int(filt is not None), C.byref(ov), mm.data_ptr(), _stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("form", ["rgba_pm1", "rgba_255", "tie56", "rgb"])
def test_inc_prep_within_one_ulp_of_the_oracle(form):
    s = O.sprites(3, start=40, step=7).astype(np.float32)
    if form == "rgba_pm1":
        imgs = s / np.float32(127.5) - np.float32(1.0)          # what the RGBA models hand to compare
    elif form == "rgba_255":
        imgs = s                                                 # indexed_to_rgba of the indexed model
    elif form == "tie56":
        imgs = s[:, 3:59, 5:61]                                  # 56: an input size where exact ties decide the pick
    else:
        imgs = s[:, 2:42, 7:57, :3] * np.float32(0.5) + np.float32(3.25)
    imgs = np.ascontiguousarray(imgs)
    want = O.prepare(imgs)
    got = _prep_gpu(imgs)
    np.testing.assert_array_max_ulp(got, want, maxulp=1)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("size,n", [(75, 3), (299, 2)])
def test_features_against_the_f64_oracle(net, convs, size, n):
    x = O.prepare(O.sprites(n, start=11, step=29), size)
    with torch.no_grad():
        f64 = O.features(x, convs, torch.float64).numpy()
        f32 = O.features(x, convs, torch.float32).numpy()
    got = net(torch.from_numpy(x).to(DEV)).cpu().numpy()
    again = net(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == (n, 2048) and np.array_equal(got, again)
    tol = max(1e-5, 1.5 * _rel(f32, f64))
    assert _rel(got, f64) <= tol, (_rel(got, f64), _rel(f32, f64))


def test_compare_against_the_oracle_fid(net, convs, weights_file, tmp_path):
    a = O.sprites(8, start=0, step=3)
    b = O.sprites(8, start=200, step=5)
    got = FID.compare(a, b, weights=weights_file, device=DEV)
    with torch.no_grad():
        fa64, fb64 = (O.features(O.prepare(s), convs, torch.float64).numpy() for s in (a, b))
        fa32, fb32 = (O.features(O.prepare(s), convs, torch.float32).numpy() for s in (a, b))
    want = FID.calculate_fid(fa64, fb64)
    dev32 = abs(FID.calculate_fid(fa32, fb32) - want) / abs(want)
    assert want > 0 and abs(got - want) / abs(want) <= max(1e-4, 1.5 * dev32), (got, want, dev32)
    # the PNG-directory form reads the same images
    folder = tmp_path / "set_b"
    folder.mkdir()
    for i, im in enumerate(b):
        png.write_png(str(folder / f"{i:02d}.png"), im)
    assert abs(FID.compare(a, str(folder), weights=weights_file, device=DEV) - got) <= 1e-9 * abs(got)
    same = FID.compare(a, a, weights=weights_file, device=DEV)
    assert abs(same) <= 1e-3 * got, (same, got)


def _fid_events(model):
    model.summary_writer.flush()
    return [(st, tag, v) for st, tag, v in tb_events.read_events(model.summary_writer.events.path) if tag.startswith("fid/")]


@pytest.mark.parametrize("family", ["rgba", "indexed"])
def test_fit_evaluates_fid_with_weights_and_skips_without(family, weights_file, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv(FID.ENV, weights_file)
    if family == "rgba":
        train, test = D.synthetic_rgba_ds(6, batch_size=4), D.synthetic_rgba_ds(5, batch_size=4, seed=3)
        model = M.Pix2PixModel(train, test, "front2right", "fid-test", lambda_l1=100.0)
    else:
        train, test = D.synthetic_indexed_ds(6, batch_size=4), D.synthetic_indexed_ds(5, batch_size=4, seed=3)
        model = M.Pix2PixIndexedModel(train, test, "front2right", "fid-idx-test", lambda_segmentation=0.01)
    model.fit(3, 3, callbacks=["evaluate_fid"])
    out = capsys.readouterr().out
    assert out.count("FID: ") == 2 and "skipped" not in out
    ev = _fid_events(model)
    assert sorted((st, tag) for st, tag, _ in ev) == [(0, "fid/test"), (0, "fid/train"), (1, "fid/test"), (1, "fid/train")]
    assert all(np.isfinite(v) and v >= 0 for _, _, v in ev)
    tr, te = model.report_fid(num_images=4, step=7)
    logged = {tag: v for st, tag, v in _fid_events(model) if st == 7}
    assert logged == {"fid/train": np.float32(tr), "fid/test": np.float32(te)}
    # without weights: report_fid refuses, the fit callback keeps the skip line and trains on
    monkeypatch.delenv(FID.ENV)
    with pytest.raises(FileNotFoundError, match=FID.ENV):
        model.report_fid(num_images=4)
    t0 = model.engine.G.t
    model.fit(1, 1, callbacks=["evaluate_fid"])
    out = capsys.readouterr().out
    assert "FID needs the InceptionV3 ImageNet weights (network fetch): skipped" in out and "FID: " not in out
    assert model.engine.G.t == t0 + 1
