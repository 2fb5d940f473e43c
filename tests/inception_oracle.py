"""CPU restatement of the FID path (reference frechet_inception_distance.py) for the FID tests: scikit-image 0.19's
resize(order=0) spelled out with scipy.ndimage, Keras' preprocess_input, InceptionV3(include_top=False, pooling="avg") in torch
(NCHW, f64 or f32), and a generator of calibrated synthetic weights (no real ImageNet weights exist in a test environment).

Written apart from palette_and_histo_gan_amd/inception.py: its own network code (layer order, concatenation order, pooling
forms); only the weight SHAPES are taken from the build's layer table, and the network below checks them as it consumes them."""
import os

import numpy as np
import scipy.ndimage as ndi
import torch
import torch.nn.functional as F

from palette_and_histo_gan_amd import inception as INC
from palette_and_histo_gan_amd import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPRITES = os.path.join(ROOT, "tests", "golden", "reference_sprites.npz")


def sprites(count, start=0, step=1):
    """uint8 (count, 64, 64, 4) RGBA sprites decoded from the PNG bytes of tests/golden/reference_sprites.npz"""
    z = np.load(SPRITES)
    offs, data = z["offsets"], z["data"]
    idx = [start + step * i for i in range(count)]
    return np.stack([png.decode_png(data[offs[i]:offs[i + 1]].tobytes()) for i in idx])


# ---- resize + preprocess_input ----------------------------------------------------------------------------------------------

def skimage_resize_order0(image, output_shape):
    """skimage.transform.resize(image, output_shape, order=0) as scikit-image 0.19.3 computes it for a float32 image (mode
    "reflect" -> ndimage "mirror", anti_aliasing on when an axis shrinks, clip to the input's range)"""
    image = np.asarray(image, np.float32)
    factors = np.divide(image.shape, output_shape)
    lo, hi = image.min(), image.max()
    if any(o < i for o, i in zip(output_shape, image.shape)):
        sigma = np.maximum(0, (factors - 1) / 2)
        image = ndi.gaussian_filter(image, sigma, cval=0, mode="mirror")
    out = ndi.zoom(image, [1 / f for f in factors], order=0, mode="mirror", cval=0, grid_mode=True)
    assert out.shape == tuple(output_shape), (out.shape, output_shape)
    return np.clip(out, lo, hi)


def preprocess_input(x):
    """keras.applications.inception_v3.preprocess_input (mode "tf"): two separate f32 operations"""
    x = np.array(x, np.float32)
    x /= np.float32(127.5)
    x -= np.float32(1.0)
    return x


def prepare(images, size=INC.SIZE):
    """reference _compare_datasets: astype(float32) -> resize each image to (size, size, 3) -> preprocess_input"""
    images = np.asarray(images).astype(np.float32)
    return preprocess_input(np.stack([skimage_resize_order0(im, (size, size, 3)) for im in images]))


# ---- InceptionV3 --------------------------------------------------------------------------------------------------------------

class _Net:
    """weights consumed in creation order; with `calibrate` each BatchNorm's moving statistics are first set to the per-channel
    mean / variance (floor 1e-3) of its convolution's output on this batch"""

    def __init__(self, convs, dtype, calibrate=False):
        self.convs, self.dtype, self.calibrate, self.i = convs, dtype, calibrate, 0

    def conv(self, x, cout, kh, kw, stride=1, padding="same"):
        c = self.convs[self.i]
        k = np.asarray(c["kernel"])
        assert k.shape == (kh, kw, x.shape[1], cout), (self.i, k.shape, (kh, kw, x.shape[1], cout))
        w = torch.from_numpy(k.astype(np.float64)).permute(3, 2, 0, 1).to(self.dtype)
        pad = ((kh - 1) // 2, (kw - 1) // 2) if padding == "same" else (0, 0)
        z = F.conv2d(x, w, stride=stride, padding=pad)
        if self.calibrate:
            zd = z.to(torch.float64)
            c["moving_mean"] = zd.mean(dim=(0, 2, 3)).numpy().astype(np.float32)
            c["moving_variance"] = np.maximum(zd.var(dim=(0, 2, 3), unbiased=False).numpy(), 1e-3).astype(np.float32)
        var = np.asarray(c["moving_variance"], np.float64)
        scale = 1.0 / np.sqrt(var + INC.BN_EPS)
        shift = np.asarray(c["beta"], np.float64) - np.asarray(c["moving_mean"], np.float64) * scale
        sc = torch.from_numpy(scale).to(self.dtype).view(1, -1, 1, 1)
        sh = torch.from_numpy(shift).to(self.dtype).view(1, -1, 1, 1)
        self.i += 1
        return torch.relu(z * sc + sh)

    @staticmethod
    def maxpool(x):
        return F.max_pool2d(x, 3, 2)

    @staticmethod
    def avgpool(x):
        return F.avg_pool2d(x, 3, 1, padding=1, count_include_pad=False)


def features(x, convs, dtype=torch.float64, calibrate=False):
    """(N, H, W, 3) preprocessed images -> (N, 2048) pooled InceptionV3 features (torch CPU, `dtype` throughout)"""
    g = _Net(convs, dtype, calibrate)
    x = torch.as_tensor(np.asarray(x)).to(dtype).permute(0, 3, 1, 2).contiguous()
    x = g.conv(x, 32, 3, 3, 2, "valid")
    x = g.conv(x, 32, 3, 3, padding="valid")
    x = g.conv(x, 64, 3, 3)
    x = g.maxpool(x)
    x = g.conv(x, 80, 1, 1, padding="valid")
    x = g.conv(x, 192, 3, 3, padding="valid")
    x = g.maxpool(x)
    for pool_ch in (32, 64, 64):
        b1 = g.conv(x, 64, 1, 1)
        b5 = g.conv(g.conv(x, 48, 1, 1), 64, 5, 5)
        b3 = g.conv(g.conv(g.conv(x, 64, 1, 1), 96, 3, 3), 96, 3, 3)
        bp = g.conv(g.avgpool(x), pool_ch, 1, 1)
        x = torch.cat([b1, b5, b3, bp], 1)
    b3 = g.conv(x, 384, 3, 3, 2, "valid")
    bd = g.conv(g.conv(g.conv(x, 64, 1, 1), 96, 3, 3), 96, 3, 3, 2, "valid")
    x = torch.cat([b3, bd, g.maxpool(x)], 1)
    for c in (128, 160, 160, 192):
        b1 = g.conv(x, 192, 1, 1)
        b7 = g.conv(g.conv(g.conv(x, c, 1, 1), c, 1, 7), 192, 7, 1)
        bd = g.conv(x, c, 1, 1)
        for kh, kw, co in ((7, 1, c), (1, 7, c), (7, 1, c), (1, 7, 192)):
            bd = g.conv(bd, co, kh, kw)
        bp = g.conv(g.avgpool(x), 192, 1, 1)
        x = torch.cat([b1, b7, bd, bp], 1)
    b3 = g.conv(g.conv(x, 192, 1, 1), 320, 3, 3, 2, "valid")
    b7 = g.conv(g.conv(g.conv(g.conv(x, 192, 1, 1), 192, 1, 7), 192, 7, 1), 192, 3, 3, 2, "valid")
    x = torch.cat([b3, b7, g.maxpool(x)], 1)
    for _ in range(2):
        b1 = g.conv(x, 320, 1, 1)
        t = g.conv(x, 384, 1, 1)
        b3 = torch.cat([g.conv(t, 384, 1, 3), g.conv(t, 384, 3, 1)], 1)
        t = g.conv(g.conv(x, 448, 1, 1), 384, 3, 3)
        bd = torch.cat([g.conv(t, 384, 1, 3), g.conv(t, 384, 3, 1)], 1)
        bp = g.conv(g.avgpool(x), 192, 1, 1)
        x = torch.cat([b1, b3, bd, bp], 1)
    assert g.i == len(convs) == 94 and x.shape[1] == 2048
    return x.mean(dim=(2, 3))


def synthetic_weights(seed=7, calib_images=4, calib_size=INC.SIZE):
    """deterministic weights that keep activations O(1) through all 94 layers: He-normal kernels, beta ~ U(-0.1, 0.1), moving
    mean / variance (floor 1e-3) of each layer set to the statistics of its output on a fixed calibration batch (sprites resized
    to calib_size, one f64 pass).  Calibrated at 299: statistics taken at 75 x 75, where the deep maps are 1 x 1, do not carry
    over to 299 (the pooled features grew to ~1e5 there); calibrated at 299 they stay O(1) at both sizes."""
    rng = np.random.default_rng(seed)
    convs = []
    for s in INC.LAYERS:
        fan_in = s.kh * s.kw * s.cin
        convs.append({"kernel": (rng.standard_normal((s.kh, s.kw, s.cin, s.cout)) * np.sqrt(2.0 / fan_in)).astype(np.float32),
                      "beta": rng.uniform(-0.1, 0.1, s.cout).astype(np.float32),
                      "moving_mean": np.zeros(s.cout, np.float32), "moving_variance": np.ones(s.cout, np.float32)})
    with torch.no_grad():
        features(prepare(sprites(calib_images, start=3, step=17), calib_size), convs, torch.float64, calibrate=True)
    return convs


def fid_f64(act1, act2):
    """the FID formula, restated independently: trace(sqrtm(s1 s2)) as the sum of the square roots of the eigenvalues of
    s1 s2 (real and >= 0 for two covariance matrices)"""
    a1, a2 = np.asarray(act1, np.float64), np.asarray(act2, np.float64)
    m1, m2 = a1.mean(0), a2.mean(0)
    d1, d2 = a1 - m1, a2 - m2
    s1, s2 = d1.T @ d1 / (len(a1) - 1), d2.T @ d2 / (len(a2) - 1)
    ev = np.linalg.eigvals(s1 @ s2)
    return float(((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(ev.real, 0, None)).sum())
