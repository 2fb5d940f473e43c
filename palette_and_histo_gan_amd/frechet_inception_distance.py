"""Fréchet Inception Distance (reference frechet_inception_distance.py): compare(a, b) of two image sets through the InceptionV3
features of inception.py.

Per image, as the reference computes it: astype(float32) -> skimage.transform.resize(image, (299, 299, 3), order=0)
(scikit-image 0.19: a gaussian anti-alias filter along every shrinking axis -- here only the channel axis of RGBA images, 4 -> 3 --
then scipy.ndimage.zoom(order=0, mode="mirror", grid_mode=True), then a clip to the image's [min, max]) -> preprocess_input
(x / 127.5 - 1) -> features.  The resize + preprocess runs on the GPU (p2p_inc_prep) from index tables built here with
scipy.ndimage.zoom itself, so its rounding of exact ties is scipy's.  The distance itself (means, covariances, sqrtm) is host
f64, as in the reference.

The weights file (inception.FORMAT) is `weights=` or the P2P_FID_WEIGHTS environment variable, read at call time; the network
is built on first use and cached per (file, device) -- unlike the reference, importing this module builds nothing.
"""
import ctypes as C
import os

import numpy as np
import scipy.linalg
import scipy.ndimage
import torch

from . import _lib as L
from . import inception as INC

ENV = "P2P_FID_WEIGHTS"
_networks = {}


def weights_path(weights=None):
    """the configured weights file, or FileNotFoundError saying how to produce one"""
    path = weights if weights is not None else os.environ.get(ENV)
    if not path:
        raise FileNotFoundError(f"FID needs the InceptionV3 weights: pass weights= or set {ENV} to a '*.inception.npz' file "
                                "(INTEGRATION.md: export it from a TensorFlow process that has keras.applications.InceptionV3)")
    if not os.path.exists(path):
        raise FileNotFoundError(f"FID weights file {path!r} (from {'weights=' if weights is not None else ENV}) does not exist")
    return os.fspath(path)


def configured_weights():
    """the file P2P_FID_WEIGHTS names, or None when FID cannot run (do_fit then skips it)"""
    path = os.environ.get(ENV)
    return path if path and os.path.exists(path) else None


def index_table(n_in, n_out):
    """output index o -> input index of scipy.ndimage.zoom(order=0, mode="mirror", grid_mode=True) along one axis of length n_in
    resized to n_out, with the zoom factor resize passes (1 / (n_in / n_out)); taken from zoom itself on an index ramp"""
    ramp = np.arange(n_in, dtype=np.float64)
    t = scipy.ndimage.zoom(ramp, 1.0 / (float(n_in) / float(n_out)), order=0, mode="mirror", grid_mode=True)
    if t.shape != (n_out,):
        raise ValueError(f"zoom of {n_in} -> {n_out} gave {t.shape[0]} samples")
    return t.astype(np.int32)


def channel_filter_weights(c_in, c_out=3):
    """(w0, w1) of the anti-alias gaussian resize applies along the channel axis (sigma = (c_in / c_out - 1) / 2, scipy's
    truncate 4.0 -> radius 1 for 4 -> 3), or None when the axis does not shrink"""
    factor = np.divide(c_in, c_out)
    sigma = max(0.0, (factor - 1) / 2)
    if sigma <= 0:
        return None
    radius = int(4.0 * float(sigma) + 0.5)
    if radius != 1:
        raise ValueError(f"{c_in} -> {c_out} channels: a {2 * radius + 1}-tap filter is not supported")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return float(phi[1]), float(phi[0])


def calculate_fid(act1, act2):
    """reference frechet_inception_distance.py:23-39 in f64: |mu1 - mu2|^2 + trace(s1 + s2 - 2 sqrtm(s1 s2)), real part"""
    a1, a2 = np.asarray(act1, np.float64), np.asarray(act2, np.float64)
    mu1, sigma1 = a1.mean(axis=0), np.cov(a1, rowvar=False)
    mu2, sigma2 = a2.mean(axis=0), np.cov(a2, rowvar=False)
    ssdiff = np.sum((mu1 - mu2) ** 2.0)
    covmean = scipy.linalg.sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(ssdiff + np.trace(sigma1 + sigma2 - 2.0 * covmean))


def network(weights=None, device="cuda:0"):
    """the cached InceptionV3Features of (weights file, device)"""
    path = os.path.abspath(weights_path(weights))
    key = (path, str(torch.device(device)))
    if key not in _networks:
        _networks[key] = INC.InceptionV3Features(path, device)
    return _networks[key]


def _load_directory_of_images(path):
    """reference :42-45 (skimage.io.imread of every file of the directory) with the build's PNG decoder"""
    from . import png
    return np.asarray([png.read_png(os.path.join(path, f)) for f in sorted(os.listdir(path))])


class _Tables:
    def __init__(self, H, W, Cc, device):
        self.rows = torch.from_numpy(index_table(H, INC.SIZE)).to(device)
        self.cols = torch.from_numpy(index_table(W, INC.SIZE)).to(device)
        self.chans = torch.from_numpy(index_table(Cc, 3)).to(device)
        self.filt = channel_filter_weights(Cc)


def activations(images, net):
    """(N, H, W, 3|4) images (array or tensor, any range; H, W <= 299) -> (N, 2048) f32 host features"""
    x = torch.as_tensor(np.asarray(images) if not isinstance(images, torch.Tensor) else images)
    if x.dim() != 4 or x.shape[3] not in (3, 4):
        raise ValueError(f"FID expects (N, H, W, 3 or 4) images, got {tuple(x.shape)}")
    N, H, W, Cc = (int(v) for v in x.shape)
    if H > INC.SIZE or W > INC.SIZE:
        # resize would also smooth the shrinking spatial axes: not implemented
        raise ValueError(f"FID supports images up to {INC.SIZE} x {INC.SIZE}, got {H} x {W}")
    if N < 1:
        raise ValueError("FID needs at least one image per set")
    dev = net.device
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    tab = _Tables(H, W, Cc, dev)
    w0, w1 = tab.filt if tab.filt is not None else (0.0, 0.0)
    buf = net.input_buffer(INC.SIZE, INC.SIZE)
    mm = torch.empty(2 * net.chunk, dtype=torch.float32, device=dev)
    out = torch.empty((N, INC.FEATURES), dtype=torch.float32, device=dev)
    view = L.Tensor(buf.data_ptr(), INC.SIZE * INC.SIZE, INC.SIZE, 3)
    st = torch.cuda.current_stream(dev).cuda_stream
    for s in range(0, N, net.chunk):
        n = min(net.chunk, N - s)
        L.call("p2p_inc_prep", n, H, W, Cc, x[s:s + n].data_ptr(), tab.rows.data_ptr(), tab.cols.data_ptr(), tab.chans.data_ptr(),
               INC.SIZE, INC.SIZE, w0, w1, int(tab.filt is not None), C.byref(view), mm.data_ptr(), st)
        net.run_chunk(n, INC.SIZE, INC.SIZE, out[s:s + n])
    return out.cpu().numpy()


def compare(dataset1_or_path, dataset2_or_path, weights=None, device="cuda:0"):
    """reference :67-68: FID between two image sets, each an (N, H, W, 3|4) array / tensor or a directory of PNG files"""
    path = weights_path(weights)            # before anything touches the GPU
    sets = [_load_directory_of_images(d) if isinstance(d, (str, os.PathLike)) else d for d in (dataset1_or_path, dataset2_or_path)]
    net = network(path, device)
    return calculate_fid(activations(sets[0], net), activations(sets[1], net))
