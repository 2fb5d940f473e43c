"""InceptionV3 feature extractor for the FID evaluation (reference frechet_inception_distance.py:76: Keras
InceptionV3(include_top=False, pooling="avg", input_shape=(299, 299, 3)) in inference mode) on the kernels of
csrc/inception.hip.

`_network` below is the layer table: the 94 conv2d_bn blocks (Conv2D without bias -> BatchNormalization(scale=False, eps 1e-3) ->
ReLU) and the pools in Keras' creation order, with the concatenation order of every mixed block.  Tracing it once gives the
weight shapes (LAYERS), tracing it for an input size gives the launch sequence and the buffer plan of that size.

Weights come from a plain `.npz` (FORMAT below; INTEGRATION.md shows the TF-side export): conv/NN/{kernel, beta, moving_mean,
moving_variance} for NN = 00..93 in the table's order, kernels in Keras' HWIO layout.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

FORMAT = "p2pgan-inceptionv3-notop-1"
BN_EPS = 1e-3
SIZE = 299            # the network's input size as the reference builds it
FEATURES = 2048
CHUNK = 32            # images per pass through the network: bounds the workspace (~450 MB at 299 x 299)
ARRAYS = ("kernel", "beta", "moving_mean", "moving_variance")

ConvSpec = namedtuple("ConvSpec", "index kh kw cin cout stride padding")

# op kinds of a traced plan
_CONV, _MAXPOOL, _AVGPOOL, _GAP = "conv", "maxpool", "avgpool", "gap"


class _Act:
    """an (N, H, W, C) activation in channels [coff, coff + C) of workspace slot `slot` (ld channels per pixel)"""

    def __init__(self, slot, H, W, C, ld=None, coff=0):
        self.slot, self.H, self.W, self.C = slot, H, W, C
        self.ld = C if ld is None else ld
        self.coff = coff

    def slice(self, coff, C):
        return _Act(self.slot, self.H, self.W, C, self.ld, self.coff + coff)


class _Trace:
    """records the layer table and the op sequence.  Slots: "in" (the preprocessed images), "x0" / "x1" (block inputs and
    concatenations, alternating), "t1" / "t2" (chained branch temporaries, alternating), "tp" (the average-pool branch)."""

    def __init__(self):
        self.convs, self.ops, self.slot_floats = [], [], {}

    def _use(self, a):
        self.slot_floats[a.slot] = max(self.slot_floats.get(a.slot, 0), a.H * a.W * a.ld)
        return a

    def input(self, H, W):
        return self._use(_Act("in", H, W, 3))

    def block_out(self, x, C, H=None, W=None):
        """the concatenation buffer a block reading `x` writes (H x W: the block's output map, x's by default)"""
        return self._use(_Act("x1" if x.slot == "x0" else "x0", x.H if H is None else H, x.W if W is None else W, C))

    def _temp(self, x, H, W, C):
        return self._use(_Act("t2" if x.slot == "t1" else "t1", H, W, C))

    def conv(self, x, cout, kh, kw, stride=1, padding="same", out=None):
        if padding == "same":
            assert stride == 1 and kh % 2 == 1 and kw % 2 == 1
            OH, OW = x.H, x.W
        else:
            OH, OW = (x.H - kh) // stride + 1, (x.W - kw) // stride + 1
        if OH < 1 or OW < 1:
            raise ValueError(f"input too small for InceptionV3: conv {len(self.convs)} would produce {OH} x {OW}")
        spec = ConvSpec(len(self.convs), kh, kw, x.C, cout, stride, padding)
        self.convs.append(spec)
        y = self._temp(x, OH, OW, cout) if out is None else out
        assert (y.H, y.W, y.C) == (OH, OW, cout), (spec, y.H, y.W, y.C)
        self.ops.append((_CONV, spec, x, y))
        return y

    def maxpool(self, x, out=None):
        OH, OW = _pooled(x)
        y = self._temp(x, OH, OW, x.C) if out is None else out
        assert (y.H, y.W, y.C) == (OH, OW, x.C)
        self.ops.append((_MAXPOOL, None, x, y))
        return y

    def avgpool(self, x):
        y = self._use(_Act("tp", x.H, x.W, x.C))
        self.ops.append((_AVGPOOL, None, x, y))
        return y

    def gap(self, x):
        self.ops.append((_GAP, None, x, None))


def _network(g, x):
    """keras.applications.inception_v3.InceptionV3, include_top=False, pooling="avg": layers in creation order"""
    x = g.conv(x, 32, 3, 3, 2, "valid")
    x = g.conv(x, 32, 3, 3, 1, "valid")
    x = g.conv(x, 64, 3, 3)
    x = g.maxpool(x)
    x = g.conv(x, 80, 1, 1, 1, "valid")
    x = g.conv(x, 192, 3, 3, 1, "valid")
    x = g.maxpool(x, out=g.block_out(x, 192, *_pooled(x)))
    for pool_ch in (32, 64, 64):                   # mixed0, mixed1, mixed2: 35 x 35
        y = g.block_out(x, 224 + pool_ch)
        g.conv(x, 64, 1, 1, out=y.slice(0, 64))
        t = g.conv(x, 48, 1, 1)
        g.conv(t, 64, 5, 5, out=y.slice(64, 64))
        t = g.conv(x, 64, 1, 1)
        t = g.conv(t, 96, 3, 3)
        g.conv(t, 96, 3, 3, out=y.slice(128, 96))
        g.conv(g.avgpool(x), pool_ch, 1, 1, out=y.slice(224, pool_ch))
        x = y
    # mixed3: 17 x 17 x 768
    y = g.block_out(x, 384 + 96 + x.C, *_pooled(x))
    g.conv(x, 384, 3, 3, 2, "valid", out=y.slice(0, 384))
    t = g.conv(x, 64, 1, 1)
    t = g.conv(t, 96, 3, 3)
    g.conv(t, 96, 3, 3, 2, "valid", out=y.slice(384, 96))
    g.maxpool(x, out=y.slice(480, x.C))
    x = y
    for c in (128, 160, 160, 192):                 # mixed4 .. mixed7: 17 x 17 x 768
        y = g.block_out(x, 768)
        g.conv(x, 192, 1, 1, out=y.slice(0, 192))
        t = g.conv(x, c, 1, 1)
        t = g.conv(t, c, 1, 7)
        g.conv(t, 192, 7, 1, out=y.slice(192, 192))
        t = g.conv(x, c, 1, 1)
        t = g.conv(t, c, 7, 1)
        t = g.conv(t, c, 1, 7)
        t = g.conv(t, c, 7, 1)
        g.conv(t, 192, 1, 7, out=y.slice(384, 192))
        g.conv(g.avgpool(x), 192, 1, 1, out=y.slice(576, 192))
        x = y
    # mixed8: 8 x 8 x 1280
    y = g.block_out(x, 320 + 192 + x.C, *_pooled(x))
    t = g.conv(x, 192, 1, 1)
    g.conv(t, 320, 3, 3, 2, "valid", out=y.slice(0, 320))
    t = g.conv(x, 192, 1, 1)
    t = g.conv(t, 192, 1, 7)
    t = g.conv(t, 192, 7, 1)
    g.conv(t, 192, 3, 3, 2, "valid", out=y.slice(320, 192))
    g.maxpool(x, out=y.slice(512, x.C))
    x = y
    for _ in range(2):                             # mixed9, mixed10: 8 x 8 x 2048
        y = g.block_out(x, 2048)
        g.conv(x, 320, 1, 1, out=y.slice(0, 320))
        t = g.conv(x, 384, 1, 1)
        g.conv(t, 384, 1, 3, out=y.slice(320, 384))
        g.conv(t, 384, 3, 1, out=y.slice(704, 384))
        t = g.conv(x, 448, 1, 1)
        t = g.conv(t, 384, 3, 3)
        g.conv(t, 384, 1, 3, out=y.slice(1088, 384))
        g.conv(t, 384, 3, 1, out=y.slice(1472, 384))
        g.conv(g.avgpool(x), 192, 1, 1, out=y.slice(1856, 192))
        x = y
    g.gap(x)
    return x


def _pooled(x):
    """map size after a 3 x 3 / 2 "valid" window (max pool and the stride-2 convolutions)"""
    return (x.H - 3) // 2 + 1, (x.W - 3) // 2 + 1


def trace(H=SIZE, W=SIZE):
    g = _Trace()
    _network(g, g.input(H, W))
    return g


LAYERS = tuple(trace().convs)          # the 94 convolutions, creation order


def parameter_count():
    """kernels + beta + moving mean + moving variance: Keras' count_params() of the model"""
    return sum(s.kh * s.kw * s.cin * s.cout + 3 * s.cout for s in LAYERS)


def expected_shape(name):
    """conv/NN/<array> -> its shape"""
    _, nn, arr = name.split("/")
    s = LAYERS[int(nn)]
    return (s.kh, s.kw, s.cin, s.cout) if arr == "kernel" else (s.cout,)


def array_names():
    return [f"conv/{i:02d}/{a}" for i in range(len(LAYERS)) for a in ARRAYS]


def save_weights(path, convs, keras_names=None):
    """convs: 94 dicts {kernel, beta, moving_mean, moving_variance} in the table's order -> `path` in FORMAT"""
    out = {"format": np.array(FORMAT)}
    for i, c in enumerate(convs):
        for a in ARRAYS:
            out[f"conv/{i:02d}/{a}"] = np.asarray(c[a], np.float32)
        if keras_names is not None:
            out[f"conv/{i:02d}/keras_names"] = np.asarray(keras_names[i])
    np.savez(path, **out)
    return path


def load_weights(path):
    """-> 94 dicts {kernel, beta, moving_mean, moving_variance} (f32) after checking the format tag, that every array is present
    and every shape against the layer table; ValueError naming the array otherwise"""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files:
            raise ValueError(f"{path}: array 'format' missing (expected {FORMAT!r})")
        tag = str(z["format"])
        if tag != FORMAT:
            raise ValueError(f"{path}: array 'format' is {tag!r}, expected {FORMAT!r}")
        convs = [{} for _ in LAYERS]
        for name in array_names():
            if name not in z.files:
                raise ValueError(f"{path}: array {name!r} missing")
            v = z[name]
            if v.shape != expected_shape(name):
                raise ValueError(f"{path}: array {name!r} has shape {v.shape}, expected {expected_shape(name)}")
            convs[int(name.split("/")[1])][name.split("/")[2]] = v.astype(np.float32)
    return convs


def _view(base, a):
    """p2p_tensor of activation `a` inside the slot tensor `base` (dense images of slot_floats each)"""
    ptr = base.data_ptr() + 4 * a.coff
    return L.Tensor(ptr, a.H * a.W, a.W, a.ld)


class InceptionV3Features:
    """(N, H, W, 3) f32 preprocessed images on `device` (H = W = 299 as the reference feeds them; any size >= 75 works) ->
    (N, 2048) f32 pooled features, CHUNK images per pass.  `weights`: a FORMAT file or the list load_weights returns."""

    def __init__(self, weights, device="cuda:0", chunk=CHUNK):
        self.device = torch.device(device)
        convs = load_weights(weights) if isinstance(weights, (str, os.PathLike)) else weights
        self.chunk = int(chunk)
        self.w, self.scale, self.shift = [], [], []
        for spec, c in zip(LAYERS, convs):
            k = np.asarray(c["kernel"], np.float32)
            assert k.shape == (spec.kh, spec.kw, spec.cin, spec.cout), (spec, k.shape)
            scale = 1.0 / np.sqrt(np.asarray(c["moving_variance"], np.float64) + BN_EPS)
            shift = np.asarray(c["beta"], np.float64) - np.asarray(c["moving_mean"], np.float64) * scale
            self.w.append(torch.from_numpy(k.reshape(-1, spec.cout).copy()).to(self.device))
            self.scale.append(torch.from_numpy(scale.astype(np.float32)).to(self.device))
            self.shift.append(torch.from_numpy(shift.astype(np.float32)).to(self.device))
        self._plans = {}

    def plan(self, H, W):
        """(trace, {slot: workspace tensor}) for H x W inputs, built once per size"""
        key = (H, W)
        if key not in self._plans:
            g = trace(H, W)
            ws = {s: torch.empty(self.chunk * n, dtype=torch.float32, device=self.device) for s, n in g.slot_floats.items()}
            self._plans[key] = (g, ws)
        return self._plans[key]

    def input_buffer(self, H=SIZE, W=SIZE):
        """the workspace the first convolution reads: (chunk, H, W, 3) f32, what prep() writes"""
        g, ws = self.plan(H, W)
        return ws["in"][: self.chunk * H * W * 3].view(self.chunk, H, W, 3)

    def run_chunk(self, n, H, W, out):
        """the network over the first n images of input_buffer(H, W) -> out (n, 2048) f32 device tensor"""
        assert 0 < n <= self.chunk and out.is_contiguous() and out.shape == (n, FEATURES)
        g, ws = self.plan(H, W)
        st = torch.cuda.current_stream(self.device).cuda_stream
        for kind, spec, x, y in g.ops:
            xv = _view(ws[x.slot], x)
            if kind == _CONV:
                pt, pl = ((spec.kh - 1) // 2, (spec.kw - 1) // 2) if spec.padding == "same" else (0, 0)
                yv = _view(ws[y.slot], y)
                L.call("p2p_inc_conv", n, x.H, x.W, spec.cin, spec.kh, spec.kw, spec.stride, pt, pl, y.H, y.W, spec.cout,
                       C.byref(xv), self.w[spec.index].data_ptr(), self.scale[spec.index].data_ptr(),
                       self.shift[spec.index].data_ptr(), C.byref(yv), st)
            elif kind in (_MAXPOOL, _AVGPOOL):
                yv = _view(ws[y.slot], y)
                L.call("p2p_inc_pool", 0 if kind == _MAXPOOL else 1, n, x.H, x.W, x.C, C.byref(xv), C.byref(yv), st)
            else:
                assert x.C == FEATURES
                L.call("p2p_inc_gap", n, x.H, x.W, x.C, C.byref(xv), out.data_ptr(), st)
        return out

    def __call__(self, images):
        """images: (N, H, W, 3) f32 tensor (any device) -> (N, 2048) f32 on self.device"""
        images = torch.as_tensor(images, dtype=torch.float32)
        N, H, W, Cc = images.shape
        assert Cc == 3, images.shape
        out = torch.empty((N, FEATURES), dtype=torch.float32, device=self.device)
        buf = self.input_buffer(H, W)
        for s in range(0, N, self.chunk):
            n = min(self.chunk, N - s)
            buf[:n].copy_(images[s:s + n])
            self.run_chunk(n, H, W, out[s:s + n])
        return out
