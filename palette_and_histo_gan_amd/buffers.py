"""Where a tensor lies in HBM: haloed NHWC activation buffers, dense buffers, the flat f32 parameter / gradient / Adam stores with
their gradient buckets, the per-layer weight copies of the MFMA kernels and the variable shapes of the two networks.  PyTorch
tensors are device-memory holders here; nothing in this module depends on the schedule of a step (engine.py)."""
from collections import OrderedDict
import ctypes as C

import numpy as np
import torch

from . import _lib as L

HALO = 2
DOWN_FILTERS = (64, 128, 256, 512, 512, 512)      # networks.py:57-64
UP_FILTERS = (512, 512, 256, 128, 64, 32)         # networks.py:66-73


def _torch_dtype(dtype):
    return torch.float32 if dtype == L.F32 else torch.bfloat16


class HaloBuf:
    """NHWC activation buffer with a zero halo of HALO pixels around every image."""

    def __init__(self, n, h, w, c, dtype, device):
        self.n, self.h, self.w, self.c, self.dtype = n, h, w, c, dtype
        self.hp, self.wp = h + 2 * HALO, w + 2 * HALO
        # No kernel reads outside the pixels of a view any more (include/p2pgan.h, Conventions; round 1's wgemm tiles ran
        # past short pixels); the 256 zeroed tail elements stay as a guard band.
        numel = n * self.hp * self.wp * c
        self._flat = torch.zeros(numel + 256, dtype=_torch_dtype(dtype), device=device)
        self.t = self._flat[:numel].view(n, self.hp, self.wp, c)
        self.esz = self.t.element_size()
        self._views = {}

    def view(self, coff=0, n0=0):
        """p2p_tensor of the interior (channel offset `coff`, first image `n0`); the descriptors are cached -- a step asks for
        ~200 of them and the buffers never move"""
        v = self._views.get((coff, n0))
        if v is None:
            off = ((n0 * self.hp + HALO) * self.wp + HALO) * self.c + coff
            v = self._views[(coff, n0)] = L.Tensor(self.t.data_ptr() + off * self.esz, self.hp * self.wp, self.wp, self.c)
        return v


class DenseBuf:
    """Dense [N*H*W][C] tensor (conv raw outputs, gradient sources)."""

    def __init__(self, n, h, w, c, torch_dtype, device):
        self.n, self.h, self.w, self.c = n, h, w, c
        self.t = torch.empty((n * h * w, c), dtype=torch_dtype, device=device)
        self.esz = self.t.element_size()
        self._views = {}

    def view(self, coff=0, n0=0):
        v = self._views.get((coff, n0))
        if v is None:
            v = self._views[(coff, n0)] = L.Tensor(self.t.data_ptr() + (n0 * self.h * self.w * self.c + coff) * self.esz,
                                                   self.h * self.w, self.w, self.c)
        return v

    def ptr(self, n0=0):
        return C.c_void_p(self.t.data_ptr() + n0 * self.h * self.w * self.c * self.esz)

    def gsrc(self, coff=0, kind=1, nslabs=1, n0=0):
        return L.GSrc(self.t.data_ptr() + n0 * self.h * self.w * self.c * self.esz, kind, nslabs,
                      self.n * self.h * self.w * self.c, self.c, coff)


def pad8(c):
    """channel count padded so that a pixel is a whole number of 16-byte chunks (bf16 and f32 alike)"""
    return (c + 7) // 8 * 8


def up32(c):
    return (c + 31) // 32 * 32


def _p(t, off_elems=0):
    return C.c_void_p(t.data_ptr() + off_elems * t.element_size())


NULL = C.c_void_p(0)


class ParamStore:
    """Flat f32 parameter / gradient / Adam-moment buffers with named views.

    `shapes` keeps the Keras variable order (names, export, iteration).  The MEMORY order is chosen for the data-parallel
    all-reduce: conv kernels first, in the order their gradients complete in the backward pass (head, up6..up1,
    down6..down1), then every small tensor (gamma/beta/bias) in one tail region.  Contiguous runs of kernels form the
    gradient buckets that are all-reduced while the backward pass is still running; the tail region goes last.
    Every tensor is 16-byte aligned."""

    BUCKET_MIN = 4 * 1024 * 1024      # floats (16 MB): a bucket closes once it holds at least this much

    def __init__(self, shapes, device):
        self.shapes = OrderedDict(shapes)
        self.offsets = OrderedDict()
        kernels = [k for k in self.shapes if k.endswith(".kernel")]
        small = [k for k in self.shapes if not k.endswith(".kernel")]
        off, self.buckets, start, self.bucket_of = 0, [], 0, {}
        for k in reversed(kernels):           # backward completion order
            self.offsets[k] = off
            off += int(np.prod(self.shapes[k]))
            off = (off + 3) // 4 * 4
            self.bucket_of[k[:-7]] = len(self.buckets)
            if off - start >= self.BUCKET_MIN:
                self.buckets.append((start, off))
                start = off
        if off > start:
            self.buckets.append((start, off))
        self.bucket_last_layer = {}           # bucket index -> layer whose gradient completes it
        for k in reversed(kernels):
            self.bucket_last_layer[self.bucket_of[k[:-7]]] = k[:-7]
        self.small_range = (off, off)
        for k in small:
            self.offsets[k] = off
            off += int(np.prod(self.shapes[k]))
            off = (off + 3) // 4 * 4
        self.small_range = (self.small_range[0], off)
        self.numel = off
        self.params = torch.zeros(off, dtype=torch.float32, device=device)
        self.grads = None                     # attached by the engine (one allocation for both networks + loss slots)
        self.m = torch.zeros(off, dtype=torch.float32, device=device)
        self.v = torch.zeros(off, dtype=torch.float32, device=device)
        self.ema = None                       # moving average of params (the generator's, engine.enable_ema): same layout
        self.t = 0                           # Adam iteration count (host mirror of t_dev)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=device)       # device-resident: graph replay advances it
        self.lr_t_dev = torch.zeros(1, dtype=torch.float32, device=device)

    def count(self):
        return int(sum(int(np.prod(s)) for s in self.shapes.values()))

    def view(self, buf, name):
        o = self.offsets[name]
        return buf[o:o + int(np.prod(self.shapes[name]))].view(self.shapes[name])

    def p(self, name):
        return _p(self.params, self.offsets[name])

    def g(self, name):
        return _p(self.grads, self.offsets[name])

    def variable_name(self, t):
        """name of the variable whose view `t` is (an entry of trainable_variables), or None"""
        if not isinstance(t, torch.Tensor) or t.device != self.params.device or t.dtype != torch.float32:
            return None
        off = t.data_ptr() - self.params.data_ptr()
        if off < 0 or off % 4 or off >= 4 * self.numel:
            return None
        if getattr(self, "_by_offset", None) is None:
            self._by_offset = {o: k for k, o in self.offsets.items()}
        name = self._by_offset.get(off // 4)
        return name if name is not None and tuple(t.shape) == tuple(self.shapes[name]) else None

    def load(self, values):
        for k in self.shapes:
            self.view(self.params, k).copy_(torch.as_tensor(np.asarray(values[k]), dtype=torch.float32))

    def export(self, buf=None):
        buf = self.params if buf is None else buf
        return OrderedDict((k, self.view(buf, k).detach().cpu().numpy().copy()) for k in self.shapes)


def generator_param_shapes(in_ch, out_ch):
    """Variable order / shapes of UnetGenerator (networks.py:53-98); conv kernels keep the Keras layouts
    HWIO (Conv2D) and (kh,kw,Cout,Cin) (Conv2DTranspose) == [tap][Cg][Cd] in both cases."""
    shapes = OrderedDict()
    c = in_ch
    for i, f in enumerate(DOWN_FILTERS, start=1):
        shapes[f"down{i}.kernel"] = (4, 4, c, f)
        if i > 1:
            shapes[f"down{i}.gamma"] = (f,)
            shapes[f"down{i}.beta"] = (f,)
        c = f
    skips = list(reversed(DOWN_FILTERS[:-1])) + [in_ch]
    for i, (f, s) in enumerate(zip(UP_FILTERS, skips), start=1):
        shapes[f"up{i}.kernel"] = (4, 4, f, c)
        shapes[f"up{i}.gamma"] = (f,)
        shapes[f"up{i}.beta"] = (f,)
        c = f + s
    shapes["last.kernel"] = (4, 4, c, out_ch)
    shapes["last.bias"] = (out_ch,)
    return shapes


def discriminator_param_shapes(in_ch):
    """PatchDiscriminator variables (networks.py:39-50)."""
    return OrderedDict([("down.kernel", (4, 4, 2 * in_ch, 64)), ("last.kernel", (4, 4, 64, 1)), ("last.bias", (1,))])


class LayerW:
    """Per-layer weight copies in the activation dtype, derived from the f32 master W[16][Cg][Cd] after every
    Adam step (p2p_weight_prep_pad):
      wt [16][up32(Cd)][hi_pad]  B operand of op G (conv forward / convT dgrad), contraction over the gathered
                                 hi view whose pixels hold hi_pad channels in HBM;
      wn [16][up32(Cg)][lo_pad]  B operand of op P (convT forward / conv dgrad), contraction over the lo view;
      wd [16][Cg][Cd]            unpadded copy, only for the direct (non-MFMA) cross-check kernels.
    Rows/columns beyond the real [Cg][Cd] block are zero."""

    def __init__(self, cg, cd, hi_pad, lo_pad, need_g, need_p):
        self.cg, self.cd, self.hi_pad, self.lo_pad = cg, cd, hi_pad, lo_pad
        self.need_g, self.need_p = need_g, need_p
        self.wt = self.wn = self.wd = None
        self.main = cg % 32 == 0 and cd % 32 == 0 and hi_pad == cg and lo_pad == cd
