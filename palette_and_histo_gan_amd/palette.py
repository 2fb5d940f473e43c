"""Soft palette histogram and palette conformance of RGBA images (build-added: the reference's histogram.py only has the RGB-uv
histogram; DESIGN.md "palette loss" holds the definitions).

`extract_palette_batch` finds every image's palette on the device (p2p_palette_extract), `soft_palette_histogram` measures how an
image's pixels distribute over a palette's slots and how far they sit from them (p2p_soft_palette_fwd) and is differentiable with
respect to the image: one torch.autograd.Function whose backward is HIP as well (p2p_soft_palette_bwd), so a loss hook of
engine.train_step_rgba_hooked or a tf.GradientTape step written with it reaches the generator.  `palette_histogram_loss` is a
handful of torch ops on the (B, K) result.  (Pix2PixPaletteModel(fused=True) does not come through here: the fused step launches the
same kernels plus p2p_palette_loss and p2p_soft_palette_tv_bwd from engine._palette_loss)  `snap_to_palette` is the hard counterpart (p2p_palette_snap: every pixel's nearest
palette colour in exact integer arithmetic, per-slot counts, off-palette pixels), not differentiable, for inference
(Pix2PixModel.generate(snap=)) and evaluation (`palette_metrics`, S2SModel.report_palette).  `project_to_palette` stands between the two: it replaces every pixel by a
palette colour -- the soft expected colour or the snap itself -- and IS differentiable (p2p_palette_project_fwd / _bwd: the exact
Jacobian of the soft projection, or the straight-through identity), so a tape step can show the discriminator what survives the snap
(Pix2PixPaletteSnapModel).  `palette_lookup` serves the palette-index model instead: it maps (B, H, W, 256)
probabilities over a palette's slots to the RGBA image they stand for (p2p_palette_lookup_fwd / _bwd: the expected colour, or the
argmax's colour with the straight-through gradient), so image-space losses reach the indexed generator (Pix2PixIndexedColourModel;
DESIGN.md 6g).  `quantize_palette` / `quantize` need no palette from elsewhere: they derive one of at most K colours from the image itself
(p2p_palette_quantize: farthest-point starting slots and Lloyd passes in exact integer arithmetic) and snap to it --
the last step of inference (Pix2PixModel.generate(snap=K), S2SModel.report_quantized).  All kernels launch on the current stream;
there is no CPU path.

The default temperature 1e-3 makes a pixel that sits on a palette colour count for that slot alone (two colours one 8-bit step apart
in one channel are 1.5e-5 apart in d, a weight ratio of 0.985; a pixel half-way between two clearly different colours is shared).
It is a design choice: on synthetic pairs neither 1e-3 nor 5e-2 changed the trained model's L1 or its share of off-palette
pixels by a resolved amount at lambda_palette = 1 (tools/quality_run.py --palette).
"""
import collections
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .configuration import MAX_PALETTE_SIZE


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _device_of(x, device):
    if device is not None:
        return torch.device(device)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device("cuda:0")


def _rgba(image_batch, dev):
    """the kernels' input: a dense f32 (B, H, W, 4) device tensor (the conversion stays on the autograd graph)"""
    img = torch.as_tensor(image_batch).to(device=dev, dtype=torch.float32).contiguous()
    if img.dim() != 4 or img.shape[3] != 4 or img.numel() == 0:
        raise ValueError(f"expected a non-empty (B, H, W, 4) RGBA batch, got {tuple(img.shape)}")
    return img


def extract_palette_batch(images, check=True, device=None):
    """Palettes of a (B, H, W, 4) batch in [-1, 1]: (palette int32 (B, 256, 4), sizes int32 (B,)) on the device.  Row b lists the
    image's distinct 8-bit RGBA colours, clamp(floor((img * 0.5 + 0.5) * 255 + 0.5), 0, 255), in ascending order of
    r + 256 g + 65536 b + 2^24 a -- transparent black first, as in the indexed pipeline -- followed by zero rows.  An image with
    more than MAX_PALETTE_SIZE colours gets size -1 and a zeroed row; with `check` the sizes are read back (a host sync) and such
    an image raises ValueError, without it nothing waits for the device."""
    L.lib()
    dev = _device_of(images, device)
    img = _rgba(images, dev).detach()
    B, H, W, _ = (int(x) for x in img.shape)
    palette = torch.empty((B, MAX_PALETTE_SIZE, 4), dtype=torch.int32, device=dev)
    sizes = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("p2p_palette_extract", B, H, W, _p(img), MAX_PALETTE_SIZE, _p(palette), _p(sizes), _stream(dev))
    if check:
        over = torch.nonzero(sizes < 0).flatten().tolist()
        if over:
            raise ValueError(f"image {over[0]} of the batch has more than {MAX_PALETTE_SIZE} distinct RGBA colours "
                             f"({len(over)} of {B} images do)")
    return palette, sizes


class SoftPaletteHistogram(torch.autograd.Function):
    """img: dense f32 (B, H, W, 4) device tensor; palette int32 (B, K, 4), sizes int32 (B,), both dense on img's device ->
    (hist (B, K), conformance (B,)).  Backward: the gradient with respect to img only; single backward."""

    @staticmethod
    def forward(ctx, img, palette, sizes, tau):
        B, H, W, _ = (int(x) for x in img.shape)
        K = int(palette.shape[1])
        dev = img.device
        hist = torch.empty((B, K), dtype=torch.float32, device=dev)
        conf = torch.empty((B,), dtype=torch.float32, device=dev)
        ws = torch.empty(max(int(L.lib().p2p_soft_palette_workspace_bytes(B, H, W)) // 4, 1), dtype=torch.float32, device=dev)
        L.call("p2p_soft_palette_fwd", B, H, W, _p(img), _p(palette), _p(sizes), K, tau, _p(hist), _p(conf), _p(ws), _stream(dev))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(img, palette, sizes)
            ctx.tau = tau
        return hist, conf

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_hist, grad_conf):
        img, palette, sizes = ctx.saved_tensors
        B, H, W, _ = (int(x) for x in img.shape)
        K = int(palette.shape[1])
        dev = img.device
        zeros = lambda g, shape: torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.to(torch.float32).contiguous()  # noqa: E731
        gh, gm = zeros(grad_hist, (B, K)), zeros(grad_conf, (B,))
        dimg = torch.empty_like(img)
        with torch.cuda.device(dev):
            L.call("p2p_soft_palette_bwd", B, H, W, _p(img), _p(palette), _p(sizes), K, ctx.tau, _p(gh), _p(gm), _p(dimg), _stream(dev))
        return dimg, None, None, None


def _checked_palette(palette, B):
    pal = torch.as_tensor(palette)
    if pal.dim() != 3 or pal.shape[0] != B or pal.shape[2] != 4 or not 1 <= pal.shape[1] <= MAX_PALETTE_SIZE:
        raise ValueError(f"expected a ({B}, K <= {MAX_PALETTE_SIZE}, 4) palette for a batch of {B}, got {tuple(pal.shape)}")
    return pal


def _palette_args(pal, sizes, B, dev):
    """the kernels' palette (B, K, 4) and sizes (B,) as dense int32 device tensors, from a checked palette"""
    pal = pal.detach().to(device=dev, dtype=torch.int32).contiguous()
    if sizes is None:
        sz = torch.full((B,), int(pal.shape[1]), dtype=torch.int32, device=dev)
    else:
        sz = torch.as_tensor(sizes)
        if tuple(sz.shape) != (B,):
            raise ValueError(f"expected {B} palette sizes, got shape {tuple(sz.shape)}")
        sz = sz.detach().to(device=dev, dtype=torch.int32).contiguous()
    return pal, sz


def soft_palette_histogram(image_batch, palette, sizes=None, temperature=1e-3, device=None):
    """(hist (B, K), conformance (B,)) of a (B, H, W, 4) batch in [-1, 1] under per-image palettes (B, K, 4) of 0..255 RGBA rows,
    K <= 256, of which the first sizes[b] are valid (None: all K).  With x = img * 0.5 + 0.5, c_k = palette_k / 255 and
    d_pk = |x_p - c_k|^2 over the four channels, w_pk = softmax_k(-(d_pk - min_j d_pj) / temperature):
        hist[b, k] = mean_p w_pk (0 for k >= sizes[b]; a row sums to 1),   conformance[b] = mean_p sum_k w_pk d_pk.
    An image with sizes[b] <= 0 (extract_palette_batch's -1 included) contributes zeros and a zero gradient; a size above K counts
    as K.  Differentiable with respect to `image_batch` only (the gradient has its shape, dtype and device)."""
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    dev = _device_of(image_batch, device)
    img = _rgba(image_batch, dev)
    B = int(img.shape[0])
    pal = _checked_palette(palette, B)
    temperature = float(temperature)
    if not 0.0 < temperature < float("inf"):
        raise ValueError(f"the temperature must be positive and finite, got {temperature}")
    pal, sz = _palette_args(pal, sizes, B, dev)
    with torch.cuda.device(dev):
        return SoftPaletteHistogram.apply(img, pal, sz, temperature)


def _checked_temperature(temperature):
    temperature = float(temperature)
    if not 0.0 < temperature < float("inf"):
        raise ValueError(f"the temperature must be positive and finite, got {temperature}")
    return temperature


def check_projection_mode(hard, gradient):
    """the (forward, backward) pairs project_to_palette accepts"""
    if gradient not in ("soft", "identity"):
        raise ValueError(f'gradient is "soft" or "identity", got {gradient!r}')
    if not hard and gradient == "identity":
        raise ValueError('hard=False with gradient="identity": the soft forward has an exact gradient (gradient="soft"); the '
                         'straight-through identity belongs to the hard forward')


class PaletteProjection(torch.autograd.Function):
    """img: dense f32 (B, H, W, 4) device tensor; palette int32 (B, K, 4), sizes int32 (B,), both dense on img's device ->
    projected image (B, H, W, 4).  Backward: with respect to img only, single backward; with `soft_gradient` the VJP of the soft
    projection at img (p2p_palette_project_bwd), without it the upstream gradient itself: nothing saved, nothing launched."""

    @staticmethod
    def forward(ctx, img, palette, sizes, tau, hard, soft_gradient):
        B, H, W, _ = (int(x) for x in img.shape)
        K = int(palette.shape[1])
        out = torch.empty_like(img)
        L.call("p2p_palette_project_fwd", B, H, W, _p(img), _p(palette), _p(sizes), K, tau, int(hard), _p(out), _stream(img.device))
        ctx.soft_gradient = soft_gradient
        if soft_gradient and ctx.needs_input_grad[0]:
            ctx.save_for_backward(img, palette, sizes)
            ctx.tau = tau
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if not ctx.soft_gradient:
            return grad_out, None, None, None, None, None
        img, palette, sizes = ctx.saved_tensors
        B, H, W, _ = (int(x) for x in img.shape)
        K = int(palette.shape[1])
        dev = img.device
        g = grad_out.to(torch.float32).contiguous()
        dimg = torch.empty_like(img)
        with torch.cuda.device(dev):
            L.call("p2p_palette_project_bwd", B, H, W, _p(img), _p(palette), _p(sizes), K, ctx.tau, _p(g), _p(dimg), _stream(dev))
        return dimg, None, None, None, None, None


def project_to_palette(image_batch, palette, sizes=None, temperature=5e-2, hard=False, gradient="soft", device=None):
    """A (B, H, W, 4) batch in [-1, 1] with every pixel replaced by a colour of its image's palette (B, K <= 256, 4) of 0..255 RGBA
    rows, of which the first sizes[b] are valid (None: all K); f32, differentiable with respect to `image_batch` only.
    With w_pk the weights of soft_palette_histogram at `temperature` and c_k = palette_k / 255:
        hard=False   y_p = 2 sum_k w_pk c_k - 1: the expected palette colour, alpha included
        hard=True    y_p = snap_to_palette(image_batch, palette, sizes).image_p, bit for bit
        gradient="soft"       dL/dimg_p = (2 / temperature) Cov_w(c) dL/dy_p, the exact Jacobian of the soft projection at the raw
                              image -- for hard=True a surrogate: the snap's own gradient is 0 almost everywhere
        gradient="identity"   dL/dimg = dL/dy (straight-through; hard=True only; nothing is saved or launched in backward)
    An image with sizes[b] <= 0 (extract_palette_batch's -1 included) passes through: its pixels and its gradient are copied.
    The default temperature 5e-2 is the soft histogram's coarse setting: at 1e-3 the soft gradient vanishes at every pixel that is
    not within ~0.03 of the midway plane between two colours."""
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    check_projection_mode(hard, gradient)
    dev = _device_of(image_batch, device)
    img = _rgba(image_batch, dev)
    B = int(img.shape[0])
    pal = _checked_palette(palette, B)
    temperature = _checked_temperature(temperature)
    pal, sz = _palette_args(pal, sizes, B, dev)
    with torch.cuda.device(dev):
        return PaletteProjection.apply(img, pal, sz, temperature, bool(hard), gradient == "soft")


class PaletteLookup(torch.autograd.Function):
    """probs: dense f32 (B, H, W, 256) device tensor; palette int32 (B, 256, 4) dense on its device -> RGBA image (B, H, W, 4).
    Backward: with respect to probs only, single backward (p2p_palette_lookup_bwd: the soft map's VJP for both forwards); only the
    palette is saved."""

    @staticmethod
    def forward(ctx, probs, palette, hard, blacken):
        B, H, W, K = (int(x) for x in probs.shape)
        out = torch.empty((B, H, W, 4), dtype=torch.float32, device=probs.device)
        L.call("p2p_palette_lookup_fwd", B, H, W, K, _p(probs), _p(palette), int(hard), int(blacken), _p(out), _stream(probs.device))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(palette)
            ctx.blacken = blacken
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        palette, = ctx.saved_tensors
        B, H, W, _ = (int(x) for x in grad_out.shape)
        K = int(palette.shape[1])
        dev = palette.device
        g = grad_out.to(torch.float32).contiguous()
        dprobs = torch.empty((B, H, W, K), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.call("p2p_palette_lookup_bwd", B, H, W, K, _p(g), _p(palette), int(ctx.blacken), _p(dprobs), _stream(dev))
        return dprobs, None, None, None


def palette_lookup(probs, palette, hard=False, blacken=False, device=None):
    """The RGBA image (B, H, W, 4), f32 in [-1, 1], of per-pixel probabilities (B, H, W, 256) over the slots of per-image palettes
    (B, 256, 4) of 0..255 RGBA rows -- what Pix2PixIndexedModel's generator puts out, seen as an image.  With
    t_k = palette_k / 127.5 - 1 (the dataset's normalisation):
        hard=False   y_p = sum_k probs_pk t_k: the expected colour; linear, a one-hot row returns t_k bit for bit
        hard=True    y_p = t_argmax_k probs_pk (ties: the lowest k): io_utils.indexed_to_rgba of the argmax, normalised
        blacken      the RGB of a slot whose alpha is 0 counts as 0, as dataset_utils.blacken_transparent_pixels leaves an image
    Differentiable with respect to `probs` only (the gradient has its shape, dtype and device): dL/dprobs_pk = <dL/dy_p, t_k> for both
    forwards -- for hard=True the straight-through surrogate, the argmax's own gradient being 0 almost everywhere.  Integer indices
    (B, H, W, 1) are not probabilities: io_utils.indexed_to_rgba maps those."""
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    dev = _device_of(probs, device)
    p = torch.as_tensor(probs)
    if p.dim() != 4 or p.shape[3] != MAX_PALETTE_SIZE or p.numel() == 0:
        raise ValueError(f"expected non-empty (B, H, W, {MAX_PALETTE_SIZE}) probabilities, got {tuple(p.shape)}"
                         + (": integer indices are mapped by io_utils.indexed_to_rgba" if p.dim() == 4 and p.shape[3] == 1 else ""))
    B = int(p.shape[0])
    pal = torch.as_tensor(palette)
    if tuple(pal.shape) != (B, MAX_PALETTE_SIZE, 4):
        raise ValueError(f"expected a ({B}, {MAX_PALETTE_SIZE}, 4) palette for a batch of {B}, got {tuple(pal.shape)}")
    p = p.to(device=dev, dtype=torch.float32).contiguous()          # stays on the autograd graph
    pal = pal.detach().to(device=dev, dtype=torch.int32).contiguous()
    with torch.cuda.device(dev):
        return PaletteLookup.apply(p, pal, bool(hard), bool(blacken))


PaletteSnap = collections.namedtuple("PaletteSnap", "index image distance counts off_palette distance_sum")


def snap_to_palette(image_batch, palette, sizes=None, device=None):
    """Every pixel of a (B, H, W, 4) batch in [-1, 1] moved to the nearest colour of its image's palette (B, K <= 256, 4) of 0..255
    RGBA rows, of which the first sizes[b] are valid (None: all K) -- the hard counterpart of soft_palette_histogram, in exact
    integer arithmetic (p2p_palette_snap, DESIGN.md "palette snap").  With q_p the pixel quantised as extract_palette_batch
    quantises it and D_pk = sum_c (q_pc - palette_kc)^2, returns PaletteSnap of device tensors:
        index (B, H, W) int32         argmin_k D_pk, ties to the lowest k
        image (B, H, W, 4) float32    palette[index] / 127.5 - 1 (the dataset's normalisation: snapping twice changes nothing)
        distance (B, H, W) int32      D at the index, 0..260100
        counts (B, K) int32           pixels per slot, 0 for k >= sizes[b]
        off_palette (B,) int64        pixels with distance > 0
        distance_sum (B,) int64       sum of distance
    An image with sizes[b] <= 0 (extract_palette_batch's -1 included) has nothing to snap to: index -1, distance 0, its pixels
    copied, zero counts and sums.  NOT differentiable: an argmin has no gradient; all outputs are detached."""
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    dev = _device_of(image_batch, device)
    img = _rgba(image_batch, dev).detach()
    B, H, W, _ = (int(x) for x in img.shape)
    pal, sz = _palette_args(_checked_palette(palette, B), sizes, B, dev)
    K = int(pal.shape[1])
    index = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    image = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
    distance = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((B, K), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.call("p2p_palette_snap", B, H, W, _p(img), _p(pal), _p(sz), K, _p(index), _p(image), _p(distance), _p(counts), _p(stats),
               _stream(dev))
    return PaletteSnap(index, image, distance, counts, stats[:, 0], stats[:, 1])


MAX_QUANTIZE_PIXELS = 1 << 14          # p2p_palette_quantize keeps an image's keys in LDS: 128 x 128 at most
MAX_QUANTIZE_ITERATIONS = 64


def _checked_quantize_args(images, colours, iterations, init):
    """everything quantize_palette can refuse without a device: raises ValueError"""
    if isinstance(colours, bool) or not isinstance(colours, int) or not 1 <= colours <= MAX_PALETTE_SIZE:
        raise ValueError(f"colours is an int in 1..{MAX_PALETTE_SIZE}, got {colours!r}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= MAX_QUANTIZE_ITERATIONS:
        raise ValueError(f"iterations is an int in 0..{MAX_QUANTIZE_ITERATIONS}, got {iterations!r}")
    shape = tuple(int(x) for x in (images if hasattr(images, "shape") else torch.as_tensor(images)).shape)
    if len(shape) != 4 or shape[3] != 4 or 0 in shape:
        raise ValueError(f"expected a non-empty (B, H, W, 4) RGBA batch, got {shape}")
    if shape[1] * shape[2] > MAX_QUANTIZE_PIXELS:
        raise ValueError(f"{shape[1]} x {shape[2]} pixels: quantize_palette takes images of at most {MAX_QUANTIZE_PIXELS} pixels (128 x 128)")
    if init is None:
        return None
    try:
        pal, sizes = init
    except (TypeError, ValueError):
        raise ValueError("init is None or a (palette (B, K, 4), sizes (B,) or None) pair") from None
    pal = _checked_palette(pal, shape[0])
    if sizes is not None and tuple(torch.as_tensor(sizes).shape) != (shape[0],):
        raise ValueError(f"expected {shape[0]} palette sizes, got shape {tuple(torch.as_tensor(sizes).shape)}")
    return pal, sizes


def quantize_palette(images, colours=16, iterations=8, init=None, device=None):
    """A palette of at most `colours` colours for every image of a (B, H, W, 4) batch in [-1, 1], derived from the image itself
    (p2p_palette_quantize): (palette int32 (B, 256, 4), sizes int32 (B,)) on the device, in extract_palette_batch's
    format -- sizes[b] distinct 0..255 RGBA rows in ascending order of r + 256 g + 65536 b + 2^24 a, then zero rows.  An image with
    at most `colours` distinct 8-bit colours gets exactly those.  Otherwise an integer k-means: `colours` starting slots by
    farthest-point selection from the image's lowest key (or the first min(sizes, colours) rows of `init`, a (palette (B, K <= 256,
    4), sizes (B,) or None) pair as generate(snap=) takes it; an image whose size is <= 0 starts from the farthest points), then up
    to `iterations` (0..64) Lloyd passes with snap_to_palette's nearest-slot rule and centroids rounded half up, stopping at a fixed
    point.  Rounded centroids can coincide: sizes[b] <= colours.  Exact integer arithmetic: the result depends only on the image's
    multiset of quantised colours.  H * W <= 2^14 (128 x 128).  NOT differentiable; no host sync."""
    checked = _checked_quantize_args(images, colours, iterations, init)
    L.lib()          # fail loudly if the HIP library is missing: there is no CPU path
    dev = _device_of(images, device)
    img = _rgba(images, dev).detach()
    B, H, W, _ = (int(x) for x in img.shape)
    K = MAX_PALETTE_SIZE
    palette = torch.empty((B, K, 4), dtype=torch.int32, device=dev)
    sizes = torch.empty((B,), dtype=torch.int32, device=dev)
    init_pal = init_sz = C.c_void_p(0)
    if checked is not None:
        pal, sz = _palette_args(checked[0], checked[1], B, dev)
        padded = torch.zeros((B, K, 4), dtype=torch.int32, device=dev)
        padded[:, :pal.shape[1]] = pal
        sz = sz.clamp(max=int(pal.shape[1]))          # rows past the given K are padding, not slots
        init_pal, init_sz = _p(padded), _p(sz)
    with torch.cuda.device(dev):
        L.call("p2p_palette_quantize", B, H, W, _p(img), colours, iterations, init_pal, init_sz, K, _p(palette), _p(sizes), C.c_void_p(0),
               _stream(dev))
    return palette, sizes


def quantize(images, colours=16, iterations=8, init=None, device=None):
    """quantize_palette followed by snap_to_palette: (PaletteSnap, palette, sizes).  PaletteSnap.image is the batch with every image
    reduced to at most `colours` colours of its own (an image that had no more keeps its colours bit for bit after 8-bit rounding),
    .index with the palette is the indexed form (io_utils.indexed_to_rgba, PNG), .distance_sum the quantisation error."""
    dev = _device_of(images, device)
    palette, sizes = quantize_palette(images, colours, iterations, init, device=dev)
    return snap_to_palette(images, palette, sizes, device=dev), palette, sizes


def palette_metrics(fake_images, real_images, device=None):
    """How far a generated batch strays from the palette of its target batch (both (B, H, W, 4) in [-1, 1]).  The palette of every
    real image is extracted on the device (no host sync) and both batches are snapped to it.  A dict of (B,) device tensors:
        off_palette    share of the fake image's pixels that are not a palette colour (distance > 0)
        rms_distance   sqrt(distance_sum / (HW * 4)) / 255: the fake pixels' RMS channel distance to their nearest colour, in [0, 1]
        histogram_tv   0.5 sum_k |counts_fake - counts_real| / HW: total variation between the two images' use of the palette
        valid          bool, False for a real image with more than MAX_PALETTE_SIZE colours (its other entries are 0 and NaN-free)
    Leave the images that are not `valid` out of any mean."""
    dev = _device_of(fake_images, device)
    real = _rgba(real_images, dev).detach()
    fake = _rgba(fake_images, dev).detach()
    if fake.shape != real.shape:
        raise ValueError(f"expected two batches of one shape, got {tuple(fake.shape)} and {tuple(real.shape)}")
    palette, sizes = extract_palette_batch(real, check=False, device=dev)
    f, r = snap_to_palette(fake, palette, sizes, device=dev), snap_to_palette(real, palette, sizes, device=dev)
    hw = float(real.shape[1] * real.shape[2])
    return {"off_palette": f.off_palette.to(torch.float32) / hw,
            "rms_distance": (torch.sqrt(f.distance_sum.to(torch.float64) / (hw * 4.0)) / 255.0).to(torch.float32),      # rounded to f32 once
            "histogram_tv": 0.5 * (f.counts - r.counts).abs().sum(-1).to(torch.float32) / hw,
            "valid": sizes > 0}


def palette_histogram_loss(h_true, h_pred):
    """Total variation between palette histograms, batch mean of 0.5 sum_k |h_pred - h_true|: 0 for equal rows, 1 for rows on
    disjoint slots.  (Not the Hellinger distance of the RGB-uv histogram: slots without mass are the rule here, and sqrt has no
    finite gradient at 0.)"""
    h_pred = torch.as_tensor(h_pred)
    h_true = torch.as_tensor(h_true).to(device=h_pred.device, dtype=h_pred.dtype)
    return 0.5 * (h_pred - h_true).abs().sum(-1).mean()
