"""Launch harvest and float64 references for tests/test_step_launches_gpu.py.

The host half (the references) needs no GPU: tests/test_step_launches_cpu.py checks it against oracle/reference_graph.py.

Convolutions are written in the tap form of include/p2pgan.h:
  op G: lo[n,y,x,d]  = sum_{kh,kw,g} hi[n, s*y+kh-1, s*x+kw-1, g] W[kh,kw,g,d]
  op P: hi[n,Y,X,g] += lo[n,y,x,d] W[kh,kw,g,d]      at Y = s*y+kh-1, X = s*x+kw-1
  op W: dW[kh,kw,g,d] = sum_{n,y,x} hi[n, s*y+kh-1, s*x+kw-1, g] lo[n,y,x,d]
with a zero border of 1 pixel before and 2 after (TF SAME for k=4: (1,1) at stride 2, (1,2) at stride 1).
"""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from palette_and_histo_gan_amd import _lib as L

F64 = torch.float64
# a launch's output in the activation dtype against f64: max |error| / max |reference| per image (test_kernels_gpu.py)
OUT_TOL = {L.F32: 2e-5, L.BF16: 6e-3}
CHUNK = 16          # images per im2col chunk of the whole-batch weight gradient


def _padded(hi):
    """hi [n,H,W,g] (f64 tensor) -> zero border 1 before / 2 after"""
    return torch.nn.functional.pad(hi, (0, 0, 1, 2, 1, 2))


def conv_g(hi, w, stride):
    """op G in float64: hi [n, s*LH, s*LW, Cg], w [4,4,Cg,Cd] -> [n, LH, LW, Cd]"""
    hi, w = torch.as_tensor(hi, dtype=F64), torch.as_tensor(w, dtype=F64)
    n, H, W_, _ = hi.shape
    lh, lw = H // stride, W_ // stride
    hp = _padded(hi)
    out = torch.zeros((n, lh, lw, w.shape[3]), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            out += hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :] @ w[kh, kw]
    return out.numpy()


def conv_p(lo, w, stride):
    """op P in float64: lo [n, LH, LW, Cd], w [4,4,Cg,Cd] -> [n, s*LH, s*LW, Cg]"""
    lo, w = torch.as_tensor(lo, dtype=F64), torch.as_tensor(w, dtype=F64)
    n, lh, lw, _ = lo.shape
    hp = torch.zeros((n, stride * lh + 3, stride * lw + 3, w.shape[2]), dtype=F64)
    for kh in range(4):
        for kw in range(4):
            hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :] += lo @ w[kh, kw].T
    return hp[:, 1:1 + stride * lh, 1:1 + stride * lw, :].numpy()


def conv_w(hi, lo, stride):
    """op W in float64 over the whole batch, CHUNK images at a time (im2col of one tap x f64 GEMM):
    hi [n, s*LH, s*LW, Cg], lo [n, LH, LW, Cd] -> dW [4,4,Cg,Cd]"""
    n, lh, lw, cd = lo.shape
    cg = hi.shape[3]
    dw = torch.zeros((4, 4, cg, cd), dtype=F64)
    for a in range(0, n, CHUNK):
        hp = _padded(torch.as_tensor(hi[a:a + CHUNK], dtype=F64))
        lo_c = torch.as_tensor(lo[a:a + CHUNK], dtype=F64).reshape(-1, cd)
        for kh in range(4):
            for kw in range(4):
                cols = hp[:, kh:kh + stride * lh:stride, kw:kw + stride * lw:stride, :].reshape(-1, cg)
                dw[kh, kw] += cols.T @ lo_c
    return dw.numpy()


def act(x, kind, alpha):
    """kind 0 none, 1 LeakyReLU(alpha), 2 ReLU (p2p_act)"""
    if kind == 1:
        return np.where(x > 0, x, alpha * x)
    if kind == 2:
        return np.maximum(x, 0.0)
    return x


def norm_act(x, gamma, beta, eps, kind, alpha, mask=None):
    """y = act(drop(gamma * (x - mean) / sqrt(var + eps) + beta)) per (image, channel); x [n,H,W,C] (f64); gamma/beta may be None
    (no normalisation); mask 0/1 keeps and scales by 2 (keras Dropout(0.5))"""
    x = np.asarray(x, np.float64)
    if gamma is not None:
        mu = x.mean(axis=(1, 2), keepdims=True)
        var = ((x - mu) ** 2).mean(axis=(1, 2), keepdims=True)
        x = (x - mu) / np.sqrt(var + eps) * gamma + beta
    if mask is not None:
        x = x * mask * 2.0
    return act(x, kind, alpha)


def pooled_moments(sp, cnt):
    """slot partials [n, slots, C, 2] = (mean, centred sum of squares) of cnt pixels each -> per (image, channel) mean and variance
    (parallel-variance rule)"""
    sp = np.asarray(sp, np.float64)
    mean = sp[..., 0].mean(axis=1)
    m2 = sp[..., 1].sum(axis=1) + cnt * ((sp[..., 0] - mean[:, None, :]) ** 2).sum(axis=1)
    return mean, m2 / (cnt * sp.shape[1])


def image_set(n, seed=0, extra=4):
    """Images whose per-image outputs are compared in full: the first and last, both sides of every power-of-two boundary from
    either end (tile / workgroup groupings of 1, 2, 4 ... images, and tiles of 256 rows that span 256 / (H*W) images), and a few
    seeded random ones."""
    s = {0, n - 1}
    t = 1
    while t < n:
        s.update({t - 1, t, n - 1 - t, n - t})
        t *= 2
    rng = np.random.default_rng(seed)
    s.update(int(i) for i in rng.integers(0, n, size=extra))
    return sorted(i for i in s if 0 <= i < n)


def per_image_err(got, ref):
    """max over images of max|got - ref| / max|ref| within the image"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    axes = tuple(range(1, got.ndim))
    return float((np.abs(got - ref).max(axis=axes) / (np.abs(ref).max(axis=axes) + 1e-30)).max())


def per_image_channel_err(got, ref, scale=None):
    """max over (image, channel) of max|got - ref| / max|scale| within the (image, channel) plane, [n,H,W,C].  scale defaults to
    ref; a normalised output passes the value in front of its activation and dropout (a plane that ReLU and dropout leave nearly
    empty is measured against what the kernel computed, not against its few surviving small values)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref if scale is None else np.asarray(scale, np.float64))
    return float((np.abs(got - ref).max(axis=(1, 2)) / (scale.max(axis=(1, 2)) + 1e-30)).max())


def moment_err(mean, var, x, eps=0.0):
    """per (image, channel) moments [n, C] against those of x [n,H,W,C] in float64: max of |mean error| / standard deviation and
    |variance error| / (variance + eps) / 5"""
    x = np.asarray(x, np.float64)
    m, v = x.mean(axis=(1, 2)), x.var(axis=(1, 2))
    e_mean = np.abs(np.asarray(mean, np.float64) - m) / np.sqrt(v + eps)
    e_var = np.abs(np.asarray(var, np.float64) - v) / (v + eps) / 5
    return float(max(e_mean.max(), e_var.max()))


def per_tap_err(got, ref):
    """weight gradient [4,4,Cg,Cd]: max over taps of max|got - ref| / max|ref| within the tap"""
    got, ref = np.asarray(got, np.float64).reshape(16, -1), np.asarray(ref, np.float64).reshape(16, -1)
    return float((np.abs(got - ref).max(axis=1) / (np.abs(ref).max(axis=1) + 1e-30)).max())


# ---------------------------------------------------------------------------------------------------------------- step plumbing
def keras_adam(p, g, m, v, t, lr, b1, b2, eps):
    """one Keras (OptimizerV2) Adam step in float64, t = iteration count after the increment (pix2pix_model.py:28-29): returns
    (p, m, v).  eps is added to sqrt(v) outside the bias correction, which lives in the step size lr_t.  The arrays are float64
    numpy arrays or torch tensors (the GPU test evaluates the whole flat buffers on the device)."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return p - lr_t * m / (v ** 0.5 + eps), m, v


def bf16_round(x):
    """float32 values rounded to the nearest bfloat16, ties to even (what the kernels' from_f32 and torch's cast do), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


_M64 = (1 << 64) - 1


def dropout_mask(n, seed, counter, group0=0):
    """the keep mask of p2p_dropout_mask(_dev) (optim.hip dropout_mask_kernel): element 8*i+k is bit 8*k+3 of
    z = splitmix64(seed * 0x9E3779B97F4A7C15 + counter * 0xD1B54A32D192ED03 + (i + group0)), with the generator's increment
    0x9E3779B97F4A7C15 added before the finaliser; counter = counter_dev * 16 + salt for the device form.  uint8 [n]."""
    base = (int(seed) * 0x9E3779B97F4A7C15 + int(counter) * 0xD1B54A32D192ED03 + int(group0) + 0x9E3779B97F4A7C15) & _M64
    with np.errstate(over="ignore"):
        z = np.uint64(base) + np.arange((n + 7) // 8, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    bits = (z[:, None] >> (np.arange(8, dtype=np.uint64) * np.uint64(8) + np.uint64(3))) & np.uint64(1)
    return bits.reshape(-1)[:n].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- launch decoding
def val(v):
    """a recorded ctypes argument as a Python value (structures for byref arguments)"""
    if v is None:
        return None
    obj = getattr(v, "_obj", None)
    if obj is not None:
        return obj
    if isinstance(v, C._SimpleCData):
        return v.value
    return v


def coff_of(ptr, ld, esz, blocks):
    """(channel offset, pixel index inside its image) of a view pointer, counted from the start of the allocation it points into.
    The caller checks that the pixel index is the view's first interior pixel: the allocation then starts on the pixel grid of
    the view and the channel offset is the one the engine used."""
    for a, s in blocks:
        if a <= ptr < a + s:
            assert (ptr - a) % esz == 0, f"view pointer {ptr:#x} is not on an element boundary"
            e = (ptr - a) // esz
            return e % ld, e // ld
    raise AssertionError(f"view pointer {ptr:#x} is in no allocation")


def elem_size(dtype):
    return 2 if dtype == L.BF16 else 4


def view_desc(t, esz, blocks):
    coff, pix = coff_of(t.ptr, t.ld, esz, blocks)
    return {"ptr": t.ptr, "img_stride": int(t.img_stride), "row_stride": int(t.row_stride), "ld": int(t.ld),
            "align": t.ptr % 16, "coff": coff, "pix": pix % int(t.img_stride)}


def gsrc_desc(g, dtype, blocks):
    return {"kind": int(g.kind), "nslabs": int(g.nslabs), "slab_stride": int(g.slab_stride), "ld": int(g.ld),
            "coff": int(g.coff), "align": g.ptr % 16 if g.ptr else 0}


def decode(name, args, blocks):
    """(name, args) -> list of plain values: ints / floats, view and gsrc descriptions, 'null' / 'ptr' for pointers"""
    types = L.SIGNATURES[name]
    assert len(types) == len(args), name
    vals = [val(a) for a in args]
    dtype = None
    if name in ("p2p_igemm", "p2p_igemm_norm_act", "p2p_conv_strip"):
        dtype = vals[1]
    elif name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewin_actbwd", "p2p_conv_fewout"):
        dtype = vals[2]
    elif name in ("p2p_wgemm", "p2p_wgemm_edge", "p2p_wgrad_small", "p2p_norm_act_fwd", "p2p_norm_act_fwd_tail",
                  "p2p_norm_act_bwd", "p2p_act_bwd", "p2p_rgbuv_points", "p2p_rgbuv_hist_fwd3", "p2p_rgbuv_hist_hellinger_bwd3",
                  "p2p_head_dgrad", "p2p_head_softmax_cce", "p2p_bce_logits", "p2p_bce_logits_pad8", "p2p_tanh_l1_fwd",
                  "p2p_tanh_l1_fwd_pair", "p2p_tanh_l1_bwd", "p2p_tanh_l1_bwd_pad8", "p2p_view_colsum", "p2p_pack_input",
                  "p2p_pack_input_multi", "p2p_pack_pair", "p2p_pack_pair_idx", "p2p_unpack", "p2p_weight_prep", "p2p_weight_prep_pad",
                  "p2p_weight_prep_batched", "p2p_adam_prep_batched"):
        dtype = vals[0]
    out = []
    for t, v in zip(types, vals):
        if t is L._TP and name == "p2p_pack_input_multi":          # an array of ndst views
            out.append(("views", tuple(tuple(sorted((k, x) for k, x in view_desc(d, elem_size(dtype), blocks).items() if k != "ptr"))
                                       for d in list(v)[:vals[8]])))
        elif t is L._TP:
            out.append(None if v is None else ("view", view_desc(v, elem_size(dtype), blocks)))
        elif t is L._GP:
            out.append(None if v is None else ("gsrc", gsrc_desc(v, dtype, blocks)))
        elif t is C.c_void_p:
            p = v.value if isinstance(v, C.c_void_p) else v
            out.append(None if not p else ("ptr", p % 16))
        elif t is C.c_float:
            out.append(float(v))
        else:
            out.append(int(v))
    return out


def signature(name, dec):
    key = []
    for d in dec:
        if isinstance(d, tuple) and d[0] in ("view", "gsrc"):
            key.append((d[0],) + tuple(sorted((k, v) for k, v in d[1].items() if k != "ptr")))
        else:
            key.append(d)
    return (name,) + tuple(key[:-1])           # the last argument is the stream


# ---------------------------------------------------------------------------------------------------------------- variant keys
# A launch's VARIANT KEY is its signature without the batch -- N and what is proportional to it -- plus what the library's host
# queries say about the kernel form the launch takes at that batch.  Two batches with the same key run the same code on more or
# fewer images; a key that only some batches produce is a kernel variant a test must reach at one of those batches.
#   entry point: (position of N, positions of the other batch-proportional arguments)
MODELLED = {
    "p2p_igemm": (2, ()), "p2p_igemm_norm_act": (2, ()), "p2p_conv_strip": (2, ()),
    "p2p_igemm_edge": (3, ()), "p2p_conv_fewin": (3, ()), "p2p_conv_fewout": (3, ()), "p2p_conv_fewin_actbwd": (3, ()),
    "p2p_head_dgrad": (1, ()),
    "p2p_wgemm": (1, ()), "p2p_wgemm_edge": (2, ()), "p2p_wgrad_small": (2, ()),
    "p2p_norm_act_fwd": (1, (8, 19)), "p2p_norm_act_fwd_tail": (1, (8, 19)),      # slab_stride, ws_bytes
    "p2p_norm_act_bwd": (1, (18,)), "p2p_act_bwd": (1, ()),                        # ws_bytes
}


def _nonzero(x):
    return "nonzero" if x else "zero"


def plan_facts(name, dec):
    """what the host queries of the library answer for the launch at its batch: the kernel form behind the entry point"""
    lib = L.lib()
    if name in ("p2p_igemm", "p2p_igemm_norm_act", "p2p_conv_strip"):
        q = dec[:7]                              # op, dtype, N, LH, LW, Cg, Cd
        hw = q[3] * q[4]
        fused_stats = name == "p2p_igemm" and dec[12] is not None        # (the slots of the epilogue the launch really runs)
        facts = [("brig_ok", lib.p2p_brig_ok(*q)), ("brig_stat_slots", lib.p2p_brig_stat_slots(*q)),
                 ("igemm_norm_act_ok", lib.p2p_igemm_norm_act_ok(*q)),
                 ("layer_stat_slots", lib.p2p_igemm_layer_stat_slots(*q) if fused_stats else 0),
                 ("conv_strip_ok", lib.p2p_conv_strip_ok(*q)), ("conv_strip_stat_slots", lib.p2p_conv_strip_stat_slots(*q))]
        if hw < 256:        # 256-row tiles hold ipt = 256 / (LH * LW) images (brig_plan; the im2col tiles run across images too)
            facts.append(("N % ipt", _nonzero(q[2] % (256 // hw))))
        return tuple(facts)
    if name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewout", "p2p_conv_fewin_actbwd"):
        q = dec[:8]                              # op, stride, dtype, N, LH, LW, cin_pad, ncols
        return (("conv_fewin_ok", lib.p2p_conv_fewin_ok(*q)), ("conv_fewout_ok", lib.p2p_conv_fewout_ok(*q)))
    if name in ("p2p_wgemm", "p2p_wgemm_edge", "p2p_wgrad_small"):
        if name == "p2p_wgemm":
            dtype, stride, (n, lh, lw, cg, cd), hi, lo = dec[0], 2, dec[1:6], dec[6], dec[7]
        else:
            dtype, stride, (n, lh, lw, cg, cd), hi, lo = dec[0], dec[1], dec[2:7], dec[7], dec[8]
        return (("wgrad_small", int(lib.p2p_wgrad_small_blocks(dtype, stride, n, lh, lw, cg, cd, hi[1]["ld"], lo[1]["ld"]) > 0)),)
    if name in ("p2p_norm_act_fwd", "p2p_norm_act_fwd_tail", "p2p_norm_act_bwd"):
        # the register-resident forms launch ((N + 7) / 8) * 8 image slots (norm_act.hip): idle slots unless N % 8 == 0
        return (("N % 8", _nonzero(dec[1] % 8)),)
    return ()


def variant_key(name, dec):
    """decoded launch (decode) of a MODELLED entry point -> its variant key"""
    n_at, prop = MODELLED[name]
    key = [name]
    for i, d in enumerate(dec[:-1]):               # the last argument is the stream
        if i == n_at or i in prop:
            continue
        if isinstance(d, tuple) and d[0] in ("view", "gsrc"):
            key.append((d[0],) + tuple(sorted((k, v) for k, v in d[1].items() if k not in ("ptr", "slab_stride"))))
        else:
            key.append(d)
    return tuple(key) + (("facts",) + plan_facts(name, dec),)


# ---------------------------------------------------------------------------------------------------------------- census
STEP_LAMBDAS = {"baseline": (100.0, None, None), "histogram": (30.0, 1.0, 24), "indexed": (0.01, None, 24)}     # bench.CONFIGS
_FAKE_BASE = 1 << 40        # the address every tensor of a dry run reports (a null pointer stays distinguishable)


def step_desc(model, B, S):
    """(model, B, S, lambda_l1, lambda_hist, palette) with the weights bench.CONFIGS uses for the model"""
    return (model, B, S) + STEP_LAMBDAS[model]


@contextlib.contextmanager
def _dry_run(log):
    """Inside: palette_and_histo_gan_amd.engine on device 'meta' runs its own code -- plans, heuristics, host queries of the
    library -- and every launch lands in `log` as (name, ctypes arguments) instead of on a GPU.  L.call, engine._stream and
    torch.Tensor.data_ptr are replaced process-wide and restored on exit (tensors of other devices keep their real data_ptr), so a
    live engine must not step inside the block.  The meta engine never records a step: _replay_key returns None off a cuda device
    (and would for the patched L.call as well)."""
    from palette_and_histo_gan_amd import engine as E
    real_ptr = torch._C.TensorBase.data_ptr
    saved = (L.call, E._stream)
    L.call = lambda name, *args: log.append((name, args))
    E._stream = lambda: C.c_void_p(0)
    torch.Tensor.data_ptr = lambda t: _FAKE_BASE if t.device.type == "meta" else real_ptr(t)
    try:
        yield E
    finally:
        L.call, E._stream = saved
        del torch.Tensor.data_ptr


class Census:
    """The launches the engine issues for a step of (model, S, dtype) at any batch, found without a GPU: one engine on device
    'meta' runs train_step_* with the launches captured (_dry_run), so every choice comes from engine.py's own _conv / _wgrad /
    _norm_* / _splitk / _msplit / _nsplit / _s2_layers and the library's *_ok / *_slots / *_blocks queries."""

    def __init__(self, model, S, dtype_name):
        self.model, self.S = model, S
        self.dtype = L.BF16 if dtype_name == "bf16" else L.F32
        self.log = []
        with _dry_run(self.log) as E:
            if model == "indexed":
                self.eng = E.Pix2PixEngine(1, 256, "softmax", S, self.dtype, device="meta", seed=47)
            else:
                self.eng = E.Pix2PixEngine(4, 4, "tanh", S, self.dtype, device="meta", seed=47)

    def launches(self, B):
        """[(name, decoded arguments)] of the second step at batch B (the one the engine records), MODELLED entry points only"""
        lam_l1, lam_hist, _ = STEP_LAMBDAS[self.model]
        eng, S = self.eng, self.S
        with _dry_run(self.log):
            for _ in range(2):
                self.log.clear()
                if self.model == "indexed":
                    x = torch.empty((B, S, S, 1), dtype=torch.int32, device="meta")
                    eng.train_step_indexed(x, x, lam_l1, global_batch=B)
                else:
                    x = torch.empty((B, S, S, 4), dtype=torch.float32, device="meta")
                    eng.train_step_rgba(x, x, lam_l1, lam_hist, global_batch=B)
            eng.plans.pop(B, None)
        blocks = [(_FAKE_BASE, 1 << 44)]
        return [(name, decode(name, args, blocks)) for name, args in self.log if name in MODELLED]

    def variant_keys(self, B):
        return {variant_key(name, dec) for name, dec in self.launches(B)}


def harvested_variant_keys(uniq):
    """the variant keys of a harvest ({signature: (name, decoded arguments)}), MODELLED entry points only"""
    return {variant_key(name, dec) for name, dec in uniq.values() if name in MODELLED}


# ---------------------------------------------------------------------------------------------------------------- off-benchmark steps
# (model, S, dtype): cap on the batch of a test case, the batches bench.CONFIGS runs for the case (re-issued by
# test_every_launch_of_the_benchmarked_step_against_f64), the batches that must be in the list whatever the census says (ragged
# tiles and idle image slots at 6, one past a group of 8 at 9, both sides of the split-K target steps at 16 | 17 and 32 | 33, 63 as
# the last batch below the B >= 64 target; f32: batch_invariant pins the splits; histogram at 128x128: the c5 family at an odd
# batch), and the bound on the number of variant classes that first appear above the cap (the census count when the list was
# written: test_step_launches_cpu.py prints them)
CASE_RULES = {
    ("baseline", 64, "bf16"): {"cap": 96, "bench": (4, 256), "required": (6, 9, 16, 17, 32, 33, 63), "above_cap_max": 135},
    ("baseline", 64, "f32"): {"cap": 96, "bench": (256,), "required": (6, 33), "above_cap_max": 6},
    ("histogram", 64, "bf16"): {"cap": 96, "bench": (256,), "required": (6, 33), "above_cap_max": 135},
    ("histogram", 128, "bf16"): {"cap": 24, "bench": (256,), "required": (5,), "above_cap_max": 127},
    ("indexed", 64, "bf16"): {"cap": 48, "bench": (128,), "required": (6, 33), "above_cap_max": 145},
}

# The batches test_every_launch_of_off_benchmark_steps_against_f64 runs.  Beyond the required ones: the batches the census needs
# to reach every variant class at or below the cap (smallest batch first among equals), and for the baseline both sides of the
# block-resident route flip of the 16x16 layers (brig_plan's minimum of 160 workgroups: 79 | 80) and the two batches at which
# p2p_igemm's launcher changes its tile form without any argument changing (49: one K group per SIMD on the 16x16 / 8x8 layers and
# 256-row tiles on the 4x4 ones; 61: 256-row tiles on the 8x8 layers -- table in tests/test_step_launches_gpu.py).  f32 batch 1:
# the lower side of that launcher's w_major flips of the 16x16 layers (2 and 4).
OFF_BENCH_BATCHES = {
    ("baseline", 64, "bf16"): (1, 2, 6, 9, 16, 17, 32, 33, 48, 49, 61, 63, 64, 79, 80),
    ("baseline", 64, "f32"): (1, 6, 8, 16, 33),
    ("histogram", 64, "bf16"): (1, 2, 4, 6, 8, 31, 33, 48, 64, 65),
    ("histogram", 128, "bf16"): (1, 2, 4, 5, 7, 8, 9, 15, 16, 20),
    ("indexed", 64, "bf16"): (1, 2, 4, 6, 8, 31, 32, 33, 48),
}
OFF_BENCH_CASES = [(model, S, dtype_name, B) for (model, S, dtype_name), bs in OFF_BENCH_BATCHES.items() for B in bs]


def describe_key(key):
    """a variant key on one line"""
    out = [key[0]]
    for x in key[1:]:
        if isinstance(x, tuple) and x and x[0] in ("view", "gsrc"):
            d = dict(x[1:])
            out.append(f"{x[0]}(ld {d['ld']} +{d['coff']} @{d['align']}" + (f" kind {d['kind']} x{d['nslabs']}" if x[0] == "gsrc" else "") + ")")
        elif isinstance(x, tuple) and x and x[0] == "facts":
            out.append("| " + " ".join(f"{a}={b}" for a, b in x[1:] if b != 0))
        elif isinstance(x, tuple) and x and x[0] == "ptr":
            out.append(f"ptr@{x[1]}")
        else:
            out.append("-" if x is None else f"{x:g}" if isinstance(x, float) else str(x))
    return " ".join(out)


def coverage(case, batches, upto=512):
    """census of one (model, S, dtype) case for B = 1 .. upto against the batches a test runs (and the benchmarked ones):
    ({class: covering batch or None} for the classes found at or below the cap, [the classes among them that no batch covers],
    {class: first batch} for the classes that first appear above the cap, {class: first batch} for every class)"""
    rule = CASE_RULES[case]
    census = Census(*case)
    tested = sorted(set(batches) | {b for b in rule["bench"]})
    first, by = {}, {}
    for B in range(1, upto + 1):
        for k in census.variant_keys(B):
            first.setdefault(k, B)
            if B in tested:
                by.setdefault(k, B)
    below = {k: by.get(k) for k, b in first.items() if b <= rule["cap"]}
    missing = sorted((k for k, b in below.items() if b is None), key=lambda k: (first[k], repr(k)))
    above = {k: b for k, b in first.items() if b > rule["cap"]}
    return below, missing, above, first
