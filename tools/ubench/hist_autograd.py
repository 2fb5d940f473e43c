"""Timing of the differentiable standalone histogram's backward (histogram.RGBuvHistogram) at the c3 shape (256 x 64 x 64).

    python tools/ubench/hist_autograd.py [--reps R] [--windows K]

Device-event timing, every shape warmed up first; each figure is the median over K windows of R launches (or steps), the spread
(min .. max over the windows) beside it.  Kernels: p2p_hist_normalize_bwd, p2p_rgbuv_hist_bwd, p2p_rgbuv_hist_general_bwd at
(64, inverse-quadratic, 0.03) and (128, RBF, 0.02), and for scale the fused step's p2p_rgbuv_hist_hellinger_bwd3 (its prep kernel +
the same bwd3 kernel).  Steps: the fused c3 step (histogram model, bf16) against the hooked step with a hook that restates
Pix2PixHistogramModel.generator_loss (engine.rgbuv_histogram + histogram.hellinger_loss under autograd), alternated window by
window.  Prints one line per figure and a JSON line at the end."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from palette_and_histo_gan_amd import dataset_utils as DU  # noqa: E402
from palette_and_histo_gan_amd import engine as E  # noqa: E402
from palette_and_histo_gan_amd import histogram as H  # noqa: E402

DEV = torch.device("cuda:0")
p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def timed(fns, reps, windows, warm=3):
    """{name: [ms per call of each window]}; the functions alternate window by window"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, reps))
    return out


def kernels(N, S, reps, windows):
    rng = np.random.default_rng(5)
    _, tgt = DU.synthetic_rgba_batch(rng, N, S, palette_size=24)
    fake = np.clip(tgt + rng.normal(scale=0.05, size=tgt.shape), -1, 1).astype(np.float32)
    tt, ft = torch.tensor(tgt, device=DEV), torch.tensor(fake, device=DEV)
    vt, vf = L.Tensor(tt.data_ptr(), S * S, S, 4), L.Tensor(ft.data_ptr(), S * S, S, 4)
    dimg = torch.empty(N * S * S * 4, dtype=torch.float32, device=DEV)
    fns, sizes = {}, {}
    # raw histograms and upstream gradients of every size timed
    for key, (size, code, sigma) in {"default": (64, 0, 0.02), "iq64": (64, 0, 0.03), "rbf128": (128, 1, 0.02)}.items():
        raw = torch.empty(N * 3 * size * size, dtype=torch.float32, device=DEV)
        if key == "default":
            L.call("p2p_rgbuv_hist_fwd", L.F32, N, S, S, C.byref(vf), p(raw), st())
        else:
            L.call("p2p_rgbuv_hist_general", L.F32, N, S, S, C.byref(vf), size, code, sigma, p(raw), st())
        g = torch.tensor(rng.normal(size=(N, size, size, 3)).astype(np.float32), device=DEV)
        gh = torch.empty_like(raw)
        sizes[key] = (size, code, sigma, raw, g, gh)
    size, code, sigma, raw, g, gh = sizes["default"]
    fns["p2p_hist_normalize_bwd (64)"] = lambda: L.call("p2p_hist_normalize_bwd", p(raw), p(g), N, 64, p(gh), st())
    fns["p2p_rgbuv_hist_bwd"] = lambda: L.call("p2p_rgbuv_hist_bwd", L.F32, N, S, S, C.byref(vf), p(gh), p(dimg), st())
    for key, label in (("iq64", "p2p_rgbuv_hist_general_bwd (64, inverse-quadratic, 0.03)"),
                       ("rbf128", "p2p_rgbuv_hist_general_bwd (128, RBF, 0.02)")):
        size_k, code_k, sigma_k, _, _, gh_k = sizes[key]
        fns[label] = (lambda size_k=size_k, code_k=code_k, sigma_k=sigma_k, gh_k=gh_k:
                      L.call("p2p_rgbuv_hist_general_bwd", L.F32, N, S, S, C.byref(vf), size_k, code_k, sigma_k, p(gh_k), p(dimg), st()))
    for key in ("iq64", "rbf128"):
        size_k, _, _, raw_k, g_k, gh_k = sizes[key]
        L.call("p2p_hist_normalize_bwd", p(raw_k), p(g_k), N, size_k, p(gh_k), st())
    # the fused step's histogram backward, for scale: Hellinger prep kernel + the same bwd3 kernel
    h_r, h_f, ghw = (torch.empty(N * 3 * 64 * 64, dtype=torch.float32, device=DEV) for _ in range(3))
    tot = torch.empty((2, N), dtype=torch.float32, device=DEV)
    sq, sqp = torch.zeros(4, dtype=torch.float32, device=DEV), torch.zeros(N, dtype=torch.float32, device=DEV)
    L.call("p2p_rgbuv_hist_fwd", L.F32, N, S, S, C.byref(vt), p(h_r), st())
    L.call("p2p_rgbuv_hist_fwd", L.F32, N, S, S, C.byref(vf), p(h_f), st())
    L.call("p2p_hellinger_fwd", p(h_r), p(h_f), N, p(tot[0]), p(tot[1]), p(sqp), p(sq), st())
    fns["p2p_rgbuv_hist_hellinger_bwd3 (fused step: prep + bwd3)"] = lambda: L.call(
        "p2p_rgbuv_hist_hellinger_bwd3", L.F32, N, S, S, C.byref(vf), p(h_r), p(h_f), p(tot[0]), p(tot[1]), p(sq),
        1.0 / (2.0 * math.sqrt(2.0) * N), p(ghw), p(dimg), st())
    # the whole autograd backward of the default op (normalize_bwd + hist_bwd + the output allocation), per call
    x = ft.clone().requires_grad_(True)
    out = H.rgbuv_histogram(x)
    gd = sizes["default"][4]
    fns["autograd backward of the op (default arguments)"] = lambda: torch.autograd.grad(out, x, gd, retain_graph=True)
    return timed(fns, reps, windows)


def steps(N, S, reps, windows):
    """fused c3 step vs the hooked step with a restated histogram-model hook (bf16, device dropout, weights updated)"""
    rng = np.random.default_rng([47, 0])
    src, tgt = DU.synthetic_rgba_batch(rng, N, S, palette_size=24)
    src, tgt = torch.tensor(src, device=DEV), torch.tensor(tgt, device=DEV)
    fused = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, device="cuda:0", seed=7)
    hooked = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, device="cuda:0", seed=7)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def gen(fp, fake, real):
        hist = H.hellinger_loss(hooked.rgbuv_histogram(real), hooked.rgbuv_histogram(fake))
        adv = bce(fp, torch.ones_like(fp))
        l1 = (real - fake).abs().mean()
        return adv + 30.0 * l1 + 1.0 * hist, adv, l1, hist

    def disc(rp, fp):
        r, f = bce(rp, torch.ones_like(rp)), bce(fp, torch.zeros_like(fp))
        return r + f, r, f

    fns = {"fused c3 step": lambda: fused.train_step_rgba(src, tgt, 30.0, lambda_hist=1.0),
           "hooked c3 step (restated histogram hook)": lambda: hooked.train_step_rgba_hooked(src, tgt, gen, disc)}
    return timed(fns, reps, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=5)
    a = ap.parse_args()
    N, S = 256, 64
    res = {}
    res.update(kernels(N, S, a.reps, a.windows))
    res.update(steps(N, S, a.step_reps, a.windows))
    summary = {}
    for k, v in res.items():
        med = statistics.median(v)
        summary[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        print(f"{k:60s} {med:9.4f} ms   ({min(v):.4f} .. {max(v):.4f})", flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "S": S, "reps": a.reps, "windows": a.windows, "ms": summary}))


if __name__ == "__main__":
    main()
