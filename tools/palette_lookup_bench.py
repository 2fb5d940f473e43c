"""Measures the palette lookup on one GPU and prints one JSON line.

Kernels: N = 4 and 128 images of 64 x 64, K = 256, softmax probabilities of N(0, 4^2) logits, a 24-colour palette padded with the
filler.  Device events around windows of --launches launches, --windows windows per entry, alternating between the entries after a
warm-up; median (min-max) in us and the bytes the algorithm needs over the median, in GB/s and as a share of the measured HBM
ceiling (6.29 TB/s, a float4 copy).  Timed: the soft forward (reads 1 KB per pixel, writes 16 B), the hard forward, the backward
(reads 16 B, writes 1 KB) and, on the same tensors as the sibling stream, p2p_softmax_bwd with a probabilities gradient only (reads
2 KB per pixel, writes 1 KB in f32).

Step (--step-batch, default 128, bf16: the c4 shape): one hooked train step of Pix2PixIndexedModel with the parent's own losses
against Pix2PixIndexedColourModel without and with the histogram term, host clock around --steps steps ending in a device
synchronise, alternating between the models, median over --windows windows.

Each GPU step of a job that runs this tool belongs under a time limit of its own: `timeout -k 10 300 python tools/palette_lookup_bench.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from palette_and_histo_gan_amd import dataset_utils as D  # noqa: E402
from palette_and_histo_gan_amd import pix2pix_model as M  # noqa: E402

DEV = "cuda:0"
S, K = 64, 256
HBM_CEILING = 6.29e12          # bytes / s: a float4 copy on this part


def _p(t):
    return C.c_void_p(t.data_ptr())


def kernels(N, n_launch, n_window):
    gen = torch.Generator(device=DEV).manual_seed(N)
    probs = torch.softmax(4.0 * torch.randn((N, S, S, K), device=DEV, generator=gen), -1).contiguous()
    pal = torch.tensor([255, 0, 220, 255], dtype=torch.int32, device=DEV).repeat(N, K, 1)
    pal[:, :24, :3] = torch.randint(0, 256, (N, 24, 3), device=DEV, dtype=torch.int32, generator=gen)
    pal[:, 0] = 0
    pal = pal.contiguous()
    g = torch.randn((N, S, S, 4), device=DEV, generator=gen)
    gp = torch.randn((N, S, S, K), device=DEV, generator=gen)
    out, dprobs, dz = torch.empty_like(g), torch.empty_like(probs), torch.empty_like(probs)
    dzv = L.Tensor(dz.data_ptr(), S * S, S, K)          # a view's strides count PIXELS (include/p2pgan.h p2p_tensor); ld = floats per pixel
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pix = N * S * S
    entries = {
        "lookup_fwd_soft": (lambda: L.call("p2p_palette_lookup_fwd", N, S, S, K, _p(probs), _p(pal), 0, 1, _p(out), st), pix * (4 * K + 16)),
        "lookup_fwd_hard": (lambda: L.call("p2p_palette_lookup_fwd", N, S, S, K, _p(probs), _p(pal), 1, 1, _p(out), st), pix * (4 * K + 16)),
        "lookup_bwd": (lambda: L.call("p2p_palette_lookup_bwd", N, S, S, K, _p(g), _p(pal), 1, _p(dprobs), st), pix * (4 * K + 16)),
        "softmax_bwd_gp": (lambda: L.call("p2p_softmax_bwd", L.F32, N, S, S, K, _p(probs), _p(gp), None, 1.0, C.byref(dzv), st), pix * 12 * K),
    }
    for run, _ in entries.values():
        for _ in range(10):
            run()
    times = {name: [] for name in entries}
    for _ in range(n_window):
        for name, (run, _) in entries.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(n_launch):
                run()
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / n_launch)
    res = {}
    for name, t in times.items():
        med, nbytes = statistics.median(t), entries[name][1]
        res[name] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2), "MiB": round(nbytes / 2 ** 20, 1),
                     "GB_per_s": round(nbytes / med / 1e3, 1), "share_of_hbm_ceiling": round(nbytes / (med * 1e-6) / HBM_CEILING, 3)}
    return res


class HookedIndexed(M.Pix2PixIndexedModel):
    """the parent's own losses through the plain hooked step: the baseline the colour model is measured against"""
    differentiable_loss_hooks = True

    def generator_loss(self, fake_predicted, fake_image, real_image):
        return super().generator_loss(fake_predicted, fake_image, real_image)


def steps(B, n_step, n_window):
    ds = D.synthetic_indexed_ds(B, batch_size=B)
    batch = next(iter(ds))
    models = {"indexed_hooked": HookedIndexed(ds, None, "front2right", "lookup-bench"),
              "indexed_colour": M.Pix2PixIndexedColourModel(ds, None, "front2right", "lookup-bench", lambda_colour=100.0),
              "indexed_colour_histogram": M.Pix2PixIndexedColourModel(ds, None, "front2right", "lookup-bench", lambda_colour=100.0,
                                                                      lambda_histogram=1.0)}
    for m in models.values():
        for i in range(3):
            m.train_step(batch, i, 1)
    torch.cuda.synchronize()
    times = {name: [] for name in models}
    for _ in range(n_window):
        for name, m in models.items():
            t0 = time.perf_counter()
            for i in range(n_step):
                m.train_step(batch, i, 1)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / n_step)
    return {name: {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
            for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-batch", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("palette_lookup_bench needs a GPU: a timing taken elsewhere says nothing")
    res = {"size": S, "K": K, "launches": args.launches, "windows": args.windows, "hbm_ceiling_TB_per_s": HBM_CEILING / 1e12}
    for N in (4, 128):
        res[f"N{N}"] = kernels(N, args.launches, args.windows)
    if not args.no_step:
        res[f"step_B{args.step_batch}_bf16"] = steps(args.step_batch, args.steps, args.windows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
