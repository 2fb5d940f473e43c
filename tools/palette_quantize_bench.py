"""Measures the palette quantiser's launches on one GPU and prints one JSON document (the method of
tools/palette_project_bench.py): device events around windows of --launches launches, --windows windows per entry, alternating
between the entries after a warm-up; median (min-max) in us.

Shapes: B = 4 and 256 images of 64 x 64, B = 256 of 128 x 128; colours 8 / 16 / 256; iterations 0 (the starting slots alone) and 8.
Inputs: sprite-like (dataset_utils.synthetic_rgba_batch targets plus N(0, 0.03) noise, clipped: 83.5 % of the pixels near one
colour, the contended slot) and uniform noise (every pixel its own colour).  Timed per configuration: p2p_palette_quantize alone,
quantize + p2p_palette_snap with all outputs (palette.quantize's launches), and, for scale, the snap alone on the quantiser's
palette.  The numpy restatement (tests/palette_quantize_oracle.py) is timed on two 64 x 64 images of each input, per image.
Run it under one `timeout`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from palette_and_histo_gan_amd import dataset_utils as D  # noqa: E402

DEV = "cuda:0"
K = 256


def _p(t):
    return C.c_void_p(t.data_ptr())


def inputs(kind, B, S, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-1.0, 1.0, size=(B, S, S, 4)).astype(np.float32)
    _, tgt = D.synthetic_rgba_batch(rng, B, S)
    return np.clip(tgt + rng.normal(0.0, 0.03, size=tgt.shape), -1.0, 1.0).astype(np.float32)


def measure(img, colours, iterations, n_launch, n_window):
    B, S = int(img.shape[0]), int(img.shape[1])
    pal = torch.empty((B, K, 4), dtype=torch.int32, device=DEV)
    sizes = torch.empty((B,), dtype=torch.int32, device=DEV)
    index = torch.empty((B, S, S), dtype=torch.int32, device=DEV)
    dist, out = torch.empty_like(index), torch.empty_like(img)
    counts = torch.empty((B, K), dtype=torch.int32, device=DEV)
    stats = torch.empty((B, 2), dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = C.c_void_p(0)

    def quantize():
        L.call("p2p_palette_quantize", B, S, S, _p(img), colours, iterations, null, null, K, _p(pal), _p(sizes), null, st)

    def snap():
        L.call("p2p_palette_snap", B, S, S, _p(img), _p(pal), _p(sizes), K, _p(index), _p(out), _p(dist), _p(counts), _p(stats), st)

    def both():
        quantize()
        snap()

    entries = {"quantize": quantize, "quantize_snap": both, "snap_alone": snap}
    for run in entries.values():          # `quantize` first: the snap runs on its palette
        for _ in range(3):
            run()
    times = {name: [] for name in entries}
    for _ in range(n_window):
        for name, run in entries.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(n_launch):
                run()
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / n_launch)
    res = {name: {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
           for name, t in times.items()}
    res["mean_size"] = round(float(sizes.to(torch.float64).mean()), 2)
    return res


def numpy_restatement(kinds):
    from tests import palette_quantize_oracle as O
    res = {}
    for kind in kinds:
        img = inputs(kind, 2, 64)
        for colours in (16, 256):
            t0 = time.perf_counter()
            O.quantize(img, colours, 8)
            res[f"{kind}_c{colours}_i8_ms_per_image"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("palette_quantize_bench needs a GPU: a timing taken elsewhere says nothing")
    kinds = ("sprite", "noise")
    res = {"launches": args.launches, "windows": args.windows, "K": K, "numpy": numpy_restatement(kinds)}
    for B, S in ((4, 64), (256, 64), (256, 128)):
        for kind in kinds:
            img = torch.as_tensor(inputs(kind, B, S)).to(DEV).contiguous()
            for colours in (8, 16, 256):
                for iterations in (0, 8):
                    res[f"B{B}_S{S}_{kind}_c{colours}_i{iterations}"] = measure(img, colours, iterations, args.launches, args.windows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
