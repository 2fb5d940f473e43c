"""Measures the palette projection's launches on one GPU and prints one JSON line (DESIGN.md "palette projection", the method of its
"palette loss" speed table): B = 256 images of 64 x 64, K = 256 and 40 with every slot valid, pixels on palette colours, half of them
with N(0, 0.05) noise.  Device events around windows of --launches launches, --windows windows per entry, alternating between the
entries after a warm-up; median (min-max) in us.  Timed: the soft forward, the hard forward and the backward of
p2p_palette_project_*, and in the same process, as references, p2p_palette_snap with all its outputs and p2p_soft_palette_bwd."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
TAU = 5e-2


def _p(t):
    return C.c_void_p(t.data_ptr())


def measure(B, S, K, n_launch, n_window):
    gen = torch.Generator(device=DEV).manual_seed(K)
    pal = torch.randint(0, 256, (B, K, 4), device=DEV, dtype=torch.int32, generator=gen)
    idx = torch.randint(0, K, (B, S * S), device=DEV, generator=gen)
    img = torch.gather(pal.to(torch.float32), 1, idx[:, :, None].expand(-1, -1, 4)).view(B, S, S, 4) / 127.5 - 1.0
    noisy = torch.rand((B, S, S, 1), device=DEV, generator=gen) < 0.5
    img = (img + noisy * 0.05 * torch.randn(img.shape, device=DEV, generator=gen)).clamp(-1.0, 1.0).contiguous()
    sizes = torch.full((B,), K, dtype=torch.int32, device=DEV)
    g = torch.randn(img.shape, device=DEV, generator=gen)
    gh, gm = torch.randn((B, K), device=DEV, generator=gen), torch.randn((B,), device=DEV, generator=gen)
    out, dimg = torch.empty_like(img), torch.empty_like(img)
    index = torch.empty((B, S, S), dtype=torch.int32, device=DEV)
    dist, counts = torch.empty_like(index), torch.empty((B, K), dtype=torch.int32, device=DEV)
    stats = torch.empty((B, 2), dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (B, S, S, _p(img), _p(pal), _p(sizes), K)
    entries = {
        "project_fwd_soft": lambda: L.call("p2p_palette_project_fwd", *head, TAU, 0, _p(out), st),
        "project_fwd_hard": lambda: L.call("p2p_palette_project_fwd", *head, TAU, 1, _p(out), st),
        "project_bwd": lambda: L.call("p2p_palette_project_bwd", *head, TAU, _p(g), _p(dimg), st),
        "palette_snap_all_outputs": lambda: L.call("p2p_palette_snap", *head, _p(index), _p(out), _p(dist), _p(counts), _p(stats), st),
        "soft_palette_bwd": lambda: L.call("p2p_soft_palette_bwd", *head, TAU, _p(gh), _p(gm), _p(dimg), st),
    }
    for run in entries.values():
        for _ in range(10):
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
    pairs = B * S * S * K
    return {name: {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                   "Gpairs_per_s": round(pairs / statistics.median(t) / 1e3, 1)} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("palette_project_bench needs a GPU: a timing taken elsewhere says nothing")
    res = {"batch": args.batch, "size": 64, "tau": TAU, "launches": args.launches, "windows": args.windows}
    for K in (256, 40):
        res[f"K{K}"] = measure(args.batch, 64, K, args.launches, args.windows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
