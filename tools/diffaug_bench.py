"""Measures the differentiable augmentation on one GPU and prints one JSON line (DESIGN.md "differentiable augmentation"):
  - p2p_diffaug_fwd and p2p_diffaug_bwd with the full policy at (256, 64, 64, 4) and (256, 128, 128, 4): device events around windows
    of --launches launches, --windows windows per entry point, alternating between the two after a warm-up; median (min-max) in us
    and the achieved GB/s over the ALGORITHMIC bytes: the sum pass reads the tensor, the apply pass reads and writes it (3 x).
    --buffers n rotates over n input/output pairs: 1 keeps the tensors in the 256 MiB Infinity Cache, 16 does not.
  - the Pix2PixDiffAugmentModel step at B = 256, 64 x 64, bf16 with the full policy beside the SAME class with policy="" (both tape
    steps, same process): host clock around --steps steps ending in a synchronise, alternating windows; the difference is the
    cost of the feature."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from palette_and_histo_gan_amd import diffaugment as A  # noqa: E402

DEV = "cuda:0"
ALL = "color,translation,cutout"


def _p(t):
    return C.c_void_p(t.data_ptr())


def launches(B, S, n_buf, n_launch, n_window):
    p = A.draw_parameters(B, S, S, ALL, seed=1, step=0)
    color, geometry = p.on(torch.device(DEV))
    ins = [torch.empty((B, S, S, 4), device=DEV).uniform_(-1, 1) for _ in range(n_buf)]
    outs = [torch.empty_like(t) for t in ins]
    ws = torch.empty(int(L.lib().p2p_diffaug_workspace_bytes(B, S, S)) // 4, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(name, i):
        L.call(name, B, S, S, _p(ins[i % n_buf]), _p(color), _p(geometry), p.ch, p.cw, 7, -1.0, _p(outs[i % n_buf]), _p(ws), st)

    names = ("p2p_diffaug_fwd", "p2p_diffaug_bwd")
    for name in names:
        for i in range(10):
            run(name, i)
    times = {name: [] for name in names}
    for _ in range(n_window):
        for name in names:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for i in range(n_launch):
                run(name, i)
            ev[1].record()
            torch.cuda.synchronize()
            times[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / n_launch)
    nbytes = 3 * B * S * S * 16
    return {name: {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                   "algorithmic_bytes": nbytes, "GBps": round(nbytes / statistics.median(t) / 1e3, 1)} for name, t in times.items()}


def steps(B, n_step, n_window, warmup):
    from palette_and_histo_gan_amd import dataset_utils as D
    from palette_and_histo_gan_amd import pix2pix_model as M
    os.chdir(tempfile.mkdtemp())
    ds = D.synthetic_rgba_ds(B, batch_size=B, palette_size=24)
    batch = tuple(torch.as_tensor(t).to(DEV) for t in next(iter(ds)))
    models = {policy: M.Pix2PixDiffAugmentModel(ds, None, "front2right", "diffaug-bench", lambda_l1=100.0, policy=policy, dtype="bf16")
              for policy in (ALL, "")}
    count = {policy: 0 for policy in models}

    def window(policy, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            models[policy].train_step(batch, count[policy], 1)
            count[policy] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for policy in models:
        window(policy, warmup)
    times = {policy: [] for policy in models}
    for _ in range(n_window):
        for policy in models:
            times[policy].append(window(policy, n_step))
    return {(policy or "empty"): {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3)}
            for policy, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-windows", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffaug_bench needs a GPU: a timing taken elsewhere says nothing")
    res = {"batch": args.batch}
    for S in (64, 128):
        for n_buf in (1, 16):
            res[f"launch_{S}_buffers{n_buf}"] = launches(args.batch, S, n_buf, args.launches, args.windows)
    if not args.no_step:
        res["step_bf16_64"] = steps(args.batch, args.steps, args.step_windows, 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
