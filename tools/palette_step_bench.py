"""What a train step of Pix2PixPaletteModel costs hooked and fused: ms per step at batch 4 and batch 256,
bf16, 64x64 synthetic sprites of 24 colours, for three models of one process --

    plain    Pix2PixModel                        (the fused, replayed step without a palette term: the floor)
    hooked   Pix2PixPaletteModel                 (engine.train_step_rgba_hooked: torch autograd between the kernels, not replayed)
    fused    Pix2PixPaletteModel(fused=True)     (engine.train_step_rgba(palette=...): HIP only, replayed)

through model.train_step on a device-resident batch, as fit() issues it.  The models alternate window by window, so a drift of the
box lands on all three; a window is K steps back to back, timed with the host clock around a window that ends in a synchronise
(the hooked step runs host code between its launches: device events would leave that out).  Per model the median, fastest and
slowest window; the criterion of DESIGN.md's tables is `slowest fused window < fastest hooked window`.  One JSON line.

    python tools/palette_step_bench.py [--windows 7] [--warmup 12] [--batches 4,256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import dataset_utils as DU         # noqa: E402
from palette_and_histo_gan_amd import pix2pix_model as M          # noqa: E402
from palette_and_histo_gan_amd.build import source_fingerprint    # noqa: E402

STEPS = {4: 200, 256: 40}          # steps per window: ~0.1-0.2 s of device time each
LAMBDAS = dict(lambda_l1=100.0, lambda_palette=10.0, lambda_conformance=1.0)
ORDER = ("plain", "hooked", "fused")


def make(kind):
    if kind == "plain":
        return M.Pix2PixModel(None, None, "front2right", "palette-bench-plain", LAMBDAS["lambda_l1"], dtype="bf16", seed=47)
    return M.Pix2PixPaletteModel(None, None, "front2right", f"palette-bench-{kind}", dtype="bf16", seed=47, fused=kind == "fused",
                                 **LAMBDAS)


def window(model, batch, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(n):
        model.train_step(batch, t, 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def run_batch(B, args, device):
    src, tgt = DU.synthetic_rgba_batch(np.random.default_rng([47, 0]), B, 64, palette_size=24)
    batch = (torch.as_tensor(src).to(device), torch.as_tensor(tgt).to(device))
    models = {k: make(k) for k in ORDER}
    n = args.steps or STEPS.get(B, 40)
    last = {}
    for k, m in models.items():
        for t in range(args.warmup):
            last[k] = m.train_step(batch, t, 1)
    assert len(models["fused"].engine._replays) == 1 and len(models["plain"].engine._replays) == 1, "the fused steps are not replayed"
    assert not models["hooked"].engine._replays and models["hooked"]._custom_hooks and not models["fused"]._custom_hooks
    ms = {k: [] for k in ORDER}
    for r in range(args.windows):
        for k in (ORDER if r % 2 == 0 else ORDER[::-1]):
            ms[k].append(window(models[k], batch, n))
    # what the two palette models report after the warm-up, for orientation only: twelve bf16 steps from the same weights on the same
    # batch, not a parity check (tests/test_palette_fused_gpu.py compares one f32 step with injected masks)
    g_h, g_f =([float(x) for x in last[k][0]] for k in ("hooked", "fused"))
    out = {"batch": B, "windows": args.windows, "steps_per_window": n,
           "ms_per_step": {k: {"median": round(statistics.median(v), 4), "fastest": round(min(v), 4), "slowest": round(max(v), 4)}
                           for k, v in ms.items()},
           "slowest_fused_below_fastest_hooked": bool(max(ms["fused"]) < min(ms["hooked"])),
           "hooked_over_fused": round(statistics.median(ms["hooked"]) / statistics.median(ms["fused"]), 3),
           "fused_minus_plain_us": round((statistics.median(ms["fused"]) - statistics.median(ms["plain"])) * 1e3, 1),
           "generator_loss_after_warmup": {"hooked": g_h, "fused": g_f}}
    del models
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--steps", type=int, default=0, help="steps per window (default: 200 at batch 4, 40 at batch 256)")
    ap.add_argument("--batches", default="4,256")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("palette_step_bench.py measures on the GPU: no device found (there is no CPU timing)")
    if args.windows < 5:
        raise SystemExit("at least five alternating windows per model")
    device = "cuda:0"
    out_path = os.path.abspath(args.out) if args.out else None
    with tempfile.TemporaryDirectory() as tmp:          # the models create their log and checkpoint folders under the working directory
        os.chdir(tmp)
        result = {"tool": "palette_step_bench", "dtype": "bf16", "source_fingerprint": source_fingerprint(),
                  "device": torch.cuda.get_device_name(0), "lambdas": LAMBDAS, "temperature": 1e-3, "palette_size": 24,
                  "timing": "host clock around K steps of model.train_step ending in a synchronise; models alternate per window",
                  "models": {"plain": "Pix2PixModel", "hooked": "Pix2PixPaletteModel", "fused": "Pix2PixPaletteModel(fused=True)"},
                  "batches": {str(B): run_batch(B, args, device) for B in (int(x) for x in args.batches.split(","))}}
        os.chdir(ROOT)
    line = json.dumps(result)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
