"""Timing of the indexed model's loss-hook path: p2p_softmax_bwd and the hooked c4 step (128 x 64 x 64, 256 palette slots, bf16).

    python tools/ubench/indexed_hooks.py [--reps R] [--windows K] [--step-reps R2]

Device-event timing, every shape warmed up first; each figure is the median over K windows of R launches (or steps), the spread
(min .. max over the windows) beside it.  Kernel: p2p_softmax_bwd at B = 128 and 256, bf16 dz, with gp only and with gp + gz; the
effective rate counts the bytes the kernel must move (f32 probs + gp [+ gz] in, bf16 dz out) over its time.  Steps: the fused c4
step (train_step_indexed, lambda_segmentation 0.01) against train_step_indexed_hooked with hooks that restate
Pix2PixIndexedModel's own losses (CCE through `_keras_logits`), alternated window by window.  Prints one line per figure and a
JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from palette_and_histo_gan_amd import dataset_utils as DU  # noqa: E402
from palette_and_histo_gan_amd import engine as E  # noqa: E402
from palette_and_histo_gan_amd import pix2pix_model as M  # noqa: E402

DEV = torch.device("cuda:0")
CN = 256
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


def kernels(S, reps, windows):
    fns, nbytes = {}, {}
    for N in (128, 256):
        M_ = N * S * S
        g = torch.Generator(device=DEV).manual_seed(N)
        probs = torch.softmax(torch.randn((M_, CN), generator=g, device=DEV) * 3.0, -1)
        gp = torch.randn((M_, CN), generator=g, device=DEV)
        gz = torch.randn((M_, CN), generator=g, device=DEV)
        dz = E.HaloBuf(N, S, S, CN, L.BF16, DEV)
        view = dz.view()
        for label, gz_k in (("gp", None), ("gp+gz", gz)):
            name = f"p2p_softmax_bwd B={N} bf16 dz, {label}"
            fns[name] = (lambda N=N, probs=probs, gp=gp, gz_k=gz_k, view=view, keep=(dz, gz):
                         L.call("p2p_softmax_bwd", L.BF16, N, S, S, CN, p(probs), p(gp), None if gz_k is None else p(gz_k), 1.0,
                                C.byref(view), st()))
            nbytes[name] = M_ * CN * (4 * (2 if gz_k is None else 3) + 2)
    return timed(fns, reps, windows), nbytes


def steps(N, S, reps, windows):
    """fused c4 step vs the hooked step with the model's own losses restated (bf16, device dropout, weights updated)"""
    rng = np.random.default_rng([47, 0])
    src, tgt, _ = DU.synthetic_indexed_batch(rng, N, S, palette_size=24)
    src, tgt = torch.as_tensor(src, device=DEV), torch.as_tensor(tgt, device=DEV)
    fused = E.Pix2PixEngine(1, CN, "softmax", S, L.BF16, device="cuda:0", seed=7)
    hooked = E.Pix2PixEngine(1, CN, "softmax", S, L.BF16, device="cuda:0", seed=7)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    cce = M.CategoricalCrossentropy()
    lam = 0.01

    def gen(fp, probs, onehot):
        adv = bce(fp, torch.ones_like(fp))
        l1 = (onehot - probs).abs().mean()
        seg = cce(onehot, probs)
        return adv + 0.0 * l1 + lam * seg, adv, l1, seg

    def disc(rp, fp):
        r, f = bce(rp, torch.ones_like(rp)), bce(fp, torch.zeros_like(fp))
        return r + f, r, f

    fns = {"fused c4 step": lambda: fused.train_step_indexed(src, tgt, lam),
           "hooked c4 step (restated indexed-model hooks)": lambda: hooked.train_step_indexed_hooked(src, tgt, gen, disc)}
    return timed(fns, reps, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=5)
    a = ap.parse_args()
    S = 64
    res, nbytes = kernels(S, a.reps, a.windows)
    res.update(steps(128, S, a.step_reps, a.windows))
    summary = {}
    for k, v in res.items():
        med = statistics.median(v)
        summary[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        rate = ""
        if k in nbytes:
            summary[k]["GB"] = round(nbytes[k] / 1e9, 3)
            summary[k]["TB_per_s"] = round(nbytes[k] / (med * 1e-3) / 1e12, 2)
            rate = f"   {nbytes[k] / 1e9:.3f} GB  {summary[k]['TB_per_s']:.2f} TB/s"
        print(f"{k:52s} {med:9.4f} ms   ({min(v):.4f} .. {max(v):.4f}){rate}", flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "S": S, "reps": a.reps, "windows": a.windows, "ms": summary}))


if __name__ == "__main__":
    main()
