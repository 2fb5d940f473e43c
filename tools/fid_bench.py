"""Measures the FID evaluation on one GPU and prints one JSON line:
  - the InceptionV3 forward (p2p_inc_* launches only) at chunk 32, 299 x 299: images/s, TFLOP/s at 11.42 GFLOP per image and
    the fraction of the 157.3 TFLOP/s f32 MFMA peak of the MI355X;
  - the wall time of one S2SModel.report_fid(44) (88 generated images, 4 x 44 images through the network, 2 host sqrtm).
Weights: random He-normal kernels with neutral BatchNorm statistics (the timing does not depend on the values), or --weights.
Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/fid_bench.py --forward-only`."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import inception as INC  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def random_weights(path, seed=0):
    rng = np.random.default_rng(seed)
    convs = [{"kernel": (rng.standard_normal((s.kh, s.kw, s.cin, s.cout)) * np.sqrt(2.0 / (s.kh * s.kw * s.cin))).astype(np.float32),
              "beta": np.zeros(s.cout, np.float32), "moving_mean": np.zeros(s.cout, np.float32),
              "moving_variance": np.ones(s.cout, np.float32)} for s in INC.LAYERS]
    return INC.save_weights(path, convs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    tmp = tempfile.mkdtemp()
    weights = args.weights or random_weights(os.path.join(tmp, "random.inception.npz"))
    flop = sum(2 * s.kh * s.kw * s.cin * s.cout * y.H * y.W for kind, s, _, y in INC.trace().ops if kind == "conv")
    net = INC.InceptionV3Features(weights, dev)
    n = net.chunk
    buf = net.input_buffer()
    buf.uniform_(-1, 1)
    out = torch.empty((n, INC.FEATURES), dtype=torch.float32, device=dev)
    for _ in range(2):
        net.run_chunk(n, INC.SIZE, INC.SIZE, out)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(args.iters):
        net.run_chunk(n, INC.SIZE, INC.SIZE, out)
    ev[1].record()
    torch.cuda.synchronize()
    sec = ev[0].elapsed_time(ev[1]) / 1e3 / args.iters
    res = {"chunk": n, "forward_ms": round(sec * 1e3, 3), "images_per_s": round(n / sec, 1),
           "gflop_per_image": round(flop / 1e9, 3), "tflops": round(flop * n / sec / 1e12, 2),
           "fraction_of_f32_mfma_peak": round(flop * n / sec / PEAK_F32_MFMA, 3)}
    if not args.forward_only:
        from palette_and_histo_gan_amd import dataset_utils as D
        from palette_and_histo_gan_amd import frechet_inception_distance as FID
        from palette_and_histo_gan_amd import pix2pix_model as M
        from palette_and_histo_gan_amd.configuration import TEST_SIZE
        os.environ[FID.ENV] = weights
        os.chdir(tmp)
        model = M.Pix2PixModel(D.synthetic_rgba_ds(TEST_SIZE, batch_size=4), D.synthetic_rgba_ds(TEST_SIZE, batch_size=4, seed=3),
                               "front2right", "fid-bench", lambda_l1=100.0)
        model.report_fid(num_images=TEST_SIZE)          # builds the network, first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = model.report_fid(num_images=TEST_SIZE)
        res["report_fid_s"] = round(time.perf_counter() - t0, 3)
        res["report_fid_images"] = TEST_SIZE
        # the parts of it: generation of 2 x 2 x 44 evaluation images, the network over 4 x 44, the host f64 FID
        t0 = time.perf_counter()
        sets = [model.select_examples_for_evaluation(TEST_SIZE, ds) for ds in (model.train_ds, model.test_ds)]
        res["select_examples_s"] = round(time.perf_counter() - t0, 3)
        fnet = FID.network(weights, dev)
        t0 = time.perf_counter()
        acts = [FID.activations(im, fnet) for pair in sets for im in pair]
        res["features_4x44_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        FID.calculate_fid(acts[0], acts[1])
        res["host_fid_s"] = round(time.perf_counter() - t0, 3)
        res["fid_values_finite"] = bool(np.isfinite(vals).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
