"""What the averaged generator costs per train step: the replayed baseline step at c1 (batch 4) and c2
(batch 256), bf16, in three forms on three engines of one process --

    a  averaging off                                   (today's step: no launch changes)
    b  fused: p2p_adam_ema_flat_dev[_excl]             (engine.enable_ema, the default form)
    c  the flat Adam launches of (a), then p2p_ema_flat over the whole generator as a launch of its own

bench.py's step protocol (device-resident synthetic batch, warm-up steps, then K steps back to back, one p2p_replay call each),
timed with device events.  The forms alternate round by round, so a drift of the box lands on all three; per form the median
over the rounds and the spread (min, max) are reported, and the differences b - a, c - a, b - c of the medians.  One JSON line.

    python tools/ema_bench.py [--steps 200] [--warmup 20] [--rounds 7] [--configs c1,c2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from palette_and_histo_gan_amd import _lib as L                 # noqa: E402
from palette_and_histo_gan_amd import dataset_utils as DU         # noqa: E402
from palette_and_histo_gan_amd import engine as E               # noqa: E402
from palette_and_histo_gan_amd.build import source_fingerprint  # noqa: E402

CONFIGS = {"c1": 4, "c2": 256}          # bench.CONFIGS: baseline model, 64x64, lambda_l1 = 100
DECAY = 0.999
G_BYTES = {"b - a (e in, e out)": 8, "c - a (p in, e in, e out)": 12}


class StandAloneEngine(E.Pix2PixEngine):
    """form c: averaging off in the engine, the average kept by one p2p_ema_flat launch behind the optimizer step (recorded and
    replayed with the step like every other call)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ema_alone = self.G.params.clone()

    def apply_adam(self, g_from=0):
        super().apply_adam(g_from)
        L.call("p2p_ema_flat", E._p(self.ema_alone), E._p(self.G.params), self.G.numel, E._p(self.G.t_dev), DECAY, 1, E._stream())


def time_steps(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def run_config(name, B, args, device):
    src, tgt = DU.synthetic_rgba_batch(np.random.default_rng([47, 0]), B, 64)
    src_d, tgt_d = torch.as_tensor(src).to(device), torch.as_tensor(tgt).to(device)
    engines = {"a": E.Pix2PixEngine(4, 4, "tanh", 64, L.BF16, device=device, seed=47),
               "b": E.Pix2PixEngine(4, 4, "tanh", 64, L.BF16, device=device, seed=47),
               "c": StandAloneEngine(4, 4, "tanh", 64, L.BF16, device=device, seed=47)}
    engines["b"].enable_ema(DECAY)
    steps = {k: (lambda e=e: e.train_step_rgba(src_d, tgt_d, 100.0, global_batch=B)) for k, e in engines.items()}
    for k in steps:
        for _ in range(args.warmup):
            steps[k]()
        assert len(engines[k]._replays) == 1, "the step is not replayed"
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for r in range(args.rounds):
        order = ("a", "b", "c") if r % 2 == 0 else ("c", "b", "a")
        for k in order:
            ms[k].append(time_steps(steps[k], args.steps))
    # the three forms trained on the same batch from the same seed: the same weights, and b's average equals c's
    same = all(torch.equal(engines["a"].G.params, engines[k].G.params) for k in ("b", "c"))
    same_avg = torch.equal(engines["b"].G.ema, engines["c"].ema_alone)
    launches = {k: sum(1 for n, _ in next(iter(e._replays.values()))[1] if n is not None and n.startswith("p2p_") and
                       not n.startswith(("p2p_event", "p2p_stream", "p2p_arm", "p2p_disarm"))) for k, e in engines.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_g = engines["a"].G.numel
    out = {"batch": B, "rounds": args.rounds, "steps_per_round": args.steps,
           "ms_per_step": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in ms.items()},
           "spread_of_a_us": round((max(ms["a"]) - min(ms["a"])) * 1e3, 2),
           "delta_us": {"b - a": round((med["b"] - med["a"]) * 1e3, 2), "c - a": round((med["c"] - med["a"]) * 1e3, 2),
                        "b - c": round((med["b"] - med["c"]) * 1e3, 2)},
           "expected_us_at_6.2_TB_s": {k: round(n_g * by / 6.2e12 * 1e6, 1) for k, by in G_BYTES.items()},
           "kernel_launches_per_step": launches, "weights_equal": bool(same), "averages_equal": bool(same_avg)}
    del engines, steps
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--configs", default="c1,c2")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench.py measures on the GPU: no device found (there is no CPU timing)")
    device = "cuda:0"
    result = {"tool": "ema_bench", "dtype": "bf16", "decay": DECAY, "source_fingerprint": source_fingerprint(),
              "device": torch.cuda.get_device_name(0), "timing": "device events around K replayed steps; forms alternate per round",
              "forms": {"a": "averaging off", "b": "fused into the Adam launches", "c": "flat Adam + p2p_ema_flat launch"},
              "configs": {name: run_config(name, CONFIGS[name], args, device) for name in args.configs.split(",")}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
