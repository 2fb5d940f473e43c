"""What the optimizer options cost per train step: the replayed baseline step at c1 (batch 4) and c2
(batch 256), bf16, in four forms on four engines of one process --

    default    the reference's optimizers                (today's step: the launch list is asserted to be the same, not timed against)
    schedule   LinearDecay on both networks              (p2p_adam_tick_sched in place of p2p_adam_tick)
    clipvalue  clipvalue on both networks                (p2p_adam_step in place of the flat Adam launches)
    clipnorm   global_clipnorm on both networks          (p2p_sumsq_partials + p2p_clip_scale per network, p2p_adam_step, and no
                                                          early Adam over the generator's head buckets)

bench.py's step protocol (device-resident synthetic batch, warm-up steps, then K steps back to back, one p2p_replay call each),
timed with device events.  The forms alternate round by round, so a drift of the box lands on all four; per form the median over
the rounds and the spread (min, max) are reported, and the differences to `default` of the medians.  One JSON line.

    python tools/optim_bench.py [--steps 200] [--warmup 20] [--rounds 7] [--configs c1,c2] [--out FILE]
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
from palette_and_histo_gan_amd import schedules as SCH          # noqa: E402
from palette_and_histo_gan_amd.build import source_fingerprint  # noqa: E402

CONFIGS = {"c1": 4, "c2": 256}          # bench.CONFIGS: baseline model, 64x64, lambda_l1 = 100
FORMS = ("default", "schedule", "clipvalue", "clipnorm")
NEW = ("p2p_adam_tick_sched", "p2p_sumsq_partials", "p2p_clip_scale", "p2p_adam_step")
# thresholds that bind on some elements / steps and not on others: the cost does not depend on whether they do
CLIPVALUE, CLIPNORM = 1e-3, 1.0


def configure(eng, form):
    for store in (eng.G, eng.D):
        if form == "schedule":
            eng.set_optimizer(store, learning_rate=SCH.LinearDecay(2e-4, 1000, 1000))
        elif form == "clipvalue":
            eng.set_optimizer(store, clipping=(CLIPVALUE, None))
        elif form == "clipnorm":
            eng.set_optimizer(store, clipping=(None, CLIPNORM))


def time_steps(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def recorded_names(eng):
    return [n for n, _ in next(iter(eng._replays.values()))[1] if n is not None]


def run_config(name, B, args, device):
    src, tgt = DU.synthetic_rgba_batch(np.random.default_rng([47, 0]), B, 64)
    src_d, tgt_d = torch.as_tensor(src).to(device), torch.as_tensor(tgt).to(device)
    engines = {k: E.Pix2PixEngine(4, 4, "tanh", 64, L.BF16, device=device, seed=47) for k in FORMS}
    for k, e in engines.items():
        configure(e, k)
    steps = {k: (lambda e=e: e.train_step_rgba(src_d, tgt_d, 100.0, global_batch=B)) for k, e in engines.items()}
    for k in steps:
        for _ in range(args.warmup):
            steps[k]()
        assert len(engines[k]._replays) == 1, "the step is not replayed"
    torch.cuda.synchronize()
    names = {k: recorded_names(e) for k, e in engines.items()}
    assert not any(n in NEW for n in names["default"]), "the default step issues a new entry point"
    ms = {k: [] for k in steps}
    for r in range(args.rounds):
        for k in (FORMS if r % 2 == 0 else FORMS[::-1]):
            ms[k].append(time_steps(steps[k], args.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_g, n_d = engines["default"].G.numel, engines["default"].D.numel
    out = {"batch": B, "rounds": args.rounds, "steps_per_round": args.steps,
           "ms_per_step": {k: {"median": round(med[k], 5), "min": round(min(v), 5), "max": round(max(v), 5)} for k, v in ms.items()},
           "spread_of_default_us": round((max(ms["default"]) - min(ms["default"])) * 1e3, 2),
           "delta_to_default_us": {k: round((med[k] - med["default"]) * 1e3, 2) for k in FORMS[1:]},
           "expected_us_at_6.2_TB_s": {"clipnorm (one more read of g)": round((n_g + n_d) * 4 / 6.2e12 * 1e6, 1)},
           "new_launches_per_step": {k: {n: names[k].count(n) for n in NEW if n in names[k]} for k in FORMS},
           "adam_launches_per_step": {k: sum(1 for n in names[k] if n.startswith("p2p_adam_") and "tick" not in n) for k in FORMS},
           "last_gradient_norm": {s: float(getattr(engines["clipnorm"], s).opt.norm_dev[0]) for s in ("G", "D")}}
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
        raise SystemExit("optim_bench.py measures on the GPU: no device found (there is no CPU timing)")
    device = "cuda:0"
    result = {"tool": "optim_bench", "dtype": "bf16", "source_fingerprint": source_fingerprint(),
              "device": torch.cuda.get_device_name(0), "timing": "device events around K replayed steps; forms alternate per round",
              "forms": {"default": "Adam(2e-4, beta_1=0.5) twice", "schedule": "LinearDecay on both networks",
                        "clipvalue": f"clipvalue {CLIPVALUE} on both", "clipnorm": f"global_clipnorm {CLIPNORM} on both"},
              "configs": {name: run_config(name, CONFIGS[name], args, device) for name in args.configs.split(",")}}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
