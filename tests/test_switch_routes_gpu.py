"""-m gpu: every kernel-selecting A/B switch (tests/switch_routes.SETTINGS) run against float64, one fresh child process per setting
(the library reads its switches once per process; the parent never replaces its own program, and one child runs at a time).

A child (python -m tests.switch_routes --setting NAME --mode gpu) runs the setting's direct cases through the checkers of
tests/test_step_launches_gpu.py -- f64 reference with that file's tolerances, NaN before the launch, sentinel around the view, fused
statistics, a second launch bit-identical -- and the setting's step case through _check_step on an engine with the setting's
attribute overrides, and reports routes, errors and output hashes as JSON.  Here, per setting:
- the JSON reports no failure;
- every case took the route the host query gives for it on this machine, and the recorded step's variant keys and routes are those
  of the meta-device census (tests/test_switch_routes_cpu.py proves from the same queries that the setting moves them);
- BIT-IDENTICAL outputs (equal SHA-256 of the output buffers, compared with the baseline child's) where the switch only reorders
  work and no sum -- decided by reading the kernels, switch_routes.BIT_IDENTICAL says what was read:
    P2P_IGEMM_WMAJOR=0         only the blockIdx -> tile map changes
    P2P_BRIG_STAGGER=0 (+CBW)  only the issue time of the weight-ring DMA of waves 4-7
    P2P_WS_SWIZZLE=0           only the place of a pixel's 64-byte chunks in the LDS strip
  and bit-identical STEP results (losses of two steps, every parameter after them) for fuse_act_bwd=0 and split_prep=0, which move
  work between launches (switch_routes.STEP_BIT_IDENTICAL).
  Everything else changes the order of a sum: another K-loop / K-group split (P2P_IGEMM_PIPE, P2P_IGEMM_BIG: the 256-row tile,
  the second K group), one or two taps per wave and the packed-tap tiles (P2P_WS_W16, P2P_WS_PACK: other MFMA accumulation
  chains), wgemm_kernel's K blocking against the pipelined kernel's (P2P_WGEMM_PIPE), two-pass against register-resident
  statistics (P2P_NORM_*_REG), the im2col kernels against the block-resident one (P2P_BRIG), the unfused statistics
  (P2P_BRIG_FUSE_NORM), other K splits (splitk_target, wgemm_pipe's msplit) and other kernels altogether (use_conv_*,
  use_head_fused).  On Gaussian operands such a route is held to the tolerance only.  Every direct convolution and weight-gradient
  case therefore runs a second time in the same child on integer-lattice operands (tests/lattice.py; the row's "exact" families),
  where the f32 accumulation is exact in any order: the stored result must be the integer reference bit for bit, on every image
  -- 0 mismatches, no tolerance -- so two routes of one case are equal to each other because both equal the reference.  (The
  normalisation cases and the step cases stay Gaussian: their sums are not contractions of products.)
- for the two engine switches the meta device cannot see (switch_routes.CENSUS_BLIND) the recorded step's launch signatures differ
  from the default engine's.

A child that times out, dies of a signal, aborts (134 / 139) or reports an illegal memory access is fatal: every remaining case of
this module then fails at once WITHOUT starting another child, and nothing is retried.

Timeout: on the first run on an MI355X the slowest test took 13.7 s (use_conv_strip=False: its GPU child with the step case, about
10 s, of which 3-4 s are the start-up, plus the query child); the `default` child with its 113 direct cases and two step probes took
under 11.5 s.  3 x the slowest child, rounded up: 45 s.
With the lattice pass (every convolution / weight-gradient case a second time, all images against the integer reference), measured
per GPU child on an MI355X (each test prints its child's time): default 8.2 s; the slowest are P2P_IGEMM_PIPE=2 and P2P_IGEMM_BIG=0
at 10.6 s each (the 49- and 256-image cases plus a step case), then wgemm_pipe=False 7.8 s, P2P_BRIG=0 7.5 s and P2P_BRIG_STAGGER=0
7.0 s; every other child took 2.4 - 6.8 s, and the slowest test (default, with its query child) 13.0 s.  No child exceeds 15 s: the
timeout stays at 45 s.
"""
import json
import subprocess
import sys
import time

import pytest

from tests import switch_routes as R

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 45           # seconds: 3 x the slowest child (module docstring)
_FATAL = []                  # set by the first child that faulted, hung or aborted: no further child is started
_DOCS = {}
_SECONDS = {}                # (setting, mode) -> wall time of the child, printed with the setting's table


def _run(name, mode):
    if _FATAL:
        pytest.fail(f"not started: an earlier child was fatal ({_FATAL[0]})")
    cmd = [sys.executable, "-m", "tests.switch_routes", "--setting", name, "--mode", mode]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, cwd=R.ROOT, env=R.child_env(name), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _FATAL.append(f"{name} ({mode}): no result after {CHILD_TIMEOUT} s")
        pytest.fail(_FATAL[0])
    text = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in text:
        _FATAL.append(f"{name} ({mode}): return code {r.returncode}")
        pytest.fail(_FATAL[0] + "\n" + text[-3000:])
    assert r.returncode == 0, f"{name} ({mode}): return code {r.returncode}\n{text[-3000:]}"
    _SECONDS[(name, mode)] = time.monotonic() - t0
    return json.loads(r.stdout), r.stderr


def _doc(name, mode="gpu"):
    """the child's JSON, run once per (setting, mode) and module"""
    if (name, mode) not in _DOCS:
        _DOCS[(name, mode)] = _run(name, mode)
    return _DOCS[(name, mode)]


def _modelled(keys):
    return sorted(k for k in keys if not k.startswith("('calls'"))


@pytest.mark.parametrize("name", list(R.SETTINGS))
def test_switch_setting_against_f64(name):
    env, attrs, base, groups, step = R.SETTINGS[name]
    doc, log = _doc(name)
    print(f"\n[{name}] " + " ".join(f"{k}={v}" for k, v in {**env, **attrs}.items()) + f" (GPU child: {_SECONDS[(name, 'gpu')]:.1f} s)")
    for cid, row in doc["cases"].items():
        errs = ", ".join(f"{f} {e:.2e} ({t:.0e})" for f, (e, t) in sorted(row["errors"].items()))
        exact = ", ".join(f"{f} {e:.4f}" if f.endswith("share") else f"{f} {int(e)}" for f, e in sorted(row.get("exact", {}).items()))
        print(f"  {cid:48s} {' + '.join(R.describe(l, c) for l, c in row['routes']):60s} {errs}" + (f" | lattice: {exact}" if exact else ""))
    if step is not None:
        print(log[log.find(f"[{name}"):] if f"[{name}" in log else log[-2000:])       # the table _check_step printed in the child
    assert not doc["failures"], "\n".join(doc["failures"])
    # the lattice pass: every convolution / weight-gradient case reports its exact families, all at 0 mismatches
    for cid, row in doc["cases"].items():
        counts = [e for f, e in row["exact"].items() if " exact " in f]
        assert cid.startswith("norm ") or counts, f"{cid}: no lattice run"
        assert not any(counts), f"{cid}: {row['exact']}"
    want, _ = _doc(name, "query")
    assert {c: r["routes"] for c, r in doc["cases"].items()} == {c: r["routes"] for c, r in want["cases"].items()}, \
        "a case ran on another route than the host query gives"
    assert all(len(r["sha256"]) >= 1 for r in doc["cases"].values())
    if step is not None:
        assert doc["step"]["keys"] == _modelled(want["step"]["keys"]), "the recorded step is not the one the census describes"
    if base is None:
        return
    base_doc, _ = _doc(base)
    assert not base_doc["failures"], f"the baseline {base} failed"
    if name in R.BIT_IDENTICAL:
        diff = [c for c, r in doc["cases"].items() if r["sha256"] != base_doc["cases"][c]["sha256"]]
        assert not diff, f"outputs differ bit-wise from {base} ({R.BIT_IDENTICAL[name]}): {diff}"
    if name in R.STEP_BIT_IDENTICAL:
        assert doc["step"]["hash"] == base_doc["probes"][repr(tuple(step))]["hash"], \
            f"the step's results differ bit-wise from the default engine's ({R.STEP_BIT_IDENTICAL[name]})"
    if name in R.CENSUS_BLIND:
        assert doc["step"]["signatures"] != base_doc["probes"][repr(tuple(step))]["signatures"], \
            f"the recorded step is the default engine's: the switch moved nothing ({R.CENSUS_BLIND[name]})"
