"""-m gpu: the pipelined K loop of wgrad_small.hip (unpacked bf16 contraction) against float64, where a software pipeline goes
wrong: in its prologue and epilogue and where one workgroup carries its fragment registers from strip to strip.

Every case runs with P2P_WS_WANT=32 (a grid-size knob: same kernel, same route, 32 workgroups along x), so that every
workgroup walks three or more strips and some walk one more than the others; the child asserts that from
p2p_wgrad_small_blocks before it launches.  The library reads its switches once per process, so each setting runs all cases in
one fresh child process (python -m tests.test_wgrad_small_loop_gpu OUT.npz): the default arm (16 waves, swizzled strips), 8
waves (P2P_WS_W16=0) and unswizzled strips (P2P_WS_SWIZZLE=0).  A child prefills the output and the workspace with NaN,
launches twice, requires the second result bit-identical to the first and writes dW; this process computes the float64
reference once per case (bf16-rounded inputs, zero halos as engine.HaloBuf makes them) and holds every setting to the bound of
the weight-gradient family in tests/test_step_launches_gpu.py (_tol, with that file's long-K scaling).  Unswizzled strips only
move a pixel's 64-byte chunks inside LDS, so that child's dW is also bit-identical to the default child's.

A child that times out, dies of a signal, aborts or reports an illegal memory access is fatal: no further child is started.
"""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = 32
CHILD_TIMEOUT = 60           # seconds: a child takes its start-up (3-4 s) plus ten launches; a hang must not outlive this

# (name, stride, N, lo map, Cg, Cd, TH): strips = N * lo / TH over 32 workgroups
CASES = [
    ("s2_32to128_1x4", 2, 25, 32, 32, 128, 8),       # tile 1x4 (up6's form), 16 K steps per strip, 100 strips: 3 or 4 each
    ("s2_64to256_2x2", 2, 81, 16, 64, 256, 8),       # tile 2x2, four d windows, 8 K steps per strip, 162 strips: 5 or 6 each
    ("s2_64to128_2x2", 2, 50, 16, 64, 128, 8),       # tile 2x2, two d windows, 100 strips
    ("s1_64to64_2x2", 1, 50, 16, 64, 64, 8),         # stride 1, 100 strips
    ("s2_40to72_masked", 2, 50, 16, 40, 72, 8),      # channel counts off the 32-channel tile: over-read pixels, masked store
]
SETTINGS = {"default": {}, "waves8": {"P2P_WS_W16": "0"}, "noswizzle": {"P2P_WS_SWIZZLE": "0"}}


def _inputs(idx):
    """bf16-rounded operands of case idx as float32 arrays (the same in the child and here)"""
    _, stride, n, lh, cg, cd, _ = CASES[idx]
    rng = np.random.default_rng(1000 + idx)
    import torch
    rnd = lambda x: torch.as_tensor(x.astype(np.float32)).to(torch.bfloat16).float().numpy()
    return rnd(rng.normal(size=(n, stride * lh, stride * lh, cg))), rnd(rng.normal(size=(n, lh, lh, cd)))


def _sum_split(nslabs, n):
    """ws_sum_split of wgrad_small.hip: p2p_wgrad_small_blocks returns the partial slabs plus this second-level split"""
    colblocks, split = (n // 4 + 63) // 64, 1
    while colblocks * split < 512 and nslabs // (split * 2) >= 4 and split < 64:
        split *= 2
    return split


# ---------------------------------------------------------------------------------------------------------------- the child
def _child(out_path):
    import torch
    from palette_and_histo_gan_amd import _lib as L
    from tests import gpu_util as U

    assert os.environ.get("P2P_WS_WANT") == str(WANT)
    res = {}
    for idx, (name, stride, n, lh, cg, cd, th) in enumerate(CASES):
        hi, lo = _inputs(idx)
        hb, lb = U.halo_from(hi, L.BF16), U.halo_from(lo, L.BF16)
        hv, lv = hb.view(), lb.view()
        nb = L.lib().p2p_wgrad_small_blocks(L.BF16, stride, n, lh, lh, cg, cd, hv.ld, lv.ld)
        numel = 16 * cg * cd
        split = _sum_split(WANT, numel)
        strips = n * (lh // th)
        # 32 workgroups along x (the slab count says so), hence strips // 32 or strips // 32 + 1 strips each
        assert nb == WANT + (split if split > 1 else 0), (name, nb, split)
        assert strips // WANT >= 3 and strips % WANT != 0, (name, strips)
        outs = []
        for _ in range(2):
            ws = torch.full((nb * numel,), float("nan"), dtype=torch.float32, device=U.DEV)
            dw = torch.full((numel,), float("nan"), dtype=torch.float32, device=U.DEV)
            L.call("p2p_wgrad_small", L.BF16, stride, n, lh, lh, cg, cd, C.byref(hv), C.byref(lv), U.ptr(dw), U.ptr(ws), U.stream())
            torch.cuda.synchronize()
            outs.append(dw.cpu().numpy())
        assert outs[0].tobytes() == outs[1].tobytes(), f"{name}: the second launch differs from the first"
        res[name] = outs[0]
    np.savez(out_path, **res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------- the tests
pytestmark = pytest.mark.gpu
_FATAL = []
_RESULTS = {}


def _run(setting):
    if setting in _RESULTS:
        return _RESULTS[setting]
    if _FATAL:
        pytest.fail(f"not started: an earlier child was fatal ({_FATAL[0]})")
    env = {k: v for k, v in os.environ.items() if not k.startswith("P2P_") or k == "P2P_LIB"}
    env.update({"P2P_WS_WANT": str(WANT), **SETTINGS[setting]})
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dw.npz")
        cmd = [sys.executable, "-m", "tests.test_wgrad_small_loop_gpu", out]
        try:
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _FATAL.append(f"{setting}: no result after {CHILD_TIMEOUT} s")
            pytest.fail(_FATAL[0])
        text = r.stdout + r.stderr
        if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in text:
            _FATAL.append(f"{setting}: return code {r.returncode}")
            pytest.fail(_FATAL[0] + "\n" + text[-3000:])
        assert r.returncode == 0, f"{setting}: return code {r.returncode}\n{text[-3000:]}"
        with np.load(out) as z:
            _RESULTS[setting] = {k: z[k] for k in z.files}
    return _RESULTS[setting]


@functools.lru_cache(maxsize=None)
def _reference(idx):
    from tests import step_launches as SL
    hi, lo = _inputs(idx)
    return SL.conv_w(hi, lo, CASES[idx][1])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_pipelined_loop_against_f64(setting, idx):
    from palette_and_histo_gan_amd import _lib as L
    from tests import step_launches as SL
    from tests import test_step_launches_gpu as SG
    name, stride, n, lh, cg, cd, _ = CASES[idx]
    got = _run(setting)[name]
    assert np.isfinite(got).all(), "NaN left in dW: an output the launch did not write, or a slab it did not fill"
    k = n * lh * lh
    long_k = max(SG.F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24)          # the scaling of _wgrad_family's "dW f32"
    err = SL.per_tap_err(got.reshape(4, 4, cg, cd), _reference(idx)) * SG.F32_TOL / long_k
    tol = SG._tol("dW f32", L.BF16)
    print(f"\n[{setting}] {name}: dW f32 {err:.2e} ({tol:.0e})")
    assert err <= tol
    if setting == "noswizzle":
        assert got.tobytes() == _run("default")[name].tobytes(), "unswizzled strips changed dW bit-wise"
