"""Not-gpu: every A/B switch of tests/switch_routes.SETTINGS moves its cases to another kernel, and every dispatch arm of the launchers
with a route query (include/p2pgan.h "route queries") is run against f64 by some GPU test -- proven with the library's host queries
(the launchers' own decision functions) before anything touches a GPU.

One child process per setting (python -m tests.switch_routes --mode query: the library reads its switches once per process), eight at
a time.  For every setting:
 (a) each direct case takes another route than under the setting's baseline row;
 (b) the meta-device census of its step case, extended with the routes of every launch, differs from the baseline's at that batch
     (two engine switches cannot be seen on the meta device: switch_routes.CENSUS_BLIND, compared on the GPU instead);
 (c) the arms that the cases of all settings reach, plus those the suite's default tests reach (tests/test_kernels_gpu.py's shapes
     and the census of every step test_step_launches_gpu.py runs), are ALL arms the header lists -- but for UNREACHED below.
"""
import json
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import switch_routes as R


def _query(name):
    r = subprocess.run([sys.executable, "-m", "tests.switch_routes", "--setting", name, "--mode", "query"], cwd=R.ROOT, env=R.child_env(name),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{name}: query child failed\n{r.stderr[-3000:]}"
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def docs():
    with ThreadPoolExecutor(max_workers=8) as ex:
        return dict(zip(R.SETTINGS, ex.map(_query, R.SETTINGS)))


def _unreached():
    """{(launcher, code): reason}.  Arms that no combination of the switches and legal arguments selects -- and, marked as such, four
    that only an absurd launch would."""
    c = R.header_arms()["_compose"]
    out = {}
    for fam in (1, 2):
        for tile in (3, 5):         # 256 x 64, 256 x 32
            for wm in (0, 1):
                out[("igemm", c("P2P_IGEMM_ROUTE", (fam, tile, 1, 3, wm)))] = (
                    "igemm_route takes the 256x64 / 256x32 tiles at M >= 131072 rows only (bigM): >= 512 workgroups of 256 threads, and "
                    "igemm_stages gives such tiles three stages only up to 320 workgroups")
            out[("igemm", c("P2P_IGEMM_ROUTE", (fam, tile, 1, 2, 1)))] = (
                "NOT unreachable, but out of any test's reach: w_major needs 16 * ncols * C > M * C weight bytes against gathered bytes, "
                "at M >= 131072 rows that is more than 8192 output channels (a >= 2 GB output); no layer here has more than 512")
    for waves in (8, 16):
        out[("ws", c("P2P_WS_ROUTE", (1, 0, waves, 0, 1)))] = (
            "ws_plan: a 1x1 window has 64-byte pixels on both sides (GT = DT = 1); the swizzle unit is pixel bytes * step / 64, which "
            "is 1 (no mask) for the lo side always and for the hi side at stride 1")
    for launcher in ("norm_fwd", "norm_bwd"):
        for ppl in (2, 4):
            for slabs in (0, 1):
                out[(launcher, c("P2P_NORM_ROUTE", (1, ppl, slabs, 0)))] = (
                    "small_geom: the lane group grows to 16 lanes before a lane takes a second pixel, and the small forms serve maps of "
                    "<= 16 pixels: always one pixel per lane (the PPL 2 / 4 instantiations are compiled and never started)")
    return out


UNREACHED = _unreached()


def test_every_switch_moves_its_direct_cases(docs):
    """(a)"""
    bad = []
    for name, (env, attrs, base, groups, step) in R.SETTINGS.items():
        for cid, row in docs[name]["cases"].items():
            assert row["routes"], (name, cid)
            if any(code < 0 for _, code in row["routes"]):
                bad.append(f"{name}: {cid}: the launcher refuses the case")
            if base is not None and row["routes"] == docs[base]["cases"][cid]["routes"]:
                bad.append(f"{name}: {cid}: same route as under {base}: {[R.describe(l, c) for l, c in row['routes']]}")
    assert not bad, "\n".join(bad)


def test_every_switch_moves_its_step(docs):
    """(b)"""
    bad = []
    for name, (env, attrs, base, groups, step) in R.SETTINGS.items():
        if base is None:
            continue
        assert groups or step, f"{name}: neither a direct case nor a step"
        if step is None or name in R.CENSUS_BLIND:
            continue
        if docs[name]["step"]["keys"] == docs[base]["steps"][repr(tuple(step))]:
            bad.append(f"{name}: the census of {step} is the one of {base}")
    assert not bad, "\n".join(bad)
    assert set(R.CENSUS_BLIND) <= set(R.SETTINGS) and set(R.BIT_IDENTICAL) | set(R.STEP_BIT_IDENTICAL) <= set(R.SETTINGS)


def test_every_dispatch_arm_is_run_or_named(docs):
    """(c)"""
    arms = R.header_arms()
    reached = {}
    for launcher, code in docs["default"]["existing"]:
        reached.setdefault((launcher, R.arm_of(launcher, code)), set()).add("the suite's default tests")
    for name, d in docs.items():
        for cid, row in d["cases"].items():
            for launcher, code in row["routes"]:
                reached.setdefault((launcher, R.arm_of(launcher, code)), set()).add(f"{name}: {cid}")
        for launcher, code in d.get("step", {}).get("routes", []):
            reached.setdefault((launcher, R.arm_of(launcher, code)), set()).add(f"{name}: step")
    listed = {(l, c) for l in ("igemm", "brig", "wgemm", "ws", "norm_fwd", "norm_bwd") for c in arms[l]}
    hand_off = {("igemm", 0), ("brig", 0)}       # P2P_IGEMM_ROUTE_BRIG / P2P_BRIG_ROUTE_NONE: another launcher takes the layer
    unknown = sorted(k for k in reached if k not in listed and k not in hand_off)
    assert not unknown, f"routes the header does not list: {[(l, c, R.describe(l, c)) for l, c in unknown]}"
    missing = sorted(listed - set(reached) - set(UNREACHED))
    assert not missing, "arms no GPU test runs:\n" + "\n".join(f"  {l} {c}: {R.describe(l, c)}" for l, c in missing)
    stale = sorted(k for k in UNREACHED if k in reached or k not in listed)
    assert not stale, f"UNREACHED entries that are reached (or no arm): {[(l, c, R.describe(l, c), sorted(reached.get((l, c), []))[:2]) for l, c in stale]}"
    new = sorted(k for k, who in reached.items() if "the suite's default tests" not in who and k in listed)
    print(f"\n{len(listed)} arms, {len(UNREACHED)} named unreachable, {len(new)} run by the switch settings only:")
    for l, c in new:
        print(f"  {l:9s} {R.describe(l, c):48s} <- {sorted(reached[(l, c)])[0]}")


def test_route_queries_refuse_what_the_launchers_refuse():
    """a query returns -1 where its launcher's own argument checks fail (same code path), and composes its codes with the header's
    macros"""
    lib = R.L.lib()
    compose = R.header_arms()["_compose"]
    t = R.L.Tensor(1 << 20, 144, 12, 64)
    import ctypes as C
    assert lib.p2p_igemm_route(R.G, R.BF, 2, 4, 4, 48, 64, C.byref(t), C.byref(t), 1, 0) == -1          # Cg % 32
    assert lib.p2p_igemm_route(R.G, R.BF, 2, 3, 4, 64, 128, C.byref(t), C.byref(t), 1, 0) == -1         # LH not a power of two
    assert lib.p2p_igemm_route(R.G, R.BF, 2, 4, 4, 64, 128, C.byref(t), C.byref(t), 3, 0) == -1         # splitk does not divide the taps
    assert lib.p2p_wgrad_small_route(R.BF, 2, 2, 8, 8, 64, 64, 64, 64) == -1 == lib.p2p_wgrad_small_blocks(R.BF, 2, 2, 8, 8, 64, 64, 64, 64) - 1
    assert lib.p2p_wgemm_route(R.BF, 2, 2, 3, 4, 64, 64, C.byref(t), C.byref(t), 1) == -1
    assert lib.p2p_brig_route(R.G, R.F, 64, 16, 16, 64, 256, 0) == 0                                     # f32: never block-resident
    name, dec = R.igemm(R.G, R.BF, 2, 4, 64, 128)
    assert R.routes(name, dec) == [("igemm", compose("P2P_IGEMM_ROUTE", (3, 0, 2, 4, 1)))]
    name, dec = R.wsmall(R.BF, 2, 2, 32, 4, 64)
    assert R.routes(name, dec) == [("ws", compose("P2P_WS_ROUTE", (2, 1, 8, 1, 0)))]
