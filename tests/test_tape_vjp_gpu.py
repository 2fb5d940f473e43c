"""-m gpu: the input-gradient VJPs of the GradientTape path (engine.tape_*, tape.py) as VALUES against the float64 oracle graph
under torch.autograd.grad with leaf inputs (tests/tape_vjp_oracle.py), in both dtypes.

  1. engine level, f32: logits / image, d(first), d(second), d(source) and every weight gradient, per tensor
     rel L2 <= max(1e-5, 1.5 x the deviation of the same oracle graph evaluated in float32 by torch on the CPU) -- DESIGN.md
     section 2's yardstick; the bound in force must stay below 1e-2 (d(source)) / 1e-4 (the discriminator's input gradients).
  2. bf16: end to end against f64 within 1.5 x (the deviation of the oracle with bf16 storage points) + 2^-7 (bound in force
     below 0.4 / 0.06), and at LAUNCH level: what the extra launches consumed is read back from the arena, the op-P
     convolutions are recomputed in float64 (tests/step_launches.conv_p, bf16-rounded master weights) and compared with the
     returned tensors per element within the bound tests/test_step_launches_gpu.py applies to an op-P bf16 launch.  Only this
     check can see a lost term in bf16: the storage noise of the end-to-end comparison (0.15 .. 0.24) is as large as the skip
     term (0.2).  Also: the op-P copy of G.down1 is re-derived after an optimizer step.
  3. pooled arenas reused with other need flags give bit-identical results.
  4. through tape.gradient: topologies whose discriminator call needs d(second input).
  5. p2p_grad_accumulate as a kernel.

Every case asserts from the reference alone, before it looks at the engine, that it could fail: d(first) and d(second) differ by
>= 1 in rel L2 (a swap cannot pass), each of the two terms of d(source) is >= 0.15 of the total (a dropped term cannot pass), and
the case keeps MIN_FLIP_MARGIN from the nearest (Leaky)ReLU kink (tests/tape_vjp_oracle.py: why the seeds are what they are).
"""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import pix2pix_model as M
from palette_and_histo_gan_amd.tf_compat import tf
from tests import gpu_util as U
from tests import step_launches as SL
from tests import tape_vjp_oracle as O

pytestmark = pytest.mark.gpu

# (B, S) -> seed.  Any seed tests/tape_vjp_oracle.search_seed accepts will do (python -m tests.tape_vjp_oracle prints the first
# per case: 102, 129, 101, 2526); 343 and 394 keep a margin of 4.1 / 4.8 where those first hits have 3.1.
SEEDS = {(1, 64): 102, (2, 64): 343, (3, 64): 394, (1, 128): 2526}
F32_FLOOR, YARD = 1e-5, 1.5
F32_CAPS = {"d_src": 1e-2, "d_first": 1e-4, "d_second": 1e-4}
BF16_SLACK = 2.0 ** -7          # <= 4 bf16 roundings of stored gradients on these chains, 2^-9 each, that the oracle does not model
BF16_CAPS = {"d_src": 0.4, "d_first": 0.06, "d_second": 0.06}
LAUNCH_TOL = SL.OUT_TOL[L.BF16]           # op-P launch, bf16 output: max |error| / max |reference| per image
NEEDS = [(True, False), (False, True), (True, True)]


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


# ---------------------------------------------------------------------------------------------------------------- engine runs
def _engine(c, dtype, params=None, **switches):
    eng = E.Pix2PixEngine(4, 4, "tanh", c.S, dtype, seed=5)
    for k, v in switches.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    eng.set_params(*(params or (O.to_np(c.Gp), O.to_np(c.Dp))))
    return eng


@pytest.fixture(scope="module")
def shared_engine():
    """one f32 engine per case for the tests that do not ask for a fresh one (their calls also reuse its pooled arenas); the
    engines and their arenas are dropped when the module is done"""
    engines = {}

    def get(c, dtype):
        key = (c.seed, c.B, c.S, dtype)
        if key not in engines:
            engines[key] = _engine(c, dtype)
        return engines[key]

    yield get
    for eng in engines.values():
        eng.free_tape_arenas()
    engines.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _host(t):
    return None if t is None else t.detach().cpu().numpy()


D_SENTINEL = 12345.0


def run_d(eng, c, need, weights, inspect=None):
    """one standalone discriminator call and its VJP on an arena: {logits, d_first, d_second, grads} (numpy; None where not
    asked).  D.grads holds a sentinel before the backward: without `weights` nothing may write it."""
    P = eng.tape_arena("D", c.B)
    try:
        logits = eng.tape_discriminator_forward(P, c.tgt, c.src)
        eng.D.grads.fill_(D_SENTINEL)
        d_first, d_second = eng.tape_discriminator_backward(P, torch.tensor(c.g_log), weights, *need)
        torch.cuda.synchronize()
        out = {"logits": _host(logits), "d_first": _host(d_first), "d_second": _host(d_second), "grads": None}
        if weights:
            out["grads"] = eng.D.export(eng.D.grads)
            assert all((g != D_SENTINEL).all() for g in out["grads"].values())
        else:
            assert bool((eng.D.grads == D_SENTINEL).all()), "a weight gradient was written without being asked for"
        if inspect is not None:
            out["inspect"] = inspect(P)
        eng.D.grads.zero_()
        return out
    finally:
        eng.release_tape_arena(P)


def run_g(eng, c, need_src=True, inspect=None):
    """one generator call and its VJP on an arena: {image, d_src, grads}"""
    P = eng.tape_arena("G", c.B)
    try:
        image = eng.tape_generator_forward(P, c.src, c.masks)
        d_src = eng.tape_generator_backward(P, torch.tensor(c.g_img), need_src)
        torch.cuda.synchronize()
        out = {"image": _host(image), "d_src": _host(d_src), "grads": eng.G.export(eng.G.grads)}
        if inspect is not None:
            out["inspect"] = inspect(P)
        return out
    finally:
        eng.release_tape_arena(P)


# ---------------------------------------------------------------------------------------------------------------- premises
def _premises(seed, B, net, S=64):
    """what makes the case able to fail, from the reference alone"""
    ref = O.reference(seed, B, net, "f64", S)
    margin = O.case_flip_margin(seed, B, net, S)
    assert margin >= O.MIN_FLIP_MARGIN, (seed, B, S, net, margin)
    if net == "D":
        swap = O.rel_l2(ref["d_first"], ref["d_second"])
        assert swap >= 1.0, swap
    else:
        total = np.linalg.norm(ref["d_src"])
        for term in ("d_down", "d_skip"):
            assert np.linalg.norm(ref[term]) >= 0.15 * total, (term, np.linalg.norm(ref[term]) / total)
    return ref


def _compare(label, got, ref, yard, keys, bound_of, caps):
    """per tensor: rel L2 of got against ref within bound_of(rel L2 of yard against ref); the bounds of `caps` stay below their
    caps; a tensor whose reference is all 0 (the dead 1x1 bottleneck) must be all 0"""
    yards = {n: y for n, y, _ in O.flat_pairs(yard, ref, keys)}
    rows, bad = [], []
    for n, g, r in O.flat_pairs(got, ref, keys):
        assert g is not None and g.shape == r.shape, (n, None if g is None else g.shape, r.shape)
        assert np.isfinite(g).all(), n
        if not r.any():
            assert not g.any(), f"{n}: the reference is exactly 0"
            continue
        dev = O.rel_l2(yards[n], r)
        bound = bound_of(dev)
        if n in caps:
            assert bound < caps[n], f"{label} {n}: the oracle alone deviates by {dev:.3g}: bound {bound:.3g} >= cap {caps[n]:.3g}"
        e = O.rel_l2(g, r)
        rows.append((n, e, bound, dev))
        if not e <= bound:
            bad.append(f"{n}: {e:.3g} > {bound:.3g} (oracle alone {dev:.3g})")
    worst = max(rows, key=lambda x: x[1] / x[2])
    shown = [x for x in rows if x[0] in caps or x is worst]
    print(f"\n[{label}] " + "; ".join(f"{n} {e:.2e} (bound {b:.2e}, oracle alone {d:.2e})" for n, e, b, d in shown))
    assert not bad, f"{label}: " + "; ".join(bad)


def _f32_bound(dev):
    return max(F32_FLOOR, YARD * dev)


def _bf16_bound(dev):
    return YARD * dev + BF16_SLACK


def _check_d(label, got, seed, B, need, weights, kind, S=64):
    ref = _premises(seed, B, "D", S)
    for k, want in zip(("d_first", "d_second"), need):
        assert (got[k] is not None) == want, f"{k} asked {want}"
    assert (got["grads"] is not None) == weights
    keys = ["logits"] + [k for k, want in zip(("d_first", "d_second"), need) if want] + (["grads"] if weights else [])
    if kind == "f32":
        _compare(label, got, ref, O.reference(seed, B, "D", "f32", S), keys, _f32_bound, F32_CAPS)
    else:
        keys = [k for k in keys if k.startswith("d_")]
        _compare(label, got, ref, O.reference(seed, B, "D", "bf16", S), keys, _bf16_bound, BF16_CAPS)


def _check_g(label, got, seed, B, kind, S=64):
    ref = _premises(seed, B, "G", S)
    if kind == "f32":
        _compare(label, got, ref, O.reference(seed, B, "G", "f32", S), ["image", "d_src", "grads"], _f32_bound, F32_CAPS)
    else:
        _compare(label, got, ref, O.reference(seed, B, "G", "bf16", S), ["d_src"], _bf16_bound, BF16_CAPS)


# ---------------------------------------------------------------------------------------------------------------- 1. f32, engine level
def test_the_oracle_helper_is_the_oracle_graph():
    """tests/tape_vjp_oracle.generator / discriminator restate rg.unet_generator / rg.patch_discriminator (two source leaves,
    noted pre-activations): same bits.  (Host arithmetic only; it carries the module's gpu mark because the suite that runs
    without a GPU is to stay as it is.)"""
    from oracle import reference_graph as rg
    c = O.case(SEEDS[(1, 64)], 1)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    masks = [t(m) for m in c.masks]
    for ctx in (contextlib.nullcontext(), rg.storage_dtype(torch.bfloat16)):
        with ctx:
            assert torch.equal(O.generator(c.Gp, t(c.src), t(c.src), masks), rg.unet_generator(c.Gp, t(c.src), masks, "tanh"))
            assert torch.equal(O.discriminator(c.Dp, t(c.tgt), t(c.src)), rg.patch_discriminator(c.Dp, t(c.tgt), t(c.src)))


@pytest.mark.parametrize("weights", [True, False], ids=["weights", "inputs-only"])
@pytest.mark.parametrize("need", NEEDS, ids=["first", "second", "both"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_discriminator_vjps_f32(shared_engine, B, need, weights):
    seed = SEEDS[(B, 64)]
    c = O.case(seed, B)
    got = run_d(shared_engine(c, L.F32), c, need, weights)
    _check_d(f"D f32 B={B} need={need} weights={weights}", got, seed, B, need, weights, "f32")


@pytest.mark.parametrize("B", [1, 2, 3])
def test_generator_vjps_f32(shared_engine, B):
    seed = SEEDS[(B, 64)]
    c = O.case(seed, B)
    _check_g(f"G f32 B={B}", run_g(shared_engine(c, L.F32), c), seed, B, "f32")


def test_both_networks_at_128x128_f32():
    seed = SEEDS[(1, 128)]
    c = O.case(seed, 1, 128)
    eng = _engine(c, L.F32)
    _check_g("G f32 128x128", run_g(eng, c), seed, 1, "f32", 128)
    _check_d("D f32 128x128", run_d(eng, c, (True, True), True), seed, 1, (True, True), True, "f32", 128)


# ---------------------------------------------------------------------------------------------------------------- 2. bf16
VARIANTS = {"default": {}, "partial-pixels": {"full_pixels": False}, "no-fewout": {"use_conv_fewout": False}}
BF16_CASES = [("default", 1), ("default", 2), ("default", 3), ("partial-pixels", 2), ("no-fewout", 2)]


def _per_image(got, ref, scale):
    """max over the images of max |got - ref| / scale[image]"""
    err = np.abs(np.asarray(got, np.float64) - ref).reshape(len(ref), -1).max(axis=1)
    return float((err / scale).max())


def _img_max(x):
    return np.abs(x).reshape(len(x), -1).max(axis=1)


def _launch_level_g(eng, ic=4):
    """reads what the two extra launches of d(source) consumed (d(raw) of down1, d(z) of the head) and recomputes them"""
    def inspect(P):
        w = eng.G.export()
        down = SL.conv_p(U.halo_to_np(P["dd"][1]), U.q(w["down1.kernel"], L.BF16), 2)
        skip = SL.conv_p(U.halo_to_np(P["dz"])[..., :eng.out_ch], U.q(w["last.kernel"], L.BF16), 1)[..., -ic:]
        return down, skip
    return inspect


def _launch_level_d(eng):
    def inspect(P):
        return SL.conv_p(U.halo_to_np(P["d_draw"]), U.q(eng.D.export()["down.kernel"], L.BF16), 2)
    return inspect


@pytest.mark.parametrize("variant,B", BF16_CASES, ids=[f"{v}-B{b}" for v, b in BF16_CASES])
def test_generator_source_gradient_bf16(variant, B):
    seed = SEEDS[(B, 64)]
    c = O.case(seed, B)
    eng = _engine(c, L.BF16, **VARIANTS[variant])
    got = run_g(eng, c, inspect=_launch_level_g(eng))
    down, skip = got["inspect"]
    # launch level: d(source) = [down1 transposed] + [source columns of the head's data gradient], each stored in bf16
    scale = _img_max(down) + _img_max(skip)
    assert (_img_max(skip) > 10 * LAUNCH_TOL * scale).all() and (_img_max(down) > 10 * LAUNCH_TOL * scale).all(), \
        "a term is too small for its loss to show"
    e = _per_image(got["d_src"], down + skip, scale)
    print(f"\n[G bf16 {variant} B={B}] launch level: {e:.2e} of max|down1 term| + max|skip term| (bound {LAUNCH_TOL:.0e})")
    assert e < LAUNCH_TOL, e
    _check_g(f"G bf16 {variant} B={B}", got, seed, B, "bf16")


@pytest.mark.parametrize("variant,B", BF16_CASES, ids=[f"{v}-B{b}" for v, b in BF16_CASES])
def test_discriminator_input_gradients_bf16(variant, B):
    seed = SEEDS[(B, 64)]
    c = O.case(seed, B)
    eng = _engine(c, L.BF16, **VARIANTS[variant])
    got = run_d(eng, c, (True, True), True, inspect=_launch_level_d(eng))
    both = got["inspect"]
    ic = eng.in_ch
    for k, name in enumerate(("d_first", "d_second")):
        want = both[..., k * ic:(k + 1) * ic]
        e = _per_image(got[name], want, _img_max(want))
        print(f"\n[D bf16 {variant} B={B}] launch level {name}: {e:.2e} (bound {LAUNCH_TOL:.0e})")
        assert e < LAUNCH_TOL, (name, e)
    assert O.rel_l2(both[..., :ic], both[..., ic:]) >= 1.0          # (the two halves of the launch differ as the references do)
    _check_d(f"D bf16 {variant} B={B}", got, seed, B, (True, True), True, "bf16")


def _model(c, dtype_name):
    m = M.Pix2PixModel(DU.synthetic_rgba_ds(4, batch_size=2), None, "front2right", "tape-vjp-test", lambda_l1=100.0,
                       dtype=dtype_name, seed=5)
    m.engine.set_params(O.to_np(c.Gp), O.to_np(c.Dp))
    return m


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_down1_copy_is_rederived_after_an_optimizer_step(dtype_name):
    """d(source), one Adam.apply_gradients on G through the tape API, d(source) again: the second equals a fresh engine loaded
    with the exported weights bit for bit, so the op-P copy of G.down1 (engine._down1_copy) followed the weights"""
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    c = O.case(SEEDS[(2, 64)], 2)
    m = _model(c, dtype_name)
    eng = m.engine
    first = run_g(eng, c)["d_src"]
    w_before = U.q(eng.G.export()["down1.kernel"], dtype)
    with tf.GradientTape() as tape:
        fake = m.generator(c.src, masks=c.masks)
        loss = (fake - torch.tensor(c.tgt, device=U.DEV)).abs().mean()
    grads = tape.gradient(loss, m.generator.trainable_variables)
    m.generator_optimizer.apply_gradients(zip(grads, m.generator.trainable_variables))
    assert m.generator_optimizer.iterations == 1
    w_after = U.q(eng.G.export()["down1.kernel"], dtype)
    assert (w_before != w_after).mean() > 0.5, "the step left down1's operand copy as it was: the test shows nothing"
    second = run_g(eng, c)["d_src"]
    fresh = _engine(c, dtype, params=(eng.G.export(), eng.D.export()))
    want = run_g(fresh, c)["d_src"]
    assert np.array_equal(second, want), O.rel_l2(second, want)
    assert not np.array_equal(first, second)


# ---------------------------------------------------------------------------------------------------------------- 3. arena reuse
def _same(a, b):
    for k in a:
        if isinstance(a[k], dict):
            assert all(np.array_equal(a[k][n], b[k][n]) for n in a[k]), k
        elif a[k] is not None:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=["f32", "bf16"])
def test_pooled_arenas_reused_with_other_need_flags(dtype):
    B = 2
    c = O.case(SEEDS[(B, 64)], B)
    eng, fresh = _engine(c, dtype), _engine(c, dtype)
    runs = []
    for need in [(True, True), (True, False), (False, True), (True, True)]:
        runs.append(run_d(eng, c, need, True))
        pool = eng._arena_pool[("D", B)]
        assert len(pool) == 1, "the calls did not share one pooled arena"
    arena = eng._arena_pool[("D", B)][0]
    assert "g_dcat2" in arena and arena["g_dcat"].c < 2 * eng.in_ch          # (both buffers were in use)
    _same(runs[0], runs[3])
    _same(runs[0], run_d(fresh, c, (True, True), True))
    g_runs = [run_g(eng, c, need) for need in (True, False, True)]
    assert len(eng._arena_pool[("G", B)]) == 1
    assert g_runs[1]["d_src"] is None
    _same(g_runs[0], g_runs[2])
    _same({k: v for k, v in g_runs[0].items() if k != "d_src"}, g_runs[1])
    _same(g_runs[0], run_g(fresh, c))


# ---------------------------------------------------------------------------------------------------------------- 4. through the tape
@pytest.mark.parametrize("name", O.TOPOLOGIES)
def test_tape_topologies_that_need_the_second_input_gradient(name):
    B = 2
    seed = SEEDS[(B, 64)]
    c = O.case(seed, B)
    ref, yard = O.topology_reference(seed, B, name, "f64"), O.topology_reference(seed, B, name, "f32")
    margin = O.flip_margin(ref["probe"], yard["probe"])
    assert margin >= O.MIN_FLIP_MARGIN, margin
    m = _model(c, "f32")
    swapped = [np.ascontiguousarray(x[::-1]) for x in c.masks]
    s_dev, t_dev = torch.tensor(c.src, device=U.DEV), torch.tensor(c.tgt, device=U.DEV)
    with tf.GradientTape(persistent=True) as tape:
        g_total, d_total = O.topology_losses(name, lambda x, sw: m.generator(x, masks=swapped if sw else c.masks),
                                             lambda a, b: m.discriminator([a, b]), s_dev, t_dev)
    gg = tape.gradient(g_total, m.generator.trainable_variables)
    dg = tape.gradient(d_total, m.discriminator.trainable_variables)
    assert all(g is not None for g in gg), "the generator is reached only through d(second input): no gradient came back"
    assert all(g is not None for g in dg)
    for a, k in ((g_total, "g_total"), (d_total, "d_total")):
        assert abs(float(a.detach()) - float(ref[k])) <= 1e-5 * abs(float(ref[k])), (k, float(a.detach()), float(ref[k]))
    got = {"G": {k: _host(g) for k, g in zip(m.engine.G.shapes, gg)}, "D": {k: _host(g) for k, g in zip(m.engine.D.shapes, dg)}}
    for net in ("G", "D"):
        _compare(f"tape {name} {net}", {"grads": got[net]}, {"grads": ref[net]}, {"grads": yard[net]}, ["grads"], _f32_bound, {})


# ---------------------------------------------------------------------------------------------------------------- 5. p2p_grad_accumulate
GUARD = 64


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 256 * 8192 + 7])
def test_grad_accumulate_kernel(n):
    """dst = src (first) / dst += src: one f32 add per element, bit for bit; the vector body, the grid-stride loop's second trip
    (n > 4 * 256 * 8192) and the scalar tail (n % 4); nothing behind n is written; misaligned buffers are refused"""
    gen = torch.Generator(device="cpu").manual_seed(n)
    src_h = torch.randn(n + GUARD, generator=gen)
    dst_h = torch.randn(n + GUARD, generator=gen) * 3.0
    src_h[n:], dst_h[n:] = -4321.0, 1234.5
    src = src_h.to(U.DEV)
    assert src.data_ptr() % 16 == 0

    def launch(dst, first):
        L.call("p2p_grad_accumulate", U.ptr(dst), U.ptr(src), n, first, U.stream())
        torch.cuda.synchronize()
        return _bits(dst)

    # first contribution: dst is not read
    dst = dst_h.to(U.DEV)
    dst[:n] = float("nan")
    assert dst.data_ptr() % 16 == 0
    got = launch(dst, 1)
    assert np.array_equal(got[:n], src_h[:n].numpy().view(np.uint32))
    assert np.array_equal(got[n:], dst_h[n:].numpy().view(np.uint32)), "elements behind n were written"
    # every further one: one f32 add
    want = (dst_h[:n].numpy().astype(np.float32) + src_h[:n].numpy().astype(np.float32)).view(np.uint32)
    got = launch(dst_h.to(U.DEV), 0)
    assert np.array_equal(got[:n], want)
    assert np.array_equal(got[n:], dst_h[n:].numpy().view(np.uint32)), "elements behind n were written"
    assert np.array_equal(launch(dst_h.to(U.DEV), 0), got), "a second launch differs"
    # a pointer that is not 16-byte aligned is refused, the destination untouched
    dst = dst_h.to(U.DEV)
    for d_off, s_off in ((4, 0), (0, 4)):
        with pytest.raises(L.P2PError, match="16-byte aligned"):
            L.call("p2p_grad_accumulate", C.c_void_p(dst.data_ptr() + d_off), C.c_void_p(src.data_ptr() + s_off), n, 0, U.stream())
        assert b"p2p_grad_accumulate: buffers must be 16-byte aligned" in L.lib().p2p_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dst), dst_h.numpy().view(np.uint32))
