"""Optimizer options without a GPU: the schedule formulas at their boundaries, the error bound of the
float32 global norm in its documented order, what the Adam constructor refuses, the launch list of a fused step under every
option (the meta-device capture of tests/step_launches.py) and the replay key."""
import math
import types

import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import schedules as SCH
from palette_and_histo_gan_amd.pix2pix_model import Adam
from tests import optimizer_oracle as OO
from tests import step_launches as SL

NEW = ("p2p_adam_tick_sched", "p2p_sumsq_partials", "p2p_clip_scale", "p2p_adam_step")
ADAM = ("p2p_adam_flat_dev", "p2p_adam_flat_dev_excl", "p2p_adam_ema_flat_dev", "p2p_adam_ema_flat_dev_excl", "p2p_adam_step",
        "p2p_adam_prep_batched")


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_schedules_give_known_answers_at_their_boundaries():
    s = SCH.ExponentialDecay(1e-3, 100, 0.5)
    assert s(0) == 1e-3 and s(100) == 1e-3 * 0.5 and s(200) == 1e-3 * 0.25
    assert s(99) == 1e-3 * math.pow(0.5, 0.99) and s(50) == pytest.approx(1e-3 * math.sqrt(0.5), rel=1e-15)
    st = SCH.ExponentialDecay(1e-3, 100, 0.5, staircase=True)
    assert st(0) == st(99) == 1e-3 and st(100) == st(199) == 5e-4 and st(200) == 2.5e-4

    pw = SCH.PiecewiseConstantDecay([10, 20, 30], [1.0, 0.5, 0.25, 0.125])
    assert [pw(t) for t in (0, 9, 10, 11, 20, 21, 30, 31, 10_000)] == [1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125]

    po = SCH.PolynomialDecay(1e-2, 100, end_learning_rate=1e-4, power=1.0)
    assert po(0) == 1e-2 and po(100) == 1e-4 and po(250) == 1e-4
    assert po(99) == (1e-2 - 1e-4) * (1.0 - 99 / 100) + 1e-4 and po(50) == pytest.approx(0.5 * (1e-2 + 1e-4), rel=1e-15)
    sq = SCH.PolynomialDecay(1.0, 10, end_learning_rate=0.0, power=2.0)
    assert sq(5) == 0.25 and sq(10) == 0.0
    cy = SCH.PolynomialDecay(1.0, 10, end_learning_rate=0.0, power=1.0, cycle=True)
    assert cy(0) == 1.0 and cy(5) == 0.5 and cy(10) == 0.0 and cy(15) == 0.25 and cy(20) == 0.0 and cy(25) == 1.0 - 25 / 30

    co = SCH.CosineDecay(2.0, 100, alpha=0.1)
    assert co(0) == 2.0 and co(100) == pytest.approx(0.2, rel=1e-15) and co(1000) == co(100)
    assert co(50) == pytest.approx(2.0 * (0.9 * 0.5 + 0.1), rel=1e-15) and co(99) > co(100)

    li = SCH.LinearDecay(2e-4, 100, 100)
    assert li(0) == li(99) == li(100) == 2e-4 and li(150) == 1e-4 and li(199) == pytest.approx(2e-6, rel=1e-12)
    assert li(200) == 0.0 and li(10_080) == 0.0
    le = SCH.LinearDecay(1.0, 2, 2, end=0.5)
    assert [le(t) for t in range(6)] == [1.0, 1.0, 1.0, 0.75, 0.5, 0.5]

    # warm-up multiplies any kind: (step + 1) / warmup_steps while step < warmup_steps, 1 from its end on
    w = SCH.LinearDecay(1.0, 8, 8, warmup_steps=4)
    assert [w(t) for t in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0] and w(12) == 0.5
    wc = SCH.Constant(3e-4, warmup_steps=10)
    assert wc(0) == 3e-4 * 0.1 and wc(9) == 3e-4 and wc(10) == 3e-4
    assert SCH.as_schedule(wc)[1] and not SCH.as_schedule(2e-4)[1] and not SCH.as_schedule(SCH.Constant(2e-4))[1]


def test_schedule_structs_hold_the_schedule_and_refuse_bad_arguments():
    s = SCH.PiecewiseConstantDecay([3, 7], [1.0, 0.1, 0.01], warmup_steps=2).struct()
    assert (s.kind, s.nbounds, list(s.bounds)[:2], list(s.values)[:3], s.warmup_steps) == (2, 2, [3.0, 7.0], [1.0, 0.1, 0.01], 2.0)
    s = SCH.ExponentialDecay(1e-3, 100, 0.5, staircase=True).struct()
    assert (s.kind, s.flag, s.initial, s.decay_steps, s.rate) == (1, 1, 1e-3, 100.0, 0.5)
    s = SCH.LinearDecay(2e-4, 5, 7, end=1e-5).struct()
    assert (s.kind, s.initial, s.hold_steps, s.decay_steps, s.end) == (5, 2e-4, 5.0, 7.0, 1e-5)
    with pytest.raises(ValueError):
        SCH.PiecewiseConstantDecay(list(range(9)), [1.0] * 10)
    with pytest.raises(ValueError):
        SCH.PiecewiseConstantDecay([1, 2], [1.0, 2.0])
    with pytest.raises(ValueError):
        SCH.ExponentialDecay(1e-3, 0, 0.5)
    with pytest.raises(ValueError):
        SCH.LinearDecay(1e-3, 1, 1, warmup_steps=-1)
    from palette_and_histo_gan_amd.tf_compat import tf
    assert tf.keras.optimizers.schedules.CosineDecay is SCH.CosineDecay and tf.keras.optimizers.Adam is Adam


# ---------------------------------------------------------------------------------------------------------------- global norm
@pytest.mark.parametrize("n", [1, 5, 1023, 1025, 4 * 256 * 1024 + 4 * 256 + 3])
def test_float32_sum_of_squares_stays_within_the_bound_of_its_order(n):
    """gradients over 6 decades of magnitude; the bound follows from the documented order (optimizer_oracle.sumsq_error_bound):
    (longest serial chain + tree depth + 2) * 2^-24 relative to the float64 sum"""
    rng = np.random.default_rng(n)
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 0, size=n)).astype(np.float32)
    chain, depth, bound = OO.sumsq_error_bound(n)
    parts = OO.sumsq_partials(g)
    total = float(OO.global_sumsq([parts]))
    exact = float((g.astype(np.float64) ** 2).sum())
    err = abs(total - exact) / exact
    print(f"n {n}: chain {chain} depth {depth} bound {bound:.3e} measured {err:.3e}")
    assert parts.size == OO.sumsq_grid(n)[1]
    assert err <= bound, (total, exact, bound)


def test_norm_restatement_order_hole_and_scale():
    rng = np.random.default_rng(1)
    g = rng.normal(size=4099).astype(np.float32)
    h = g.copy()
    h[1001:2050] = 0.0
    assert np.array_equal(OO.sumsq_partials(g, 1001, 2050), OO.sumsq_partials(h))             # a hole is a run of zeros
    norm = OO.global_norm([OO.sumsq_partials(g)])
    assert norm.dtype == np.float32 and abs(float(norm) - np.linalg.norm(g.astype(np.float64))) < 1e-3
    assert OO.clip_scale(norm, norm) == 1.0 and OO.clip_scale(norm, 2 * norm) == 1.0          # exactly 1 at and below the threshold
    assert OO.clip_scale(norm, 0.5 * norm) == np.float32(0.5)
    assert np.isnan(OO.clip_scale(np.float32(np.inf), 1.0)) and np.isnan(OO.clip_scale(np.float32(np.nan), 1.0))
    # fma32 is ONE rounding: a case where rounding the float64 sum first gives the other float32
    a, b, c = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(2.0 ** -54)
    assert OO.fma32(a, b, c) == np.float32(1 + 2 ** -11 + 2 ** -23) and (np.float64(a) * np.float64(b)).astype(np.float32) == np.float32(1 + 2 ** -11)


# ---------------------------------------------------------------------------------------------------------------- constructor
def test_adam_constructor_refusals_and_settings():
    for kw in ({"clipnorm": 1.0}, {"weight_decay": 1e-2}, {"amsgrad": True}):
        with pytest.raises(NotImplementedError, match="supported: learning_rate"):
            Adam(2e-4, **kw)
    with pytest.raises(ValueError, match="disagree"):
        Adam(2e-4, clipvalue=1.0, global_clipnorm=1.0)
    for kw in ({"clipvalue": 0.0}, {"clipvalue": -1.0}, {"global_clipnorm": 0.0}, {"global_clipnorm": -2.0}):
        with pytest.raises(ValueError, match="positive"):
            Adam(2e-4, **kw)
    with pytest.raises(TypeError):
        Adam("fast")
    with pytest.raises(TypeError):
        Adam(2e-4, nesterov=True)
    o = Adam(SCH.LinearDecay(2e-4, 2, 2), beta_1=0.5, global_clipnorm=1.0, amsgrad=False)
    assert o.learning_rate == SCH.LinearDecay(2e-4, 2, 2) and o.global_clipnorm == 1.0 and o.clipvalue is None
    assert o.last_global_norm is None and o.iterations == 0 and o.current_learning_rate() == 2e-4
    o.clipvalue = None
    with pytest.raises(ValueError):
        o.clipvalue = 0.5                   # beside global_clipnorm
    assert o.clipvalue is None
    assert o.get_config()["learning_rate"].startswith("LinearDecay(") and o.get_config()["beta_1"] == 0.5


# ---------------------------------------------------------------------------------------------------------------- launch lists
def _step_calls(configure=None, dtype="bf16", B=4):
    """[(name, ctypes arguments)] of the second fused step of a meta-device engine whose optimizers `configure` has set"""
    c = SL.Census("baseline", 64, dtype)
    if configure is not None:
        configure(c.eng)
    c.launches(B)
    return list(c.log), c.eng


def _names(calls):
    return [n for n, _ in calls]


def test_default_optimizers_issue_none_of_the_new_entry_points():
    calls, eng = _step_calls()
    names = _names(calls)
    assert not any(n in NEW for n in names)
    assert names.count("p2p_adam_tick") == 2 and sum(n in ADAM for n in names) == 2       # G, D (no early head off a GPU)
    # ... argument for argument: the tick takes each store's own rate and betas, the flat launches a by-value scale of 1
    for n, a in calls:
        if n == "p2p_adam_tick":
            assert [SL.val(x) for x in a[2:5]] == [np.float32(2e-4), 0.5, np.float32(0.999)]
        if n in ADAM:
            assert a[-2 if "ema" not in n else -5] == 1.0


def test_each_option_adds_exactly_its_launches():
    sched = SCH.LinearDecay(2e-4, 2, 2)
    calls, eng = _step_calls(lambda e: e.set_optimizer(e.G, learning_rate=sched))
    names = _names(calls)
    assert names.count("p2p_adam_tick_sched") == 1 and names.count("p2p_adam_tick") == 1
    assert not any(n in NEW[1:] for n in names) and sum(n in ADAM for n in names) == 2
    s = SL.val(next(a for n, a in calls if n == "p2p_adam_tick_sched")[2])
    assert s is eng.G.opt.sched and (s.kind, s.hold_steps, s.decay_steps) == (5, 2.0, 2.0)

    calls, eng = _step_calls(lambda e: e.set_optimizer(e.G, clipping=(0.01, None)))
    names = _names(calls)
    assert names.count("p2p_adam_step") == 1 and sum(n in ADAM for n in names) == 2        # G; D as before
    assert not any(n in NEW[:3] for n in names)
    for a in (SL.val(a[0]) for n, a in calls if n == "p2p_adam_step"):
        assert not a.gscale_dev and a.hyper.contents.clipvalue == np.float32(0.01)

    calls, eng = _step_calls(lambda e: e.set_optimizer(e.G, clipping=(None, 1.0)))
    names = _names(calls)
    assert [n for n in names if n in NEW or n in ADAM] == ["p2p_sumsq_partials", "p2p_clip_scale", "p2p_adam_step",
                                                            next(n for n in names[::-1] if n in ADAM)]
    assert names[-1] != "p2p_adam_step" and names.count("p2p_adam_tick") == 2
    a = SL.val(next(a for n, a in calls if n == "p2p_adam_step")[0])
    assert a.n == eng.G.numel and a.gscale_dev and a.hyper.contents.clipvalue == 0.0
    n_, ex_lo, ex_hi = (int(x) for x in next(a for n, a in calls if n == "p2p_sumsq_partials")[1:4])
    assert n_ == eng.G.numel and (ex_lo, ex_hi) == (a.ex_lo, a.ex_hi)

    calls, eng = _step_calls(lambda e: [e.set_optimizer(s, clipping=(None, 0.5)) for s in (e.G, e.D)])
    order = [n for n in _names(calls) if n in NEW or n in ADAM]
    assert order == ["p2p_sumsq_partials", "p2p_clip_scale", "p2p_adam_step"] * 2
    # for a clipped generator no Adam launch precedes the norm
    first = _names(calls).index("p2p_clip_scale")
    assert not any(n in ADAM for n in _names(calls)[:first])


def test_clipping_is_refused_with_the_fused_adam():
    c = SL.Census("baseline", 64, "bf16")
    c.eng.fuse_adam = True
    with pytest.raises(ValueError, match="fuse_adam"):
        c.eng.set_optimizer(c.eng.G, clipping=(None, 1.0))
    c.eng.set_optimizer(c.eng.D, learning_rate=SCH.CosineDecay(2e-4, 100), beta1=0.0)         # schedules only touch the tick
    c.launches(4)
    names = _names(c.log)
    assert names.count("p2p_adam_tick_sched") == 1 and "p2p_adam_prep_batched" in names


def test_engine_properties_set_both_networks_and_stores_differ():
    c = SL.Census("baseline", 64, "f32")
    eng = c.eng
    eng.lr, eng.beta1 = 5e-4, 0.6
    for s in (eng.G, eng.D):
        assert s.opt.lr.value == np.float32(5e-4) and s.opt.b1.value == s.opt.hyper.beta1 == np.float32(0.6)
    eng.set_optimizer(eng.D, learning_rate=4e-4, beta1=0.0)
    assert eng.lr == np.float32(5e-4) and eng.D.opt.lr.value == np.float32(4e-4) and eng.D.opt.hyper.beta1 == 0.0
    assert eng.G.opt.b1 is not eng.D.opt.b1
    eng.ema_decay = 0.99
    assert eng.G.opt.hyper.ema_decay == np.float32(0.99) == eng.ema_decay


def test_replay_key_separates_what_changes_the_call_list(monkeypatch):
    c = SL.Census("baseline", 64, "bf16")
    eng = c.eng
    monkeypatch.setattr(eng, "device", torch.device("cuda:0"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(cuda_stream=0, stream_id=0))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)

    def key():
        k = eng._replay_key("rgba", 4, None, None, True)
        assert k is not None
        return k
    keys = [key()]
    eng.lr, eng.beta2 = 1e-3, 0.9                    # values are slots: the same recording
    assert key() == keys[0]
    for setting in ({"learning_rate": SCH.ExponentialDecay(1e-3, 10, 0.9)}, {"clipping": (0.1, None)}, {"clipping": (None, 0.1)}):
        for store in (eng.G, eng.D):
            eng.set_optimizer(store, **setting)
            keys.append(key())
            eng.set_optimizer(store, learning_rate=SCH.CosineDecay(1e-3, 10) if "learning_rate" in setting else None,
                              clipping=(0.2, None) if setting.get("clipping", (None,))[0] else
                              (None, 0.2) if "clipping" in setting else None)
            assert key() == keys[-1]                 # another schedule object or threshold: still the same recording
            eng.set_optimizer(store, learning_rate=2e-4, clipping=(None, None))
            assert key() == keys[0]
    assert len(set(keys)) == len(keys) == 7
