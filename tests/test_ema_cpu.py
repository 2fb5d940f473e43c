"""The averaged generator without a GPU: the NumPy restatement of its recurrence (tests/ema_oracle.py, what
tests/test_ema_gpu.py holds the kernels to bit for bit) against closed forms, and the engine's launch list with averaging on
against off (dry run on device 'meta', tests/step_launches.py)."""
import numpy as np
import pytest

from tests import ema_oracle as EO
from tests import step_launches as SL


def test_a_constant_parameter_leaves_the_average_where_it_is_bit_for_bit():
    rng = np.random.default_rng(1)
    p = (rng.normal(size=1000) * 0.02).astype(np.float32)
    p[:3] = [0.0, np.float32(1e-40), -3.0]          # a zero and a denormal
    for warmup in (True, False):
        e = p.copy()
        for t in range(1, 30):
            e = EO.ema_step(e, p, t, 0.999, warmup)
            assert e.dtype == np.float32 and np.array_equal(e.view(np.int32), p.view(np.int32))
    # the one value whose bits move: -0 + (+0) is +0 in IEEE arithmetic -- equal as a number, and no initialiser draws it
    z = EO.ema_step(np.float32([-0.0]), np.float32([-0.0]), 1)
    assert z[0] == 0.0 and not np.signbit(z[0])


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_without_warmup_the_average_approaches_a_constant_geometrically(decay):
    """e_k = p + d^k (e_0 - p), run in f64: to f64 rounding (a few ulp per step of the quantities' size)"""
    rng = np.random.default_rng(2)
    p, e0 = rng.normal(size=257), rng.normal(size=257)
    e = e0.copy()
    for k in range(1, 201):
        e = EO.ema_step(e, p, k, decay, warmup=False, dtype=np.float64)
        want = p + decay ** k * (e0 - p)
        assert np.abs(e - want).max() <= 4 * k * np.finfo(np.float64).eps * np.abs(np.concatenate([p, e0])).max()
    assert np.abs(e - p).max() < np.abs(e0 - p).max() * decay ** 199


def test_beta_t_follows_the_warmup_ramp_and_then_the_cap():
    f = np.float32
    for t in (1, 2, 9, 10, 8991, 8992):
        b = EO.beta_t(t, 0.999, True)
        assert type(b) is np.float32
        ramp = (f(1) + f(t)) / (f(10) + f(t))
        assert b == min(f(0.999), ramp)
        assert abs(float(b) - min(0.999, (1 + t) / (10 + t))) < 1e-7
    assert [float(EO.beta_t(t)) for t in (1, 2, 9, 10)] == [float(f(2) / f(11)), float(f(3) / f(12)), float(f(10) / f(19)), float(f(11) / f(20))]
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990: the ramp below, the cap from there on
    assert float(EO.beta_t(8989)) < float(f(0.999)) and (1 + 8989) / (10 + 8989) < 0.999 <= (1 + 8990) / (10 + 8990)
    assert all(EO.beta_t(t) == f(0.999) for t in (8990, 8991, 8992, 100000))
    assert all(EO.beta_t(t, 0.999, False) == f(0.999) for t in (1, 10, 8992))
    assert EO.beta_t(3, 0.5, True) == f(4) / f(13) and EO.beta_t(30, 0.5, True) == f(0.5)


# ---------------------------------------------------------------------------------------------------------------- launch list
FUSED = {"p2p_adam_flat_dev": "p2p_adam_ema_flat_dev", "p2p_adam_flat_dev_excl": "p2p_adam_ema_flat_dev_excl"}


def _step_calls(census, B):
    census.launches(B)                     # leaves the second step's calls, every entry point, in census.log
    return [(name, args) for name, args in census.log]


@pytest.mark.parametrize("B", [4, 256])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_averaging_replaces_the_generators_adam_launches_and_adds_none(B, level):
    off, on = SL.Census("baseline", 64, "bf16"), SL.Census("baseline", 64, "bf16")
    off.eng.elide_dead_bottleneck = on.eng.elide_dead_bottleneck = level
    with SL._dry_run(on.log):
        on.eng.enable_ema()
    assert on.eng.ema_enabled and not off.eng.ema_enabled and off.eng.G.ema is None
    a, b = _step_calls(off, B), _step_calls(on, B)
    assert len(a) == len(b) > 60
    g_numel = off.eng.G.numel
    swapped = []
    for (na, xa), (nb, xb) in zip(a, b):
        if na == nb:
            assert len(xa) == len(xb)
            continue
        assert FUSED.get(na) == nb, (na, nb)
        swapped.append(na)
        # the same element count (and hole), with e and (t_dev, decay, warmup) added
        assert len(xb) == len(xa) + 4
        assert [int(v) for v in xa[4:-6]] == [int(v) for v in xb[5:-9]]
    adam_off = [(n, x) for n, x in a if n in FUSED]
    # both networks step through these entry points; the generator's launches cover its flat buffer once, the discriminator's stay
    d_launches = [n for n, x in adam_off if int(x[4]) == off.eng.D.numel]
    assert len(d_launches) == 1 and len(swapped) == len(adam_off) - 1 >= 1
    assert sum(int(x[4]) for n, x in adam_off) == g_numel + off.eng.D.numel
    assert ("p2p_adam_flat_dev_excl" in swapped) == (level == 2)
    assert not any(n == "p2p_ema_flat" for n, _ in b)
    # averaging off is today's list: nothing of the feature in it
    assert not any("ema" in n for n, _ in a)


def test_the_tiled_adam_path_gets_one_averaging_pass_of_its_own():
    on = SL.Census("baseline", 64, "bf16")
    on.eng.fuse_adam = True
    off_names = [n for n, _ in _step_calls(on, 4)]
    with SL._dry_run(on.log):
        on.eng.enable_ema(0.99, warmup=False)
    names = [n for n, _ in _step_calls(on, 4)]
    assert names.count("p2p_ema_flat") == 1 and [n for n in names if n != "p2p_ema_flat"] == off_names
    assert names.index("p2p_ema_flat") > max(i for i, n in enumerate(names) if n == "p2p_adam_prep_batched")
