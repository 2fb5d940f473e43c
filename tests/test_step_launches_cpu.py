"""The float64 references of tests/test_step_launches_gpu.py (tests/step_launches.py) against the oracle's convolutions, and the
host-only census of the kernel variants a train step takes at every batch against the batches the GPU tests run."""
import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from tests import step_launches as SL


@pytest.mark.parametrize("n,lh,cg,cd,stride", [(3, 4, 5, 7, 2), (2, 5, 3, 6, 1), (2, 1, 4, 3, 2), (1, 8, 2, 2, 1)])
def test_tap_form_equals_the_oracle_convolutions(n, lh, cg, cd, stride):
    rng = np.random.default_rng(3)
    hi = rng.normal(size=(n, stride * lh, stride * lh, cg))
    lo = rng.normal(size=(n, lh, lh, cd))
    w = rng.normal(size=(4, 4, cg, cd))
    hi_t = torch.tensor(hi, requires_grad=True)
    w_t = torch.tensor(w, requires_grad=True)
    g = rg.conv4x4_s2(hi_t, w_t) if stride == 2 else rg.conv4x4_s1_bias(hi_t, w_t, None)
    (g * torch.tensor(lo)).sum().backward()
    np.testing.assert_allclose(SL.conv_g(hi, w, stride), g.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(SL.conv_p(lo, w, stride), hi_t.grad.numpy(), rtol=1e-12, atol=1e-12)
    old = SL.CHUNK
    try:
        SL.CHUNK = 2                 # several chunks
        np.testing.assert_allclose(SL.conv_w(hi, lo, stride), w_t.grad.numpy(), rtol=1e-12, atol=1e-12)
    finally:
        SL.CHUNK = old


def test_norm_act_equals_the_oracle_block():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(2, 4, 4, 6)) * 2 + 0.3
    gamma, beta = 1 + 0.2 * rng.normal(size=6), 0.2 * rng.normal(size=6)
    mask = rng.integers(0, 2, size=x.shape)
    want = rg.leaky_relu(rg.dropout(rg.instance_norm(torch.tensor(x), torch.tensor(gamma), torch.tensor(beta)),
                                    torch.tensor(mask, dtype=torch.float64))).numpy()
    np.testing.assert_allclose(SL.norm_act(x, gamma, beta, rg.IN_EPS, 1, rg.LEAKY_ALPHA, mask), want, rtol=1e-12, atol=1e-12)


def test_pooled_moments_and_image_set():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(3, 64, 5))          # 3 images, 64 pixels, 5 channels; 4 slots of 16 pixels
    parts = x.reshape(3, 4, 16, 5)
    sp = np.stack([parts.mean(axis=2), ((parts - parts.mean(axis=2, keepdims=True)) ** 2).sum(axis=2)], axis=-1)
    mean, var = SL.pooled_moments(sp, 16)
    np.testing.assert_allclose(mean, x.mean(axis=1), rtol=1e-12)
    np.testing.assert_allclose(var, x.var(axis=1), rtol=1e-12)
    s = SL.image_set(256)
    assert {0, 255, 3, 4, 63, 64, 127, 128, 191, 192}.issubset(s) and len(s) < 40
    assert SL.image_set(1) == [0]


def test_moment_err_is_per_image_and_channel():
    rng = np.random.default_rng(6)
    x = rng.normal(size=(3, 4, 4, 2)) * [1.0, 100.0]
    m, v = x.mean(axis=(1, 2)), x.var(axis=(1, 2))
    assert SL.moment_err(m, v, x) < 1e-12
    m2 = m.copy()
    m2[1, 0] += 0.01 * np.sqrt(v[1, 0])          # small next to the other channel's scale, 1 % of this channel's deviation
    assert abs(SL.moment_err(m2, v, x) - 0.01) < 1e-9


def test_keras_adam_equals_the_oracle_restatement():
    from oracle import np_restatement as npr
    rng = np.random.default_rng(7)
    n = 257
    p = rng.normal(size=n) * 0.02
    g = rng.normal(size=n) * 10.0 ** rng.integers(-8, 1, size=n)
    g[::17] = 0.0
    m, v = rng.normal(size=n) * 1e-3, rng.random(size=n) * 1e-4
    for t in (1, 3, 50):
        want = npr.keras_adam_step(p, g, m, v, t, lr=2e-4, b1=0.5, b2=0.999, eps=1e-7)
        got = SL.keras_adam(p, g, m, v, t, 2e-4, 0.5, 0.999, 1e-7)
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)


def test_dropout_mask_restatement_is_splitmix64():
    # the first output of SplitMix64 seeded with 0 is 0xE220A8397B1DCDAF: bit 3 of its bytes, lowest first
    assert SL.dropout_mask(8, 0, 0, 0).tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    z = 0xE220A8397B1DCDAF
    assert [(z >> (8 * k + 3)) & 1 for k in range(8)] == [1, 1, 1, 1, 1, 1, 0, 0]
    # the call counter, the seed and the element group enter the generator's state linearly: group g of (seed, counter) is the
    # first group of the state shifted by g, and a tail shorter than 8 is a prefix
    full = SL.dropout_mask(8 * 5, 1234, 16 * 7 + 3, 40)
    assert np.array_equal(SL.dropout_mask(8, 1234, 16 * 7 + 3, 43), full[24:32])
    assert np.array_equal(SL.dropout_mask(37, 1234, 16 * 7 + 3, 40), full[:37])
    m = SL.dropout_mask(1 << 16, 5, 9)
    assert set(np.unique(m).tolist()) == {0, 1} and abs(m.mean() - 0.5) < 0.01


def test_bf16_round_matches_torch_at_ties():
    # values exactly halfway between two bfloat16 numbers, with even and odd lower neighbours, and their neighbours
    hi = np.arange(0x3F80, 0x3F90, dtype=np.uint32) << 16
    ties = (hi | 0x8000).view(np.float32)
    near = np.concatenate([ties, (hi | 0x7FFF).view(np.float32), (hi | 0x8001).view(np.float32), -ties,
                           np.float32([0.0, -0.0, 1e-40, 3.0e38, 1.0, -2.5])])
    want = torch.as_tensor(near).to(torch.bfloat16).float().numpy()
    assert np.array_equal(SL.bf16_round(near).view(np.uint32), want.view(np.uint32))
    rng = np.random.default_rng(8)
    x = (rng.normal(size=4096) * 10.0 ** rng.integers(-6, 6, size=4096)).astype(np.float32)
    assert np.array_equal(SL.bf16_round(x).view(np.uint32), torch.as_tensor(x).to(torch.bfloat16).float().numpy().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- census
CASES = sorted(SL.CASE_RULES)
_COVERAGE = {}


def _coverage(case, batches=None):
    """the census of a case over B = 1 .. 512, computed once per (case, batch list)"""
    batches = SL.OFF_BENCH_BATCHES[case] if batches is None else tuple(batches)
    if (case, batches) not in _COVERAGE:
        _COVERAGE[(case, batches)] = SL.coverage(case, batches)
    return _COVERAGE[(case, batches)]


def _problems(case, batches):
    """what keeps a batch list from satisfying the coverage condition of a case (empty: satisfied)"""
    rule = SL.CASE_RULES[case]
    below, missing, above, first = _coverage(case, batches)
    out = []
    if not set(rule["required"]) <= set(batches):
        out.append(f"required batches missing: {sorted(set(rule['required']) - set(batches))}")
    if max(batches) > rule["cap"]:
        out.append(f"batch {max(batches)} is above the cap {rule['cap']}")
    if missing:
        out.append(f"{len(missing)} variant classes no tested batch produces, e.g. first at B={first[missing[0]]}: "
                   f"{SL.describe_key(missing[0])}")
    if len(above) > rule["above_cap_max"]:
        out.append(f"{len(above)} classes first appear above the cap, {rule['above_cap_max']} when the list was written")
    return out


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_off_benchmark_batches_reach_every_variant_class_below_the_cap(case):
    """Every variant class (step_launches.variant_key) that the engine's own dry run produces for any batch from 1 to the cap is
    produced by a batch of OFF_BENCH_CASES or by the case's bench config, the required batches are in the list, and the classes
    that first appear above the cap are listed and their number is bounded."""
    rule, batches = SL.CASE_RULES[case], SL.OFF_BENCH_BATCHES[case]
    below, missing, above, first = _coverage(case, batches)
    print(f"\n[{' '.join(map(str, case))}] {len(below)} variant classes up to batch {rule['cap']}, covered by:")
    for k in sorted(below, key=lambda k: (below[k] or 0, repr(k))):
        print(f"  B={below[k]!s:>4s}  {SL.describe_key(k)}")
    print(f"  {len(above)} classes first appear above the cap (upper side covered by the bench batches {rule['bench']}):")
    for k in sorted(above, key=lambda k: (above[k], repr(k))):
        print(f"  first at B={above[k]:4d}  {SL.describe_key(k)}")
    problems = _problems(case, batches)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("case,batch,uncovers", [(("baseline", 64, "bf16"), 17, False), (("baseline", 64, "bf16"), 6, True),
                                                 (("baseline", 64, "f32"), 33, True)])
def test_coverage_condition_notices_a_dropped_batch(case, batch, uncovers):
    """Without one of its required batches a list no longer satisfies the condition of the test above.  Without 6 (bf16) or 33
    (f32) the census itself finds variant classes that nothing else reaches.  Without 17 it does not: every class 17 produces is
    also produced by another batch of the list (test_variant_key_drops_the_batch_and_keeps_the_plan shows that 16 and 17 differ),
    and 17 stays in the list only because the rules of the case require both sides of the split-K step -- that case shows no
    more than that the required batches are enforced."""
    rest = tuple(b for b in SL.OFF_BENCH_BATCHES[case] if b != batch)
    problems = _problems(case, rest)
    print(f"\n  without B={batch}: " + "; ".join(problems))
    assert any(p.startswith("required batches missing") for p in problems)
    assert any("no tested batch produces" in p for p in problems) == uncovers


def test_variant_key_drops_the_batch_and_keeps_the_plan():
    """two batches on the same side of every threshold give one key set; a split-K step gives another"""
    c = SL.Census("baseline", 64, "bf16")
    k = {B: c.variant_keys(B) for B in (40, 56, 16, 17)}
    assert k[40] == k[56], "batches 40 and 56 (both N % 8 == 0, between the split-K steps at 32 and 64) differ"
    assert k[16] != k[17], "the split-K target step at B <= 16 changes no variant key"
    names = {key[0] for key in k[40]}
    assert {"p2p_igemm", "p2p_wgemm", "p2p_wgrad_small", "p2p_norm_act_fwd", "p2p_norm_act_bwd", "p2p_conv_fewin"} <= names


# ---------------------------------------------------------------------------------------------------------------- switch table
def test_every_switch_of_the_table_is_in_the_replay_key():
    """A recorded step holds its kernel choices by value, so every entry of engine.SWITCHES must change the switch part of the
    replay key when it is flipped to another legal value; the same settings give the same key."""
    import inspect
    from palette_and_histo_gan_amd import engine as E
    eng = SL.Census("baseline", 64, "bf16").eng
    assert "_SWITCH_VALUES(self)" in inspect.getsource(E.Pix2PixEngine._replay_key)
    base = E._SWITCH_VALUES(eng)
    assert len(base) == len(E.SWITCHES) and E._SWITCH_VALUES(eng) == base
    for attr, _, default, _ in E.SWITCHES:
        obj, name = E._switch_holder(eng, attr)
        old = getattr(obj, name)
        assert type(old) is type(default), attr
        setattr(obj, name, (not old) if isinstance(old, bool) else (1 - old if old in (0, 1) else 2 * old))
        try:
            assert E._SWITCH_VALUES(eng) != base, f"flipping {attr} leaves the replay key as it was"
        finally:
            setattr(obj, name, old)
    assert E._SWITCH_VALUES(eng) == base


def test_engine_reads_the_environment_only_through_the_switch_table():
    """one read of the environment in engine.py: the loop over the table in Pix2PixEngine.__init__"""
    import inspect
    from palette_and_histo_gan_amd import engine as E
    assert inspect.getsource(E).count("os.environ") == 1 and "getenv" not in inspect.getsource(E)
    init = inspect.getsource(E.Pix2PixEngine.__init__)
    loop = init.index("for attr, env, default, parse in SWITCHES + GATES:")
    assert loop < init.index("os.environ") < init.index("setattr(obj, name", loop)
