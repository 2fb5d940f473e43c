"""tests/index_head_cases.py without a GPU: the generated inputs have the properties the GPU tests rely on (exact in both dtypes,
argmax of the f32 softmax = first maximum of the logits, enough tied pixels, exact lattice logits, saturated targets), and NumPy
restatements of three wrong kernels are caught on the tie cases -- which is how the cases prove that they can fail."""
import numpy as np
import pytest

from tests import index_head_cases as IC
from tests import step_launches as SL

# (C, the tie share the case must have).  C = 256 draws from 65 values: the maximum is unique with probability
# sum_i (1 - i / 65)^(C - 1) ~ 0.02 (C = 256), 0.28 (C = 100), 0.58 (C = 65); a tie needs two classes (C = 1: none).
# The tie cases (asserted share >= 1/2) are those with C >= 100.
CLASS_COUNTS = ((1, 0.0), (65, 0.3), (100, 0.5), (256, 0.5), (512, 0.5))
BIG = ((5, 58, 58, 100), (3, 210, 210, 256))          # the grid-stride cases of the two kernels


def _cases():
    for n, h, w in IC.SOFTMAX_SHAPES:
        for c, share in CLASS_COUNTS:
            yield n, h, w, c, share
    yield BIG[0] + (0.5,)


@pytest.mark.parametrize("n,h,w,c,share", list(_cases()), ids=lambda v: str(v))
def test_quarter_step_logits(n, h, w, c, share):
    z = IC.quarter_logits(n, h, w, c)
    assert z.dtype == np.float32 and z.shape == (n, h, w, c) and not z.flags.writeable
    assert np.array_equal(SL.bf16_round(z), z)                                         # exact in bf16
    k = z.astype(np.float64) * 4
    assert np.array_equal(k, np.rint(k)) and k.min() >= -IC.K_LIM and k.max() <= IC.K_LIM
    want = IC.first_max(z)
    # the f32 restatement of exp(z - max) / sum has the same first maximum as z on EVERY pixel, and equal logits equal probabilities
    p = IC.softmax_f32(z)
    assert np.array_equal(np.argmax(p, -1), want)
    assert np.array_equal(p == p.max(-1, keepdims=True), z == z.max(-1, keepdims=True))
    assert np.array_equal(IC.softmax_ref(z, IC.targets(n, h, w, c), 1.0)["idx"], want)
    tied = IC.tied_share(z)
    print(f"\n  {n}x{h}x{w}x{c}: tied share {tied:.3f}")
    if c == 1:
        assert tied == 0.0 and not want.any()
        return
    if c >= IC.TIE_CLASSES or n * h * w >= 67:       # (C = 65 is no tie case: its share is asserted where there are pixels to count)
        assert tied >= share, tied
    if share >= 0.5:            # a tie case: each wrong argmax is caught on at least 10 % of its pixels
        for wrong in (IC.argmax_ties_highest, IC.argmax_upper_half_preferred):
            miss = float((wrong(z) != want).mean())
            print(f"  {wrong.__name__}: differs on {miss:.3f}")
            assert miss >= 0.1, (wrong.__name__, miss)


def test_big_softmax_case_ties():
    """the one long case, on its first image only (the draws of the images are identically distributed)"""
    n, h, w, c = BIG[1]
    z = IC.quarter_logits(1, h, w, c, seed=1)
    assert IC.tied_share(z) >= 0.5
    assert float((IC.argmax_ties_highest(z) != IC.first_max(z)).mean()) >= 0.1
    assert n * h * w > 8192 * 16 and (n * h * w) % 16


def test_targets_walk_every_class_and_lane_position():
    t = IC.targets(2, 8, 64)
    assert t.shape == (2, 8, 64) and t.min() == 0 and t.max() == 255
    flat = t.reshape(-1)
    for a in range(0, flat.size - 255, 64):
        assert len(set(flat[a:a + 256])) == 256                  # every class within any 256 consecutive pixels
    # the fused kernel matches the target inside a lane at cr = 32 i + (e & 3) + 8 (e >> 2), e < 16, i < 4, for the channel base
    # 128 cw + 4 h: every (cw, h, i, e) occurs as a target
    seen = {(c >> 7, (c >> 2) & 1, (c >> 5) & 3, (c & 3) | (((c >> 3) & 3) << 2)) for c in flat}
    assert len(seen) == 2 * 2 * 4 * 16
    assert IC.targets(1, 1, 17, 100).max() < 100


@pytest.mark.parametrize("case", IC.HEAD_CASES, ids=lambda c: c.id)
def test_head_cases(case):
    x, w, bias, z, t = IC.head_operands(case)
    assert x.shape == (case.n, case.h, 64, 33) and w.shape == (4, 4, 33, 256) and z.shape == (case.n, case.h, 64, 256)
    assert case.h % 4 == 0 and (x != 0).all()
    zi = z / case.step
    assert np.array_equal(zi, np.rint(zi))
    # distinct logits differ by at least one step >= 2^-4, equal ones are equal bit for bit
    srt = np.sort(z, -1)
    gaps = np.diff(srt, axis=-1)
    assert case.step >= 2.0 ** -4 and (gaps[gaps > 0] >= case.step).all()
    want = IC.first_max(z)
    tied = IC.tied_share(z)
    sat = IC.saturated_share(z, t)
    print(f"\n  {case.id}: step {case.step:g}, logits std {zi.std() * case.step:.2f} ({zi.std():.1f} steps), max |z| {np.abs(z).max():g}, "
          f"tied share {tied:.4f}, saturated share {sat:.3f}")
    assert 60 < zi.std() < 80
    if case.name == "moderate":
        assert case.step in (2.0 ** -4, 2.0 ** -3) and sat == 0.0
        assert np.array_equal(np.argmax(IC.softmax_f32(z), -1), want)
    if case.name == "saturated":
        assert case.step == 1.0 and sat >= 0.5
        # wrong kernel 3: -log(p_t) of the underflowed f32 probability is inf on those pixels; the log-sum-exp reference is finite
        bad = IC.cce_from_probability_f32(z, t)
        ref = IC.softmax_ref(z, t, 1.0, want_probs=False)["cce"]
        assert np.isfinite(ref).all() and ref.max() > -IC.EXP_UNDERFLOW
        assert float(np.isinf(bad).mean()) >= 0.5 and not np.isfinite(bad.mean())
    if case.dup:
        assert tied == 1.0                                          # every pixel ties exactly
        src = IC.DUP_MAPS[case.dup](np.arange(256))
        assert np.array_equal(z, z[..., src]) and (src[want] == want).all()       # the winner is the lowest member of its group
        assert float((IC.argmax_ties_highest(z) != want).mean()) == 1.0
        for bit in IC.DUP_BITS[case.dup]:
            miss = float((IC.argmax_upper_half_preferred(z, bit) != want).mean())
            assert miss >= 0.1, (bit, miss)
            assert miss == 1.0
        # and a tie-break that is wrong at ANOTHER level is not what this case is for: the right answer there
        other = next(b for b in (1, 4, 32, 128) if b not in IC.DUP_BITS[case.dup] and not (case.dup == "fourway" and b == 64))
        print(f"  upper-half-preferred at bit {other}: differs on {float((IC.argmax_upper_half_preferred(z, other) != want).mean()):.4f}")


def test_wrong_kernels_agree_where_nothing_ties():
    """the restatements differ from the reference ONLY through their defect"""
    z = np.arange(24, dtype=np.float32).reshape(2, 12)[:, ::-1] / 4
    for wrong in (IC.argmax_ties_highest, IC.argmax_upper_half_preferred):
        assert np.array_equal(wrong(z), IC.first_max(z))
    assert np.array_equal(IC.argmax_upper_half_preferred(-z, 4), IC.first_max(-z))
    t = np.array([3, 7])
    np.testing.assert_allclose(IC.cce_from_probability_f32(z, t), IC.softmax_ref(z, t, 1.0)["cce"], rtol=1e-5)
    tie = np.array([[1.0, 3.0, 3.0, 0.0, 3.0, 1.0]], np.float32)
    assert IC.first_max(tie)[0] == 1 and IC.argmax_ties_highest(tie)[0] == 4 and IC.argmax_upper_half_preferred(tie)[0] == 4
    assert IC.argmax_upper_half_preferred(tie, 1)[0] == 1 and IC.argmax_upper_half_preferred(tie, 2)[0] == 2
