"""Not-gpu: the host side of the differentiable augmentation (diffaugment.draw_parameters, the validation of diff_augment and of a
hand-built parameter table) and self-checks of tests/diffaugment_oracle.py, the yardstick of tests/test_diffaugment_gpu.py."""
import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import diffaugment as A
from tests import diffaugment_oracle as O

F64 = torch.float64
ALL = "color,translation,cutout"


# ---------------------------------------------------------------------------------------------------- draw_parameters
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (7, 64, 64), (256, 128, 128), (5, 8, 20), (400, 7, 3)])
def test_drawn_tables_have_the_papers_ranges(B, H, W):
    p = A.draw_parameters(B, H, W, seed=3, step=11)
    assert p.color.dtype == torch.float32 and tuple(p.color.shape) == (B, 3) and p.color.device.type == "cpu"
    assert p.geometry.dtype == torch.int32 and tuple(p.geometry.shape) == (B, 4) and p.geometry.device.type == "cpu"
    assert (p.ch, p.cw) == (H // 2, W // 2) and p.batch == B
    b, s, k = p.color.numpy().T
    assert -0.5 <= b.min() and b.max() <= 0.5 and 0.0 <= s.min() and s.max() <= 2.0 and 0.5 <= k.min() and k.max() <= 1.5
    ty, tx, y0, x0 = p.geometry.numpy().T
    assert -(H // 8) <= ty.min() and ty.max() <= H // 8 and -(W // 8) <= tx.min() and tx.max() <= W // 8
    assert -(p.ch // 2) <= y0.min() and y0.max() <= H - p.ch + p.ch // 2
    assert -(p.cw // 2) <= x0.min() and x0.max() <= W - p.cw + p.cw // 2


def test_a_large_draw_reaches_both_ends_of_every_integer_range():
    p = A.draw_parameters(4096, 64, 32)
    ty, tx, y0, x0 = p.geometry.numpy().T
    assert (ty.min(), ty.max()) == (-8, 8) and (tx.min(), tx.max()) == (-4, 4)
    assert (y0.min(), y0.max()) == (-16, 48) and (x0.min(), x0.max()) == (-8, 24)
    b, s, k = p.color.numpy().T
    assert abs(b.mean()) < 0.02 and abs(s.mean() - 1.0) < 0.04 and abs(k.mean() - 1.0) < 0.02


def _same(p, q):
    return torch.equal(p.color, q.color) and torch.equal(p.geometry, q.geometry) and (p.ch, p.cw) == (q.ch, q.cw)


def test_the_draw_is_stateless():
    a = A.draw_parameters(6, 64, 64, seed=47, step=5)
    A.draw_parameters(9, 32, 32, seed=1, step=2)          # nothing in between moves it
    assert _same(a, A.draw_parameters(6, 64, 64, seed=47, step=5))
    assert not _same(a, A.draw_parameters(6, 64, 64, seed=47, step=6))
    assert not _same(a, A.draw_parameters(6, 64, 64, seed=48, step=5))
    assert _same(A.draw_parameters(6, 64, 64), A.draw_parameters(6, 64, 64, seed=A.SEED, step=0))


@pytest.mark.parametrize("policy", ["", "color", "cutout", "translation,color", "cutout, translation", ALL])
def test_the_policy_does_not_move_any_column(policy):
    assert _same(A.draw_parameters(5, 64, 48, policy, seed=9, step=4), A.draw_parameters(5, 64, 48, ALL, seed=9, step=4))


# ---------------------------------------------------------------------------------------------------- validation
def test_policy_names():
    assert A.POLICIES == ("color", "translation", "cutout")
    assert A.policy_bits("") == 0 and A.policy_bits(ALL) == 7 and A.policy_bits("cutout,color") == 5 and A.policy_bits(" translation ") == 2
    for bad in ("colour", "color,flip", "color translation"):
        with pytest.raises(ValueError, match="unknown augmentation"):
            A.policy_bits(bad)
        with pytest.raises(ValueError, match="unknown augmentation"):
            A.draw_parameters(2, 8, 8, bad)
        with pytest.raises(ValueError, match="unknown augmentation"):
            A.diff_augment(np.zeros((2, 8, 8, 4), np.float32), A.draw_parameters(2, 8, 8), bad)


def test_wrong_image_shapes_and_tables_are_refused_before_any_device_is_touched():
    p = A.draw_parameters(2, 8, 8)
    for shape in ((2, 8, 8, 3), (2, 8, 8, 1), (2, 8, 8), (2, 4, 8, 8, 4), (0, 8, 8, 4)):
        with pytest.raises(ValueError, match="RGBA"):
            A.diff_augment(np.zeros(shape, np.float32), p)
    with pytest.raises(ValueError, match="2 rows for a batch of 3"):
        A.diff_augment(np.zeros((3, 8, 8, 4), np.float32), p)
    with pytest.raises(ValueError, match="AugmentParameters"):
        A.diff_augment(np.zeros((2, 8, 8, 4), np.float32), (p.color, p.geometry))
    color, geometry = np.zeros((2, 3), np.float32), np.zeros((2, 4), np.int32)
    A.AugmentParameters(color, geometry, 4, 4)          # numpy tables of the right kind are taken
    for c, g, ch, cw in ((color[:, :2], geometry, 4, 4), (color, geometry[:, :3], 4, 4), (color[0], geometry, 4, 4),
                         (color.astype(np.float64), geometry, 4, 4), (color, geometry.astype(np.int64), 4, 4),
                         (color, geometry.astype(np.float32), 4, 4), (color[:1], geometry, 4, 4), (color, geometry, -1, 4),
                         (color, geometry, 4, 2.5)):
        with pytest.raises(ValueError):
            A.AugmentParameters(c, g, ch, cw)


# ---------------------------------------------------------------------------------------------------- the oracle
def _case(seed, B=2, H=4, W=6):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=(B, H, W, 4))
    g = rng.normal(size=(B, H, W, 4))
    color = np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(0, 2, B), rng.uniform(0.5, 1.5, B)], axis=1).astype(np.float32)
    geometry = np.array([[1, -2, -1, 2], [-1, 1, 2, -1]], np.int32)[:B]          # shifts both ways, boxes over three borders
    return x, g, color, geometry, H // 2, W // 2


def test_gradcheck_of_the_oracle():
    x, _, color, geometry, ch, cw = _case(1)
    xt = torch.tensor(x, dtype=F64, requires_grad=True)
    for policy in (ALL, "color"):
        assert torch.autograd.gradcheck(lambda t: O.diff_augment(t, color, geometry, ch, cw, policy), (xt,), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("policy", ["", "color", "translation", "cutout", "color,translation", "color,cutout", "translation,cutout", ALL])
def test_the_closed_form_vjp_equals_autograd_of_the_oracle(policy):
    x, g, color, geometry, ch, cw = _case(2, H=6, W=10)
    _, want = O.evaluate(x, g, color, geometry, ch, cw, policy, F64)
    got = O.vjp_closed_form(torch.tensor(g, dtype=F64), color, geometry, ch, cw, policy).numpy()
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    if "color" not in O.stages(policy):
        assert np.array_equal(got, want)


def test_identity_policy_and_neutral_rows_of_the_oracle():
    x, g, color, geometry, ch, cw = _case(3)
    xt = torch.tensor(x, dtype=F64)
    assert torch.equal(O.diff_augment(xt, color, geometry, ch, cw, ""), xt)
    neutral = np.array([[0.0, 1.0, 1.0]] * 2, np.float32)
    out = O.diff_augment(xt, neutral, geometry, ch, cw, "color")
    assert (out - xt).abs().max() < 1e-15 and torch.equal(out[..., 3], xt[..., 3])
    # order of the string does not matter; a shift of H or more leaves only fill; a box outside the image cuts nothing
    assert torch.equal(O.diff_augment(xt, color, geometry, ch, cw, "cutout,color"), O.diff_augment(xt, color, geometry, ch, cw, "color,cutout"))
    far = np.array([[4, 0, 0, 0], [0, -6, 0, 0]], np.int32)
    assert bool((O.diff_augment(xt, color, far, ch, cw, "translation", fill=-1.0) == -1.0).all())
    outside = np.array([[0, 0, 4, 0], [0, 0, -2, -3]], np.int32)
    assert torch.equal(O.diff_augment(xt, color, outside, ch, cw, "cutout"), xt)
    # one pixel by hand: image 0 moves down 1 and left 2, the box covers rows -1..0, columns 2..4
    out = O.diff_augment(xt, color, geometry, ch, cw, "translation,cutout")
    assert torch.equal(out[0, 1, 0], xt[0, 0, 2]) and torch.equal(out[0, 3, 3], xt[0, 2, 5])
    assert bool((out[0, 0] == -1.0).all()) and bool((out[0, :, 4:] == -1.0).all()) and bool((out[0, 1, 4] == -1.0).all())


def test_the_mean_of_v_is_the_mean_of_x_plus_b():
    """why one per-image sum of the raw input suffices: the saturation step keeps every pixel's channel mean"""
    x, _, color, _, _, _ = _case(4, B=2, H=5, W=7)
    xt = torch.tensor(x, dtype=F64)
    for i in range(2):
        b, s, k = (float(v) for v in color[i])
        u = xt[i, ..., :3] + b
        sbar = u.mean(-1, keepdim=True)
        v = (u - sbar) * s + sbar
        assert abs(float(v.mean()) - (float(xt[i, ..., :3].mean()) + b)) < 1e-15
        # and the contrast step keeps the image mean
        assert abs(float(((v - v.mean()) * k + v.mean()).mean()) - float(v.mean())) < 1e-15
