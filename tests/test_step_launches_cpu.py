"""The float64 references of tests/test_step_launches_gpu.py (tests/step_launches.py) against the oracle's convolutions."""
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
