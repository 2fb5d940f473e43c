"""Not-gpu tests of the indexed model's loss hooks: CategoricalCrossentropy follows Keras' cached-logits rule (a probabilities
tensor that carries `_keras_logits` is evaluated on those logits), and the C ABI of the softmax VJP matches its binding."""
import os
import re

import numpy as np
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import pix2pix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=3, B=2, S=5, Cn=256):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, S, S, Cn), generator=g, dtype=torch.float32) * 3.0
    z[0, 0, 0] = torch.linspace(-30.0, 30.0, Cn)         # a row whose low classes underflow below 1e-7
    t = torch.randint(0, Cn, (B, S, S), generator=g)
    t[0, 0, 0] = 0                                       # target probability ~ exp(-60)
    onehot = torch.nn.functional.one_hot(t, Cn).float()
    return z, onehot


def test_cce_on_probabilities_with_cached_logits_is_the_log_softmax_form():
    z, onehot = _case()
    assert float(torch.softmax(z, -1)[0, 0, 0, 0]) < 1e-7
    cce = M.CategoricalCrossentropy()
    zl = z.clone().requires_grad_(True)
    p = torch.softmax(z, -1).requires_grad_(True)
    p._keras_logits = zl
    got = cce(onehot, p)
    want = -(onehot.double() * torch.log_softmax(z.double(), -1)).sum(-1).mean()
    assert abs(got.item() - want.item()) <= 1e-6 * want.item()
    # the uncapped pixel alone is worth ~60 / 50 over the mean: the clipped fallback caps it at -log 1e-7 = 16.1
    fallback = cce(onehot, torch.softmax(z, -1))
    assert got.item() - fallback.item() > (60.0 - 16.2) / 50.0
    assert torch.equal(cce(onehot, p), cce(onehot, None, logits=zl))
    # autograd reaches the logits leaf, not the probabilities leaf
    got.backward()
    assert p.grad is None and zl.grad is not None
    zd = z.double().requires_grad_(True)
    (-(onehot.double() * torch.log_softmax(zd, -1)).sum(-1).mean()).backward()
    assert torch.allclose(zl.grad.double(), zd.grad, atol=1e-8)


def test_cce_without_the_attribute_is_unchanged():
    z, onehot = _case(seed=4)
    p = torch.softmax(z, -1)
    q = p / p.sum(-1, keepdim=True)
    want = -(onehot * q.clamp(1e-7, 1.0 - 1e-7).log()).sum(-1).mean()
    cce = M.CategoricalCrossentropy()
    assert torch.equal(cce(onehot, p), want)
    # a tensor derived from the probabilities loses the attribute, as in Keras
    leaf = p.clone().requires_grad_(True)
    leaf._keras_logits = z.clone().requires_grad_(True)
    derived = leaf * 1
    assert not hasattr(derived, "_keras_logits")
    assert torch.equal(cce(onehot, derived).detach(), want)
    cce(onehot, derived).backward()
    assert leaf.grad is not None and leaf._keras_logits.grad is None
    assert torch.equal(cce(onehot, np.asarray(p)), want)


def test_softmax_bwd_declaration_matches_the_binding():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pgan.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+p2p_softmax_bwd\s*\(([^)]*)\)\s*;", text)
    assert m, "p2p_softmax_bwd is not declared in include/p2pgan.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(L.SIGNATURES["p2p_softmax_bwd"]) == 11
    assert L.SIGNATURES["p2p_softmax_bwd"][8] is L._f and "float scale" in args[8]
    src = open(os.path.join(ROOT, "palette_and_histo_gan_amd", "csrc", "replay.hip")).read()
    assert "P2P_E(p2p_softmax_bwd)" in src
