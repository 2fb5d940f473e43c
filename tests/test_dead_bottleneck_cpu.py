"""The premise of Pix2PixEngine.elide_dead_bottleneck, without a GPU: in the f64 restatement of the reference graph the encoder
block that normalises a 1x1 map receives no gradient for its kernel and its gamma -- exactly 0.0, for random weights, inputs and
dropout masks -- while its beta stays live; and the engine's own launch list (dry run on device 'meta', tests/step_launches.py)
drops that block's GEMMs with the switch on and nothing at 128x128."""
from collections import Counter

import numpy as np
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import engine as E
from tests import step_launches as SL

F64 = torch.float64


def _dead_block(S):
    """name of the encoder block whose output map is 1x1 under InstanceNorm (found by shape), or None"""
    for i in range(2, len(E.DOWN_FILTERS) + 1):
        if S // 2 ** i == 1:
            return f"down{i}"
    return None


def test_the_1x1_blocks_kernel_and_gamma_receive_exactly_zero_gradient_in_f64():
    B, S = 2, 64
    rng = np.random.default_rng(606)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, F64), rng)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S)
    masks = [torch.tensor(rng.integers(0, 2, size=s).astype(np.uint8), dtype=F64) for s in rg.dropout_mask_shapes(B, S)]
    ref = rg.train_step_rgba(Gp, Dp, torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64), masks, lambda_l1=100.0)
    name = _dead_block(S)
    assert name is not None and tuple(Gp[name + ".kernel"].shape) == (4, 4, 512, 512)
    g = ref["g_grads"]
    assert torch.count_nonzero(g[name + ".kernel"]) == 0, "the kernel of the 1x1 block has a gradient"
    assert torch.count_nonzero(g[name + ".gamma"]) == 0, "the gamma of the 1x1 block has a gradient"
    assert float(g[name + ".beta"].abs().max()) > 0.0, "the beta of the 1x1 block is dead too: the test shows nothing"
    # every other kernel is live: the zeros above are the block's, not the case's
    assert all(float(v.abs().max()) > 0.0 for k, v in g.items() if k.endswith(".kernel") and k != name + ".kernel")


def _launches(S, B, level, model="baseline"):
    census = SL.Census(model, S, "bf16")
    census.eng.elide_dead_bottleneck = level
    return [(name, tuple(d for d in dec[:8] if isinstance(d, int))) for name, dec in census.launches(B)]


GEMMS = ("p2p_igemm", "p2p_igemm_norm_act", "p2p_wgemm")


def test_the_engine_drops_the_dead_gemms_at_64_and_nothing_at_128():
    assert SL.Census("baseline", 64, "bf16").eng._dead == 6 and SL.Census("baseline", 128, "bf16").eng._dead is None
    for model in ("baseline", "indexed"):
        off, on, two = (_launches(64, 3, lvl, model) for lvl in (0, 1, 2))
        gemms = {lvl: [c for c in calls if c[0] in GEMMS] for lvl, calls in ((0, off), (1, on), (2, two))}
        gone = list((Counter(gemms[0]) - Counter(gemms[1])).elements())
        # the forward and data-gradient p2p_igemm (op 0 / 1) and the p2p_wgemm of the 1x1 block: (.., N, 1, 1, 512, 512); the first
        # decoder block works at the same shape and keeps its three
        assert sorted(n for n, _ in gone) == ["p2p_igemm", "p2p_igemm", "p2p_wgemm"], gone
        assert sorted(a[0] for n, a in gone if n == "p2p_igemm") == [0, 1], gone
        assert all(a[-4:] == (1, 1, 512, 512) for _, a in gone), gone
        assert len(gemms[1]) == len(gemms[0]) - 3 and gemms[2] == gemms[1]
        # level 1 keeps both normalisation launches of the block (on a dense zero map), level 2 replaces them
        norms = {lvl: [c for c in calls if c[0].startswith("p2p_norm_act") and c[1][1:5] == (3, 1, 1, 512)] for lvl, calls in ((0, off), (1, on), (2, two))}
        assert len(norms[0]) == len(norms[1]) == 2 and norms[2] == [], norms
    assert _launches(128, 1, 0) == _launches(128, 1, 1) == _launches(128, 1, 2)
