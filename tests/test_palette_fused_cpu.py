"""Not-gpu: the fused palette step's C ABI (p2p_palette_loss, p2p_soft_palette_tv_bwd, p2p_finish_losses2), the argument rules of
engine.train_step_rgba(palette=) and Pix2PixPaletteModel(fused=True), and the launches of the step captured on the meta device
(tests/step_launches.py): a step without `palette` issues what it issued before the keyword existed -- the list recorded then is
tests/golden/fused_palette_parent_launches.json, entry point and a hash of every argument but pointers -- and a palette step issues
those launches plus extract, forward (real), forward (fake), loss and backward."""
import ctypes
import hashlib
import json
import os
import re

import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import step_launches as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"p2p_palette_loss": 10, "p2p_soft_palette_tv_bwd": 14, "p2p_finish_losses2": 9}
TERMS = (50.0, 20.0, 5e-2)


def test_library_exports_the_fused_palette_entry_points_with_the_bound_signatures():
    if not os.path.exists(L.LIB_PATH):
        from palette_and_histo_gan_amd import build
        build.build_library(verbose=False)
    lib = ctypes.CDLL(L.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p2pgan.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/p2pgan.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(L.SIGNATURES[name]) == nargs, (name, args)
        for a, t in zip(args, L.SIGNATURES[name]):
            want = L._vp if "*" in a else (L._f if a.startswith("float") else L._i)
            assert t is want, (name, a, t)
        assert L.lib().p2p_replay_fn_nargs(L.lib().p2p_replay_fn_index(name.encode())) == nargs
    # the entry points that stay: same argument counts as before
    for name, nargs in {"p2p_palette_extract": 8, "p2p_soft_palette_fwd": 12, "p2p_soft_palette_bwd": 12, "p2p_finish_losses": 7}.items():
        assert len(L.SIGNATURES[name]) == nargs == L.lib().p2p_replay_fn_nargs(L.lib().p2p_replay_fn_index(name.encode()))


def test_host_side_refusals_carry_their_messages():
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(ctypes.byref(buf, (-ctypes.addressof(buf)) % 16), ctypes.c_void_p)
    err = lambda: lib.p2p_last_error()          # noqa: E731
    # p2p_palette_loss(B, K, h_real, h_fake, conf_fake, sizes, inv_batch, out_tv, out_conf, stream)
    assert lib.p2p_palette_loss(2, 8, None, p, p, p, 0.5, p, p, None) < 0 and b"p2p_palette_loss: null" in err()
    assert lib.p2p_palette_loss(2, 8, p, p, p, p, 0.5, p, None, None) < 0 and b"null" in err()
    assert lib.p2p_palette_loss(2, 257, p, p, p, p, 0.5, p, p, None) < 0 and b"K = 257" in err()
    assert lib.p2p_palette_loss(2, 0, p, p, p, p, 0.5, p, p, None) < 0 and b"K = 0" in err()
    assert lib.p2p_palette_loss(0, 8, p, p, p, p, 0.5, p, p, None) < 0 and b"batch" in err()
    # p2p_soft_palette_tv_bwd(N, H, W, img, palette, sizes, K, tau, h_real, h_fake, w_tv, w_conf, dimg, stream)
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, p, p, p, 8, 1e-3, None, p, 1.0, 1.0, p, None) < 0 and b"p2p_soft_palette_tv_bwd: null" in err()
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, None, p, p, 8, 1e-3, p, p, 1.0, 1.0, p, None) < 0 and b"null" in err()
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, p, p, p, 257, 1e-3, p, p, 1.0, 1.0, p, None) < 0 and b"257" in err()
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, p, p, p, 8, 0.0, p, p, 1.0, 1.0, p, None) < 0 and b"temperature" in err()
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, p, p, p, 8, -1.0, p, p, 1.0, 1.0, p, None) < 0 and b"temperature" in err()
    unaligned = ctypes.c_void_p(p.value + 4)
    assert lib.p2p_soft_palette_tv_bwd(1, 2, 2, p, p, p, 8, 1e-3, p, p, 1.0, 1.0, unaligned, None) < 0 and b"unaligned" in err()
    # p2p_finish_losses2(slots, aux_slot, aux2_slot, l1_slot, lambda_l1, lambda_aux, lambda_aux2, out, stream)
    assert lib.p2p_finish_losses2(None, 4, 5, 3, 1.0, 1.0, 1.0, p, None) < 0 and b"p2p_finish_losses2" in err()
    assert lib.p2p_finish_losses2(p, -1, 5, 3, 1.0, 1.0, 1.0, p, None) < 0 and b"p2p_finish_losses2" in err()


def test_fused_model_argument_rules():
    class OwnGeneratorLoss(M.Pix2PixPaletteModel):
        def generator_loss(self, fake_predicted, fake_image, real_image):
            return super().generator_loss(fake_predicted, fake_image, real_image)

    class OwnDiscriminatorLoss(M.Pix2PixPaletteModel):
        def discriminator_loss(self, real_predicted, fake_predicted):
            return super().discriminator_loss(real_predicted, fake_predicted)

    # refused by the constructor, before a dataset or a device is touched
    for cls, hook in ((OwnGeneratorLoss, "generator_loss"), (OwnDiscriminatorLoss, "discriminator_loss")):
        with pytest.raises(ValueError, match=rf"{cls.__name__}\.{hook} overrides the loss.*fused=False"):
            cls(None, None, "front2right", "palette-fused-test", 100.0, 1.0, fused=True)


def _engine(E, dtype=L.F32, S=64):
    return E.Pix2PixEngine(4, 4, "tanh", S, dtype, device="meta", seed=47)


def test_engine_argument_rules():
    log = []
    with SL._dry_run(log) as E:
        eng = _engine(E)
        log.clear()                                          # (the constructor prepares the weight copies)
        x = torch.empty((2, 64, 64, 4), dtype=torch.float32, device="meta")
        with pytest.raises(ValueError, match="mutually exclusive"):
            eng.train_step_rgba(x, x, 100.0, 1.0, palette=TERMS)
        with pytest.raises(ValueError, match="mutually exclusive"):
            eng.train_step_empty(100.0, lambda_hist=1.0, palette=TERMS)
        with pytest.raises(ValueError, match="temperature"):
            eng.train_step_rgba(x, x, 100.0, palette=(1.0, 1.0, 0.0))
        with pytest.raises(ValueError, match="lambda_palette, lambda_conformance, temperature"):
            eng.train_step_rgba(x, x, 100.0, palette=(1.0, 1e-3))
        assert not log                                       # refused before any launch
        idx = E.Pix2PixEngine(1, 256, "softmax", 64, L.BF16, device="meta", seed=47)
        with pytest.raises(ValueError, match="RGBA"):
            idx.train_step_empty(0.0, palette=TERMS)


def _captured(dtype_name, B, lam_hist=None, palette=None, S=64):
    """[(entry point, hash of its decoded arguments)] of the second step at batch B on the meta device"""
    log = []
    with SL._dry_run(log) as E:
        eng = _engine(E, L.BF16 if dtype_name == "bf16" else L.F32, S)
        for _ in range(2):
            log.clear()
            x = torch.empty((B, S, S, 4), dtype=torch.float32, device="meta")
            eng.train_step_rgba(x, x, 100.0, lam_hist, global_batch=B, palette=palette)
    blocks = [(SL._FAKE_BASE, 1 << 44)]
    out = []
    for name, args in log:
        sig = SL.signature(name, SL.decode(name, args, blocks))
        out.append([name, hashlib.sha1(repr(sig).encode()).hexdigest()[:12]])
    return out, log


GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "fused_palette_parent_launches.json")))
PALETTE_LAUNCHES = ["p2p_palette_extract", "p2p_soft_palette_fwd", "p2p_soft_palette_fwd", "p2p_palette_loss", "p2p_soft_palette_tv_bwd"]


@pytest.mark.parametrize("case", sorted(GOLD))
def test_a_step_without_palette_issues_the_launches_it_issued_before(case):
    dtype_name, B, lam_hist = case.split(":")
    got, _ = _captured(dtype_name, int(B), None if lam_hist == "None" else float(lam_hist))
    assert got == GOLD[case]


@pytest.mark.parametrize("case", [c for c in sorted(GOLD) if c.endswith(":None")])
def test_a_palette_step_adds_the_five_palette_launches_and_no_others(case):
    dtype_name, B, _ = case.split(":")
    B = int(B)
    got, log = _captured(dtype_name, B, palette=TERMS)
    assert [n for n, _ in got if n in PALETTE_LAUNCHES] == PALETTE_LAUNCHES
    rest = [(n, h) for n, h in got if n not in PALETTE_LAUNCHES]
    gold = GOLD[case]
    # what remains is the default step, launch for launch; three launches carry the palette terms in their arguments
    touched = {"p2p_tanh_l1_fwd_pair", "p2p_tanh_l1_fwd", "p2p_tanh_l1_bwd_pad8", "p2p_tanh_l1_bwd", "p2p_finish_losses"}
    assert [("p2p_finish_losses" if n == "p2p_finish_losses2" else n) for n, _ in rest] == [n for n, _ in gold]
    for (n, h), (gn, gh) in zip(rest, gold):
        if gn not in touched:
            assert h == gh, (n, gn)
    # the order of the chain: extract and the real histogram before the generator's first convolution, the other three between the
    # tanh forward and the tanh backward
    names = [n for n, _ in got]
    first_conv = min(i for i, n in enumerate(names) if n not in ("p2p_pack_pair", "p2p_palette_extract", "p2p_soft_palette_fwd",
                                                                 "p2p_dropout_mask_dev", "p2p_counter_add", "p2p_adam_tick"))
    assert names.index("p2p_palette_extract") < names.index("p2p_soft_palette_fwd") < first_conv
    tanh_fwd = next(i for i, n in enumerate(names) if n.startswith("p2p_tanh_l1_fwd"))
    tanh_bwd = next(i for i, n in enumerate(names) if n.startswith("p2p_tanh_l1_bwd"))
    assert tanh_fwd + 1 == len(names) - 1 - names[::-1].index("p2p_soft_palette_fwd")
    assert names[tanh_fwd + 1:tanh_fwd + 4] == PALETTE_LAUNCHES[2:] and tanh_fwd + 4 <= tanh_bwd
    # their arguments: the weights of the issue (w_tv = lambda_palette / 2 / Bg, w_conf = lambda_conformance / Bg, 1 / Bg), loss
    # slots 4 and 5, the unrounded fake copy handed to the tanh forward, the gradient slab to the tanh backward
    by = {}
    for name, args in log:
        by.setdefault(name, []).append([SL.val(a) for a in args])
    loss, bwd, fin = by["p2p_palette_loss"][0], by["p2p_soft_palette_tv_bwd"][0], by["p2p_finish_losses2"][0]
    assert loss[0] == B and loss[1] == 256 and loss[6] == pytest.approx(1.0 / B)
    assert bwd[:3] == [B, 64, 64] and bwd[6] == 256 and bwd[7] == pytest.approx(TERMS[2])
    assert bwd[10] == pytest.approx(TERMS[0] * 0.5 / B) and bwd[11] == pytest.approx(TERMS[1] / B)
    assert fin[1:4] == [4, 5, 3] and fin[4:7] == [100.0, TERMS[0], TERMS[1]]
    fwd = by[names[tanh_fwd]][0]
    assert fwd[-2] is not None and fwd[-2] != 0              # fake_f32
    extra = by[names[tanh_bwd]][0][-4]
    assert extra is not None and (extra.kind, extra.nslabs, extra.ld, extra.coff) == (2, 1, 4, 0)


def test_an_empty_shard_writes_the_five_term_result():
    log = []
    with SL._dry_run(log) as E:
        eng = _engine(E)
        log.clear()
        eng.train_step_empty(100.0, palette=TERMS, apply_update=False)
    assert [n for n, _ in log] == ["p2p_finish_losses2"]
