"""Float64 / float32 / bf16-storage references of the tape's vector-Jacobian products (tests/test_tape_vjp_gpu.py): the oracle graph
(oracle/reference_graph.py) under torch.autograd.grad with leaf inputs.  Host only; every case is computed once and cached, and
the cached arrays are read-only.

Seeds.  An f32 evaluation of this graph carries every pre-activation with some rounding noise; one that lies within that noise of
0 takes the other branch of its (Leaky)ReLU than float64 does, and the gradient through that entry appears or vanishes: on a
layer of n entries per image every gradient downstream moves by about 1 / sqrt(n) (1e-3 .. 5e-3 of its L2 norm, DESIGN.md
section 2).  torch's f32 evaluation and the engine's round differently, so either may flip where the other does not, and the
yardstick "1.5 x the f32 oracle's own deviation" then compares a flip with no flip.  flip_margin measures, from the two oracle
evaluations alone, how far the case is from that: the smallest |pre-activation| (float64) over the entries that have a branch,
in units of the layer's RMS difference between the f32 and the f64 evaluation.  The tests assert MIN_FLIP_MARGIN on it before
they look at the engine; search_seed below finds seeds that keep it (a margin of 3 leaves the entry nearest its kink a 0.3 % chance to flip
under Gaussian noise of that size)."""
import functools

import numpy as np
import torch

from oracle import reference_graph as rg

F64 = torch.float64
MIN_FLIP_MARGIN = 3.0


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))


def params(seed):
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, F64), rng)
    return rng, Gp, Dp


def to_np(p):
    return {k: v.detach().numpy() for k, v in p.items()}


def draw_masks(rng, B, S):
    return [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]


def batch(rng, B, S):
    """rg.synthetic_rgba_batch builds 64x64 sprites; a larger image is a grid of them (the tape arenas at 128x128)"""
    if S == 64:
        return rg.synthetic_rgba_batch(rng, B, 64, palette_size=24)
    k = S // 64
    tiles = [rg.synthetic_rgba_batch(rng, B, 64, palette_size=24) for _ in range(k * k)]

    def join(i):
        return np.ascontiguousarray(np.concatenate([np.concatenate([tiles[r * k + c][i] for c in range(k)], axis=2)
                                                    for r in range(k)], axis=1))
    return join(0), join(1)


# ---------------------------------------------------------------------------------------------------------------- the two networks
def generator(p, x_down, x_skip, masks, probe=None):
    """rg.unet_generator(p, x, masks, "tanh") with the source entering twice: x_down feeds down1, x_skip the last concat
    (networks.py:92-94), so autograd gives the two terms of d(source) separately.  probe (a list) receives the value in front
    of every (Leaky)ReLU that has a branch to take: entries a dropout mask zeroes are exactly 0 in every precision, and the
    1x1 map is beta exactly (InstanceNorm of one pixel)."""
    def note(v, mask=None):
        if probe is not None and v.shape[1] * v.shape[2] > 1:
            probe.append(v.detach()[mask.bool()] if mask is not None else v.detach().reshape(-1))

    x, skips = x_down, []
    for i in range(1, 7):
        x = rg.conv4x4_s2(x, p[f"down{i}.kernel"])
        if i > 1:
            x = rg.instance_norm(x, p[f"down{i}.gamma"], p[f"down{i}.beta"])
        note(x)
        x = rg._q(rg.leaky_relu(x))
        skips.append(x)
    skips = list(reversed(skips[:-1])) + [x_skip]
    for i, skip in enumerate(skips, start=1):
        x = rg.instance_norm(rg.convT4x4_s2(x, p[f"up{i}.kernel"]), p[f"up{i}.gamma"], p[f"up{i}.beta"])
        m = masks[i - 1] if rg.UP_DROPOUT[i - 1] else None
        note(x, m)
        if m is not None:
            x = rg.dropout(x, m)
        x = torch.cat([rg._q(torch.relu(x)), skip], dim=-1)
    return rg._q(torch.tanh(rg.conv4x4_s1_bias(x, p["last.kernel"], p["last.bias"])))


def discriminator(p, first, second, probe=None):
    """rg.patch_discriminator with the value in front of its LeakyReLU noted"""
    x = rg.conv4x4_s2(torch.cat([first, second], dim=-1), p["down.kernel"])
    if probe is not None:
        probe.append(x.detach().reshape(-1))
    return rg.conv4x4_s1_bias(rg._q(rg.leaky_relu(x)), p["last.kernel"], p["last.bias"])


def flip_margin(probe64, probe32):
    """see the module docstring: min over the layers of min |x64| / rms(x32 - x64)"""
    assert len(probe64) == len(probe32) and probe64
    return float(min(a.abs().min() / (b.double() - a).pow(2).mean().sqrt() for a, b in zip(probe64, probe32)))


# ---------------------------------------------------------------------------------------------------------------- engine-level cases
class Case:
    """the inputs of one seeded case: weights, a batch, dropout masks, upstream gradients"""

    def __init__(self, seed, B, S=64):
        self.seed, self.B, self.S = seed, B, S
        rng, self.Gp, self.Dp = params(seed)
        self.src, self.tgt = batch(rng, B, S)
        self.masks = draw_masks(rng, B, S)
        self.g_img = rng.standard_normal((B, S, S, 4)).astype(np.float32)
        self.g_log = rng.standard_normal((B, S // 2, S // 2, 1)).astype(np.float32)


def _ro(d):
    for v in d.values():
        if isinstance(v, dict):
            _ro(v)
        elif isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _np64(v):
    return {k: _np64(x) for k, x in v.items()} if isinstance(v, dict) else v.double().numpy()


def _eval(c, net, dt, storage):
    """{name: numpy f64} of one network's call and VJP in dtype `dt`, optionally with the engine's bf16 storage points; under
    "probe" the pre-activations for flip_margin (torch tensors in `dt`)"""
    def t(a):
        return torch.tensor(np.asarray(a), dtype=dt)

    out, probe = {}, []

    def run():
        if net == "D":
            p = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in c.Dp.items()}
            a, b = t(c.tgt).requires_grad_(True), t(c.src).requires_grad_(True)
            logits = discriminator(p, a, b, probe)
            grads = torch.autograd.grad(logits, [a, b] + list(p.values()), grad_outputs=t(c.g_log))
            out.update(logits=logits.detach(), d_first=grads[0], d_second=grads[1], grads=dict(zip(p, grads[2:])))
        else:
            p = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in c.Gp.items()}
            xd, xs = t(c.src).requires_grad_(True), t(c.src).requires_grad_(True)
            img = generator(p, xd, xs, [t(m) for m in c.masks], probe)
            grads = torch.autograd.grad(img, [xd, xs] + list(p.values()), grad_outputs=t(c.g_img))
            out.update(image=img.detach(), d_down=grads[0], d_skip=grads[1], d_src=grads[0].double() + grads[1].double(),
                       grads=dict(zip(p, grads[2:])))
    if storage is None:
        run()
    else:
        with rg.storage_dtype(storage):
            run()
    res = _ro(_np64(out))
    res["probe"] = probe
    return res


@functools.lru_cache(maxsize=None)
def case(seed, B, S=64):
    return Case(seed, B, S)


@functools.lru_cache(maxsize=None)
def reference(seed, B, net, kind="f64", S=64):
    """kind: "f64" the reference, "f32" the same graph evaluated in float32 by torch on the CPU (the yardstick of DESIGN.md
    section 2), "bf16" the float64 graph with the engine's bf16 storage points"""
    c = case(seed, B, S)
    if kind == "f32":
        return _eval(c, net, torch.float32, None)
    return _eval(c, net, F64, torch.bfloat16 if kind == "bf16" else None)


def case_flip_margin(seed, B, net, S=64):
    return flip_margin(reference(seed, B, net, "f64", S)["probe"], reference(seed, B, net, "f32", S)["probe"])


# ---------------------------------------------------------------------------------------------------------------- tape topologies
TOPOLOGIES = ("second_only", "two_generators", "one_image_twice")


def topology_losses(name, G, Dn, s, t):
    """(generator loss, discriminator loss) of a step whose discriminator call needs d(second input).  G(x, swapped) is the
    generator on x (swapped: the call whose images -- and dropout masks -- come in reversed batch order, so every image goes
    through the arithmetic of its unswapped twin and the case's flip margin holds for both calls); Dn(a, b) the discriminator."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    if name == "second_only":
        fp = Dn(t, G(s, False))
    elif name == "two_generators":
        fp = Dn(G(s, False), G(torch.flip(s, dims=[0]), True))
    else:
        f = G(s, False)
        fp = Dn(f, f)
    rp = Dn(t, s)
    return bce(fp, torch.ones_like(fp)), bce(fp, torch.zeros_like(fp)) + bce(rp, torch.ones_like(rp))


def _eval_topology(c, name, dt):
    def t(a):
        return torch.tensor(np.asarray(a), dtype=dt)

    Gl = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in c.Gp.items()}
    Dl = {k: v.detach().clone().to(dt).requires_grad_(True) for k, v in c.Dp.items()}
    masks, probe = [t(m) for m in c.masks], []
    swapped = [torch.flip(m, dims=[0]) for m in masks]
    g_total, d_total = topology_losses(name, lambda x, sw: generator(Gl, x, x, swapped if sw else masks, probe),
                                       lambda a, b: discriminator(Dl, a, b, probe), t(c.src), t(c.tgt))
    gg = torch.autograd.grad(g_total, list(Gl.values()), retain_graph=True)
    dg = torch.autograd.grad(d_total, list(Dl.values()))
    res = _ro(_np64({"g_total": g_total.detach(), "d_total": d_total.detach(), "G": dict(zip(Gl, gg)), "D": dict(zip(Dl, dg))}))
    res["probe"] = probe
    return res


@functools.lru_cache(maxsize=None)
def topology_reference(seed, B, name, kind="f64"):
    return _eval_topology(case(seed, B), name, torch.float32 if kind == "f32" else F64)


def flat_pairs(got, ref, keys=None):
    """[(name, got, ref)] over the tensors of a result, the weight gradients under "grads" as "grads/<name>" """
    out = []
    for k in (keys or [k for k in ref if k != "probe"]):
        if k == "grads":
            out += [(f"grads/{n}", got["grads"][n], ref["grads"][n]) for n in ref["grads"]]
        else:
            out.append((k, got[k], ref[k]))
    return out


# ---------------------------------------------------------------------------------------------------------------- seed search
def _forward_margin(c, what):
    """flip_margin of the engine-level call of network `what` ("G" / "D") or of a topology, from forward passes alone"""
    probes = []
    for dt in (F64, torch.float32):
        Gp, Dp = ({k: v.detach().to(dt) for k, v in p.items()} for p in (c.Gp, c.Dp))
        masks = [torch.tensor(m, dtype=dt) for m in c.masks]
        swapped = [torch.flip(m, dims=[0]) for m in masks]
        s, t = torch.tensor(c.src, dtype=dt), torch.tensor(c.tgt, dtype=dt)
        probe = []
        with torch.no_grad():
            if what == "G":
                generator(Gp, s, s, masks, probe)
            elif what == "D":
                discriminator(Dp, t, s, probe)
            else:
                topology_losses(what, lambda x, sw: generator(Gp, x, x, swapped if sw else masks, probe),
                                lambda a, b: discriminator(Dp, a, b, probe), s, t)
        probes.append(probe)
    return flip_margin(*probes)


def search_seed(B, S=64, first=101, last=4000):
    """the first seed whose case keeps MIN_FLIP_MARGIN in both networks (at B = 2, 64x64 also in the tape topologies) and whose
    f32 oracle alone stays below the caps of tests/test_tape_vjp_gpu.py; about one seed in 4 (B = 1), 100 (B = 2, 3) and
    2 000 (128x128) qualifies, a 128x128 seed takes about a second to try"""
    whats = ("G", "D") + (TOPOLOGIES if (B, S) == (2, 64) else ())
    for seed in range(first, last):
        c = Case(seed, B, S)
        if any(_forward_margin(c, w) < MIN_FLIP_MARGIN for w in whats):
            continue
        r64, r32 = (_eval(c, "G", dt, None) for dt in (F64, torch.float32))
        d64, d32 = (_eval(c, "D", dt, None) for dt in (F64, torch.float32))
        if (1.5 * rel_l2(r32["d_src"], r64["d_src"]) < 1e-2
                and all(1.5 * rel_l2(d32[k], d64[k]) < 1e-4 for k in ("d_first", "d_second"))):
            return seed
    return None


if __name__ == "__main__":          # python -m tests.tape_vjp_oracle: the SEEDS table of tests/test_tape_vjp_gpu.py
    for B, S in ((1, 64), (2, 64), (3, 64), (1, 128)):
        print(f"(B, S) = ({B}, {S}): seed {search_seed(B, S)}", flush=True)
