"""-m gpu: every launch a benchmarked train step makes, re-issued on test-owned buffers and compared with float64.

The kernels pick their variant from the launch size (256-row im2col tiles, the block-resident kernel, K splits, register-resident
norm forms ...), so small-shape tests do not reach what bench.py runs.  For each bench.CONFIGS entry the engine is built as bench.py
builds it, the recorded step's call list (the list p2p_replay re-issues) is reduced to unique launch signatures, and every launch of
an entry point with a checker below is re-issued with the recorded integer / float arguments and view geometry on seeded operands:
- per-image outputs are compared in full for a set of images (tests/step_launches.image_set), per image (per image and channel for
  normalised outputs); weight gradients over the whole batch, per tap;
- every output element of the view is NaN before and finite after; everything around the view (halo ring, other channels up to ld,
  the tail of the buffer) holds a sentinel that must be bit-for-bit unchanged;
- fused InstanceNorm statistics (slot partials) equal the f64 moments of the stored output;
- a second launch on the same inputs is bit-identical.
The losses, reductions, packing, weight copies, Adam and the dropout RNG are checked the same way: losses and column sums against
f64 (loss rows as sums of their P2P_LOSS_BLOCKS partials), packing and weight copies bit for bit against the dtype rounding of
their input with zero padding, Adam against the f64 Keras step at t = 1 and t = 3 on flat buffers laid out like the recorded
store (every element no task covers keeps its sentinel), the masks bit for bit against tests/step_launches.dropout_mask.  Device
task tables are copied from the engine while it is alive and re-issued as fresh tables over test-owned buffers.  Forms that no
benchmarked step issues are re-issued with hand-written arguments (test_entry_points_no_benchmarked_step_issues), and
test_one_keras_update_per_parameter_per_step checks that a replayed step moves every parameter by exactly one Adam step.

Lattice mode.  The checkers of the contractions (LATTICE_CHECKERS: convolutions, weight gradients, the indexed head's data
gradient, column sums) take operands="lattice": operands from tests/lattice.py (small integers times a power of two, small
integer biases, +-64 lattice steps in the channels around an input view), on which f32 accumulation is exact in any order.  View
geometry, NaN before the launch, the sentinel around the view and the bit-identical second launch stay; ALL images are compared,
and the compared quantity is the number of elements that differ from tests/lattice.expected -- families "exact out" / "exact dW" /
"exact slabs" (the slab sum, and every slab element on the lattice) / "exact colsum", which pass only at 0; a mismatch message
lists the first ten positions with got - want in lattice steps.  bf16 outputs add "insensitive share", the share of reference
sums outside +-256 (bound 0.01: a condition on the inputs).  "stats", "stats f64" and "norm out" keep their tolerances.  The
recorded steps of this file stay Gaussian; the lattice pass runs in tests/test_lattice_gpu.py and in the children of
tests/test_switch_routes_gpu.py.

Off-benchmark batches (test_every_launch_of_off_benchmark_steps_against_f64).  batch() has no drop_remainder and parallel.py
puts a remainder on the earlier ranks, so a step can have any batch, and the batch picks the kernel.  What the ENGINE and the
library's host queries pick (entry point, split-K, msplit, nsplit, statistics slots, block-resident / fused / strip / few-channel
routes, N % ipt and N % 8 classes) is in the variant key (tests/step_launches.variant_key); tests/test_step_launches_cpu.py runs
the engine's own step on device 'meta' for B = 1 .. 512 and asserts that step_launches.OFF_BENCH_BATCHES reaches every key found
up to the cap.  What a LAUNCHER picks from N behind an unchanged argument list is listed here, with the batches at which it flips
for the layer shapes of S = 64 (S = 128 in brackets where it differs) and the tested batch on either side ("above the cap": the
flip is beyond the case's cap, the upper side is the benchmarked batch of c2 / c4 / c5):
  brig.hip brig_plan     ntiles = ceil(N / ipt), ipt = 256 / (LH*LW)   partial last tile when N % ipt != 0: key class "N % ipt"; 6, 9 | 16, 32
  brig.hip brig_plan     ntiles * nnt < 160 -> im2col route             in the key (brig_ok): three 16x16 layers flip at 80 (79 | 80) [S = 128: 20 (16 | 20)];
                                                                        the fourth (op G 64 -> 128: ncols 128, cbw = 1 only, nnt = 1) at 160 and the
                                                                        8x8 layers at 157 / 160, above the cap
  brig.hip brig_plan     cbw = 1 while ntiles * (ncols / bn2) < 192     16x16 layers run cbw = 1 from 80 on and flip at 192: above the cap
  igemm.hip igemm_bm     256-row tiles once ceil(M/256)*(ncols/128)*gz  4x4 layers 49..56, 8x8 layers 61..62, 2x2 layer from 65 on: 48 | 49, 61 | 63,
                         >= 256 (M = N*LH*LW, gz = phases * splitk)     64 | 79; also behind p2p_igemm_stat_slots (in the key where statistics are fused)
  igemm.hip pipe_try     kg2 (second wave splits K) while tiles <= 384  16x16 / 8x8 layers lose it at 49 and regain it with the next split-K step: 48 | 49, 63 | 64
  igemm.hip igemm_launch bigM = M >= 131072 (64- / 32-column tiles)     p2p_igemm: N >= 128 on 32x32 maps, above the cap.  p2p_igemm_edge (f32 steps and the
                                                                        indexed head): 64x64 maps at 32 (f32 16 | 33, indexed 31 | 32), 32x32 maps of 2N
                                                                        images at 64 and of N images at 128: above the cap (c2-f32)
  igemm.hip igemm_go     nst = 3 LDS stages while nblk <= 320 (nblk =   p2p_igemm, 64-column op-P 16x16 layers: 3 | 2 at 41 (33 | 48; f32 33 | 256)
                         ceil(M / BM) * column tiles * gz) and          [S = 128, 32x32: 11 (9 | 15)]; f32 32 -> 128 on 32x32: 11 (8 | 16).  p2p_igemm_edge
                         taps * C * esz >= 512, else 2                  (f32): 64x64 maps 11 (8 | 16), 32x32 of 2N images 21 (16 | 33), of N images 41
                                                                        (33 | 256); indexed head (bf16) 11 (8 | 31)
  igemm.hip igemm_common w_major = weight bytes > gathered input bytes  16x16 layers at 2 and 4 (1 | 2 | 6; histogram / indexed 1 | 2 | 4; f32 1 | 6)
                         (16 * ncols * C against N * pixels * C)        [S = 128: 4 and 8 (2 | 4, 7 | 8)]; 8x8 op G 128 -> 256 at 16 (9 | 16), the other
                                                                        8x8 layers at 32 (17 | 32; f32 16 | 33) [S = 128: 32 / 64 above the cap]; 4x4 op G
                                                                        256 -> 512 at 128, the other 4x4 layers at 256: above the cap
  igemm.hip stat_slots   M % bm, hw % bm                                in the key (layer_stat_slots): 6, 9 | 8, 16
  norm_act.hip norm_bwd_reg_geom  widest CG with N * (C / CG) >= 512    C=256 8x8: 16, 32, 64, 128; C=128 16x16: 32, 64, 128, 256; C=64 32x32: 64, 128:
                                                                        9 | 16, 17 | 32, 33 | 63 | 64; 128 and 256 above the cap
  norm_act.hip fwd/bwd   grid ((N + 7) / 8) * 8 * (C / CG)              idle image slots when N % 8 != 0: key class "N % 8"; 6, 9 | 8, 16
  norm_act.hip fwd       sp2 doubles while N * (C / CG) * sp2 < 2048    apply-only pass (statistics from the conv epilogue).  S = 64: only up6 (64x64, C = 32)
                         and the split keeps >= prr pixels, sp2 <= 64   runs it below batch 256: sp2 64 | 32 at 64 (63 | 64), then 128, 256 above the cap.
                                                                        [S = 128: 64x64 C = 64, 128x128 C = 32 flip at 64; the others later: above the cap]
  norm_act.hip fwd/bwd   sp = 1 if N * sp * C * 8 > ws_bytes            never: the engine sizes ws for max(B, 2) * 16 * 1024 pairs
  norm_act.hip bwd       narrow: N * (C / 32) >= 1024, nsplit > 1       C=256 8x8 from 128 on: above the cap
  norm_act.hip small     grid ceil(N * (C / 8) << lgG / 256)            grid size only (maps of <= 16 pixels)
  conv_strip.hip cs_plan blocks = min(N * LH / TH, 256)                 persistent workgroups walk several strips past N = 32 (TH = 4): 32 | 33
  conv_fewin / fewout    fi_plan / fo_plan: N * (LH / TH) < 2^31        never at these sizes; grid size only (fewin_ok / fewout_ok are in the key)
  wgrad_small.hip ws_plan  blocks = min(N * LH / TH, want), want 32..512 one strip per workgroup below, several above: between 4 and 64 by layer
                                                                        (2 | 6 | 9 | 16 .. 64 | 79); wgrad_small > 0 is in the key
  wgrad_small.hip ws_sum_split  doubles while colblocks * split < 512   follows blocks (above): 2 | 6 | 16 | 33 | 64
                         and nslabs / (2 * split) >= 4
  wgemm.hip wgemm_pipe_ok  M % 64, chunk % 64 (M = N*LH*LW / msplit)    1x1 .. 4x4 layers: 1, 2, 6, 9 (M % 64 != 0) | 16, 32, 64; msplit is in the key
                         and 16 * (Cg/128) * (Cd/128) * msplit <= 448  follows msplit (in the key)
  conv_direct.hip view_colsum  nb = ceil(M / chunk) partials            grid size only
  hist.hip launch_hist_bwd3  nsplit (pixel partition of an image) doubles  S = 64: 8 below 64, 4 for 64 .. 127 (48 | 64), 2 for 128 .. 255, 1 from 256 (c3).
                         while N * nsplit < 256 and H*W / (2 nsplit)    nsplit = 2 lies between the cap and c3: re-issued at N = 128 by DIRECT
                         >= 512                                         (test_entry_points_no_benchmarked_step_issues).  [S = 128: 32 below 16, 16 for
                                                                        16 .. 31 (15 | 16); 8, 4, 2 above the cap; 1 from 256 (c5)]
  hist.hip fwd3 / points / hellinger_fwd   grid (N, ...)                grid size only
  losses.hip tanh_l1_bwd, optim.hip pack / unpack   blocks = min(ceil(N*H*W / 256), 4096)   one element per thread up to N*H*W = 2^20, grid-stride loop beyond:
                                                                        N > 256 at S = 64, N > 64 at S = 128: above the cap (upper side c5 only)
  optim.hip dropout_mask  blocks = min(ceil(n / 8 / 256), 2048)         n = N * res^2 * C of one mask > 2^22: N > 256 at S = 64 [N > 64]: above the cap
  softmax.hip softmax_cce  blocks = min(ceil(M / 16), MAX_BLOCKS)       not in the recorded steps (the indexed step fuses the head: head_softmax.hip)
  head_softmax.hip, losses.hip forward, sprites.hip   N enters grid sizes (N * H / 4 workgroups; P2P_LOSS_BLOCKS fixed), workspace offsets and the
                                                                        1 / (N ...) scales only
The flip batches of the igemm.hip, norm_act.hip sp2 and hist.hip rows were computed from the launch arguments of the census with the
launchers' formulas; those of the wgrad_small.hip and wgemm.hip rows by hand.
The rows brig_plan (route, cbw), igemm_bm, pipe_try, igemm_launch, igemm_go, igemm_common (w_major), norm_bwd_reg_geom and
wgemm_pipe_ok can now be read off the library instead: p2p_igemm_route / p2p_igemm_edge_route / p2p_brig_route / p2p_wgemm_route /
p2p_wgrad_small_route / p2p_norm_act_fwd_route / p2p_norm_act_bwd_route (include/p2pgan.h "route queries") call the launchers' own
decision functions and return the tile, K groups, stages, block order, wave tiling and norm form of a launch;
tests/switch_routes.routes maps a decoded launch to them, and tests/test_switch_routes_cpu.py asserts with them that every arm of
those launchers is run by this file, by test_kernels_gpu.py or by a switch setting of tests/test_switch_routes_gpu.py.  (softmax.hip:
the generic head IS in a recorded step once engine.use_head_fused is off -- OUT_OF_SCOPE below says where it is checked.)
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bench
from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from tests import gpu_util as U
from tests import lattice as LT
from tests import step_launches as SL

pytestmark = pytest.mark.gpu

OUT_TOL = SL.OUT_TOL                        # test_kernels_gpu.py: activation-dtype outputs
F32_TOL = 2e-5                              # f32 slabs / statistics of short contractions (test_kernels_gpu.py)
SENTINEL = -1234.5                          # exact in bf16 and f32
TAIL = 256                                  # elements of sentinel behind every output buffer

CONFIGS = [("c1", "bf16"), ("c2", "bf16"), ("c3", "bf16"), ("c4", "bf16"), ("c5", "bf16"), ("c2", "f32")]

# entry points of a recorded step that this file does not re-issue, with the reason.  A call that is neither here nor in
# CHECKERS fails the test: a new entry point cannot slip past.
OUT_OF_SCOPE = {
    "p2p_event_record": "stream operation", "p2p_stream_wait_event": "stream operation", "p2p_arm_stop_event": "stream operation",
    "p2p_event_create": "stream operation", "p2p_disarm_stop_event": "stream operation",
    # the generic indexed head (engine.use_head_fused = False, or a shape p2p_head_softmax_ok refuses; its convolution is a
    # p2p_igemm_edge launch with a checker): against f64 in both dtypes in test_hist_indexed_gpu.py::test_softmax_cce_argmax_kernel
    # and against the fused head at the c4 launch shape in ::test_fused_indexed_head_at_the_c4_launch_shape_against_the_generic_path
    "p2p_softmax_cce_argmax": "generic indexed head: checked against f64 by tests/test_hist_indexed_gpu.py",
}


_val, _esz, _decode, _signature = SL.val, SL.elem_size, SL.decode, SL.signature        # (shared with the host-only census)


def _blocks():
    """(address, size) of every allocated block of torch's caching allocator on the device"""
    out = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            if b["state"] == "active_allocated":
                out.append((addr, b["size"]))
            addr += b["size"]
    return out


# ---------------------------------------------------------------------------------------------------------------- harvest
def _build(cfg, dtype_name):
    """cfg: the name of a bench.CONFIGS entry, or a step description (model, B, S, lambda_l1, lambda_hist, palette) of its own"""
    model, B, S, lam_l1, lam_hist, palette = bench.CONFIGS[cfg] if isinstance(cfg, str) else cfg
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    if model == "indexed":
        eng = E.Pix2PixEngine(1, 256, "softmax", S, dtype, device=U.DEV, seed=47)
        src, tgt, _ = DU.synthetic_indexed_batch(np.random.default_rng([47, 0]), B, S, palette)
        src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
        return eng, lambda: eng.train_step_indexed(src_d, tgt_d, lam_l1, global_batch=B)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, device=U.DEV, seed=47)
    src, tgt = bench.synthetic_batch(0, B, S, palette)
    src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
    return eng, lambda: eng.train_step_rgba(src_d, tgt_d, lam_l1, lam_hist, global_batch=B)


def _raw_ptr(v):
    v = _val(v)
    return v.value if isinstance(v, C.c_void_p) else v


def _in_store(eng, ptr, what):
    """(network, store, element offset) of a pointer into one of the flat params / grads / m / v buffers"""
    for sid, store in (("G", eng.G), ("D", eng.D)):
        for buf in (store.params, store.grads, store.m, store.v):
            a = buf.data_ptr()
            if a <= ptr < a + 4 * buf.numel():
                assert (ptr - a) % 4 == 0, what
                return sid, store, (ptr - a) // 4
    raise AssertionError(f"{what}: pointer {ptr:#x} is in no flat parameter buffer")


def _tables(eng):
    """host copies of the engine's device-resident argument tables, by device address: the p2p_prep_task tables of the weight
    copies (_prep_table) and of the fused Adam (_adam_tables), and the part_tasks rows of every plan's dgamma / dbeta reduction"""
    out = {}
    for raw, *_ in list(eng._prep_table.values()) + list(eng._adam_tables.values()):
        if raw is not None:
            out[raw.data_ptr()] = ("prep", raw.cpu().numpy().tobytes())
    for P in eng.plans.values():
        if P.get("part_tasks") is not None:
            out[P["part_tasks"].data_ptr()] = ("colsum", tuple(tuple(r) for r in P["part_tasks"].cpu().tolist()))
    return out


def _decode_tasks(eng, raw, ntasks, what):
    """p2p_prep_task entries -> (Cg, Cd, wn_rows, wn_cols, wt_rows, wt_cols, has_wn, has_wt, tiles_g, tiles_d, first_block,
    network of the master, element offset of the master in its params buffer)"""
    arr = (L.PrepTask * ntasks).from_buffer_copy(raw[:C.sizeof(L.PrepTask) * ntasks])
    out = []
    for t in arr:
        sid, store, off = _in_store(eng, t.w, what)
        assert t.w == store.params.data_ptr() + 4 * off, f"{what}: a task's master is not in params"
        out.append((t.Cg, t.Cd, t.wn_rows, t.wn_cols, t.wt_rows, t.wt_cols, int(bool(t.wn)), int(bool(t.wt)), t.tiles_g, t.tiles_d,
                    t.first_block, sid, off))
    return tuple(out)


def _decode_device_args(eng, tables, name, args, dec):
    """the arguments _decode cannot read from the pointer alone: device task tables (copied while the engine is alive; a pointer
    that is none of the engine's tables fails) and positions inside the flat parameter stores"""
    if name in ("p2p_weight_prep_batched", "p2p_adam_prep_batched", "p2p_colsum_batched"):
        i = {"p2p_weight_prep_batched": 1, "p2p_adam_prep_batched": 2, "p2p_colsum_batched": 1}[name]
        ptr = _raw_ptr(args[i])
        kind, data = tables.get(ptr, (None, None))
        assert kind == ("colsum" if name == "p2p_colsum_batched" else "prep"), \
            f"{name}: argument table {ptr:#x} is none of the engine's tables"
        dec[i] = ("tasks", data if kind == "colsum" else _decode_tasks(eng, data, int(_val(args[i + 1])), name))
    if name == "p2p_adam_prep_batched":
        sid, store, off = _in_store(eng, _raw_ptr(args[5]), name)
        assert off == 0, f"{name}: params is not the start of a store"
        dec[5] = ("store", sid, store.numel)
    if name == "p2p_colsum_batched":
        sid, store, off = _in_store(eng, _raw_ptr(args[4]), name)
        dec[4] = ("store", sid, store.grads.numel(), off)
    if name == "p2p_adam_flat_dev":
        sid, store, off = _in_store(eng, _raw_ptr(args[0]), name)
        dec[0] = ("store", sid, store.numel, off)
    return dec


def _overrides(fuse):
    """the engine attributes a step case sets (engine.SWITCHES / GATES names, "side.x" for the weight-gradient stream helper): a
    dict, or the fuse_adam switch alone (None: bench.py's defaults)"""
    if isinstance(fuse, dict):
        return fuse
    return {} if fuse is None else {"fuse_adam": fuse}


def harvest(cfg, dtype_name, overrides=None):
    """unique launch signatures of the recorded step of one bench config or step description (_build): {signature: (name, decoded
    args)}, and the raw count.  overrides: engine switch attributes to set before the first step (_overrides; bench.py runs the
    defaults)"""
    eng, step = _build(cfg, dtype_name)
    for attr, value in _overrides(overrides).items():
        holder, name = E._switch_holder(eng, attr)
        assert hasattr(holder, name), f"the engine has no switch {attr}"
        setattr(holder, name, value)
    try:
        for _ in range(2):         # the first step of a kind is eager, the second one is recorded (_begin_record)
            step()
        torch.cuda.synchronize()
        assert len(eng._replays) == 1, f"{cfg}: the step was not recorded"
        rec = next(iter(eng._replays.values()))[1]
        assert rec, f"{cfg}: empty recording"
        blocks = _blocks()
        tables = _tables(eng)
        uniq, names = {}, []
        for name, args in rec:
            assert name is not None, "single-GPU step with a collective segment"
            names.append(name)
            if name not in CHECKERS:
                continue
            dec = _decode_device_args(eng, tables, name, args, _decode(name, args, blocks))
            uniq.setdefault(_signature(name, dec), (name, dec))
        return uniq, names
    finally:
        del eng
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- buffers
def _shift(base, off0, esz, align):
    """element shift that puts a view's first element base + (s + off0) * esz at its recorded alignment mod 16, on a 64-byte
    boundary plus that alignment (the whole-pixel stores of the packing and loss kernels require up to 32-byte alignment)"""
    for mod in (64, 16):
        for s in range(128):
            if (base + (s + off0) * esz) % mod == align:
                return s
    raise AssertionError(f"no shift gives alignment {align}")


class OutBuf:
    """A test-owned buffer laid out like a recorded output view: same pixel strides, ld, channel offset and 16-byte alignment.
    The nc channels of the view's pixels start as NaN, everything else (halo ring, the other channels, TAIL elements) as SENTINEL."""

    def __init__(self, desc, n, h, w, nc, tdt, esz):
        ld, coff = desc["ld"], desc["coff"]
        rs, ist = desc["row_stride"], desc["img_stride"]
        halo = (rs - w) // 2
        assert rs == w + 2 * halo and ist == (h + 2 * halo) * rs, f"view geometry {desc} does not fit {h}x{w} with a halo"
        assert coff + nc <= ld, (desc, nc)
        _check_grid(desc, h, w)
        hp, wp = h + 2 * halo, w + 2 * halo
        numel = n * hp * wp * ld
        off0 = (halo * wp + halo) * ld + coff
        self.flat_all = torch.empty(numel + TAIL + 128, dtype=tdt, device=U.DEV)
        base = self.flat_all.data_ptr()
        s = _shift(base, off0, esz, desc["align"])
        self.flat = self.flat_all[s:s + numel + TAIL]
        self.t = self.flat[:numel].view(n, hp, wp, ld)
        self.sl = (slice(None), slice(halo, halo + h), slice(halo, halo + w), slice(coff, coff + nc))
        self.view = L.Tensor(base + (s + off0) * esz, ist, rs, ld)
        self.mask = torch.ones(self.flat.shape, dtype=torch.bool, device=U.DEV)
        self.mask[:numel].view(n, hp, wp, ld)[self.sl] = False
        self.reset()

    def reset(self):
        self.flat.fill_(SENTINEL)
        self.t[self.sl] = float("nan")
        self._before = self.flat.clone()

    def region(self):
        return self.t[self.sl].double().cpu().numpy()

    def check_around(self, what):
        got, want = self.flat[self.mask], self._before[self.mask]
        assert torch.equal(_bits(got), _bits(want)), \
            f"{what}: an element outside the view changed"
        r = self.t[self.sl]
        assert not bool(torch.isnan(r).any()), f"{what}: {int(torch.isnan(r).sum())} elements of the view were not written"


class FlatOut:
    """f32 output of a given length (slabs, statistics, weight gradients): NaN, then TAIL sentinel elements"""

    def __init__(self, numel, align=0):
        self.numel = numel
        self.all = torch.empty(numel + TAIL + 4, dtype=torch.float32, device=U.DEV)
        s = next(s for s in range(4) if (self.all.data_ptr() + 4 * s) % 16 == align)
        self.flat = self.all[s:s + numel + TAIL]
        self.reset()

    def reset(self):
        self.flat[:self.numel] = float("nan")
        self.flat[self.numel:] = SENTINEL

    def ptr(self):
        return C.c_void_p(self.flat.data_ptr())

    def values(self):
        return self.flat[:self.numel].double().cpu().numpy()

    def check_around(self, what):
        assert bool((self.flat[self.numel:] == SENTINEL).all()), f"{what}: written past the end"
        assert not bool(torch.isnan(self.flat[:self.numel]).any()), f"{what}: elements not written"


def _check_grid(desc, h, w):
    """the recorded view starts at the first interior pixel of an image of its buffer (halo = (row_stride - w) / 2)"""
    halo = (desc["row_stride"] - w) // 2
    if "pix" in desc:
        assert desc["pix"] == halo * desc["row_stride"] + halo, f"view {desc} is not at the first interior pixel of a {h}x{w} image"


def in_view(desc, x, dtype, fill_rng, other=None):
    """input view with the recorded geometry holding x [n,h,w,c] at the recorded channel offset.  The other channels of the pixels
    hold random values (a kernel must not use them; other(shape): the values to put there instead, tests/lattice.other_channels),
    the halo ring and the tail are zero (the gathering kernels read the halo as the convolution's zero padding, include/p2pgan.h
    Conventions).  Returns (keep-alive tensor, p2p_tensor)."""
    n, h, w, c = x.shape
    ld, coff, rs, ist = desc["ld"], desc["coff"], desc["row_stride"], desc["img_stride"]
    halo = (rs - w) // 2
    assert rs == w + 2 * halo and ist == (h + 2 * halo) * rs and coff + c <= ld, (desc, x.shape)
    _check_grid(desc, h, w)
    esz = _esz(dtype)
    hp, wp = h + 2 * halo, w + 2 * halo
    numel = n * hp * wp * ld
    off0 = (halo * wp + halo) * ld + coff
    flat_all = torch.zeros(numel + TAIL + 128, dtype=U.tdt(dtype), device=U.DEV)
    base = flat_all.data_ptr()
    s = _shift(base, off0, esz, desc["align"])
    t = flat_all[s:s + numel].view(n, hp, wp, ld)
    fill = U.q(fill_rng.normal(size=(n, h, w, ld)), dtype) if other is None else other((n, h, w, ld))
    t[:, halo:halo + h, halo:halo + w, :] = torch.as_tensor(fill).to(U.DEV).to(t.dtype)
    t[:, halo:halo + h, halo:halo + w, coff:coff + c] = torch.as_tensor(x).to(U.DEV).to(t.dtype)
    return flat_all, L.Tensor(base + (s + off0) * esz, ist, rs, ld)


def gsrc_in(desc, n, h, w, c, dtype, rng, live=None, scale=1.0):
    """gradient source with the recorded kind / slabs / ld / offset: returns (keep-alive, p2p_gsrc, summed f64 values [n,h,w,c]).
    live [n*h*w, c] (bool): the source is zero where it is False; scale: standard deviation of the values"""
    pix = n * h * w
    ld, coff, ns, ss = desc["ld"], desc["coff"], max(desc["nslabs"], 1), desc["slab_stride"]
    if desc["kind"] == 2:
        assert ss >= pix * ld, desc
        data = (rng.normal(size=(ns, ss)) * scale).astype(np.float32)
        if live is not None:
            for k in range(ns):
                data[k, :pix * ld].reshape(pix, ld)[:, coff:coff + c] *= live
        t = torch.as_tensor(data.reshape(-1)).to(U.DEV)
        vals = np.zeros((pix, c), np.float32)
        for k in range(ns):
            vals = vals + data[k, :pix * ld].reshape(pix, ld)[:, coff:coff + c]       # f32, slab order
        ref = vals.astype(np.float64)
    else:
        data = U.q(rng.normal(size=(pix, ld)) * scale, dtype)
        if live is not None:
            data[:, coff:coff + c] *= live
        t = torch.as_tensor(data).to(U.DEV).to(U.tdt(dtype)).contiguous()
        ref = data[:, coff:coff + c].astype(np.float64)
    g = L.GSrc(t.data_ptr(), desc["kind"], desc["nslabs"], ss, ld, coff)
    return t, g, ref.reshape(n, h, w, c)


def _prep(dtype, w, cg, cd, wn_shape=None, wt_shape=None):
    """p2p_weight_prep_pad: wn [16][rows][cols] and / or wt [16][rows][cols] in the activation dtype"""
    w_d = U.dev(w.reshape(-1))
    wn = torch.zeros(16 * wn_shape[0] * wn_shape[1], dtype=U.tdt(dtype), device=U.DEV) if wn_shape else None
    wt = torch.zeros(16 * wt_shape[0] * wt_shape[1], dtype=U.tdt(dtype), device=U.DEV) if wt_shape else None
    L.call("p2p_weight_prep_pad", dtype, U.ptr(w_d), cg, cd, U.ptr(wn) if wn is not None else None, *(wn_shape or (0, 0)),
           U.ptr(wt) if wt is not None else None, *(wt_shape or (0, 0)), U.stream())
    return wn if wn is not None else wt


# ---------------------------------------------------------------------------------------------------------------- checkers
class Launch:
    """one re-issued launch: outputs (OutBuf / FlatOut), the launch closure and the evaluation (returns {family: worst error})"""

    def __init__(self, outs, go, evaluate):
        self.outs, self.go, self.evaluate = outs, go, evaluate


def _lattice_mode(operands):
    assert operands in ("gaussian", "lattice"), operands
    return operands == "lattice"


def _other(lat, rng, step):
    """what in_view puts into the channels around the view: Gaussian values, or +-64 steps of the tensor in lattice mode"""
    return (lambda shape: LT.other_channels(rng, shape, step)) if lat else None


def _exact_family(errs, msgs, family, got, want, step, names):
    """lattice mode: the number of elements that are not the expected value as a family that passes only at 0, and the first ten
    positions with their deltas for the assertion message"""
    errs[family] = float(len(LT.mismatches(got, want)))
    if errs[family]:
        msgs.append(f"{family}: " + LT.describe_mismatches(got, want, step, names))


def _sensitive(errs, dtype, sum_int):
    """lattice mode, bf16 outputs: the share of reference sums outside +-256 (where bf16 no longer tells every integer apart) as
    a family bounded by 0.01.  A condition on the inputs, computed from the reference alone"""
    if dtype == L.BF16:
        errs["insensitive share"] = 1.0 - LT.sensitive_share(sum_int)


def _conv_family(name, a, rng, operands="gaussian"):
    """p2p_igemm, p2p_conv_strip, p2p_igemm_norm_act (stride 2, full channel counts) and the edge forms p2p_igemm_edge,
    p2p_conv_fewin, p2p_conv_fewout, p2p_conv_fewin_actbwd (cin_pad contracted channels, ncols outputs, stride 1 or 2).
    operands="lattice": integer-lattice operands (tests/lattice.py), every image compared, the result exact"""
    lat = _lattice_mode(operands)
    edge = name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewout", "p2p_conv_fewin_actbwd")
    if edge:
        op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows = a[:9]
        in_d, out_d = a[9][1], a[10][1]
        if op == L.OP_G:
            cg, cd, in_shape, out_shape = cin_pad, ncols, (stride * LH, stride * LW, cin_pad), (LH, LW, ncols)
        else:
            cg, cd, in_shape, out_shape = ncols, cin_pad, (LH, LW, cin_pad), (stride * LH, stride * LW, ncols)
    else:
        op, dtype, N, LH, LW, cg, cd = a[:7]
        stride = 2
        hi_d, lo_d = a[7][1], a[8][1]
        in_d, out_d = (hi_d, lo_d) if op == L.OP_G else (lo_d, hi_d)
        in_shape = (2 * LH, 2 * LW, cg) if op == L.OP_G else (LH, LW, cd)
        out_shape = (LH, LW, cd) if op == L.OP_G else (2 * LH, 2 * LW, cg)
    tdt, esz = U.tdt(dtype), _esz(dtype)
    sk = a[7 + 3] if name == "p2p_igemm" else 1
    step = sx = 1.0
    if lat:
        # contraction length: 16 taps of the input channels (op G), 4 (stride 2) or 16 (stride 1) of them per output pixel (op P);
        # split-K slabs are f32 whatever the dtype
        K = (16 if op == L.OP_G or stride == 1 else 4) * in_shape[2]
        out_bf16 = dtype == L.BF16 and sk == 1
        x, sx = LT.operands(rng, (N,) + in_shape, "x", K, dtype, out_bf16)
        w, sw = LT.operands(rng, (4, 4, cg, cd), "w", K, dtype, out_bf16)
        step = sx * sw
    else:
        x = U.q(rng.normal(size=(N,) + in_shape), dtype)
        w = U.q(rng.normal(scale=1.0 / np.sqrt(16 * in_shape[2]), size=(4, 4, cg, cd)), dtype)
    keep_in, in_v = in_view(in_d, x, dtype, rng, _other(lat, rng, sx))
    if edge:
        if op == L.OP_G:
            wbuf = _prep(dtype, w, cg, cd, wt_shape=(w_rows, cin_pad))
        else:
            wbuf = _prep(dtype, w, cg, cd, wn_shape=(w_rows, cin_pad))
    else:
        wbuf = _prep(dtype, w, cg, cd, wn_shape=(cg, cd)) if op == L.OP_P else _prep(dtype, w, cg, cd, wt_shape=(cd, cg))
    nout = out_shape[2]
    res_h, res_w = out_shape[0], out_shape[1]
    outs, extra = [], {}
    slabs = None
    out = OutBuf(out_d, N, res_h, res_w, nout, tdt, esz)      # (not written with split-K slabs)
    if name == "p2p_igemm" and sk > 1:
        slabs = FlatOut(sk * N * res_h * res_w * nout, a[11][1] if a[11] else 0)
        outs.append(slabs)
    else:
        outs.append(out)
    hv, lv = (in_v, out.view) if op == L.OP_G else (out.view, in_v)
    spart = None
    stat_idx = {"p2p_igemm": 12, "p2p_conv_strip": 10}.get(name)
    if stat_idx is not None and a[stat_idx] is not None:
        slots = (L.lib().p2p_igemm_layer_stat_slots(op, dtype, N, LH, LW, cg, cd) if name == "p2p_igemm"
                 else L.lib().p2p_conv_strip_stat_slots(op, dtype, N, LH, LW, cg, cd))
        assert slots > 0, (name, a)
        spart = FlatOut(N * slots * nout * 2, a[stat_idx][1])
        outs.append(spart)
        extra["slots"] = slots
    bias = gate = gamma = beta = None
    if name in ("p2p_igemm_edge", "p2p_conv_fewin", "p2p_conv_fewout") and a[12] is not None:
        bias = LT.small_ints(rng, ncols, step) if lat else rng.normal(size=ncols).astype(np.float32)
    bias_d = U.dev(bias) if bias is not None else None
    if name == "p2p_conv_fewin_actbwd":
        gate = LT.operands(rng, (N, res_h, res_w, nout), "x", 1, dtype, True)[0] if lat else U.q(rng.normal(size=(N, res_h, res_w, nout)), dtype)
        keep_gate, gate_v = in_view(a[12][1], gate, dtype, rng, _other(lat, rng, 1.0))
    if name == "p2p_igemm_norm_act":
        gamma = (1 + 0.2 * rng.normal(size=nout)).astype(np.float32)
        beta = (0.2 * rng.normal(size=nout)).astype(np.float32)
        g_d, b_d = U.dev(gamma), U.dev(beta)
        y = OutBuf(a[15][1], N, res_h, res_w, nout, tdt, esz)
        stats = FlatOut(N * nout * 2, a[16][1])
        outs += [y, stats]

    def go():
        st = U.stream()
        if name == "p2p_igemm":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), sk,
                   slabs.ptr() if slabs else None, spart.ptr() if spart else None, st)
        elif name == "p2p_conv_strip":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), spart.ptr() if spart else None, st)
        elif name == "p2p_igemm_norm_act":
            L.call(name, op, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), U.ptr(wbuf), U.ptr(g_d), U.ptr(b_d), a[12], a[13],
                   a[14], C.byref(y.view), stats.ptr(), st)
        elif name == "p2p_conv_fewin_actbwd":
            L.call(name, op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows, C.byref(in_v), C.byref(out.view), U.ptr(wbuf),
                   C.byref(gate_v), a[13], st)
        else:
            L.call(name, op, stride, dtype, N, LH, LW, cin_pad, ncols, w_rows, C.byref(in_v), C.byref(out.view), U.ptr(wbuf),
                   U.ptr(bias_d) if bias_d is not None else None, a[13], a[14], st)

    def evaluate():
        errs, msgs = {}, []
        imgs = list(range(N)) if lat else SL.image_set(N, seed=N * 7 + LH)
        conv = (SL.conv_g(x[imgs], w, stride) if op == L.OP_G else SL.conv_p(x[imgs], w, stride))
        where = ("image", "y", "x", "channel")
        if slabs is not None:
            sl = slabs.values().reshape(sk, N, res_h, res_w, nout)
            got = sl.sum(0)[imgs]
            if lat:     # the slab SUM is the reference and every slab element is on the lattice; which taps a slab holds is the kernel's business
                _exact_family(errs, msgs, "exact slabs", got, LT.expected(conv, L.F32), step, where)
                off = int((np.rint(sl / step) != sl / step).sum())
                if off:
                    errs["exact slabs"] += off
                    msgs.append(f"exact slabs: {off} slab elements are no integer multiple of the lattice step")
                assert not msgs, "; ".join(msgs)
                return errs
            errs["f32 slabs"] = SL.per_image_err(got, conv)
            return errs
        full = out.region()
        got = full[imgs]
        if name == "p2p_conv_fewin_actbwd":
            ref = conv * np.where(gate[imgs] > 0, 1.0, a[13])
        elif name == "p2p_igemm_norm_act":
            ref = conv
        else:
            ref = conv + (bias if bias is not None else 0.0)
            ref = SL.act(ref, a[13], a[14]) if edge else ref
        if lat:
            if name == "p2p_conv_fewin_actbwd":
                want = LT.expected(conv, dtype, alpha=a[13], gate=gate)
            elif edge:
                want = LT.expected(conv, dtype, bias=bias, act=a[13], alpha=a[14])
            else:
                want = LT.expected(conv, dtype)         # (p2p_igemm_norm_act: the raw convolution output)
            _exact_family(errs, msgs, "exact out", got, want, step, where)
            _sensitive(errs, dtype, LT.to_int(conv, step) + (LT.to_int(bias, step) if bias is not None else 0))
        else:
            errs["out " + ("bf16" if dtype == L.BF16 else "f32")] = SL.per_image_err(got, ref)
        if spart is not None:
            mean, var = SL.pooled_moments(spart.values().reshape(N, extra["slots"], nout, 2), res_h * res_w / extra["slots"])
            errs["stats"] = SL.moment_err(mean, var, full)                       # every image: the stored output's moments
            errs["stats f64"] = SL.moment_err(mean[imgs], var[imgs], conv)       # the compared images: the f64 convolution's
        if name == "p2p_igemm_norm_act":
            st_v = stats.values().reshape(N, nout, 2)
            var = 1.0 / st_v[..., 1].astype(np.float64) ** 2 - a[12]
            errs["stats"] = SL.moment_err(st_v[..., 0], var, full, eps=a[12])
            errs["stats f64"] = SL.moment_err(st_v[imgs][..., 0], var[imgs], conv, eps=a[12])
            want = SL.norm_act(got, gamma, beta, a[12], a[13], a[14])
            pre = SL.norm_act(got, gamma, beta, a[12], 0, 0.0)
            errs["norm out"] = SL.per_image_channel_err(y.region()[imgs], want, np.maximum(np.abs(want), np.abs(pre)))
        assert not msgs, "; ".join(msgs)
        return errs

    keep = (keep_in, wbuf, bias_d) + ((keep_gate,) if gate is not None else ()) + ((g_d, b_d) if gamma is not None else ())
    launch = Launch(outs, go, evaluate)
    launch.keep = keep
    return launch


def _wgrad_family(name, a, rng, operands="gaussian"):
    """p2p_wgemm (stride 2), p2p_wgemm_edge, p2p_wgrad_small: dW over the whole batch.  operands="lattice": exact"""
    lat = _lattice_mode(operands)
    if name == "p2p_wgemm":
        dtype, N, LH, LW, cg, cd = a[:6]
        stride, hi_d, lo_d, ms = 2, a[6][1], a[7][1], a[9]
    else:
        dtype, stride, N, LH, LW, cg, cd = a[:7]
        hi_d, lo_d = a[7][1], a[8][1]
        ms = a[10] if name == "p2p_wgemm_edge" else None
    s_hi = s_lo = 1.0
    if lat:             # dW is f32 in both dtypes: the widest alphabet, K = N * LH * LW products of two activations
        hi, s_hi = LT.operands(rng, (N, stride * LH, stride * LW, cg), "x", N * LH * LW, dtype, False)
        lo, s_lo = LT.operands(rng, (N, LH, LW, cd), "x", N * LH * LW, dtype, False)
    else:
        hi = U.q(rng.normal(size=(N, stride * LH, stride * LW, cg)), dtype)
        lo = U.q(rng.normal(size=(N, LH, LW, cd)), dtype)
    keep_hi, hv = in_view(hi_d, hi, dtype, rng, _other(lat, rng, s_hi))
    keep_lo, lv = in_view(lo_d, lo, dtype, rng, _other(lat, rng, s_lo))
    dw = FlatOut(16 * cg * cd, a[8 if name == "p2p_wgemm" else 9][1])
    if name == "p2p_wgrad_small":
        nb = L.lib().p2p_wgrad_small_blocks(dtype, stride, N, LH, LW, cg, cd, hv.ld, lv.ld)
        assert nb > 0, a
        ws_n = nb * 16 * cg * cd
    else:
        ws_n = L.lib().p2p_wgemm_workspace_bytes(N, LH, LW, cg, cd, ms) // 4
    ws = torch.full((max(ws_n, 4),), float("nan"), dtype=torch.float32, device=U.DEV)

    def go():
        st = U.stream()
        if name == "p2p_wgemm":
            L.call(name, dtype, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), ms, U.ptr(ws) if a[10] else None, st)
        elif name == "p2p_wgemm_edge":
            L.call(name, dtype, stride, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), ms, U.ptr(ws) if a[11] else None, st)
        else:
            L.call(name, dtype, stride, N, LH, LW, cg, cd, C.byref(hv), C.byref(lv), dw.ptr(), U.ptr(ws), st)

    def evaluate():
        ref = SL.conv_w(hi, lo, stride)
        if lat:
            errs, msgs = {}, []
            _exact_family(errs, msgs, "exact dW", dw.values().reshape(4, 4, cg, cd), LT.expected(ref, L.F32), s_hi * s_lo,
                          ("kh", "kw", "g", "d"))
            assert not msgs, "; ".join(msgs)
            return errs
        k = N * LH * LW
        # K = N*LH*LW products of activation-dtype values (exact in f32), summed in f32 in a fixed blocked order.  The rounding
        # error of a sum of K random-sign terms grows like sqrt(K) * 2^-24 relative to the result; 4 * sqrt(K) * 2^-24 is 2e-5
        # at K = 2^12 and 2.4e-4 at K = 2^20 (c5: 256 images of 64x64), far below one missing K block (~6 %).
        tol = max(F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24)
        return {"dW f32": SL.per_tap_err(dw.values().reshape(4, 4, cg, cd), ref) * F32_TOL / tol}

    launch = Launch([dw], go, evaluate)
    launch.keep = (keep_hi, keep_lo, ws)
    return launch


def _norm_fwd(name, a, rng):
    """p2p_norm_act_fwd / p2p_norm_act_fwd_tail"""
    dtype, N, H, W, Cc = a[:5]
    raw_kind, nslabs, slab_stride = a[6], a[7], a[8]
    has_norm = a[9] is not None
    eps, act, alpha = a[11], a[12], a[13]
    nsplit = a[20]
    tdt, esz = U.tdt(dtype), _esz(dtype)
    pix = N * H * W
    if raw_kind == 2:
        sl = (rng.normal(size=(nslabs, slab_stride)) * 0.8 + 0.1).astype(np.float32)
        acc = np.zeros((pix, Cc), np.float32)
        for k in range(nslabs):
            acc = acc + sl[k, :pix * Cc].reshape(pix, Cc)
        x = U.q(acc, dtype).reshape(N, H, W, Cc)
        raw_t = torch.as_tensor(sl.reshape(-1)).to(U.DEV)
    else:
        x = U.q(rng.normal(size=(N, H, W, Cc)) * 2 + 0.3, dtype)
        raw_t = torch.as_tensor(x.reshape(-1)).to(U.DEV).to(tdt)
    gamma = (1 + 0.2 * rng.normal(size=Cc)).astype(np.float32)
    beta = (0.2 * rng.normal(size=Cc)).astype(np.float32)
    g_d, b_d = U.dev(gamma), U.dev(beta)
    mask = rng.integers(0, 2, size=(N, H, W, Cc)).astype(np.uint8) if a[14] is not None else None
    mask_d = U.dev(mask.reshape(-1), torch.uint8) if mask is not None else None
    tail_ch = a[22] if name == "p2p_norm_act_fwd_tail" else 0
    out = OutBuf(a[15][1], N, H, W, Cc + tail_ch, tdt, esz)     # the tail channels follow this layer's channels in the view
    outs = [out]
    raw_out = None
    if a[16] is not None:
        raw_out = OutBuf({"ld": Cc, "coff": 0, "row_stride": W, "img_stride": H * W, "align": a[16][1]}, N, H, W, Cc, tdt, esz)
        outs.append(raw_out)
    stats = None
    if a[17] is not None:
        stats = FlatOut(N * Cc * 2, a[17][1])
        outs.append(stats)
    ws_bytes = a[19]
    ws = torch.full((max(ws_bytes // 4, 4),), float("nan"), dtype=torch.float32, device=U.DEV)
    if nsplit < 0:
        # apply-only pass over statistics slots written by a convolution epilogue: slot k holds the mean and the centred sum of
        # squares of the k-th run of H*W/slots pixels of the image -- disjoint groups with different moments, so the kernel must
        # pool them (parallel-variance rule) to reach the image's mean and variance
        slots = -nsplit
        assert (H * W) % slots == 0, (H, W, slots)
        grp = x.astype(np.float64).reshape(N, slots, H * W // slots, Cc)
        mom = np.stack([grp.mean(axis=2), ((grp - grp.mean(axis=2, keepdims=True)) ** 2).sum(axis=2)], axis=-1)   # [N][slots][C][2]
        ws[:N * slots * Cc * 2] = torch.as_tensor(mom.reshape(-1).astype(np.float32)).to(U.DEV)
    tail = None
    if tail_ch:
        tail = U.q(rng.normal(size=(N, H, W, tail_ch)), dtype)
        keep_tail, tail_v = in_view(a[21][1], tail, dtype, rng)

    def go():
        args = (dtype, N, H, W, Cc, U.ptr(raw_t), raw_kind, nslabs, slab_stride, U.ptr(g_d) if has_norm else None,
                U.ptr(b_d) if has_norm else None, eps, act, alpha, U.ptr(mask_d) if mask is not None else None, C.byref(out.view),
                C.c_void_p(raw_out.view.ptr) if raw_out else None, stats.ptr() if stats else None, U.ptr(ws), ws_bytes, nsplit)
        if name == "p2p_norm_act_fwd_tail":
            L.call(name, *args, C.byref(tail_v), a[22], U.stream())
        else:
            L.call(name, *args, U.stream())

    def evaluate():
        errs = {}
        imgs = SL.image_set(N, seed=N * 5 + H)
        want = SL.norm_act(x[imgs], gamma if has_norm else None, beta if has_norm else None, eps, act, alpha,
                           mask[imgs] if mask is not None else None)
        pre = SL.norm_act(x[imgs], gamma if has_norm else None, beta if has_norm else None, eps, 0, 0.0) * (2.0 if mask is not None else 1.0)
        reg = out.region()
        errs["norm out"] = SL.per_image_channel_err(reg[imgs][..., :Cc], want, np.maximum(np.abs(want), np.abs(pre)))
        if tail is not None:
            assert np.array_equal(reg[..., Cc:], tail.astype(np.float64)), "tail channels"
        if raw_out is not None:
            assert np.array_equal(raw_out.region(), x.astype(np.float64)), "raw_out is not the rounded slab sum"
        if stats is not None and has_norm:
            st_v = stats.values().reshape(N, Cc, 2)
            errs["stats"] = SL.moment_err(st_v[..., 0], 1.0 / st_v[..., 1].astype(np.float64) ** 2 - eps, x, eps=eps)
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (raw_t, g_d, b_d, mask_d, ws) + ((keep_tail,) if tail is not None else ())
    return launch


def _act_bwd(name, a, rng):
    """p2p_act_bwd: draw = (g1 + g2) * (act_out > 0 ? 1 : alpha)"""
    dtype, N, H, W, Cc = a[:5]
    alpha = a[8]
    gate = U.q(rng.normal(size=(N, H, W, Cc)), dtype)
    keep_gate, gate_v = in_view(a[5][1], gate, dtype, rng)
    k1, g1, r1 = gsrc_in(a[6][1], N, H, W, Cc, dtype, rng)
    k2, g2, r2 = gsrc_in(a[7][1], N, H, W, Cc, dtype, rng) if a[7] is not None else (None, None, 0.0)
    out = OutBuf(a[9][1], N, H, W, Cc, U.tdt(dtype), _esz(dtype))

    def go():
        L.call(name, dtype, N, H, W, Cc, C.byref(gate_v), C.byref(g1), C.byref(g2) if g2 is not None else None, alpha,
               C.byref(out.view), U.stream())

    def evaluate():
        want = (r1 + r2) * np.where(gate > 0, 1.0, alpha)
        return {"out " + ("bf16" if dtype == L.BF16 else "f32"): SL.per_image_err(out.region(), want)}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep_gate, k1, k2)
    return launch


def _norm_bwd(name, a, rng):
    """p2p_norm_act_bwd: d(raw) of y = act(drop(InstanceNorm(raw))) for dy = g1 + g2, and the per-image dgamma / dbeta partials"""
    dtype, N, H, W, Cc = a[:5]
    act, alpha = a[9], a[10]
    assert a[6] is not None and a[7] is not None, "the backward pass of a block without normalisation"
    tdt, esz = U.tdt(dtype), _esz(dtype)
    eps = rg.IN_EPS                # (the backward pass reads mean / rstd from stats; eps is not an argument)
    x = U.q(rng.normal(size=(N, H, W, Cc)) * 2 + 0.3, dtype)
    xd = x.astype(np.float64)
    mean, var = xd.mean(axis=(1, 2)), xd.var(axis=(1, 2))
    stats = np.stack([mean, 1.0 / np.sqrt(var + eps)], axis=-1).astype(np.float32)       # what the forward pass leaves
    gamma = (1 + 0.2 * rng.normal(size=Cc)).astype(np.float32)
    beta = (0.2 * rng.normal(size=Cc)).astype(np.float32)
    mask = rng.integers(0, 2, size=(N, H, W, Cc)).astype(np.uint8) if a[11] is not None else None
    # the gradient sources are zero where the activation's input is within 1e-3 of 0: an f32 gate that rounds to the other side
    # of 0 than the f64 one then changes nothing (at batch 256 the compared planes hold ~10^7 elements)
    pre = SL.norm_act(xd, gamma, beta, eps, 0, 0.0)
    live = (np.abs(pre) > 1e-3).reshape(N * H * W, Cc)
    k1, g1, r1 = gsrc_in(a[12][1], N, H, W, Cc, dtype, rng, live)
    k2, g2, r2 = gsrc_in(a[13][1], N, H, W, Cc, dtype, rng, live) if a[13] is not None else (None, None, 0.0)
    raw_t = torch.as_tensor(x.reshape(-1)).to(U.DEV).to(tdt)
    st_d, g_d, b_d = U.dev(stats.reshape(-1)), U.dev(gamma), U.dev(beta)
    mask_d = U.dev(mask.reshape(-1), torch.uint8) if mask is not None else None
    draw = OutBuf(a[14][1], N, H, W, Cc, tdt, esz)
    dgam, dbet = FlatOut(N * Cc, a[15][1]), FlatOut(N * Cc, a[16][1])
    ws_bytes, nsplit = a[18], a[19]
    ws = torch.full((max(ws_bytes // 4, 4),), float("nan"), dtype=torch.float32, device=U.DEV)

    def go():
        L.call(name, dtype, N, H, W, Cc, U.ptr(raw_t), U.ptr(st_d), U.ptr(g_d), U.ptr(b_d), act, alpha,
               U.ptr(mask_d) if mask is not None else None, C.byref(g1), C.byref(g2) if g2 is not None else None, C.byref(draw.view),
               dgam.ptr(), dbet.ptr(), U.ptr(ws), ws_bytes, nsplit, U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=N * 3 + H)
        xt = torch.tensor(xd[imgs], requires_grad=True)
        gt = torch.tensor(gamma, dtype=torch.float64)
        bt = torch.tensor(beta, dtype=torch.float64)
        y = (xt - xt.mean(dim=(1, 2), keepdim=True)) * torch.rsqrt(xt.var(dim=(1, 2), unbiased=False, keepdim=True) + eps) * gt + bt
        if mask is not None:
            y = y * torch.tensor(mask[imgs], dtype=torch.float64) * 2.0
        y = torch.where(y > 0, y, alpha * y) if act == L.ACT_LEAKY else (torch.relu(y) if act == L.ACT_RELU else y)
        dy = torch.as_tensor((r1 + r2)[imgs] if a[13] is not None else r1[imgs])
        (y * dy).sum().backward()
        # per-image partials in closed form: dgamma_n = sum dz * xhat, dbeta_n = sum dz, dz = d(loss)/d(gamma * xhat + beta)
        xh = (xd[imgs] - mean[imgs][:, None, None]) / np.sqrt(var[imgs][:, None, None] + eps)
        z = xh * gamma + beta
        drop = mask[imgs] * 2.0 if mask is not None else 1.0
        zm = z * drop
        slope = np.where(zm > 0, 1.0, alpha if act == L.ACT_LEAKY else (0.0 if act == L.ACT_RELU else 1.0))
        dz = dy.numpy() * slope * drop
        fam = "d(raw) " + ("bf16" if dtype == L.BF16 else "f32")
        errs = {fam: SL.per_image_err(draw.region()[imgs], xt.grad.numpy())}
        want_g, want_b = (dz * xh).sum(axis=(1, 2)), dz.sum(axis=(1, 2))
        got_g, got_b = dgam.values().reshape(N, Cc)[imgs], dbet.values().reshape(N, Cc)[imgs]
        errs["dgamma/dbeta"] = max(SL.per_image_err(got_g, want_g), SL.per_image_err(got_b, want_b))
        return errs

    launch = Launch([draw, dgam, dbet], go, evaluate)
    launch.keep = (k1, k2, raw_t, st_d, g_d, b_d, mask_d, ws)
    return launch


def _sprites(rng, N, S):
    """real sprites and a noisy 'fake' of them (f32 NHWC in [-1, 1], alpha channel included)"""
    _, real = DU.synthetic_rgba_batch(rng, N, S, palette_size=24)
    fake = np.clip(real + rng.normal(scale=0.05, size=real.shape), -1, 1).astype(np.float32)
    return np.asarray(real, np.float32), fake


def _hist_ref(img):
    """normalised histograms [n,64,64,3] of f32 images, float64, a few images at a time"""
    return np.concatenate([rg.rgbuv_histogram(torch.tensor(img[i:i + 4], dtype=torch.float64)).numpy()
                           for i in range(0, len(img), 4)])


def _raw_to_norm(raw, N):
    """raw histograms [N][3][64][64] -> [N][64][64][3] divided by the per-image total (p2p_hist_normalize)"""
    r = np.asarray(raw, np.float64).reshape(N, 3, 64, 64).transpose(0, 2, 3, 1)
    return r / r.sum(axis=(1, 2, 3), keepdims=True)


def _points(name, a, rng):
    """p2p_rgbuv_points: the distinct colours of every tile of 1024 pixels with their pixel counts"""
    dtype, N, H, W, _, cap = a[:6]
    real, _ = _sprites(rng, N, H)
    keep, view = in_view(a[4][1], real, dtype, rng)
    pts = FlatOut(N * cap * 4, a[6][1])
    npts = torch.full((N + 64,), -7, dtype=torch.int32, device=U.DEV)

    def go():
        pts.flat[:pts.numel] = 0.0           # entries past npoints[n] are not written
        L.call(name, dtype, N, H, W, C.byref(view), cap, pts.ptr(), U.ptr(npts), U.stream())

    def evaluate():
        assert bool((pts.flat[pts.numel:] == SENTINEL).all()), "points written past N * cap entries"
        got_n = npts[:N].cpu().numpy()
        assert (npts[N:] == -7).all(), "npoints written past N"
        p = pts.values().reshape(N, cap, 4)
        tiles = (H * W + 1023) // 1024
        for n in SL.image_set(N, seed=N):
            rgb = real[n].reshape(-1, 4)[:, :3]
            colours = np.unique(rgb, axis=0)
            k = int(got_n[n])
            if k < 0:
                assert len(colours) > cap // tiles, (n, len(colours))
                continue
            want = {}
            for t in range(tiles):
                u, c = np.unique(rgb[t * 1024:(t + 1) * 1024], axis=0, return_counts=True)
                for col, cnt in zip(map(tuple, u), c):
                    want.setdefault(col, []).append(int(cnt))
            got = {}
            for r in p[n, :k]:
                got.setdefault(tuple(np.float32(r[:3])), []).append(int(r[3]))
            assert sorted(got) == sorted(want) and all(sorted(got[c]) == sorted(want[c]) for c in want), f"image {n}: colour list"
        return {"points": 0.0}

    launch = Launch([], go, evaluate)
    launch.keep = (keep, pts, npts)
    launch.fixed = (pts.flat, npts)
    return launch


def _hist_fwd3(name, a, rng):
    """p2p_rgbuv_hist_fwd3 (with the colour list of p2p_rgbuv_points where the step passes one): raw histograms [N][3][64][64]"""
    dtype, N, H, W = a[:4]
    cap = a[7]
    real, _ = _sprites(rng, N, H)
    keep, view = in_view(a[4][1], real, dtype, rng)
    hist = FlatOut(N * 3 * 64 * 64, a[8][1])
    ws = torch.full((L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4 + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    pts = npts = None
    if a[5] is not None:
        pts = torch.zeros(N * cap * 4 + 4, dtype=torch.float32, device=U.DEV)
        npts = torch.zeros(N, dtype=torch.int32, device=U.DEV)
        L.call("p2p_rgbuv_points", dtype, N, H, W, C.byref(view), cap, U.ptr(pts), U.ptr(npts), U.stream())

    def go():
        L.call(name, dtype, N, H, W, C.byref(view), U.ptr(pts) if pts is not None else None,
               U.ptr(npts) if npts is not None else None, cap, hist.ptr(), U.ptr(ws), U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=N + H)
        got = _raw_to_norm(hist.values(), N)[imgs]
        return {"histogram": SL.per_image_err(got, _hist_ref(real[imgs]))}

    launch = Launch([hist], go, evaluate)
    launch.keep = (keep, ws, pts, npts)
    return launch


def _hist_bwd3(name, a, rng):
    """p2p_rgbuv_hist_hellinger_bwd3: coef * d(sum_n s_n)/d(fake) / sqrt(sq_sum), s_n = sum (sqrt(p_n) - sqrt(t_n))^2 of the
    normalised histograms (histogram.py:84-89; coef = lambda / (2 sqrt(2) B)).  The histogram inputs are produced by
    p2p_rgbuv_hist_fwd3 (checked against f64 by its own re-issue); the gradient is compared with f64 autograd of the oracle."""
    dtype, N, H, W = a[:4]
    coef = a[10]
    real, fake = _sprites(rng, N, H)
    keep_f, fview = in_view(a[4][1], fake, dtype, rng)
    rt = torch.as_tensor(real).to(U.DEV).contiguous()
    rview = L.Tensor(rt.data_ptr(), H * W, W, 4)
    ws = torch.empty(L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(N) // 4 + 4, dtype=torch.float32, device=U.DEV)
    h_r, h_f = (torch.empty(N * 3 * 64 * 64, dtype=torch.float32, device=U.DEV) for _ in range(2))
    for v, out in ((rview, h_r), (fview, h_f)):
        L.call("p2p_rgbuv_hist_fwd3", dtype, N, H, W, C.byref(v), None, None, 1024, U.ptr(out), U.ptr(ws), U.stream())
    hr, hf = h_r.double().cpu().numpy().reshape(N, -1), h_f.double().cpu().numpy().reshape(N, -1)
    tot_r, tot_f = hr.sum(axis=1), hf.sum(axis=1)
    sq = float(((np.sqrt(hf / tot_f[:, None]) - np.sqrt(hr / tot_r[:, None])) ** 2).sum())
    tot = U.dev(np.stack([tot_r, tot_f]).astype(np.float32))
    sq_d = U.dev(np.array([sq, 0, 0, 0], np.float32))
    gh = torch.full((N * 3 * 64 * 64,), float("nan"), dtype=torch.float32, device=U.DEV)
    dimg = FlatOut(N * H * W * 4, a[12][1])

    def go():
        L.call(name, dtype, N, H, W, C.byref(fview), U.ptr(h_r), U.ptr(h_f), U.ptr(tot[0]), U.ptr(tot[1]), U.ptr(sq_d), coef, U.ptr(gh),
               dimg.ptr(), U.stream())

    def evaluate():
        imgs = SL.image_set(N, seed=2 * N + H)
        got = dimg.values().reshape(N, H, W, 4)[imgs]
        assert not got[..., 3].any(), "alpha gradient"
        t_ref = _hist_ref(real[imgs])
        ref = np.zeros_like(got)
        for j in range(0, len(imgs), 4):
            ft = torch.tensor(fake[imgs[j:j + 4]], dtype=torch.float64, requires_grad=True)
            s = ((torch.sqrt(rg.rgbuv_histogram(ft)) - torch.sqrt(torch.tensor(t_ref[j:j + 4]))) ** 2).sum()
            s.backward()
            ref[j:j + 4] = ft.grad.numpy() * coef / np.sqrt(sq)
        return {"hist grad": SL.per_image_err(got, ref)}

    launch = Launch([dimg], go, evaluate)
    launch.keep = (keep_f, rt, ws, h_r, h_f, tot, sq_d, gh)
    return launch


def _head_dgrad(name, a, rng, operands="gaussian"):
    """p2p_head_dgrad: op P, stride 1, of the indexed head into the first `cout` channels of the output view.
    operands="lattice": every image, exact"""
    lat = _lattice_mode(operands)
    dtype, N, H, W, ncls, cout = a[:6]
    w_rows = a[8]
    step = sx = 1.0
    if lat:
        dz, sx = LT.operands(rng, (N, H, W, ncls), "x", 16 * ncls, dtype, dtype == L.BF16)
        w, sw = LT.operands(rng, (4, 4, cout, ncls), "w", 16 * ncls, dtype, dtype == L.BF16)
        step = sx * sw
        keep, dzv = in_view(a[6][1], dz, dtype, rng, _other(lat, rng, sx))
    else:
        dz = U.q(rng.normal(size=(N, H, W, ncls)), dtype)
        keep, dzv = in_view(a[6][1], dz, dtype, rng)
        w = U.q(rng.normal(scale=1.0 / np.sqrt(16 * ncls), size=(4, 4, cout, ncls)), dtype)
    wn = _prep(dtype, w, cout, ncls, wn_shape=(w_rows, ncls))
    out = OutBuf(a[9][1], N, H, W, cout, U.tdt(dtype), _esz(dtype))

    def go():
        L.call(name, dtype, N, H, W, ncls, cout, C.byref(dzv), U.ptr(wn), w_rows, C.byref(out.view), U.stream())

    def evaluate():
        if lat:
            errs, msgs = {}, []
            conv = SL.conv_p(dz, w, 1)
            _exact_family(errs, msgs, "exact out", out.region(), LT.expected(conv, dtype), step, ("image", "y", "x", "channel"))
            _sensitive(errs, dtype, LT.to_int(conv, step))
            assert not msgs, "; ".join(msgs)
            return errs
        imgs = SL.image_set(N, seed=N + 11)
        return {"out bf16": SL.per_image_err(out.region()[imgs], SL.conv_p(dz[imgs], w, 1))}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep, wn)
    return launch


def _head_softmax(name, a, rng):
    """p2p_head_softmax_cce: Conv2D(ncls, 4, stride 1, SAME, bias) + softmax + CCE + argmax + gradient + bias gradient"""
    dtype, N, H, W, cin_pad, ncls = a[:6]
    gscale, inv = a[11], a[12]
    x = U.q(rng.normal(size=(N, H, W, cin_pad)), dtype)
    keep_x, xv = in_view(a[6][1], x, dtype, rng)
    w = U.q(rng.normal(scale=2.0 / np.sqrt(16 * cin_pad), size=(4, 4, cin_pad, ncls)), dtype)
    wt = _prep(dtype, w, cin_pad, ncls, wt_shape=(ncls, cin_pad))
    bias = (0.1 * rng.normal(size=ncls)).astype(np.float32)
    bias_d = U.dev(bias)
    tgt = rng.integers(0, ncls, size=(N, H, W, 1)).astype(np.float32)
    keep_t, tv = in_view(a[9][1], tgt, dtype, rng)
    fidx = OutBuf(a[10][1], N, H, W, 1, U.tdt(dtype), _esz(dtype))
    dz = OutBuf(a[13][1], N, H, W, ncls, U.tdt(dtype), _esz(dtype))
    outs = [fidx, dz]
    dbias = None
    if a[14] is not None:
        dbias = FlatOut(ncls, a[14][1])
        outs.append(dbias)
    ws = torch.full((L.lib().p2p_head_softmax_workspace_bytes(N, H) // 4 + 4,), float("nan"), dtype=torch.float32, device=U.DEV)
    loss = FlatOut(2, a[16][1])
    outs.append(loss)

    def go():
        L.call(name, dtype, N, H, W, cin_pad, ncls, C.byref(xv), U.ptr(wt), U.ptr(bias_d), C.byref(tv), C.byref(fidx.view), gscale, inv,
               C.byref(dz.view), dbias.ptr() if dbias else None, U.ptr(ws), loss.ptr(), U.stream())

    def evaluate():
        imgs = set(SL.image_set(N, seed=N + 13))
        got_dz, got_idx = dz.region(), fidx.region()[..., 0]
        onehot_err = cce = 0.0
        worst_dz, argmax_bad, argmax_n = 0.0, 0, 0
        for j in range(0, N, 8):            # whole batch: the losses are batch sums
            z = SL.conv_g(x[j:j + 8], w, 1) + bias
            zt = torch.tensor(z)
            logp = torch.log_softmax(zt, -1)
            p = logp.exp().numpy()
            ti = tgt[j:j + 8, ..., 0].astype(np.int64)
            cce += float(-np.take_along_axis(logp.numpy(), ti[..., None], -1).sum())
            oh = np.eye(ncls)[ti]
            onehot_err += float(np.abs(oh - p).sum())
            sel = [i - j for i in range(j, min(j + 8, N)) if i in imgs]
            if sel:
                worst_dz = max(worst_dz, SL.per_image_err(got_dz[j:j + 8][sel], gscale * (p - oh)[sel]))
                top2 = np.sort(p[sel], -1)[..., -2:]
                clear = (top2[..., 1] - top2[..., 0]) > 1e-6 * top2[..., 1]
                argmax_bad += int(((got_idx[j:j + 8][sel] != p[sel].argmax(-1)) & clear).sum())
                argmax_n += int(clear.size)
        assert argmax_bad == 0, f"{argmax_bad} of {argmax_n} argmax indices differ from f64"
        lv = loss.values()
        errs = {"out bf16": worst_dz}
        k = N * H * W
        long_k = max(F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24) / F32_TOL       # long-K f32 sums: see _wgrad_family
        errs["loss f32"] = max(abs(lv[0] - inv * cce) / (inv * cce), abs(lv[1] - inv / ncls * onehot_err) / (inv / ncls * onehot_err)) / long_k
        if dbias is not None:       # column sums of the stored (rounded) gradient
            want = got_dz.sum(axis=(0, 1, 2))
            errs["dbias f32"] = float(np.abs(dbias.values() - want).max() / np.abs(want).max()) / long_k
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (keep_x, wt, bias_d, keep_t, ws)
    return launch


# ---------------------------------------------------------------------------------------------------------------- step plumbing
LOSS_BLOCKS = 256                 # P2P_LOSS_BLOCKS (include/p2pgan.h): one loss partial per workgroup and term
ADAM_LR = 2e-4                    # (the step size enters through lr_t_dev; any value serves)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _long_k(k):
    """the bound of a sum of k f32 terms relative to F32_TOL (see _wgrad_family)"""
    return max(F32_TOL, 4 * np.sqrt(k) * 2.0 ** -24) / F32_TOL


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


class Buf:
    """A test-owned flat buffer holding `init` followed by TAIL sentinel elements.  The elements in `written` are what the launch
    writes (NaN before the launch when `nan`) or updates in place (restored by reset); every other element must be bit-for-bit
    unchanged after the launch."""

    def __init__(self, init, written=None, nan=False, align=0):
        init = init.reshape(-1).to(U.DEV)
        n, esz = init.numel(), init.element_size()
        self.numel = n
        fill = SENTINEL if init.is_floating_point() else (0xA5 if init.dtype == torch.uint8 else -7)
        self.all = torch.empty(n + TAIL + 16, dtype=init.dtype, device=U.DEV)
        s = next(s for s in range(16) if (self.all.data_ptr() + esz * s) % 16 == align)
        self.flat = self.all[s:s + n + TAIL]
        self._init = torch.cat([init, torch.full((TAIL,), fill, dtype=init.dtype, device=U.DEV)])
        self.written = torch.zeros(n + TAIL, dtype=torch.bool, device=U.DEV)
        if written is not None:
            self.written[:n] = written.reshape(-1).to(U.DEV)
        self.nan = nan
        self.reset()

    def reset(self):
        self.flat.copy_(self._init)
        if self.nan:
            self.flat[self.written] = float("nan")
        self._before = self.flat.clone()

    def ptr(self, off=0):
        return C.c_void_p(self.flat.data_ptr() + off * self.flat.element_size())

    def body(self):
        return self.flat[:self.numel]

    def check_around(self, what):
        keep = ~self.written
        assert torch.equal(_bits(self.flat[keep]), _bits(self._before[keep])), f"{what}: an element outside the written range changed"
        if self.nan:
            r = self.flat[self.written]
            assert not bool(torch.isnan(r).any()), f"{what}: {int(torch.isnan(r).sum())} elements were not written"


def _out_all(numel, tdt, align=0):
    """a flat output every element of which the launch writes"""
    return Buf(torch.zeros(numel, dtype=tdt), torch.ones(numel, dtype=torch.bool), nan=True, align=align)


def _half_out(desc, n, h, w, skip, nc, tdt, esz):
    """OutBuf for channels [skip, skip + nc) of a recorded view, and the view as the kernel gets it (from channel 0)"""
    d = dict(desc, coff=desc["coff"] + skip, align=(desc["align"] + skip * esz) % 16)
    ob = OutBuf(d, n, h, w, nc, tdt, esz)
    return ob, L.Tensor(ob.view.ptr - skip * esz, ob.view.img_stride, ob.view.row_stride, ob.view.ld)


def _vd(h, w, ld, coff=0, halo=0, align=0):
    """a view description (as _decode makes it) for the direct tests: [h][w] pixels with a halo ring, ld channels"""
    rs = w + 2 * halo
    return {"img_stride": (h + 2 * halo) * rs, "row_stride": rs, "ld": ld, "align": align, "coff": coff, "pix": halo * rs + halo}


# ---- losses
def _bce(name, a, rng):
    """p2p_bce_logits(_pad8): BCE partials of D(real) / D(fake) and the gradients (pix2pix_model.py:44-56)"""
    dtype, N2, n_real, H, W = a[:5]
    inv = a[6]
    pad8 = name == "p2p_bce_logits_pad8"
    tdt, esz = U.tdt(dtype), _esz(dtype)
    x = U.q(rng.normal(size=(N2, H, W, 1)) * 3, dtype)
    keep, lv = in_view(a[5][1], x, dtype, rng)
    nc = 8 if pad8 else 1
    dld = OutBuf(a[7][1], N2, H, W, nc, tdt, esz)
    dlg = OutBuf(a[8][1], N2 - n_real, H, W, nc, tdt, esz) if a[8] is not None else None
    part = FlatOut(3 * LOSS_BLOCKS, a[9][1])
    outs = [dld, part] + ([dlg] if dlg else [])

    def go():
        L.call(name, dtype, N2, n_real, H, W, C.byref(lv), inv, C.byref(dld.view), C.byref(dlg.view) if dlg else None, part.ptr(),
               U.stream())

    def evaluate():
        xd = x[..., 0].astype(np.float64)
        s = 1.0 / (1.0 + np.exp(-xd))
        sp = np.maximum(xd, 0) + np.log1p(np.exp(-np.abs(xd)))           # BCE(0, x); BCE(1, x) = sp - x
        real = (np.arange(N2) < n_real)[:, None, None]
        fam = "out " + ("bf16" if dtype == L.BF16 else "f32")
        got = dld.region()
        errs = {fam: SL.per_image_err(got[..., 0], np.where(real, s - 1.0, s) * inv)}
        if pad8:
            assert (got[..., 1:] == 0).all(), f"{name}: padding channels of dlogits_d are not 0"
        if dlg is not None:
            gg = dlg.region()
            errs[fam] = max(errs[fam], SL.per_image_err(gg[..., 0], (s[n_real:] - 1.0) * inv))
            if pad8:
                assert (gg[..., 1:] == 0).all(), f"{name}: padding channels of dlogits_g are not 0"
        rows = part.values().reshape(3, LOSS_BLOCKS).sum(axis=1)
        want = [inv * (sp[:n_real] - xd[:n_real]).sum(), inv * sp[n_real:].sum(), inv * (sp[n_real:] - xd[n_real:]).sum()]
        errs["loss f32"] = max(abs(r - w) / max(abs(w), 1e-30) for r, w in zip(rows, want)) / _long_k(N2 * H * W)
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (keep,)
    return launch


def _tanh_fwd(name, a, rng):
    """p2p_tanh_l1_fwd(_pair): fake = tanh(z) in the activation dtype (pair form: [fake | source] pixels, the source half copied
    from real_pair), the unrounded f32 copy and the L1 partials against the stored fake"""
    pair = name == "p2p_tanh_l1_fwd_pair"
    if pair:
        dtype, N, H, W = a[:4]
        Cc, zd, rd, fd, inv, pi, fi = 4, a[4][1], a[5][1], a[6][1], a[7], 8, 9
    else:
        dtype, N, H, W, Cc = a[:5]
        zd, rd, fd, inv, pi, fi = a[5][1], a[6][1], a[7][1], a[8], 9, 10
    tdt, esz = U.tdt(dtype), _esz(dtype)
    rc = 8 if pair else Cc
    z = U.q(rng.normal(size=(N, H, W, Cc)) * 1.5, dtype)
    real = U.q(rng.uniform(-1, 1, size=(N, H, W, rc)), dtype)
    keep_z, zv = in_view(zd, z, dtype, rng)
    keep_r, rv = in_view(rd, real, dtype, rng)
    fake = OutBuf(fd, N, H, W, rc, tdt, esz)
    part = FlatOut(LOSS_BLOCKS, a[pi][1])
    f32 = FlatOut(N * H * W * Cc, a[fi][1]) if a[fi] is not None else None
    outs = [fake, part] + ([f32] if f32 else [])

    def go():
        shape = (N, H, W) if pair else (N, H, W, Cc)
        L.call(name, dtype, *shape, C.byref(zv), C.byref(rv), C.byref(fake.view), inv, part.ptr(), f32.ptr() if f32 else None,
               U.stream())

    def evaluate():
        t = np.tanh(z.astype(np.float64))
        got = fake.region()
        errs = {"out " + ("bf16" if dtype == L.BF16 else "f32"): SL.per_image_err(got[..., :Cc], t)}
        if pair:
            assert np.array_equal(got[..., 4:], real[..., 4:].astype(np.float64)), f"{name}: the source half is not a copy of real_pair's"
        if f32 is not None:
            errs["fake f32"] = SL.per_image_err(f32.values().reshape(N, H, W, Cc), t)
        want = inv * np.abs(real[..., :Cc].astype(np.float64) - got[..., :Cc]).sum()
        errs["loss f32"] = abs(part.values().sum() - want) / max(abs(want), 1e-30) / _long_k(N * H * W * Cc)
        return errs

    launch = Launch(outs, go, evaluate)
    launch.keep = (keep_z, keep_r)
    return launch


def _tanh_bwd(name, a, rng):
    """p2p_tanh_l1_bwd(_pad8): dz = (g_d + g_extra + l1_scale * sign(fake - real)) * (1 - fake^2); some real values equal fake
    (sign 0).  The gradient sources are scaled to l1_scale so that the L1 term is visible"""
    pad8 = name == "p2p_tanh_l1_bwd_pad8"
    if pad8:
        dtype, N, H, W = a[:4]
        Cc, o = 4, 4
    else:
        dtype, N, H, W, Cc = a[:5]
        o = 5
    fd, rd, gdd, gxd, l1, dzd = a[o][1], a[o + 1][1], a[o + 2], a[o + 3], a[o + 4], a[o + 5][1]
    tdt, esz = U.tdt(dtype), _esz(dtype)
    f = U.q(np.tanh(rng.normal(size=(N, H, W, Cc)) * 1.5), dtype)
    r = U.q(rng.uniform(-1, 1, size=(N, H, W, Cc)), dtype)
    eq = rng.random(size=f.shape) < 0.15
    r[eq] = f[eq]
    keep_f, fv = in_view(fd, f, dtype, rng)
    keep_r, rv = in_view(rd, r, dtype, rng)
    sc = abs(l1) if l1 else 1.0
    k1, g1, r1 = gsrc_in(gdd[1], N, H, W, Cc, dtype, rng, scale=sc) if gdd is not None else (None, None, 0.0)
    k2, g2, r2 = gsrc_in(gxd[1], N, H, W, Cc, dtype, rng, scale=sc) if gxd is not None else (None, None, 0.0)
    dz = OutBuf(dzd, N, H, W, 8 if pad8 else Cc, tdt, esz)

    def go():
        shape = (N, H, W) if pad8 else (N, H, W, Cc)
        L.call(name, dtype, *shape, C.byref(fv), C.byref(rv), C.byref(g1) if g1 else None, C.byref(g2) if g2 else None, l1,
               C.byref(dz.view), U.stream())

    def evaluate():
        fd64 = f.astype(np.float64)
        want = (r1 + r2 + l1 * np.sign(fd64 - r)) * (1.0 - fd64 ** 2)
        got = dz.region()
        if pad8:
            assert (got[..., 4:] == 0).all(), f"{name}: padding channels of dz are not 0"
        return {"out " + ("bf16" if dtype == L.BF16 else "f32"): SL.per_image_err(got[..., :Cc], want)}

    launch = Launch([dz], go, evaluate)
    launch.keep = (keep_f, keep_r, k1, k2)
    return launch


def _partials_sum(name, a, rng):
    """p2p_loss_partials_sum: out[k] = sum of the LOSS_BLOCKS partials of row k"""
    K = a[1]
    part = (rng.random(size=K * LOSS_BLOCKS) * 2 + 0.01).astype(np.float32)
    pd = U.dev(part)
    out = FlatOut(K, a[2][1])

    def go():
        L.call(name, U.ptr(pd), K, out.ptr(), U.stream())

    def evaluate():
        want = part.astype(np.float64).reshape(K, LOSS_BLOCKS).sum(axis=1)
        return {"loss f32": float((np.abs(out.values() - want) / want).max()) / _long_k(LOSS_BLOCKS)}

    launch = Launch([out], go, evaluate)
    launch.keep = (pd,)
    return launch


def _finish_losses(name, a, rng):
    """p2p_finish_losses against its formula (include/p2pgan.h): [g_total, g_adv, g_l1, g_aux, d_total, d_real, d_fake]"""
    aux, l1s, lam1, lamx = a[1], a[2], a[3], a[4]
    slots = (rng.random(size=8) + 0.1).astype(np.float32)
    sd = U.dev(slots)
    out = FlatOut(7, a[5][1])

    def go():
        L.call(name, U.ptr(sd), aux, l1s, lam1, lamx, out.ptr(), U.stream())

    def evaluate():
        s = slots.astype(np.float64)
        ax = s[aux] if aux >= 0 else 0.0
        want = [s[2] + lam1 * s[l1s] + lamx * ax, s[2], s[l1s], ax, s[0] + s[1], s[0], s[1]]
        got = out.values()
        for i in (1, 2, 3, 5, 6):
            assert got[i] == want[i], f"{name}: out[{i}] = {got[i]} is not slot value {want[i]} (aux_slot {aux}, l1_slot {l1s})"
        return {"loss f32": max(abs(got[i] - want[i]) / abs(want[i]) for i in (0, 4))}

    launch = Launch([out], go, evaluate)
    launch.keep = (sd,)
    return launch


def _raw_hists(rng, N):
    x = rng.random(size=(N, 3 * 64 * 64)) ** 3 * 50
    x[rng.random(size=x.shape) < 0.2] = 0.0
    return x.astype(np.float32)


def _hellinger_fwd(name, a, rng):
    """p2p_hellinger_fwd: per-image totals of both raw histograms, per-image and summed Hellinger sums of squares"""
    N = a[2]
    E = 3 * 64 * 64
    ht, hp = _raw_hists(rng, N), _raw_hists(rng, N)
    htd, hpd = U.dev(ht.reshape(-1)), U.dev(hp.reshape(-1))
    tt, tp, sqp, sq = FlatOut(N, a[3][1]), FlatOut(N, a[4][1]), FlatOut(N, a[5][1]), FlatOut(1, a[6][1])

    def go():
        L.call(name, U.ptr(htd), U.ptr(hpd), N, tt.ptr(), tp.ptr(), sqp.ptr(), sq.ptr(), U.stream())

    def evaluate():
        T, Pp = ht.astype(np.float64).sum(axis=1), hp.astype(np.float64).sum(axis=1)
        s = ((np.sqrt(hp / Pp[:, None]) - np.sqrt(ht / T[:, None])) ** 2).sum(axis=1)
        e = max(float((np.abs(tt.values() - T) / T).max()), float((np.abs(tp.values() - Pp) / Pp).max()),
                float((np.abs(sqp.values() - s) / s).max())) / _long_k(E)
        return {"loss f32": max(e, abs(sq.values()[0] - s.sum()) / s.sum() / _long_k(E * N))}

    launch = Launch([tt, tp, sqp, sq], go, evaluate)
    launch.keep = (htd, hpd)
    return launch


def _hellinger_finish(name, a, rng):
    """p2p_hellinger_finish: loss = sqrt(sq_sum) / sqrt(2) * inv_global_batch"""
    inv = a[1]
    sq = float(np.float32(rng.random() * 3 + 0.5))
    sqd = U.dev(np.array([sq, 0, 0, 0], np.float32))
    out = FlatOut(1, a[2][1])

    def go():
        L.call(name, U.ptr(sqd), inv, out.ptr(), U.stream())

    def evaluate():
        want = np.sqrt(sq) / np.sqrt(2.0) * inv
        return {"loss f32": abs(out.values()[0] - want) / want}

    launch = Launch([out], go, evaluate)
    launch.keep = (sqd,)
    return launch


def _hist_normalize(name, a, rng):
    """p2p_hist_normalize: raw [N][3][64][64] -> [N][64][64][3] / per-image total"""
    N = a[1]
    raw = _raw_hists(rng, N)
    rd = U.dev(raw.reshape(-1))
    out = FlatOut(N * 3 * 64 * 64, a[2][1])

    def go():
        L.call(name, U.ptr(rd), N, out.ptr(), U.stream())

    def evaluate():
        return {"histogram": SL.per_image_err(out.values().reshape(N, 64, 64, 3), _raw_to_norm(raw, N))}

    launch = Launch([out], go, evaluate)
    launch.keep = (rd,)
    return launch


# ---- reductions
def _colsum(name, a, rng, operands="gaussian"):
    """p2p_colsum: out[c] = scale * sum_r part[r][c].  operands="lattice": exact (one f32 multiply by the scale, which rounds once
    whether it is applied to the sum or -- a power of two -- to the terms)"""
    lat = _lattice_mode(operands)
    rows, cols, scale = a[1], a[2], a[3]
    if lat:
        part, step = LT.operands(rng, (rows, cols), "x", rows, L.F32, False)
    else:
        part = rng.normal(0.3, 1.0, size=(rows, cols)).astype(np.float32)
    pd = U.dev(part.reshape(-1))
    out = FlatOut(cols, a[4][1])

    def go():
        L.call(name, U.ptr(pd), rows, cols, scale, out.ptr(), U.stream())

    def evaluate():
        if lat:
            errs, msgs = {}, []
            want = np.float32(scale) * LT.expected(part.astype(np.float64).sum(axis=0), L.F32)
            _exact_family(errs, msgs, "exact colsum", out.values(), want, step * scale, ("column",))
            assert not msgs, "; ".join(msgs)
            return errs
        return {"colsum f32": _rel(out.values(), scale * part.astype(np.float64).sum(axis=0)) / _long_k(rows)}

    launch = Launch([out], go, evaluate)
    launch.keep = (pd,)
    return launch


def _view_colsum(name, a, rng, operands="gaussian"):
    """p2p_view_colsum: column sums over every pixel of a view (bias gradients), with its workspace.  operands="lattice": exact"""
    lat = _lattice_mode(operands)
    dtype, N, H, W, Cc = a[:5]
    step = 1.0
    if lat:
        x, step = LT.operands(rng, (N, H, W, Cc), "x", N * H * W, dtype, False)
    else:
        x = U.q(rng.normal(0.3, 1.0, size=(N, H, W, Cc)), dtype)
    keep, vv = in_view(a[5][1], x, dtype, rng, _other(lat, rng, step))
    out = FlatOut(Cc, a[6][1])
    need = L.lib().p2p_view_colsum_workspace_bytes(dtype, N, H, W, Cc, C.byref(vv)) // 4
    ws = torch.full((max(need, 16),), float("nan"), dtype=torch.float32, device=U.DEV)

    def go():
        L.call(name, dtype, N, H, W, Cc, C.byref(vv), out.ptr(), U.ptr(ws), U.stream())

    def evaluate():
        if lat:
            errs, msgs = {}, []
            _exact_family(errs, msgs, "exact colsum", out.values(), LT.expected(x.astype(np.float64).sum(axis=(0, 1, 2)), L.F32), step,
                          ("column",))
            assert not msgs, "; ".join(msgs)
            return errs
        return {"colsum f32": _rel(out.values(), x.astype(np.float64).sum(axis=(0, 1, 2))) / _long_k(N * H * W)}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep, ws)
    return launch


def _colsum_batched(name, a, rng, operands="gaussian"):
    """p2p_colsum_batched: task {part_off, rows, cols, out_off} sums a [rows][cols] block into out + out_off; the rest of the
    output buffer (the recorded one is the generator's flat gradient buffer) keeps its values.  operands="lattice": exact"""
    lat = _lattice_mode(operands)
    tasks = [tuple(t) for t in a[1][1]]
    ntasks, maxc = a[2], a[3]
    numel = a[4][2] - a[4][3]
    assert len(tasks) == ntasks and maxc == max(t[2] for t in tasks), (ntasks, maxc, tasks)
    if lat:
        part, step = LT.operands(rng, (max(po + r * c for po, r, c, _ in tasks),), "x", max(t[1] for t in tasks), L.F32, False)
    else:
        part = rng.normal(0.3, 1.0, size=max(po + r * c for po, r, c, _ in tasks)).astype(np.float32)
    pd = U.dev(part)
    written = torch.zeros(numel, dtype=torch.bool)
    for _, _, c, oo in tasks:
        written[oo:oo + c] = True
    out = Buf(torch.full((numel,), SENTINEL), written, nan=True)
    table = torch.tensor(tasks, dtype=torch.int32, device=U.DEV)

    def go():
        L.call(name, U.ptr(pd), U.ptr(table), ntasks, maxc, out.ptr(), U.stream())

    def evaluate():
        got = out.body().double().cpu().numpy()
        e = 0.0
        errs, msgs = {"exact colsum": 0.0}, []
        for k, (po, r, c, oo) in enumerate(tasks):
            want = part[po:po + r * c].astype(np.float64).reshape(r, c).sum(axis=0)
            if lat:
                one = {}
                _exact_family(one, msgs, f"exact colsum (task {k})", got[oo:oo + c], LT.expected(want, L.F32), step, ("column",))
                errs["exact colsum"] += sum(one.values())
            e = max(e, _rel(got[oo:oo + c], want) / _long_k(r))
        if lat:
            assert not msgs, "; ".join(msgs)
            return errs
        return {"colsum f32": e}

    launch = Launch([out], go, evaluate)
    launch.keep = (pd, table)
    return launch


# ---- packing (exact: the activation-dtype rounding of the input, ties to even)
def _exact(got, want, what):
    assert np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64)), f"{what}: not the dtype rounding of the input"


def _pack_pair(name, a, rng):
    """p2p_pack_pair(_idx): v_src = [source | 0], v_c6 = the same pixel, v_dreal = [target | source] ([target source 0 ..] for
    indices), v_dfake = its source half ([0 source 0 ..] for indices)"""
    dtype, N, H, W = a[:4]
    tdt, esz = U.tdt(dtype), _esz(dtype)
    idx = name == "p2p_pack_pair_idx"
    if idx:
        src = rng.integers(0, 256, size=(N, H, W)).astype(np.int32)
        tgt = rng.integers(0, 256, size=(N, H, W)).astype(np.int32)
        sd, td = U.dev(src, torch.int32), U.dev(tgt, torch.int32)
    else:
        src = rng.uniform(-1, 1, size=(N, H, W, 4)).astype(np.float32)
        tgt = rng.uniform(-1, 1, size=(N, H, W, 4)).astype(np.float32)
        sd, td = U.dev(src), U.dev(tgt)
    vs = OutBuf(a[6][1], N, H, W, 8, tdt, esz)
    vc = OutBuf(a[7][1], N, H, W, 8, tdt, esz) if a[7] is not None else None
    vr = OutBuf(a[8][1], N, H, W, 8, tdt, esz)
    vf = vf_view = None
    if a[9] is not None:
        if idx:
            vf = OutBuf(a[9][1], N, H, W, 8, tdt, esz)
            vf_view = vf.view
        else:
            vf, vf_view = _half_out(a[9][1], N, H, W, 4, 4, tdt, esz)
    outs = [o for o in (vs, vc, vr, vf) if o is not None]

    def go():
        L.call(name, dtype, N, H, W, U.ptr(sd), U.ptr(td), C.byref(vs.view), C.byref(vc.view) if vc else None, C.byref(vr.view),
               C.byref(vf_view) if vf else None, U.stream())

    def evaluate():
        z = np.zeros((N, H, W, 1))
        if idx:
            s, t = src[..., None].astype(np.float64), tgt[..., None].astype(np.float64)
            want_s = np.concatenate([s] + [z] * 7, -1)
            want_r = np.concatenate([t, s] + [z] * 6, -1)
            want_f = np.concatenate([z, s] + [z] * 6, -1)
        else:
            s, t = U.q(src, dtype), U.q(tgt, dtype)
            want_s = np.concatenate([s, np.zeros_like(s)], -1)
            want_r = np.concatenate([t, s], -1)
            want_f = s
        _exact(vs.region(), want_s, f"{name} v_src")
        if vc is not None:
            _exact(vc.region(), want_s, f"{name} v_c6")
        _exact(vr.region(), want_r, f"{name} v_dreal")
        if vf is not None:
            _exact(vf.region(), want_f, f"{name} v_dfake")
        return {"exact": 0.0}

    launch = Launch(outs, go, evaluate)
    launch.keep = (sd, td)
    return launch


def _pack_input(name, a, rng):
    """p2p_pack_input(_multi): a dense f32 or int32 [N][H][W][C] batch into one or up to four views"""
    dtype, N, H, W, Cc = a[:5]
    is_int = a[6]
    tdt, esz = U.tdt(dtype), _esz(dtype)
    if is_int:
        src = rng.integers(-300, 300, size=(N, H, W, Cc)).astype(np.int32)
        sd = U.dev(src, torch.int32)
        want = U.q(src.astype(np.float32), dtype)
    else:
        src = rng.uniform(-1, 1, size=(N, H, W, Cc)).astype(np.float32)
        sd = U.dev(src)
        want = U.q(src, dtype)
    descs = [dict(d) for d in a[7][1]] if name == "p2p_pack_input_multi" else [a[7][1]]
    outs = [OutBuf(d, N, H, W, Cc, tdt, esz) for d in descs]
    arr = (L.Tensor * len(outs))(*[o.view for o in outs])

    def go():
        if name == "p2p_pack_input_multi":
            L.call(name, dtype, N, H, W, Cc, U.ptr(sd), is_int, arr, len(outs), U.stream())
        else:
            L.call(name, dtype, N, H, W, Cc, U.ptr(sd), is_int, C.byref(outs[0].view), U.stream())

    def evaluate():
        for k, o in enumerate(outs):
            _exact(o.region(), want, f"{name} view {k}")
        return {"exact": 0.0}

    launch = Launch(outs, go, evaluate)
    launch.keep = (sd, arr)
    return launch


def _unpack(name, a, rng):
    """p2p_unpack: a view -> dense f32 [N][H][W][C]"""
    dtype, N, H, W, Cc = a[:5]
    x = U.q(rng.normal(size=(N, H, W, Cc)), dtype)
    keep, v = in_view(a[5][1], x, dtype, rng)
    out = FlatOut(N * H * W * Cc, a[6][1])

    def go():
        L.call(name, dtype, N, H, W, Cc, C.byref(v), out.ptr(), U.stream())

    def evaluate():
        _exact(out.values().reshape(N, H, W, Cc), x, name)
        return {"exact": 0.0}

    launch = Launch([out], go, evaluate)
    launch.keep = (keep,)
    return launch


def _copy_ref(w, cg, cd, rows, cols, transpose, tdt):
    """operand copy [16][rows][cols] of the master W[16][Cg][Cd] (transposed: [16][Cd][Cg]) in tdt, zero outside the real block"""
    w3 = w.reshape(16, cg, cd)
    if transpose:
        w3 = w3.transpose(1, 2)
    out = torch.zeros((16, rows, cols), dtype=tdt, device=w.device)
    r, c = min(rows, w3.shape[1]), min(cols, w3.shape[2])
    out[:, :r, :c] = w3[:, :r, :c].to(tdt)
    return out.reshape(-1)


def _copy_buf(rows, cols, tdt):
    n = 16 * rows * cols
    return Buf(torch.zeros(n, dtype=tdt), torch.ones(n, dtype=torch.bool), nan=True)


def _check_copy(buf, want, what):
    assert torch.equal(_bits(buf.body()), _bits(want)), f"{what}: not the dtype rounding of the master (or padding not 0)"


def _weight_prep(name, a, rng):
    """p2p_weight_prep(_pad): wn [16][wn_rows][wn_cols] and / or wt [16][wt_rows][wt_cols] from the f32 master"""
    dtype, cg, cd = a[0], a[2], a[3]
    if name == "p2p_weight_prep":
        shapes = ((cg, cd) if a[4] else None, (cd, cg) if a[5] else None)
    else:
        shapes = ((a[5], a[6]) if a[4] else None, (a[8], a[9]) if a[7] else None)
    tdt = U.tdt(dtype)
    w = torch.as_tensor(rng.normal(scale=0.05, size=16 * cg * cd).astype(np.float32)).to(U.DEV)
    bufs = [_copy_buf(*s, tdt) if s else None for s in shapes]

    def go():
        pn, pt = (b.ptr() if b else None for b in bufs)
        if name == "p2p_weight_prep":
            L.call(name, dtype, U.ptr(w), cg, cd, pn, pt, U.stream())
        else:
            L.call(name, dtype, U.ptr(w), cg, cd, pn, *(shapes[0] or (0, 0)), pt, *(shapes[1] or (0, 0)), U.stream())

    def evaluate():
        for k, (b, s) in enumerate(zip(bufs, shapes)):
            if b is not None:
                _check_copy(b, _copy_ref(w, cg, cd, s[0], s[1], k == 1, tdt), f"{name} {'wt' if k else 'wn'}")
        return {"exact": 0.0}

    launch = Launch([b for b in bufs if b], go, evaluate)
    launch.keep = (w,)
    return launch


def _task_table(tasks, masters, bufs):
    """a fresh p2p_prep_task table pointing at test-owned buffers (tasks as decoded by _decode_tasks)"""
    arr = (L.PrepTask * len(tasks))()
    for k, (t, wp, (bn, bt)) in enumerate(zip(tasks, masters, bufs)):
        cg, cd, wnr, wnc, wtr, wtc, _, _, tg, td, first = t[:11]
        e = arr[k]
        e.w = wp
        e.wn = bn.flat.data_ptr() if bn else None
        e.wt = bt.flat.data_ptr() if bt else None
        e.Cg, e.Cd, e.wn_rows, e.wn_cols, e.wt_rows, e.wt_cols = cg, cd, wnr, wnc, wtr, wtc
        e.tiles_g, e.tiles_d, e.first_block = tg, td, first
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(U.DEV)


def _task_copies(t, tdt):
    cg, cd, wnr, wnc, wtr, wtc, has_wn, has_wt = t[:8]
    return (_copy_buf(wnr, wnc, tdt) if has_wn else None, _copy_buf(wtr, wtc, tdt) if has_wt else None)


def _check_task_copies(name, tasks, masters, bufs, tdt):
    for k, (t, w, (bn, bt)) in enumerate(zip(tasks, masters, bufs)):
        cg, cd, wnr, wnc, wtr, wtc = t[:6]
        if bn is not None:
            _check_copy(bn, _copy_ref(w, cg, cd, wnr, wnc, False, tdt), f"{name} task {k} ({cg}x{cd}) wn")
        if bt is not None:
            _check_copy(bt, _copy_ref(w, cg, cd, wtr, wtc, True, tdt), f"{name} task {k} ({cg}x{cd}) wt")


def _weight_prep_batched(name, a, rng):
    """p2p_weight_prep_batched: every task's copies from a fresh master"""
    dtype, tasks, ntasks, total = a[0], a[1][1], a[2], a[3]
    tdt = U.tdt(dtype)
    masters = [torch.as_tensor(rng.normal(scale=0.05, size=16 * t[0] * t[1]).astype(np.float32)).to(U.DEV) for t in tasks]
    bufs = [_task_copies(t, tdt) for t in tasks]
    table = _task_table(tasks, [m.data_ptr() for m in masters], bufs)

    def go():
        L.call(name, dtype, U.ptr(table), ntasks, total, U.stream())

    def evaluate():
        _check_task_copies(name, tasks, masters, bufs, tdt)
        return {"exact": 0.0}

    launch = Launch([b for pair in bufs for b in pair if b], go, evaluate)
    launch.keep = (masters, table)
    return launch


# ---- optimizer
def _adam_state(numel, ranges, t, seed):
    """flat params / grads / m / v of `numel` f32 elements: SENTINEL everywhere but in `ranges`, which hold masters, gradients
    spread over 1e-8..1 with random signs and some exact zeros, and (t > 1) the moments of earlier steps.  Generated on the device."""
    gen = torch.Generator(device=U.DEV)
    gen.manual_seed(seed)

    def rn(k):
        return torch.randn(k, generator=gen, device=U.DEV, dtype=torch.float64)

    def ru(k):
        return torch.rand(k, generator=gen, device=U.DEV, dtype=torch.float64)

    def spread(k):
        return torch.sign(rn(k)) * 10.0 ** (-8.0 * ru(k))

    p, g, m, v = (torch.full((numel,), SENTINEL, dtype=torch.float32, device=U.DEV) for _ in range(4))
    written = torch.zeros(numel, dtype=torch.bool, device=U.DEV)
    for lo, hi in ranges:
        k = hi - lo
        p[lo:hi] = (rn(k) * 0.02).float()
        gg = spread(k)
        gg[ru(k) < 0.03] = 0.0
        g[lo:hi] = gg.float()
        if t > 1:
            prev = spread(k)
            m[lo:hi] = (0.5 * prev).float()
            v[lo:hi] = (1e-3 * prev ** 2 * (1.0 + ru(k))).float()
        else:
            m[lo:hi] = 0.0
            v[lo:hi] = 0.0
        written[lo:hi] = True
    return p, g, m, v, written


def _adam_errs(p, m, v, p0, g, m0, v0, t, b1, b2, eps, sel=None):
    """normalised errors of an f32 Adam step against the f64 Keras step (1.0 = the bound of test_adam_matches_keras_formulation:
    p rtol 1e-6 / atol 1e-7, v rtol 5e-5; m rtol 1e-6 of its inputs' scale)"""
    if sel is not None:
        p, m, v, p0, g, m0, v0 = (x[sel] for x in (p, m, v, p0, g, m0, v0))
    p0, g, m0, v0 = (x.double() for x in (p0, g, m0, v0))
    pr, mr, vr = SL.keras_adam(p0, g, m0, v0, t, ADAM_LR, b1, b2, eps)
    ep = ((p.double() - pr).abs() / (1e-6 * pr.abs() + 1e-7)).max()
    em = ((m.double() - mr).abs() / (1e-6 * torch.maximum(mr.abs(), torch.maximum(m0.abs(), g.abs())) + 1e-30)).max()
    ev = ((v.double() - vr).abs() / (5e-5 * vr.abs() + 1e-30)).max()
    return {"adam p": float(ep), "adam m": float(em), "adam v": float(ev)}


def _lr_t(t, b1, b2):
    return float(np.float32(ADAM_LR * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)))


def _adam_tick(name, a, rng, t=1):
    """p2p_adam_tick: t_dev += 1, lr_t_dev = lr sqrt(1 - b2^t) / (1 - b1^t)"""
    lr, b1, b2 = a[2], a[3], a[4]
    tb = Buf(torch.tensor([t - 1], dtype=torch.int32), torch.ones(1, dtype=torch.bool))
    lb = Buf(torch.zeros(1), torch.ones(1, dtype=torch.bool), nan=True)

    def go():
        L.call(name, tb.ptr(), lb.ptr(), lr, b1, b2, U.stream())

    def evaluate():
        assert int(tb.body()[0]) == t, f"{name}: t_dev {int(tb.body()[0])} after a tick from {t - 1}"
        want = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        return {"adam lr_t": abs(float(lb.body()[0]) - want) / want / 1e-6}

    return Launch([tb, lb], go, evaluate)


def _adam_flat(name, a, rng, t=1):
    """p2p_adam_flat(_dev) on [off, off + n) of a flat buffer laid out like the recorded store: every other element (the rest of
    the store, the small-tensor tail or the kernels in front of it) keeps its sentinel"""
    if name == "p2p_adam_flat_dev":
        _, sid, numel, off = a[0]
        n, b1, b2, eps, gs = a[4], a[6], a[7], a[8], a[9]
    else:
        numel, off = a[4] + 64, 32                # (direct test: a region inside a larger buffer)
        n, lr, b1, b2, eps, gs = a[4], a[6], a[7], a[8], a[9], a[10]
        assert lr == ADAM_LR, lr
    p, g, m, v, written = _adam_state(numel, [(off, off + n)], t, seed=int(rng.integers(1 << 30)))
    pb, mb, vb = (Buf(x, written) for x in (p, m, v))
    gb = Buf(g)
    lrd = U.dev(np.array([_lr_t(t, b1, b2), 0, 0, 0], np.float32))

    def go():
        if name == "p2p_adam_flat_dev":
            L.call(name, pb.ptr(off), gb.ptr(off), mb.ptr(off), vb.ptr(off), n, U.ptr(lrd), b1, b2, eps, gs, U.stream())
        else:
            L.call(name, pb.ptr(off), gb.ptr(off), mb.ptr(off), vb.ptr(off), n, t, ADAM_LR, b1, b2, eps, gs, U.stream())

    def evaluate():
        sl = slice(off, off + n)
        return _adam_errs(pb.body()[sl], mb.body()[sl], vb.body()[sl], p[sl], g[sl] * gs, m[sl], v[sl], t, b1, b2, eps)

    launch = Launch([pb, mb, vb, gb], go, evaluate)
    launch.keep = (lrd,)
    return launch


def _adam_prep(name, a, rng, t=1):
    """p2p_adam_prep_batched: the masters at their recorded offsets inside a params / grads / m / v store that is otherwise
    sentinel (the other part's kernels and the small-tensor tail of p2p_adam_flat_dev included); operand copies = the dtype
    rounding of the new master, zero padding"""
    dtype, n_elems, tasks, ntasks, total = a[0], a[1], a[2][1], a[3], a[4]
    _, sid, numel = a[5]
    b1, b2, eps = a[10], a[11], a[12]
    tdt = U.tdt(dtype)
    ranges = [(t_[12], t_[12] + 16 * t_[0] * t_[1]) for t_ in tasks]
    assert all(t_[11] == sid for t_ in tasks), f"{name}: a task's master lies outside the store passed as params"
    assert sum(hi - lo for lo, hi in ranges) == n_elems, (n_elems, ranges)
    p, g, m, v, written = _adam_state(numel, ranges, t, seed=int(rng.integers(1 << 30)))
    pb, mb, vb = (Buf(x, written) for x in (p, m, v))
    gb = Buf(g)
    bufs = [_task_copies(t_, tdt) for t_ in tasks]
    table = _task_table(tasks, [pb.flat.data_ptr() + 4 * lo for lo, _ in ranges], bufs)
    lrd = U.dev(np.array([_lr_t(t, b1, b2), 0, 0, 0], np.float32))

    def go():
        L.call(name, dtype, n_elems, U.ptr(table), ntasks, total, pb.ptr(), gb.ptr(), mb.ptr(), vb.ptr(), U.ptr(lrd), b1, b2, eps,
               U.stream())

    def evaluate():
        errs = _adam_errs(pb.body(), mb.body(), vb.body(), p, g, m, v, t, b1, b2, eps, sel=written)
        _check_task_copies(name, tasks, [pb.body()[lo:hi] for lo, hi in ranges], bufs, tdt)
        return errs

    launch = Launch([pb, mb, vb, gb] + [b for pair in bufs for b in pair if b], go, evaluate)
    launch.keep = (table, lrd)
    return launch


# ---- dropout RNG
def _dropout(name, a, rng):
    """p2p_dropout_mask(_dev) bit for bit against tests/step_launches.dropout_mask, at a device counter that is not 0"""
    n, seed = a[1], a[2]
    cb = None
    if name == "p2p_dropout_mask_dev":
        cval = 3
        salt, eoff = a[4], a[5]
        cb = Buf(torch.tensor([cval], dtype=torch.int64))
        counter, group0 = cval * 16 + salt, eoff // 8
    else:
        counter, group0 = a[3], 0
    mb = Buf(torch.full((n,), 0xA5, dtype=torch.uint8), torch.ones(n, dtype=torch.bool))

    def go():
        if cb is not None:
            L.call(name, mb.ptr(), n, seed, cb.ptr(), salt, eoff, U.stream())
        else:
            L.call(name, mb.ptr(), n, seed, counter, U.stream())

    def evaluate():
        got = mb.body().cpu().numpy()
        want = SL.dropout_mask(n, seed, counter, group0)
        bad = int((got != want).sum())
        assert bad == 0, f"{name}: {bad} of {n} mask bytes differ from the generator (n {n}, seed {seed}, counter {counter})"
        return {"exact": 0.0}

    return Launch([mb] + ([cb] if cb else []), go, evaluate)


def _counter_add(name, a, rng):
    """p2p_counter_add: counter += inc, exactly, in 64 bits"""
    inc = a[1]
    c0 = (1 << 40) + 12345
    cb = Buf(torch.tensor([c0], dtype=torch.int64), torch.ones(1, dtype=torch.bool))

    def go():
        L.call(name, cb.ptr(), inc, U.stream())

    def evaluate():
        assert int(cb.body()[0]) == c0 + inc, f"{name}: {int(cb.body()[0])} != {c0} + {inc}"
        return {"exact": 0.0}

    return Launch([cb], go, evaluate)


ADAM_STEPS = (1, 3)         # re-issued at t = 1 (m = v = 0) and at t = 3
VARIANTS = {n: [{"t": t} for t in ADAM_STEPS] for n in ("p2p_adam_tick", "p2p_adam_flat", "p2p_adam_flat_dev", "p2p_adam_prep_batched")}


CHECKERS = {n: _conv_family for n in ("p2p_igemm", "p2p_igemm_norm_act", "p2p_conv_strip", "p2p_igemm_edge", "p2p_conv_fewin",
                                      "p2p_conv_fewin_actbwd", "p2p_conv_fewout")}
CHECKERS.update({n: _wgrad_family for n in ("p2p_wgemm", "p2p_wgemm_edge", "p2p_wgrad_small")})
CHECKERS.update({"p2p_norm_act_fwd": _norm_fwd, "p2p_norm_act_fwd_tail": _norm_fwd, "p2p_act_bwd": _act_bwd,
                 "p2p_norm_act_bwd": _norm_bwd, "p2p_rgbuv_points": _points, "p2p_rgbuv_hist_fwd3": _hist_fwd3,
                 "p2p_rgbuv_hist_hellinger_bwd3": _hist_bwd3, "p2p_head_dgrad": _head_dgrad, "p2p_head_softmax_cce": _head_softmax})
CHECKERS.update({"p2p_bce_logits": _bce, "p2p_bce_logits_pad8": _bce, "p2p_tanh_l1_fwd": _tanh_fwd, "p2p_tanh_l1_fwd_pair": _tanh_fwd,
                 "p2p_tanh_l1_bwd": _tanh_bwd, "p2p_tanh_l1_bwd_pad8": _tanh_bwd, "p2p_loss_partials_sum": _partials_sum,
                 "p2p_finish_losses": _finish_losses, "p2p_hellinger_fwd": _hellinger_fwd, "p2p_hellinger_finish": _hellinger_finish,
                 "p2p_hist_normalize": _hist_normalize, "p2p_colsum": _colsum, "p2p_view_colsum": _view_colsum,
                 "p2p_colsum_batched": _colsum_batched, "p2p_pack_pair": _pack_pair, "p2p_pack_pair_idx": _pack_pair,
                 "p2p_pack_input": _pack_input, "p2p_pack_input_multi": _pack_input, "p2p_unpack": _unpack,
                 "p2p_weight_prep": _weight_prep, "p2p_weight_prep_pad": _weight_prep, "p2p_weight_prep_batched": _weight_prep_batched,
                 "p2p_adam_tick": _adam_tick, "p2p_adam_flat": _adam_flat, "p2p_adam_flat_dev": _adam_flat,
                 "p2p_adam_prep_batched": _adam_prep, "p2p_dropout_mask": _dropout, "p2p_dropout_mask_dev": _dropout,
                 "p2p_counter_add": _counter_add})


# the checkers with an operands="lattice" mode (tests/lattice.py): the contractions, whose f32 accumulation is exact on such operands
LATTICE_CHECKERS = (_conv_family, _wgrad_family, _head_dgrad, _view_colsum, _colsum, _colsum_batched)


def _tol(family, dtype):
    if family.startswith("exact "):
        return 1.0              # lattice mode: a count of elements that are not the expected value; passes only at 0
    if family == "insensitive share":
        return 0.01 + 1e-12     # lattice mode, bf16: at least 0.99 of the reference sums lie within +-256
    if family.startswith("out") or family == "stats f64":
        return OUT_TOL[dtype]
    if family.startswith("d(raw)"):
        return 1e-2 if dtype == L.BF16 else 1e-4       # test_kernels_gpu.py::test_norm_act_fwd_bwd
    if family == "histogram":
        return 1e-4                                     # test_hist_indexed_gpu.py: f32 logf / division against f64
    if family == "hist grad":
        return 2e-3                                     # test_hist_indexed_gpu.py: gradient spanning ~6 decades (1/(x+1e-6))
    if family.startswith("adam"):
        return 1.0              # (normalised by the Keras bounds in _adam_errs / _adam_tick)
    if family in ("fake f32", "colsum f32", "exact"):
        return F32_TOL          # (f32 tanh against f64; column sums already scaled by the long-K bound; exact: 0)
    if family in ("loss f32", "dbias f32", "points"):
        return F32_TOL          # (loss / bias sums already scaled by the long-K bound; points: exact)
    if family == "norm out":
        return OUT_TOL[dtype]
    if family == "dW f32":
        return F32_TOL          # (already scaled by the long-K bound in _wgrad_family)
    if family == "f32 slabs":
        return F32_TOL
    # statistics (per image and channel: mean error / standard deviation, relative variance error / 5) and the dgamma / dbeta
    # partials (test_kernels_gpu.py: 1e-4)
    return 1e-4


def _reissue(name, dec, seed):
    errs = {}
    for kw in VARIANTS.get(name, [{}]):
        for fam, e in _reissue_one(name, dec, seed, kw).items():
            errs[fam] = max(errs.get(fam, 0.0), e)
    return errs


def _reissue_one(name, dec, seed, kw):
    rng = np.random.default_rng(seed)
    launch = CHECKERS[name](name, dec, rng, **kw)
    launch.go()
    torch.cuda.synchronize()
    for o in launch.outs:
        o.check_around(name)
    first = [o.flat.clone() for o in launch.outs]
    fixed = [t.clone() for t in getattr(launch, "fixed", ())]
    for o in launch.outs:
        o.reset()
    launch.go()
    torch.cuda.synchronize()
    for t, f in zip(getattr(launch, "fixed", ()), fixed):
        assert torch.equal(t, f), f"{name}: second launch differs"
    for o, f in zip(launch.outs, first):
        assert torch.equal(_bits(o.flat), _bits(f)), f"{name}: second launch differs"
    errs = launch.evaluate()
    del launch
    return errs


STEP_CASES = [(c, d, None) for c, d in CONFIGS] + [("c2", "bf16", True)]


def _check_step(cfg, dtype_name, fuse, label):
    """harvest the recorded step, refuse unknown entry points, re-issue every unique launch (NaN before, sentinel around, a second
    launch bit-identical) against f64 with the per-family tolerances, print the table; returns the harvest.  fuse: the fuse_adam
    switch, or a dict of engine switch attributes (_overrides)"""
    uniq, names = harvest(cfg, dtype_name, fuse)
    fuse = _overrides(fuse).get("fuse_adam")
    if fuse:
        assert "p2p_adam_prep_batched" in names, "the fused-Adam step issues no p2p_adam_prep_batched"
    unknown = sorted({n for n in names if n not in CHECKERS and n not in OUT_OF_SCOPE})
    assert not unknown, f"{label}: entry points neither re-issued nor listed as out of scope: {unknown}"
    dtype = L.BF16 if dtype_name == "bf16" else L.F32
    table, failures = {}, []
    for k, (sig, (name, dec)) in enumerate(sorted(uniq.items(), key=lambda kv: repr(kv[0]))):
        row = table.setdefault(name, {"launches": 0, "worst": {}})
        row["launches"] += 1
        try:
            errs = _reissue(name, dec, seed=1000 + k)
        except AssertionError as e:
            failures.append(f"{name} {dec[:10]}: {e}")
            continue
        for fam, e in errs.items():
            row["worst"][fam] = max(row["worst"].get(fam, 0.0), e)
            if not e < _tol(fam, dtype):
                failures.append(f"{name} {[d for d in dec if not isinstance(d, tuple)][:12]}: {fam} error {e:.3g} >= {_tol(fam, dtype):.3g}")
        torch.cuda.empty_cache()
    print(f"\n[{label} {dtype_name}{' fused Adam' if fuse else ''}] {len(names)} calls per step, {len(uniq)} unique re-issued launch signatures")
    print(f"  {'entry point':28s} {'launches':>8s}  worst error per family (tolerance)")
    for name in sorted(table):
        r = table[name]
        fams = ", ".join(f"{f} {e:.2e} ({_tol(f, dtype):.0e})" for f, e in sorted(r["worst"].items()))
        print(f"  {name:28s} {r['launches']:8d}  {fams}")
    assert not failures, "\n".join(failures)
    assert table, f"{label}: no launch re-issued"
    return uniq


@pytest.mark.parametrize("cfg,dtype_name,fuse", STEP_CASES, ids=[f"{c}-{d}" + ("-fused-adam" if f else "") for c, d, f in STEP_CASES])
def test_every_launch_of_the_benchmarked_step_against_f64(cfg, dtype_name, fuse):
    """fuse: also the step with Adam and the operand copies in one launch per part (p2p_adam_prep_batched on the G_head / G_rest /
    D tables), the engine's other Adam path"""
    _check_step(cfg, dtype_name, fuse, cfg)


_CENSUS = {}


@pytest.mark.parametrize("model,S,dtype_name,B", SL.OFF_BENCH_CASES, ids=[f"{m}-{s}-{d}-b{b}" for m, s, d, b in SL.OFF_BENCH_CASES])
def test_every_launch_of_off_benchmark_steps_against_f64(model, S, dtype_name, B):
    """The same check at the batches of step_launches.OFF_BENCH_CASES (module docstring: chosen so that every kernel variant the
    engine picks at or below the cap is re-issued at a batch that picks it).  The variant keys of the recorded step must be the
    ones the host-only census gives for the batch: the census that chose the batches describes the engine that runs."""
    uniq = _check_step(SL.step_desc(model, B, S), dtype_name, None, f"{model} {S}x{S} batch {B}")
    case = (model, S, dtype_name)
    if case not in _CENSUS:
        _CENSUS[case] = SL.Census(*case)
    got, want = SL.harvested_variant_keys(uniq), _CENSUS[case].variant_keys(B)
    only_step = sorted(SL.describe_key(k) for k in got - want)
    only_census = sorted(SL.describe_key(k) for k in want - got)
    assert got == want, f"the census has drifted from the engine at batch {B}:\n  recorded step only: {only_step}\n  census only: {only_census}"


def _direct_cases():
    """(name, dtype, decoded args) of the entry points and forms that no benchmarked step issues: the partial-store forms
    (P2P_FULL_PIXELS=0), generate() / hooked-step launches, the unbatched weight copies, the host-step Adam, an unaligned
    dropout mask, the histogram backward at the one pixel partition no tested step reaches"""
    def v(*a, **k):
        return ("view", _vd(*a, **k))
    P, BF, F = ("ptr", 0), L.BF16, L.F32
    gs1 = ("gsrc", {"kind": 1, "nslabs": 0, "slab_stride": 0, "ld": 8, "coff": 0, "align": 0})
    gs2 = ("gsrc", {"kind": 2, "nslabs": 2, "slab_stride": 3 * 16 * 16 * 4, "ld": 4, "coff": 0, "align": 0})
    b1, b2, eps = float(np.float32(0.5)), float(np.float32(0.999)), float(np.float32(1e-7))
    multi = ("views", tuple(tuple(sorted(d.items())) for d in (_vd(8, 8, 8, halo=1), _vd(8, 8, 40, halo=1, coff=32))))
    return [
        ("p2p_bce_logits", BF, [BF, 6, 3, 8, 8, v(8, 8, 1), 1 / 192, v(8, 8, 8, halo=1), v(8, 8, 8, halo=1), P, None]),
        ("p2p_bce_logits_pad8", F, [F, 4, 4, 8, 8, v(8, 8, 1), 1 / 256, v(8, 8, 8, halo=1), None, P, None]),
        ("p2p_tanh_l1_fwd", BF, [BF, 3, 16, 16, 3, v(16, 16, 3), v(16, 16, 8, halo=1), v(16, 16, 8, halo=1), 1 / 2304, P, P, None]),
        ("p2p_tanh_l1_fwd", F, [F, 3, 16, 16, 4, v(16, 16, 4), v(16, 16, 8, halo=1), v(16, 16, 8, halo=1), 1 / 3072, P, None, None]),
        ("p2p_tanh_l1_bwd", BF, [BF, 3, 16, 16, 3, v(16, 16, 8, halo=1), v(16, 16, 8, halo=1), gs1, gs2, 1e-3, v(16, 16, 4, halo=1),
                                 None]),
        ("p2p_tanh_l1_bwd", F, [F, 3, 16, 16, 4, v(16, 16, 8, halo=1), v(16, 16, 8, halo=1), gs1, None, 1e-3, v(16, 16, 4, halo=1),
                                None]),
        ("p2p_colsum", F, [P, 37, 19, 0.5, P, None]),
        ("p2p_hist_normalize", F, [P, 3, P, None]),
        # launch_hist_bwd3's nsplit = 2 (N in 128 .. 255 at 64x64): above the cap of the off-benchmark steps, below c3's batch
        ("p2p_rgbuv_hist_hellinger_bwd3", F, [F, 128, 64, 64, v(64, 64, 4), P, P, P, P, P, 1.0 / (2 * np.sqrt(2.0) * 128), P, P, None]),
        ("p2p_pack_pair", BF, [BF, 2, 8, 8, P, P, v(8, 8, 8, halo=1), v(8, 8, 40, halo=1, coff=32), v(8, 8, 8, halo=1),
                               v(8, 8, 8, halo=1), None]),
        ("p2p_pack_pair_idx", F, [F, 2, 8, 8, P, P, v(8, 8, 8, halo=1), v(8, 8, 40, halo=1, coff=32), v(8, 8, 8, halo=1),
                                  v(8, 8, 8, halo=1), None]),
        ("p2p_pack_input", BF, [BF, 2, 8, 8, 3, P, 0, v(8, 8, 8, halo=1, coff=2, align=4), None]),
        ("p2p_pack_input", F, [F, 2, 8, 8, 1, P, 1, v(8, 8, 4, halo=1), None]),
        ("p2p_pack_input_multi", BF, [BF, 2, 8, 8, 4, P, 0, multi, 2, None]),
        ("p2p_pack_input_multi", BF, [BF, 2, 8, 8, 1, P, 1, multi, 2, None]),
        ("p2p_unpack", BF, [BF, 2, 8, 8, 5, v(8, 8, 8, halo=1, coff=1, align=2), P, None]),
        ("p2p_weight_prep", BF, [BF, P, 40, 24, P, P, None]),
        ("p2p_weight_prep", F, [F, P, 64, 64, P, None, None]),
        ("p2p_weight_prep_pad", BF, [BF, P, 4, 64, P, 32, 64, P, 64, 8, None]),
        ("p2p_adam_flat", F, [P, P, P, P, 10007, 1, ADAM_LR, b1, b2, eps, 1.0, None]),
        ("p2p_dropout_mask", F, [P, 1003, 77, 5, None]),
        ("p2p_dropout_mask_dev", F, [P, 1001, 77, P, 4, 64, None]),
    ]


DIRECT = _direct_cases()


@pytest.mark.parametrize("k", range(len(DIRECT)), ids=[f"{n}-{'bf16' if d == L.BF16 else 'f32'}" for n, d, _ in DIRECT])
def test_entry_points_no_benchmarked_step_issues(k):
    name, dtype, dec = DIRECT[k]
    errs = _reissue(name, dec, seed=2000 + k)
    bad = {f: e for f, e in errs.items() if not e < _tol(f, dtype)}
    print(f"\n  {name}: " + ", ".join(f"{f} {e:.2e}" for f, e in sorted(errs.items())))
    assert not bad, f"{name}: {bad}"


def test_every_checker_runs_somewhere():
    """an entry point with a checker is either in a benchmarked step's recording (test above) or in DIRECT; this lists the ones
    that only DIRECT reaches, so that a checker cannot silently go unused"""
    direct = {n for n, _, _ in DIRECT}
    recorded_only = {"p2p_bce_logits_pad8", "p2p_tanh_l1_fwd_pair", "p2p_tanh_l1_bwd_pad8", "p2p_loss_partials_sum",
                     "p2p_finish_losses", "p2p_hellinger_fwd", "p2p_hellinger_finish", "p2p_view_colsum", "p2p_colsum_batched",
                     "p2p_weight_prep_batched", "p2p_adam_tick", "p2p_adam_flat_dev", "p2p_adam_prep_batched", "p2p_counter_add"}
    new = {n for n, f in CHECKERS.items() if f in (_bce, _tanh_fwd, _tanh_bwd, _partials_sum, _finish_losses, _hellinger_fwd,
                                                   _hellinger_finish, _hist_normalize, _colsum, _view_colsum, _colsum_batched,
                                                   _pack_pair, _pack_input, _unpack, _weight_prep, _weight_prep_batched, _adam_tick,
                                                   _adam_flat, _adam_prep, _dropout, _counter_add)}
    assert new <= direct | recorded_only, sorted(new - direct - recorded_only)


# ---------------------------------------------------------------------------------------------------------------- one Adam step
ADAM_CASES = [(c, d, False) for c, d in CONFIGS] + [("c2", "bf16", True)]


def _copy_sets(eng):
    """(label, operand copy, new master, Cg, Cd, rows, cols, transposed) of every weight copy the engine keeps"""
    for (sid, name), lw in eng.W.items():
        store = eng._store(sid)
        master = store.view(store.params, name + ".kernel").reshape(-1)
        for tag, buf, rows, cols, tr in (("wn", lw.wn, E.up32(lw.cg), lw.lo_pad, False), ("wt", lw.wt, E.up32(lw.cd), lw.hi_pad, True),
                                         ("wd", lw.wd, lw.cg, lw.cd, False)):
            if buf is not None:
                yield f"{sid}.{name}.{tag}", buf, master, lw.cg, lw.cd, rows, cols, tr


@pytest.mark.parametrize("cfg,dtype_name,fuse", ADAM_CASES, ids=[f"{c}-{d}" + ("-fused" if f else "") for c, d, f in ADAM_CASES])
def test_one_keras_update_per_parameter_per_step(cfg, dtype_name, fuse):
    """The replayed step of a bench config moves every element of both networks' params / m / v by exactly one Keras Adam step
    driven by the gradients the step left in `grads` (a duplicated or missing update is about one Adam step away), refreshes
    every operand copy from the new master, and advances t and the dropout counter by one."""
    eng, step = _build(cfg, dtype_name)
    try:
        eng.fuse_adam = fuse
        step()
        step()                          # eager, recorded
        torch.cuda.synchronize()
        assert len(eng._replays) == 1, f"{cfg}: the step was not recorded"
        stores = (("G", eng.G), ("D", eng.D))
        snap = {sid: (st.params.clone(), st.m.clone(), st.v.clone(), st.t, int(st.t_dev[0])) for sid, st in stores}
        ctr = int(eng.mask_counter_dev[0])
        step()                          # replayed
        torch.cuda.synchronize()
        lr, b1, b2, eps = eng.lr, eng.beta1, eng.beta2, eng.adam_eps
        missed, worst = [], {}
        for sid, st in stores:
            p0, m0, v0, t_host, t_dev = snap[sid]
            assert st.t == t_host + 1 and int(st.t_dev[0]) == t_dev + 1, f"{sid}: t {t_host} -> {st.t}, t_dev {t_dev} -> {int(st.t_dev[0])}"
            g = st.grads.double()
            pr, mr, vr = SL.keras_adam(p0.double(), g, m0.double(), v0.double(), t_dev + 1, lr, b1, b2, eps)
            ep = (st.params.double() - pr).abs() / (1e-6 * pr.abs() + 1e-7)
            em = (st.m.double() - mr).abs() / (1e-6 * torch.maximum(mr.abs(), torch.maximum(m0.double().abs(), g.abs())) + 1e-30)
            ev = (st.v.double() - vr).abs() / (5e-5 * vr.abs() + 1e-30)
            for fam, e in (("p", ep), ("m", em), ("v", ev)):
                worst[f"{sid} {fam}"] = float(e.max())
            ok = (ep <= 1) & (em <= 1) & (ev <= 1)
            covered = torch.zeros_like(ok)
            for key, shape in st.shapes.items():
                o, n = st.offsets[key], int(np.prod(shape))
                covered[o:o + n] = True
                if not bool(ok[o:o + n].all()):
                    missed.append(f"{sid}.{key} ({int((~ok[o:o + n]).sum())} of {n})")
            if not bool(ok[~covered].all()):
                missed.append(f"{sid} alignment padding")
        bad_copies = [label for label, buf, master, cg, cd, rows, cols, tr in _copy_sets(eng)
                      if not torch.equal(_bits(buf), _bits(_copy_ref(master, cg, cd, rows, cols, tr, eng.tdt)))]
        print(f"\n[{cfg} {dtype_name}{' fused Adam' if fuse else ''}] worst / bound: "
              + ", ".join(f"{k} {e:.2e}" for k, e in sorted(worst.items())))
        assert not missed, f"{cfg}: tensors not moved by exactly one Keras step: {missed}"
        assert not bad_copies, f"{cfg}: operand copies that are not the rounding of the new master: {bad_copies}"
        assert int(eng.mask_counter_dev[0]) == ctr + 1, f"dropout counter {ctr} -> {int(eng.mask_counter_dev[0])}"
    finally:
        del eng
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- replay key
def _calls_of(rec):
    return [(n, tuple(int(_val(v)) for t, v in zip(L.SIGNATURES[n], args) if t is C.c_int))
            for n, args in rec if n is not None and n not in ("p2p_event_record", "p2p_stream_wait_event", "p2p_arm_stop_event")]


@pytest.mark.parametrize("attr,dtype,B", [("batch_invariant", L.F32, 8), ("wgemm_pipe", L.BF16, 64)])
def test_recorded_step_issues_what_the_eager_step_issues(attr, dtype, B):
    """batch_invariant and wgemm_pipe choose kernels and K splits when the step is recorded: a recording must not be replayed after
    one of them has changed (engine._replay_key).  Both start off and are switched on: the buffers of the step are sized when it
    first runs, and the switched-off settings need the larger split-K / weight-gradient workspaces."""
    S = 64
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, device=U.DEV, seed=47)
    setattr(eng, attr, False)
    src, tgt = bench.synthetic_batch(0, B, S, None)
    src_d, tgt_d = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)

    def step():
        return eng.train_step_rgba(src_d, tgt_d, 100.0, global_batch=B)

    def eager_calls():
        log = []
        orig = L.call

        def logger(name, *args):
            orig(name, *args)
            log.append((name, args))
        L.call = logger
        try:
            step()
        finally:
            L.call = orig
        return _calls_of(log)

    try:
        step()
        step()                                    # recorded
        assert len(eng._replays) == 1
        before = eager_calls()
        setattr(eng, attr, True)
        after = eager_calls()
        assert after != before, f"flipping {attr} changes no launch at batch {B}: the test shows nothing"
        step()
        step()                                    # eager + recorded under the new setting, or a stale replay
        torch.cuda.synchronize()
        last = next(reversed(eng._replays.values()))[1]
        assert _calls_of(last) == after, f"the step replayed after flipping {attr} is not what an eager step issues"
    finally:
        del eng
        gc.collect()
        torch.cuda.empty_cache()
