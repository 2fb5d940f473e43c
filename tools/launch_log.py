#!/usr/bin/env python3
"""The complete launch log of a train step, without a GPU: the engine runs on device 'meta' (tests.step_launches._dry_run) and
every launch of the SECOND step is printed, one per line: entry point and every argument, integers and floats exactly.  Two
trees that print the same log issue the same step, which is how a change to the engine's host code is shown to change no launch.

  python tools/launch_log.py MODEL S DTYPE BATCH [attr=value ...] [--aux]
      MODEL baseline | histogram | indexed;  DTYPE bf16 | f32;  attr=value: engine switches (full_pixels=False, side.enabled=0)
      --aux: generate, discriminate and the tape forward / backward calls at that batch instead of the train step

A meta tensor has no address and _dry_run gives them all the same one, which cannot tell two buffers apart.  Here every storage
(views share it: untyped_storage()._cdata) gets an address window of its own, and the log names a pointer by the position of its
storage among the storages the log has mentioned so far plus the byte offset into it: @3+0x1200.  Weight-copy task tables are
built on the host and lose their bytes on 'meta'; a pointer to one prints the table behind it."""
import ast
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from palette_and_histo_gan_amd import _lib as L  # noqa: E402
from tests import step_launches as SL  # noqa: E402

WINDOW = 40                 # a storage's window is 1 << WINDOW bytes
_real_ptr = torch._C.TensorBase.data_ptr
_real_frombuffer = torch.frombuffer
_storages, _window_of, _tables, _labels = [], {}, {}, {}       # (every storage seen is held: no handle is used twice)


def _data_ptr(t):
    if t.device.type != "meta":
        return _real_ptr(t)
    st = t.untyped_storage()
    w = _window_of.get(st._cdata)
    if w is None:
        _storages.append(st)
        w = _window_of[st._cdata] = len(_storages)
    if getattr(t, "_host_bytes", None) is not None:
        _tables[w] = t._host_bytes
    return (w << WINDOW) + t.storage_offset() * t.element_size()


class _HostTable:
    """torch.frombuffer(...) of a dry run: .to('meta') keeps the bytes beside the tensor"""

    def __init__(self, buf, **kw):
        self.t = _real_frombuffer(buf, **kw)

    def to(self, device):
        out = self.t.to(device)
        out._host_bytes = bytes(self.t.numpy().tobytes())
        return out


def ptr(p):
    if not p:
        return "null"
    w = p >> WINDOW
    if w not in _labels:
        _labels[w] = len(_labels)
    text = f"@{_labels[w]}+{p & ((1 << WINDOW) - 1):#x}"
    if w in _tables and len(_tables[w]) % C.sizeof(L.PrepTask) == 0:
        tasks = (L.PrepTask * (len(_tables[w]) // C.sizeof(L.PrepTask))).from_buffer_copy(_tables.pop(w))
        text += "[" + " ".join(struct(t) for t in tasks) + "]"
    return text


def struct(s):
    return "{" + ",".join(f"{n}={ptr(getattr(s, n)) if t is C.c_void_p else getattr(s, n)}" for n, t in s._fields_) + "}"


def arg(t, v):
    v = getattr(v, "_obj", v)                  # C.byref(x)
    if isinstance(v, C.Array):
        return "[" + " ".join(struct(x) for x in v) + "]"
    if isinstance(v, C.Structure):
        return struct(v)
    if isinstance(v, C._SimpleCData):          # a pointer, or a slot the entry point reads when it is called
        return ptr(v.value) if isinstance(v, C.c_void_p) else repr(v.value)
    if t is C.c_float:
        return repr(float(v))
    if t in (C.c_int, C.c_longlong):
        return str(int(v))
    return ptr(v)


def main():
    model, S, dtype, B = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    lam_l1, lam_hist, _ = SL.STEP_LAMBDAS[model]
    log = []
    with SL._dry_run(log) as E:
        torch.Tensor.data_ptr, torch.frombuffer = _data_ptr, _HostTable
        try:
            indexed = model == "indexed"
            eng = E.Pix2PixEngine(*((1, 256, "softmax") if indexed else (4, 4, "tanh")), S, L.BF16 if dtype == "bf16" else L.F32,
                                  device="meta", seed=47)
            for kv in (a for a in sys.argv[5:] if "=" in a):
                *path, name = kv.split("=")[0].split(".")
                obj = eng
                for p in path:
                    obj = getattr(obj, p)
                assert hasattr(obj, name), f"the engine has no switch {kv.split('=')[0]}"
                setattr(obj, name, ast.literal_eval(kv.split("=", 1)[1]))
            x = torch.empty((B, S, S, 1 if indexed else 4), dtype=torch.int32 if indexed else torch.float32, device="meta")
            y = torch.empty_like(x)
            if "--aux" in sys.argv:
                eng.generate_indexed(x) if indexed else eng.generate(x)
                eng.discriminate(y, x)
                if not indexed:
                    G, D = eng.tape_arena("G", B), eng.tape_arena("D", B)
                    img = eng.tape_generator_forward(G, x)
                    logits = eng.tape_discriminator_forward(D, img, x)
                    eng.tape_discriminator_backward(D, logits, True, True, True)
                    eng.tape_generator_backward(G, img, True)
            else:
                for _ in range(2):
                    log.clear()
                    if indexed:
                        eng.train_step_indexed(x, y, lam_l1, global_batch=B)
                    else:
                        eng.train_step_rgba(x, y, lam_l1, lam_hist, global_batch=B)
        finally:
            torch.frombuffer = _real_frombuffer
    for name, args in log:
        print(name, *(arg(t, v) for t, v in zip(L.SIGNATURES[name], args)))


if __name__ == "__main__":
    main()
