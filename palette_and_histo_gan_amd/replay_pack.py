"""A recorded step as an array of p2p_replay_call records (include/p2pgan.h): how one ctypes argument is packed.  Pure host code:
what is recorded, and when, is the engine's business (engine.py, _REC)."""
import ctypes as C

from . import _lib as L


class ReplayCall(C.Structure):
    """include/p2pgan.h p2p_replay_call"""
    MAX_ARGS = 24
    _fields_ = [("fn", C.c_int), ("nargs", C.c_int), ("ind64", C.c_uint), ("ind32", C.c_uint), ("a", C.c_ulonglong * 24)]


_M64 = (1 << 64) - 1
_F32 = __import__("struct").Struct("<f")
_U32 = __import__("struct").Struct("<I")


def _pack_arg(argtype, v):
    """one recorded ctypes argument as (8-byte slot, indirection width): what ctypes would hand to the entry point.  A ctypes
    scalar OBJECT (c_void_p / c_float / c_longlong instance) is read when the call is issued, exactly as ctypes does -- the
    engine's batch, result and hyper-parameter slots rely on that -- so it is packed as the object's address."""
    if isinstance(v, C._SimpleCData):
        width = C.sizeof(v)
        if width not in (4, 8):
            raise TypeError(f"cannot replay a {type(v).__name__} argument")
        return C.addressof(v), width
    if argtype is C.c_float:
        return _U32.unpack(_F32.pack(v))[0], 0
    if argtype in (C.c_int, C.c_longlong):
        return int(v) & _M64, 0
    # pointers: void* and pointers to structures
    if v is None:
        return 0, 0
    if isinstance(v, int):
        return v & _M64, 0
    if isinstance(v, (C.Structure, C.Array)):
        return C.addressof(v), 0
    obj = getattr(v, "_obj", None)          # C.byref(x)
    if obj is not None:
        return C.addressof(obj), 0
    raise TypeError(f"cannot replay an argument of type {type(v).__name__}")


def pack_replay(rec):
    """list of (entry point name, ctypes arguments) -> (array of p2p_replay_call, n).  The caller keeps `rec` alive: the records
    hold the addresses of the ctypes objects inside it."""
    lib = L.lib()
    arr = (ReplayCall * len(rec))()
    for k, (name, args) in enumerate(rec):
        types = L.SIGNATURES[name]
        fn = lib.p2p_replay_fn_index(name.encode())
        if fn < 0 or len(args) != len(types) or lib.p2p_replay_fn_nargs(fn) != len(types):
            raise L.P2PError(f"{name} with {len(args)} arguments is not replayable")
        c = arr[k]
        c.fn, c.nargs = fn, len(args)
        i64 = i32 = 0
        for j, (t, v) in enumerate(zip(types, args)):
            c.a[j], ind = _pack_arg(t, v)
            if ind == 8:
                i64 |= 1 << j
            elif ind == 4:
                i32 |= 1 << j
        c.ind64, c.ind32 = i64, i32
    return arr, len(rec)
