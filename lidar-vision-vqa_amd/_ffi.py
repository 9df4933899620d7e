"""ctypes binding of the C-ABI library liblvq_hip.so (include/lvq.h).

PyTorch is plumbing here: it owns device memory (`tensor.data_ptr()`), the current HIP stream and
`torch.distributed`; every byte of arithmetic on the hot path happens inside the library.  There is
NO fallback: if the library is missing or a call returns an error code, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import List, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LVQ_LIB_PATH") or os.path.join(_HERE, "liblvq_hip.so")     # LVQ_LIB_PATH: another build of the same ABI (A/B runs)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lvq.h")

LVQ_OK = 0
LVQ_EUNSUPPORTED = -5      # include/lvq.h: shape outside what a kernel family implements (callers may pick another route)


class LvqError(RuntimeError):
    pass


_lib: Optional[ctypes.CDLL] = None


class Tuning(ctypes.Structure):
    """include/lvq.h: lvq_tuning -- the kernel-family choices the library takes from its caller (it never reads the environment)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "attn_no32", "attn32_nw", "attn_pipe", "attn_nsplit", "attn_qt", "attn_nw", "gemm_no_gemv", "gemm_stream_c_mb", "gemm_no256",
        "gemm_no256x256", "gemm_256x256_min_tiles", "gemm_ln_tiles", "pillar_vfe_generic", "voxel_path", "pairs_one_wg",
        "ca_fused_variant")] + [("ca_fused_stamps", ctypes.c_uint64), ("conv_rows_grid", ctypes.c_int32), ("pillar_vfe_path", ctypes.c_int32),
                                   ("reserved", ctypes.c_int32 * 6)]


TUNING_FIELDS = tuple(n for n, _ in Tuning._fields_ if n != "reserved")


def tuning_from_env(env=None) -> dict:
    """The LVQ_* variables of INTEGRATION.md as an lvq_tuning record.  They are a convenience of THIS mirror, read once when the
    library is loaded (and again by set_tuning()); a C / C++ caller fills the struct itself."""
    e = os.environ if env is None else env

    def flag(name):
        return 1 if e.get(name) else 0

    def num(name):
        return int(e[name]) if e.get(name) else 0

    return {
        "attn_no32": flag("LVQ_ATTN_NO32"), "attn32_nw": num("LVQ_ATTN32_NW"),
        "attn_pipe": -1 if e.get("LVQ_ATTN_NO_PIPE") else flag("LVQ_ATTN_PIPE"),
        "attn_nsplit": num("LVQ_ATTN_NSPLIT"), "attn_qt": num("LVQ_ATTN_QT"), "attn_nw": num("LVQ_ATTN_NW"),
        "gemm_no_gemv": flag("LVQ_GEMM_NO_GEMV"),
        "gemm_stream_c_mb": -1 if e.get("LVQ_GEMM_NO_STREAM_C") else num("LVQ_GEMM_STREAM_C_MB"),
        "gemm_no256": flag("LVQ_GEMM_NO256"), "gemm_no256x256": flag("LVQ_GEMM_NO256X256"),
        "gemm_256x256_min_tiles": num("LVQ_GEMM_256X256_MIN_TILES"), "gemm_ln_tiles": flag("LVQ_GEMM_LN_TILES"),
        "pillar_vfe_generic": flag("LVQ_PILLAR_VFE_GENERIC"),
        "voxel_path": 2 if e.get("LVQ_VOXEL_LEGACY") else flag("LVQ_VOXEL_BINNED"),
        "pairs_one_wg": flag("LVQ_PAIRS_ONE_WG"), "ca_fused_variant": num("LVQ_CA_DBG"), "ca_fused_stamps": 0,
        "conv_rows_grid": 0,                   # test hook only: no environment variable
        "pillar_vfe_path": flag("LVQ_PILLAR_VFE_ONE_PER_WAVE"),
    }


def set_tuning(**fields) -> dict:
    """lvq_set_tuning: the record implied by the environment, overridden by `fields` (names of include/lvq.h: lvq_tuning).
    set_tuning() with no arguments restores the environment's choices.  Returns the record now in force."""
    rec = tuning_from_env()
    for k, v in fields.items():
        if k not in TUNING_FIELDS:
            raise LvqError(f"lvq_tuning has no field {k!r}")
        rec[k] = int(v)
    t = Tuning()
    for k, v in rec.items():
        setattr(t, k, v)
    check(lib().lvq_set_tuning(ctypes.byref(t)), "lvq_set_tuning")
    return rec


def get_tuning() -> dict:
    t = Tuning()
    check(lib().lvq_get_tuning(ctypes.byref(t)), "lvq_get_tuning")
    return {k: int(getattr(t, k)) for k in TUNING_FIELDS}


class tuning:
    """`with tuning(attn_nsplit=1): ...` -- a kernel-family choice for the calls inside (process-wide: not for concurrent launch threads)."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.old = get_tuning()
        cur = dict(self.old)
        cur.update({k: int(v) for k, v in self.fields.items()})
        _push(cur)
        return self

    def __exit__(self, *exc):
        _push(self.old)
        return False


def _push(rec: dict):
    t = Tuning()
    for k, v in rec.items():
        if k not in TUNING_FIELDS:
            raise LvqError(f"lvq_tuning has no field {k!r}")
        setattr(t, k, v)
    check(lib().lvq_set_tuning(ctypes.byref(t)), "lvq_set_tuning")


_C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
_C_RETURNS = dict(_C_TYPES, **{"void": None, "const char *": ctypes.c_char_p})


def prototypes(text: Optional[str] = None) -> dict:
    """{name: (restype, [argtypes])} of every function declared in include/lvq.h (or in `text`): the header is the only statement
    of a signature, and lib() binds every entry point from this table.  Pointers, arrays and lvq_stream_t travel as c_void_p;
    a type outside the table raises LvqError (nothing is guessed)."""
    if text is None:
        with open(HEADER_PATH) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(lvq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.split())
        args = []
        for p in (q.strip() for q in params.split(",") if q.strip() != "void"):
            if "*" in p or "[" in p or p.split()[0] == "lvq_stream_t":
                args.append(ctypes.c_void_p)
            else:
                args.append(_C_TYPES.get(" ".join(p.split()[:-1])))
        if ret not in _C_RETURNS or None in args:
            raise LvqError(f"include/lvq.h: no ctypes mapping for a type of `{ret} {name}({' '.join(params.split())})`")
        out[name] = (_C_RETURNS[ret], args)
    return out


def declared_symbols() -> List[str]:
    """Every function name declared in include/lvq.h (used by the export test and INTEGRATION.md)."""
    return sorted(prototypes())


def lib() -> ctypes.CDLL:
    """Load liblvq_hip.so (built by __graft_entry__.build() / `make -C lidar-vision-vqa_amd/csrc`) and give every entry point the
    argtypes / restype of its declaration in include/lvq.h: callers pass plain Python values, a wrong width is an ArgumentError."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LvqError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU/PyTorch fallback for the hot path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
        _push(tuning_from_env())               # the library itself never reads the environment (include/lvq.h: lvq_tuning)
    return _lib


def check(rc: int, what: str):
    if rc != LVQ_OK:
        raise LvqError(f"{what} failed: {lib().lvq_strerror(rc).decode()} ({rc})")


def stream_ptr(device=None) -> ctypes.c_void_p:
    """Current torch HIP stream as the ABI's lvq_stream_t."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def require_cuda(*tensors: torch.Tensor):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise LvqError("lidar_vision_vqa_amd ops run on an MI355X only: got a CPU tensor "
                           "(there is deliberately no CPU fallback; the CPU checker lives in oracle/)")
        if t is not None and not t.is_contiguous():
            raise LvqError("tensor must be contiguous")


_WORKSPACES = {}


def workspace(nbytes: int, device, tag: str, *, per_stream: bool = False, floor: int = 0) -> torch.Tensor:
    """Grow-only scratch buffer handed to the C ABI (the library never allocates): one per (device, tag), or per (device, tag,
    current stream) with per_stream.  Calls that share a tag share the bytes, so they must not overlap on different streams."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, tag, torch.cuda.current_stream(device).cuda_stream if per_stream else None)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _WORKSPACES[key] = torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)
    return buf


def version_of(tensors, extra=()) -> tuple:
    """Identity of what was derived from `tensors`: (data_ptr, _version, shape, device) of every non-None one, then `extra` (whatever
    else the derived value depends on and should REPLACE it when it changes: a mode, a flag, an eps).  In-place updates, load_state_dict,
    a replaced .data, .to() / .double() and a view of another shape all change it.  Known limit: a train()-mode BatchNorm forward
    updates running_mean / running_var in place without moving their _version (seen on the CPU; unmeasured on ROCm), so a fold made
    before it is served after it -- the kernels run eval() models only."""
    return tuple([(t.data_ptr(), t._version, t.shape, t.device) for t in tensors if t is not None]) + tuple(extra)


def derived(cache: dict, key, tensors, build, extra=()):
    """The one rule for values that depend on weights alone: cache[key] = (version, value), served while version_of(tensors, extra) is
    what it was stored under, else rebuilt by build().  What goes into `key` is kept side by side, what goes into `extra` replaces the
    entry.  A build() that raises leaves the entry as it was."""
    ver = version_of(tensors, extra)
    hit = cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    val = build()
    cache[key] = (ver, val)
    return val


def fold_batchnorm(bn):
    """An eval()-mode BatchNorm as a per-channel affine -> (scale, shift), fp32."""
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.float() * scale
    return scale.contiguous(), shift.contiguous()


def attention_relpos_plan(gh: int, gw: int, precision: int):
    """lvq_attention_relpos_plan (host only, a hook for tests): (K | V stages, dynamic LDS bytes) of the kernel that the fused
    relative-position attention launches on a gh x gw grid; precision 1 = plain bf16, 3 = hi + lo."""
    stages, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
    check(lib().lvq_attention_relpos_plan(gh, gw, precision, ctypes.byref(stages), ctypes.byref(nbytes)),
          f"lvq_attention_relpos_plan ({gh} x {gw}, precision {precision})")
    return stages.value, nbytes.value


def f32x(vals: Sequence[float]):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def i32x(vals: Sequence[int]):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def ptr_array(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


i64 = ctypes.c_int64
cint = ctypes.c_int
cfloat = ctypes.c_float
csize = ctypes.c_size_t
