"""ctypes binding of libgdmcf_hip.so, derived from the C ABI's own text: include/gdmcf_hip.h is parsed once at import, and
every signature, the fields of GdDwAdamw and GdKnTail and the GDMCF_* constants follow from it.  A new entry point is declared in the header and
defined in a .hip file; nothing is restated here.  The header is plain C99 in one style (`<type> <name>` parameters, /* */
comments), which is all the parser reads.  Type map, for parameters, return types and struct members (`const` is dropped):
    int -> c_int    int64_t -> c_int64    uint64_t -> c_uint64    size_t -> c_size_t    float -> c_float    double -> c_double
    char* -> c_char_p    any other pointer -> c_void_p    anything else -> ImportError naming the declaration

The product path has NO CPU fallback: if the HIP library is missing, or a kernel is asked to run
without a GPU, this module raises -- it never routes through PyTorch eager or the oracle.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgdmcf_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "gdmcf_hip.h"))

P = c_void_p
_CTYPES = {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "size_t": c_size_t, "float": c_float, "double": c_double}


def _uncomment(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _code(text):
    """A header's declarations: no comments, no preprocessor lines, no `extern "C" {` / `}` lines."""
    return re.sub(r'^[ \t]*(#.*|extern\s+"C"\s*\{|\})[ \t]*$', "", _uncomment(text), flags=re.M)


def _ctype(ctype, where):
    words = re.sub(r"\bconst\b", " ", ctype).replace("*", " * ").split()
    if "*" in words:
        return c_char_p if words == ["char", "*"] else c_void_p
    if " ".join(words) not in _CTYPES:
        raise ImportError(f"gdmcf_hip.h: no ctypes type for '{' '.join(ctype.split())}' in the declaration of {where}")
    return _CTYPES[" ".join(words)]


def _declarator(decl, where):
    """('<type>', '<name>') of a parameter or a struct member; the stars may sit on either side of the space."""
    m = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", decl, flags=re.S)
    if not m:
        raise ImportError(f"gdmcf_hip.h: cannot read '{decl.strip()}' in the declaration of {where}")
    return m.groups()


def parse_functions(text):
    """{name: (restype, [argtypes])} of every `<ret> gdmcf_<name>(<params>);` of a header text, in the header's order."""
    code = _code(text)
    out = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(gdmcf_\w+)\s*\(([^()]*)\)\s*;", code):
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype(ret, name), [_ctype(_declarator(p, name)[0], name) for p in params])
    # a declaration the pattern skipped must not become a function that ctypes calls with its default int arguments
    mentioned = re.findall(r"(gdmcf_\w+)\s*\(", code)
    if len(mentioned) != len(out):
        raise ImportError(f"gdmcf_hip.h: {len(mentioned)} gdmcf_*( but {len(out)} declarations read; unreadable: "
                          f"{sorted(set(mentioned) - set(out)) or 'none, a name is repeated'}")
    return out


def parse_constants(text):
    """{name: int} of every `#define GDMCF_<NAME> <integer or (-integer)>` and every `NAME = n` member of an anonymous enum."""
    text = _uncomment(text)
    out = {n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+(GDMCF_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for member in filter(str.strip, body.split(",")):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", member)
            if not m:
                raise ImportError(f"gdmcf_hip.h: enum member '{member.strip()}' is not `NAME = integer`")
            out[m.group(1)] = int(m.group(2))
    return out


def parse_structs(text):
    """{name: [(member, ctype), ...]} of every `typedef struct <name> { ... } <name>;`; a line may declare several members."""
    out = {}
    for name, body in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\1\s*;", _code(text)):
        out[name] = []
        for line in filter(str.strip, body.split(";")):
            first, *more = line.split(",")
            ctype, member = _declarator(first, "struct " + name)
            if more and "*" in line:  # (`float *a, b;` declares one pointer and one float)
                raise ImportError(f"gdmcf_hip.h: struct {name}: '{line.strip()}' must declare one pointer member per line")
            out[name] += [(m.strip(), _ctype(ctype, "struct " + name)) for m in [member] + more]
    return out


try:
    with open(HEADER_PATH) as _f:
        _HEADER = _f.read()
except OSError as e:
    raise ImportError(f"{HEADER_PATH} is missing: gdmcf_amd._lib derives its ctypes binding from the C header, which sits "
                      "beside the package in the source tree.") from e
_SIGNATURES = parse_functions(_HEADER)
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
CONSTANTS = parse_constants(_HEADER)
GDMCF_OK, E_SHAPE, E_ARG, E_UNSUPPORTED, E_HIP, E_WORKSPACE, N_TABLES = (
    CONSTANTS["GDMCF_" + n] for n in ("OK", "E_SHAPE", "E_ARG", "E_UNSUPPORTED", "E_HIP", "E_WORKSPACE", "N_TABLES"))
TABLE_NAMES = (
    "betas", "alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next", "sqrt_alphas_cumprod",
    "sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
    "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
    "posterior_mean_coef1", "posterior_mean_coef2",
)


class GdDwAdamw(ctypes.Structure):
    """One entry of gdmcf_linear_bwd_weight_adamw_multi_f32's list (include/gdmcf_hip.h): the arguments of one
    gdmcf_linear_bwd_weight_adamw_f32 call."""
    _fields_ = parse_structs(_HEADER)["GdDwAdamw"]


class GdKnTail(ctypes.Structure):
    """The tail job of gdmcf_linear_bwd_input_tail_f32 (include/gdmcf_hip.h): the arguments of the row-partial reducer, of
    gdmcf_row_loss_finish_mean_f64 and of gdmcf_rowscale_f32."""
    _fields_ = parse_structs(_HEADER)["GdKnTail"]


_lib = None


def load():
    """Loads the shared library (building nothing).  Raises ImportError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m gdmcf_amd.build` (hipcc, gfx950). "
            "gdmcf_amd has no CPU / PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError -> the .so is stale; rebuild
        fn.restype = res
        fn.argtypes = args
    if lib.gdmcf_version() != 1:
        raise ImportError("libgdmcf_hip.so ABI version mismatch; rebuild with `python -m gdmcf_amd.build --force`")
    _lib = lib
    return lib


_EXC = {E_SHAPE: AssertionError, E_ARG: ValueError, E_UNSUPPORTED: NotImplementedError, E_HIP: RuntimeError,
        E_WORKSPACE: RuntimeError}


def check(rc):
    if rc != GDMCF_OK:
        msg = load().gdmcf_last_error().decode(errors="replace")
        raise _EXC.get(rc, RuntimeError)(msg or f"gdmcf error {rc}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"gdmcf_amd: {what} must live on the MI355X (got device '{t.device}'); "
                           "the HIP path has no CPU fallback")


def shadow_info(data_ptr):
    """(bf16 pointer, rows, cols, ld) of the registered bf16 shadow of a float32 base pointer, or None."""
    p16 = ctypes.c_void_p()
    rows, cols, ld = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    if not load().gdmcf_bf16_shadow_info(data_ptr, ctypes.byref(p16), ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(ld)):
        return None
    return int(p16.value), int(rows.value), int(cols.value), int(ld.value)


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def philox_randn(shape, device, seed, offset, stream_id=4, out=None):
    """[rows, cols] float32 N(0,1) drawn by gdmcf_randn_f32 (Philox4x32-10, Box-Muller) -- the device draw that stands where
    the reference calls th.randn_like (gaussian_diffusion.py:328-331, :210-217).  No CPU path: `device` must be a GPU."""
    import torch
    rows, cols = int(shape[0]), int(shape[1])
    if out is None:
        out = torch.empty(rows, cols, dtype=torch.float32, device=device)
    require_gpu(out, "philox_randn output")
    check(load().gdmcf_randn_f32(out.data_ptr(), out.stride(0), rows, cols, int(stream_id), int(seed) & (2 ** 64 - 1),
                                 int(offset) & (2 ** 64 - 1), stream_ptr()))
    return out


def schedule_tables(kind, noise_scale, noise_min, noise_max, steps, beta_fixed=True):
    """Host float64 tables [13][T] via the C ABI (no GPU needed)."""
    import numpy as np
    out = np.zeros((N_TABLES, steps), dtype=np.float64)
    rc = load().gdmcf_schedule_build(kind, float(noise_scale), float(noise_min), float(noise_max), int(steps),
                                     int(bool(beta_fixed)), out.ctypes.data_as(c_void_p))
    check(rc)
    return out


class Bf16Shadow:
    """A bf16 shadow of a 2-D float32 device tensor (include/gdmcf_hip.h, gdmcf_bf16_shadow_set): zero-padded
    [round_up(rows, 64)][round_up(cols, 64)] bfloat16 buffer.  Registered on construction; `unregister()` /
    `register()` bracket code that writes the float32 tensor with kernels that do not maintain shadows; the
    registration is dropped with the object."""

    def __init__(self, t, sync=True):
        import weakref

        import torch
        require_gpu(t, "bf16 shadow source")
        if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
            raise RuntimeError("gdmcf_amd: a bf16 shadow needs a 2-D float32 tensor with unit column stride")
        self.rows, self.cols = t.shape
        self.ptr = t.data_ptr()
        self.ld = t.stride(0)
        self.buf = torch.zeros((self.rows + 63) // 64 * 64, (self.cols + 63) // 64 * 64, dtype=torch.bfloat16,
                               device=t.device)
        self._lib = load()
        self._fin = weakref.finalize(self, self._lib.gdmcf_bf16_shadow_clear, self.ptr)
        self.register()
        if sync:
            self.sync()

    def register(self):
        check(self._lib.gdmcf_bf16_shadow_set(self.ptr, self.buf.data_ptr(), self.rows, self.cols, self.buf.stride(0)))

    def unregister(self):
        self._lib.gdmcf_bf16_shadow_clear(self.ptr)

    def sync(self):
        """Refresh the shadow from the float32 tensor (needed after anything but a gdmcf kernel wrote it)."""
        check(self._lib.gdmcf_bf16_shadow_sync(self.ptr, self.ld, stream_ptr()))

    def close(self):
        self._fin()
