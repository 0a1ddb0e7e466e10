"""CPU (-m "not gpu"): gdmcf_amd._lib derives its ctypes binding from include/gdmcf_hip.h.  The parser on a synthetic header;
signatures and constants pinned by hand, independent of the parser; every declared symbol exported by the built library and
bound as derived; GdDwAdamw's layout against the C compiler's."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

from gdmcf_amd import _lib, engine_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gdmcf_hip.h")
P = c_void_p

SYNTHETIC = """\
/* the comment's own gdmcf_fake(int a); is no declaration,
 * on any of its lines */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GDMCF_OK 0
#define GDMCF_E_BAD (-7)   /* a parenthesised negative value */
#define GDMCF_N_THINGS 13
enum { GDMCF_MODE_A = 0, GDMCF_MODE_B = 3 };
typedef struct GdPair {
    const float* x;
    int a, b, c;
    int64_t ld;
    double w;
} GdPair;
int gdmcf_none(void);
const char* gdmcf_name(char* buf_host, size_t n);
int64_t gdmcf_three(int a,
                    int64_t b, /* between parameters */
                    uint64_t c);
uint64_t gdmcf_stars(float *x, float* y, const float* const* z, void** w);
size_t gdmcf_reals(double d, float f);
float gdmcf_f(const GdPair* list);
double gdmcf_d();
void* gdmcf_p(const void* q /* NULL: all */);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    assert _lib.parse_functions(SYNTHETIC) == {
        "gdmcf_none": (c_int, []),
        "gdmcf_name": (c_char_p, [c_char_p, c_size_t]),
        "gdmcf_three": (c_int64, [c_int, c_int64, c_uint64]),
        "gdmcf_stars": (c_uint64, [P, P, P, P]),
        "gdmcf_reals": (c_size_t, [c_double, c_float]),
        "gdmcf_f": (c_float, [P]),
        "gdmcf_d": (c_double, []),
        "gdmcf_p": (P, [P]),
    }
    assert list(_lib.parse_functions(SYNTHETIC))[:3] == ["gdmcf_none", "gdmcf_name", "gdmcf_three"]  # the header's order
    assert _lib.parse_constants(SYNTHETIC) == {"GDMCF_OK": 0, "GDMCF_E_BAD": -7, "GDMCF_N_THINGS": 13, "GDMCF_MODE_A": 0,
                                               "GDMCF_MODE_B": 3}
    assert _lib.parse_structs(SYNTHETIC) == {"GdPair": [("x", P), ("a", c_int), ("b", c_int), ("c", c_int), ("ld", c_int64),
                                                        ("w", c_double)]}


@pytest.mark.parametrize("decl,named", [
    ("int gdmcf_wide(unsigned long n);", "gdmcf_wide"),     # a parameter type outside the map
    ("long gdmcf_ret(int n);", "gdmcf_ret"),                # a return type outside the map
    ("int gdmcf_bare(int, float x);", "gdmcf_bare"),        # a parameter without a name
    ("int gdmcf_cb(void (*fn)(int), int n);", "gdmcf_cb"),  # the pattern cannot match it: caught by the count
    ("int gdmcf_twice(int n);\nint gdmcf_twice(int n);", "repeated"),
])
def test_parser_refuses_what_it_cannot_read(decl, named):
    with pytest.raises(ImportError, match=named):
        _lib.parse_functions("int gdmcf_ok(int a);\n" + decl + "\nint gdmcf_after(void);\n")


def test_struct_and_enum_parsers_refuse_what_they_cannot_read():
    with pytest.raises(ImportError, match="GdBad"):
        _lib.parse_structs("typedef struct GdBad { unsigned n; } GdBad;")
    with pytest.raises(ImportError, match="GdBad"):
        _lib.parse_structs("typedef struct GdBad { float *a, b; } GdBad;")  # (in C, b is no pointer)
    with pytest.raises(ImportError, match="GDMCF_B"):
        _lib.parse_constants("enum { GDMCF_A = 0, GDMCF_B };")


PINS = {
    "gdmcf_last_error": (c_char_p, []),
    "gdmcf_device_info": (c_int, [P, P, c_char_p, c_int]),
    "gdmcf_schedule_build": (c_int, [c_int, c_double, c_double, c_double, c_int, c_int, P]),
    "gdmcf_linear_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gdmcf_bf16_shadow_get": (P, [P]),
    "gdmcf_linear_fwd_f32": (c_int, [P, c_int64, P, c_int64, P, c_int, c_int, c_int, c_int, P, c_int64, P, c_size_t, P]),
    "gdmcf_randn_f32": (c_int, [P, c_int64, c_int, c_int, c_int, c_uint64, c_uint64, P]),
    "gdmcf_spmm_stream_f32": (c_int, [P, c_int, P, c_int64, P, c_int, P, P, c_int, c_int, c_int, P, c_int64, c_int, P, c_int64, P, P,
                                      c_int, c_int64, c_float, c_double, P]),
    "gdmcf_adam_hyper_fill": (c_int, [P, c_int, c_float, c_float, c_float, c_float, c_float, c_int64, c_float]),
    "gdmcf_linear_bwd_weight_adamw_multi_f32": (c_int, [P, c_int, P]),
    "gdmcf_debug_dr_tn_plan": (c_int, [c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int, c_int, P, P, P, P, P, P]),
}


@pytest.mark.parametrize("name", sorted(PINS))
def test_signatures_pinned_by_hand(name):
    assert _lib._SIGNATURES[name] == PINS[name]


def test_constants_and_struct_fields_pinned_by_hand():
    assert _lib.GDMCF_OK == 0
    assert (_lib.E_SHAPE, _lib.E_ARG, _lib.E_UNSUPPORTED, _lib.E_HIP, _lib.E_WORKSPACE) == (-1, -2, -3, -4, -5)
    assert _lib.N_TABLES == 13 == len(_lib.TABLE_NAMES)
    assert engine_core._GEMM_MODES == {"f32": 0, "bf16": 1, "f32x3": 2}
    assert _lib.GdDwAdamw._fields_ == [
        ("dZ", P), ("lddz", c_int64), ("A", P), ("lda", c_int64), ("rowscale", P), ("a_scale_col", c_int), ("M", c_int),
        ("N", c_int), ("K", c_int), ("W", P), ("ldw", c_int64), ("exp_avg", P), ("exp_avg_sq", P), ("db", P), ("lr", c_float),
        ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float), ("step", c_int),
        ("grad_scale", c_float)]


def _scrape(path):
    """{name: [parameter text, ...]} by this test's own reading of the header: commas counted, nothing else understood."""
    code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {name: [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
            for name, params in re.findall(r"\b(gdmcf_\w+)\s*\(([^)]*)\)\s*;", code)}


DECLARED = _scrape(HEADER)


def test_every_declaration_is_bound():
    assert len(DECLARED) >= 71 and set(DECLARED) == set(_lib.EXPORTED_SYMBOLS) == set(_lib._SIGNATURES)


@pytest.mark.parametrize("name", _lib.EXPORTED_SYMBOLS)
def test_symbol_is_declared_exported_and_bound(name):
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} declared in include/gdmcf_hip.h but not exported by libgdmcf_hip.so"
    res, args = _lib._SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args
    params = DECLARED[name]
    assert len(args) == len(params), (len(args), params)
    # pointers where the header has pointers, scalars where it has scalars
    for p, t in zip(params, args):
        assert ("*" in p) == (t in (c_void_p, c_char_p)), (p, t)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof(GdDwAdamw) and every member's offsetof, as a C99 program that includes the header prints them, against the
    ctypes structure derived from the header's text."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    names = [n for n, _ in _lib.GdDwAdamw._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("%%zu\\n", sizeof(GdDwAdamw));\n' % HEADER
                   + "".join('    printf("%%zu\\n", offsetof(GdDwAdamw, %s));\n' % n for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    size, *offsets = [int(v) for v in r.stdout.split()]
    assert len(names) == 21 and ctypes.sizeof(_lib.GdDwAdamw) == size
    assert [getattr(_lib.GdDwAdamw, n).offset for n in names] == offsets
