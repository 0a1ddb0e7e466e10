"""CPU (-m "not gpu"): the C ABI of the one-hot backbones' CSR-fed input builder, gdmcf_onehot_prep_input_csr_f32 -- declared
in include/gdmcf_hip.h, exported by the built library, bound by gdmcf_amd._lib with as many arguments as the header names."""
import os
import re

from gdmcf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gdmcf_onehot_prep_input_csr_f32"


def test_onehot_prep_input_csr_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gdmcf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, f"{NAME} is not declared in include/gdmcf_hip.h"
    params = [p.strip() for p in m.group(1).split(",") if p.strip()]
    lib = _lib.load()
    assert hasattr(lib, NAME), f"{NAME} declared but not exported by libgdmcf_hip.so"
    assert NAME in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGNATURES[NAME]
    assert len(args) == len(params), (len(args), params)
    assert getattr(lib, NAME).argtypes == args
    # pointers where the header has pointers, scalars where it has scalars
    for p, t in zip(params, args):
        assert ("*" in p) == (t is _lib.P), (p, t)


def test_onehot_prep_input_csr_rejects_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: an empty batch and missing CSR arrays come back as error codes."""
    lib = _lib.load()
    f = getattr(lib, NAME)
    bad_shape = f(None, None, None, None, 0.99, None, 0, 0, 0, None, 0, None, 0, None, 0, 0.0, 0, None, None, 0, 0, 10, None, 64,
                  None, None, 0, None)
    assert bad_shape == _lib.E_SHAPE
    no_csr = f(None, None, None, None, 0.99, None, 0, 0, 0, None, 0, None, 0, None, 0, 0.0, 0, None, None, 0, 2, 10, 4096, 64,
               None, None, 0, None)
    assert no_csr == _lib.E_ARG
