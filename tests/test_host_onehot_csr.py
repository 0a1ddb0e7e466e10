"""CPU (-m "not gpu"): the one-hot backbones' CSR-fed input builder, gdmcf_onehot_prep_input_csr_f32, checks its arguments
before any launch (its declaration, export and binding: tests/test_host_abi.py)."""
from gdmcf_amd import _lib

NAME = "gdmcf_onehot_prep_input_csr_f32"


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
