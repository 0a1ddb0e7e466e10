"""CPU: the host side of the reverse loop from CSR rows -- gdmcf_gather_fwd_f32's refusals (its declaration, export and binding:
tests/test_host_abi.py; gather_fwd.hip in the build lists: test_build_lists_name_every_source_and_header), the `sparse` keyword of
driver.evaluate, and a CsrBatch on the CPU refused like any CPU tensor."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd.data_utils import CsrBatch, DeviceCSR


def _call(lib, B=2, N=8, E=0, pre=None, indptr=None, indices=None, rows=None, table=None, a=None, tblE=None, out=None, act=0,
          ldt=8, I=4):
    return lib.gdmcf_gather_fwd_f32(pre, 8, None, indptr, indices, rows, table, ldt, I, a, 16, tblE, 8, E, None, act, B, N, out, 8,
                                    None)


def test_gather_entry_point_checks_its_arguments():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory)."""
    lib = _lib.load()
    assert "gdmcf_gather_fwd_f32" in _lib.EXPORTED_SYMBOLS
    p = 4096  # a 16-byte aligned stand-in
    assert _call(lib, B=0, pre=p, out=p) == _lib.E_SHAPE                      # an empty batch
    assert _call(lib, B=0) == _lib.E_SHAPE                                    # ... before the null pointers
    assert _call(lib, N=0, pre=p, out=p) == _lib.E_SHAPE
    assert _call(lib, pre=p) == _lib.E_ARG                                    # no output
    assert _call(lib, out=p) == _lib.E_ARG                                    # none of pre / CSR rows / a
    assert _call(lib, out=p, E=10) == _lib.E_ARG                              # E > 0 without a
    assert _call(lib, out=p, indptr=p, indices=p, rows=p) == _lib.E_ARG       # CSR rows without their table
    assert _call(lib, out=p, indptr=p, table=p) == _lib.E_ARG                 # ... without indices / row ids
    assert _call(lib, out=p, pre=p, a=p, E=10) == _lib.E_ARG                  # a without tblE
    assert _call(lib, out=p, pre=p, a=p, E=0) == _lib.E_ARG                   # a with E == 0
    assert _call(lib, out=p, pre=p, act=2) == _lib.E_ARG
    assert _call(lib, out=p, indptr=p, indices=p, rows=p, table=p, ldt=10) == _lib.E_SHAPE   # ldt % 4 != 0
    assert _call(lib, out=p, indptr=p, indices=p, rows=p, table=p + 4) == _lib.E_SHAPE       # table not 16-byte aligned
    assert _call(lib, out=p, indptr=p, indices=p, rows=p, table=p, ldt=4) == _lib.E_SHAPE    # ldt < N
    assert b"gather_fwd" in lib.gdmcf_last_error()


def test_evaluate_has_the_sparse_keyword_off_by_default():
    par = inspect.signature(driver.evaluate).parameters["sparse"]
    assert par.default is False


def test_csr_batch_on_the_cpu_is_refused_like_a_cpu_tensor():
    I = 64
    x = sp.csr_matrix((np.random.default_rng(0).random((4, I)) < 0.2).astype(np.float64))
    batch = DeviceCSR(x, "cpu").batch(torch.arange(4))
    assert isinstance(batch, CsrBatch) and not batch.is_cuda
    model = gdmcf_amd.DNN([I, 16], [16, I], 10).eval()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu")
    with pytest.raises(RuntimeError, match="MI355X"):
        diff.p_sample(model, batch, 0, False)
    onehot = gdmcf_amd.DNNOneHot([I, 16], [16, I], 10).eval()
    ddiff = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu", CatOneHot=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        ddiff.p_sample(onehot, batch, 0, False)
    with pytest.raises(RuntimeError, match="MI355X"):
        onehot(batch, torch.zeros(4, dtype=torch.int64), None)
