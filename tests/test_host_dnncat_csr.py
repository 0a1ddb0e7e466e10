"""CPU (-m "not gpu"): the DNNCat backbone's opt-in to rows that stay sparse (`csr_rows=True`) and the argument checks of the two
entry points behind it, gdmcf_cat_prep_input_csr_f32 and gdmcf_cat_grad_bits_f32, which refuse before any launch (their
declaration, export and binding: tests/test_host_abi.py)."""
import copy
import ctypes
import pickle

import gdmcf_amd
from gdmcf_amd import _lib


def _model(**kw):
    return gdmcf_amd.DNNCat([64, 16], [16, 64], 10, **kw)


def test_csr_rows_is_an_opt_in_on_the_instance():
    assert gdmcf_amd.DNNCat.csr_rows is False
    m = _model()
    assert m.csr_rows is False and "csr_rows" not in vars(m)
    assert _model(csr_rows=False).csr_rows is False
    s = _model(csr_rows=True)
    assert s.csr_rows is True and gdmcf_amd.DNNCat.csr_rows is False
    for clone in (pickle.loads(pickle.dumps(s)), copy.deepcopy(s)):
        assert clone.csr_rows is True
    for clone in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert clone.csr_rows is False


# Non-null stand-ins for the pointer arguments: host memory the checks never dereference (every call below is refused before
# the first launch).  16-byte aligned, as the entries ask of xin, x_t and the workspace.
_MEM = ctypes.create_string_buffer(4096 + 16)
P = (ctypes.addressof(_MEM) + 15) & ~15


def prep_args(**kw):
    """Valid arguments of gdmcf_cat_prep_input_csr_f32 for B = 2, I = 40, E = 10 (given classes), then `kw` on top."""
    a = dict(indptr=P, indices=P, rows=P, ts_U=None, discrete=0.99, sampled=P, lds=40, offset_noise=1, ts=P, ca=None, cb=None,
             noise_mode=0, noise=None, ldn=0, drop_mode=0, keep=None, ldkeep=0, drop_p=0.5, seed=3, offset_prep=2, cat_w=P,
             cat_b=P, emb_w=P, emb_b=P, E=10, B=2, I=40, xin=P, ldxin=64, xt_out=P, ldxt=64, temb_out=P, x0bits_out=P,
             ldx0bits=2, clsbits_out=P, ldclsbits=2, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def grad_args(**kw):
    """Valid arguments of gdmcf_cat_grad_bits_f32 for B = 2, I = 40 up to the workspace, then `kw` on top."""
    a = dict(dxin=P, lddx=64, xt=P, ldxt=64, x0bits=P, ldx0bits=2, clsbits=P, ldclsbits=2, drop_mode=0, keep=None, ldkeep=0,
             drop_p=0.5, seed=3, offset=2, B=2, I=40, ws=P, ws_bytes=0, grad_w=P, grad_b=P, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def test_cat_prep_input_csr_checks_its_arguments_before_launching():
    f = _lib.load().gdmcf_cat_prep_input_csr_f32
    for kw in (dict(B=0), dict(ldx0bits=1), dict(ldclsbits=1), dict(ldxin=66), dict(ldxin=48), dict(ldxt=36), dict(E=0)):
        assert f(*prep_args(**kw)) == _lib.E_SHAPE, kw
    for kw in (dict(indptr=None), dict(indices=None), dict(rows=None), dict(ts=None), dict(cat_w=None), dict(cat_b=None),
               dict(emb_w=None), dict(x0bits_out=None), dict(clsbits_out=None),      # null pointers; both bitmaps are required
               dict(noise_mode=3), dict(drop_mode=-1), dict(drop_mode=3),            # bad modes
               dict(lds=39),                                                         # given classes need lds >= I
               dict(sampled=None, ts_U=None),                                        # drawn classes need ts_U
               dict(ca=P), dict(ca=P, cb=P, noise_mode=1), dict(drop_mode=1), dict(drop_mode=1, keep=P, ldkeep=39),
               dict(drop_p=1.0)):
        assert f(*prep_args(**kw)) == _lib.E_ARG, kw
    assert b"cat_prep_input_csr" in _lib.load().gdmcf_last_error()


def test_cat_grad_bits_checks_its_arguments_before_launching():
    lib = _lib.load()
    f = lib.gdmcf_cat_grad_bits_f32
    for kw in (dict(B=0), dict(I=0), dict(lddx=39), dict(ldxt=39), dict(ldx0bits=1), dict(ldclsbits=1)):
        assert f(*grad_args(**kw)) == _lib.E_SHAPE, kw
    for kw in (dict(dxin=None), dict(xt=None), dict(x0bits=None), dict(clsbits=None), dict(grad_w=None), dict(grad_b=None),
               dict(drop_mode=3), dict(drop_mode=1), dict(drop_mode=1, keep=P, ldkeep=39), dict(drop_p=-0.1)):
        assert f(*grad_args(**kw)) == _lib.E_ARG, kw
    # a short, a missing and a misaligned workspace (the partial layout is the dense kernel's: gdmcf_cat_grad_ws_bytes)
    need = lib.gdmcf_cat_grad_ws_bytes(2, 40)
    assert need == 2 * 16
    for kw in (dict(ws_bytes=need - 1), dict(ws=None, ws_bytes=need), dict(ws=P + 4, ws_bytes=need)):
        assert f(*grad_args(**kw)) == _lib.E_WORKSPACE, kw
    assert b"cat_grad_bits" in lib.gdmcf_last_error()
