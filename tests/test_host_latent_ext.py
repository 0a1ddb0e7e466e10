"""CPU: the host side of `latent="extended"` -- the refusals of gdmcf_latent_step_ex_f32 and gdmcf_latent_acc_f32, the new
keywords' defaults, and the truth tables of the two predicates that pick the routes (GaussianDiffusion._latent_reverse_ok and
recommend.route_of) with `extended=True`, the old answers asserted unchanged beside them."""
import importlib
import inspect

import numpy as np

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.engine_core import EpsTables

rec = importlib.import_module("gdmcf_amd.recommend")  # (the package attribute of this name is the function)
P = 4096  # stands in for device memory: the entry points refuse before anything reads it


def _ex(lib, A=P, M=P, pc=P, c1=P, c2=P, pn=P, h=None, r=None, ldr=8, qc=None, qa=None, qb=None, qn=None, ldqc=8, ldqn=8, act=0, B=2,
        N=8, K=8, lda=8, ldm=8, ldpc=8, ldpn=8, ldh=8):
    return lib.gdmcf_latent_step_ex_f32(A, lda, M, ldm, None, pc, ldpc, c1, c2, r, ldr, None, act, B, N, K, pn, ldpn, h, ldh, qc, ldqc,
                                        qa, qb, qn, ldqn, None, 0, None)


def _acc(lib, qc=P, qa=P, A=8192, qb=P, qn=P, B=2, K=8, ldqc=8, lda=8, ldqn=8):
    return lib.gdmcf_latent_acc_f32(qc, ldqc, qa, A, lda, qb, B, K, qn, ldqn, None)


def test_both_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    for name in ("gdmcf_latent_step_ex_f32", "gdmcf_latent_acc_f32"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is not None
    assert len(lib.gdmcf_latent_step_ex_f32.argtypes) == 29 and len(lib.gdmcf_latent_acc_f32.argtypes) == 11


def test_latent_step_ex_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    for dim in ("B", "N", "K"):
        assert _ex(lib, **{dim: 0}) == _lib.E_SHAPE
    for ptr in ("A", "M", "pc", "c1", "c2", "pn"):
        assert _ex(lib, **{ptr: None}) == _lib.E_ARG
    assert _ex(lib, act=2) == _lib.E_ARG
    for ld in ("lda", "ldm", "ldpc", "ldpn"):
        assert _ex(lib, **{ld: 7}) == _lib.E_SHAPE
    assert _ex(lib, h=P, ldh=7) == _lib.E_SHAPE
    assert _ex(lib, r=P, ldr=7) == _lib.E_SHAPE                                   # ldr < N
    q = dict(qc=P, qa=P, qb=P, qn=P)
    for missing in ("qc", "qa", "qb"):
        assert _ex(lib, **dict(q, **{missing: None})) == _lib.E_ARG               # an accumulator without one of its operands
    assert _ex(lib, **q, ldqc=7) == _lib.E_SHAPE and _ex(lib, **q, ldqn=7) == _lib.E_SHAPE  # ldq < K
    assert _ex(lib, **dict(q, qn=P), A=P) == _lib.E_ARG                           # q_next == A
    assert b"latent_step_ex" in lib.gdmcf_last_error()


def test_latent_acc_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    for dim in ("B", "K"):
        assert _acc(lib, **{dim: 0}) == _lib.E_SHAPE
    for ptr in ("qc", "qa", "A", "qb", "qn"):
        assert _acc(lib, **{ptr: None}) == _lib.E_ARG
    for ld in ("ldqc", "lda", "ldqn"):
        assert _acc(lib, **{ld: 7}) == _lib.E_SHAPE
    assert _acc(lib, A=P, qn=P) == _lib.E_ARG                                     # q_next == A
    assert b"latent_acc" in lib.gdmcf_last_error()


def test_the_new_keywords_and_their_defaults():
    assert inspect.signature(rec.recommend).parameters["latent"].default is True
    assert inspect.signature(rec.recommend).parameters["latent"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(rec.route_of).parameters["extended"].default is False
    assert inspect.signature(gdmcf_amd.GaussianDiffusion._latent_reverse_ok).parameters["extended"].default is False
    for fn in (gdmcf_amd.GaussianDiffusion.p_sample, gdmcf_amd.GaussianDiffusionDiscrete.p_sample, driver.evaluate):
        assert inspect.signature(fn).parameters["latent"].default is False


def _diff(mean_type=ModelMeanType.START_X, scale=0.01, schedule="linear-var", discrete=False):
    if discrete:
        return gdmcf_amd.GaussianDiffusionDiscrete(mean_type, schedule, scale, 0.001, 0.01, 5, "cpu", CatOneHot=True)
    return gdmcf_amd.GaussianDiffusion(mean_type, schedule, scale, 0.001, 0.01, 5, "cpu")


def test_eps_tables_follow_the_item_space_recursion():
    """x_0 = G x_T - D (o Q^ + b) against the unrolled item-space loop, in float64, for a scalar 'model' a_t."""
    for schedule in ("linear-var", "linear", "cosine", "binomial"):
        d = _diff(ModelMeanType.EPSILON, schedule=schedule)
        et = d._eps_tables()
        assert isinstance(et, EpsTables) and et.ok and et.D > 0 and (et.g > 0).all() and (et.d > 0).all()
        assert d._eps_tables() is et  # made once per table set
        T = d.steps
        a = np.linspace(-0.8, 0.9, T)
        x, q = 0.37, 0.0
        for t in range(T - 1, -1, -1):
            x = float(et.g[t]) * x - float(et.d[t]) * (1.7 * a[t] + 0.2)
            q = float(et.qa[t]) * q + float(et.qb[t]) * a[t]
        want = et.G * 0.37 - et.D * (1.7 * q + 0.2)
        assert abs(x - want) <= 1e-5 * max(abs(x), 1.0), (schedule, x, want)


def test_latent_reverse_ok_truth_table_with_extended():
    I = 64
    dnn = gdmcf_amd.DNN([I, 16], [16, I], 10).eval()
    cat = gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval()
    onehot = gdmcf_amd.DNNOneHot([I, 16], [16, I], 10).eval()
    x0, eps = _diff(), _diff(ModelMeanType.EPSILON)
    dx0, deps = _diff(discrete=True), _diff(ModelMeanType.EPSILON, discrete=True)
    # (diffusion, model) -> (old answer, extended answer)
    table = [(x0, dnn, True, True), (eps, dnn, False, True), (dx0, onehot, True, True), (deps, onehot, False, True),
             (dx0, cat, False, True), (deps, cat, False, True)]
    for schedule in ("linear", "cosine", "binomial"):
        table.append((_diff(ModelMeanType.EPSILON, schedule=schedule), dnn, False, True))
    for d, m, old, new in table:
        assert bool(d._latent_reverse_ok(m)) is old and bool(d._latent_reverse_ok(m, False, None)) is old
        assert bool(d._latent_reverse_ok(m, extended=True)) is new
    # everything else stays on the item route under both spellings
    for d in (x0, eps):
        for ext in (False, True):
            assert not d._latent_reverse_ok(dnn, True, None, extended=ext)       # sampling noise
            assert not d._latent_reverse_ok(dnn, False, {}, extended=ext)        # capture
            assert not d._latent_reverse_ok(gdmcf_amd.DNN([I, 16], [16, I], 10, norm=True).eval(), extended=ext)
            assert not d._latent_reverse_ok(gdmcf_amd.DNN([I, 16], [16, I], 10).train(), extended=ext)  # active dropout
            for dt in ("bf16", "f32x3"):
                assert not d._latent_reverse_ok(gdmcf_amd.DNN([I, 16], [16, I], 10, gemm_dtype=dt).eval(), extended=ext)
    for mt in (ModelMeanType.START_X, ModelMeanType.EPSILON):
        assert not _diff(mt, scale=0.0)._latent_reverse_ok(dnn, extended=True)   # noise_scale == 0

    class Sub(gdmcf_amd.DNNCat):
        pass
    assert not dx0._latent_reverse_ok(Sub([I, 16], [16, I], 10).eval(), extended=True)  # exact types
    # the eps tables: a non-finite coefficient, D <= 0
    bad = _diff(ModelMeanType.EPSILON)
    et = bad._eps_tables()
    et.ok = False
    assert not bad._latent_reverse_ok(dnn, extended=True) and not bad._latent_reverse_ok(dnn)
    assert not EpsTables([1.0, np.inf], [0.0, 0.5], [1.0, 1.0], [0.1, 0.1], 2).ok
    assert not EpsTables([1.0, 1.0], [0.0, 0.5], [1.0, 1.0], [-0.1, -0.1], 2).ok  # D < 0
    assert EpsTables([1.0, 1.0], [0.0, 0.5], [1.0, 1.0], [0.1, 0.1], 2).ok
    # x0 under "extended" keeps the x0 conditions: c2[0] == 0
    bad = _diff()
    bad._t32 = dict(bad._t32, c2=bad._t32["c2"].clone())
    bad._t32["c2"][0] = 1e-3
    assert not bad._latent_reverse_ok(dnn, extended=True)


def _csr(I, values=None):
    """What route_of reads of a DeviceCSR -- `values` (None: binary rows) and identity -- without a device."""
    d = DeviceCSR.__new__(DeviceCSR)
    d.values = None if values is None else object()
    d.shape = (6, I)
    return d


def test_route_truth_table_with_extended():
    I = 64
    dnn = gdmcf_amd.DNN([I, 16], [16, I], 10).eval()
    cat = gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval()
    rows, other, valued = _csr(I), _csr(I), _csr(I, 2.0)
    x0, eps = _diff(), _diff(ModelMeanType.EPSILON)
    dx0, deps = _diff(discrete=True), _diff(ModelMeanType.EPSILON, discrete=True)
    # the old answers, unchanged
    assert rec.route_of(x0, dnn, rows) == "latent-csr" and rec.route_of(x0, dnn, rows, 3) == "latent"
    for d, m in ((eps, dnn), (dx0, cat), (deps, cat)):
        assert rec.route_of(d, m, rows) == "item" and rec.route_of(d, m, rows, 3) == "item"
    # extended: x0 as before, DNNCat like DNN
    assert rec.route_of(x0, dnn, rows, extended=True) == "latent-csr"
    for masks in (None, (), (rows,), (other,)):
        assert rec.route_of(dx0, cat, rows, extended=True, masks=masks) == "latent-csr"
    assert rec.route_of(dx0, cat, rows, 3, extended=True) == "latent"
    assert rec.route_of(dx0, cat, valued, extended=True) == "latent"
    # extended, eps: latent-csr only with the rows themselves among the masks
    for d, m in ((eps, dnn), (deps, cat)):
        assert rec.route_of(d, m, rows, extended=True, masks=(rows,)) == "latent-csr"
        assert rec.route_of(d, m, rows, extended=True, masks=(other, rows)) == "latent-csr"
        for masks in (None, (), (other,)):
            assert rec.route_of(d, m, rows, extended=True, masks=masks) == "latent"
        assert rec.route_of(d, m, rows, 3, extended=True, masks=(rows,)) == "latent"
        assert rec.route_of(d, m, valued, extended=True, masks=(valued,)) == "latent"
        assert rec.route_of(d, m, rows, 0, True, extended=True, masks=(rows,)) == "item"  # sampling noise
