"""CPU: the exhaustive table of the reverse loop's routes (gdmcf_amd.reverse_route.plan, recommend.route_of) over
every backbone x diffusion x target x noise scale x model state x call arguments.  The expected answers are data: they were
recorded from the predicates as they stood before the plan existed (GaussianDiffusion._latent_reverse_ok, _sparse_reverse_ok, the
DNNCat clause of GaussianDiffusionDiscrete.p_sample, recommend.route_of) over the same enumeration, and are kept in
tests/golden/reverse_route_table.json -- one entry per (model, state, diffusion, target, noise scale), one letter per call:
p_sample i / l = item / latent route, upper case where a CsrBatch stays sparse; recommend i / l / c = item / latent / latent-csr."""
import itertools
import json
import os

import numpy as np
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType
from gdmcf_amd.data_utils import DeviceCSR

I, T = 64, 5
TABLE = os.path.join(os.path.dirname(__file__), "golden", "reverse_route_table.json")


class SubDNN(gdmcf_amd.DNN):  # declares nothing of its own: the item route, dense rows
    pass


class SubCat(gdmcf_amd.DNNCat):
    pass


_EMB = dict(item_num=I, user_num=9)
BACKBONES = dict(DNN=(gdmcf_amd.DNN, {}), DNNOneHot=(gdmcf_amd.DNNOneHot, {}), DNNOneHotEmbedding=(gdmcf_amd.DNNOneHotEmbedding, _EMB),
                 DNNOneHotEmbeddingGCN=(gdmcf_amd.DNNOneHotEmbeddingGCN, _EMB), DNNCat=(gdmcf_amd.DNNCat, {}), SubDNN=(SubDNN, {}),
                 SubCat=(SubCat, {}))
# state -> (constructor keywords, training mode, dropout p or None: as constructed)
STATES = dict(eval=({}, False, None), train=({}, True, None), train_p0=({}, True, 0.0), norm=(dict(norm=True), False, None),
              bf16=(dict(gemm_dtype="bf16"), False, None))
REFUSED = {(b, s) for b in ("DNNCat", "SubCat") for s in ("norm", "bf16")}  # DNNCat builds neither F.normalize nor bf16 inputs
DIFFUSIONS = ("GaussianDiffusion", "Discrete", "Discrete+indexIn")
# the calls of one entry, in the order of the letters
P_SAMPLE_CALLS = list(itertools.product((False, True, "extended"), (0, 2), ("dense", "binary", "valued"), (False, True), (None, {})))
RECOMMEND_CALLS = list(itertools.product((True, "extended"), ("none", "rows", "other"), (0, 2), ("binary", "valued"), (False, True)))


def _model(backbone, state):
    """The model of one state, or None where the constructor does not allow it."""
    (cls, kw), (extra, training, p) = BACKBONES[backbone], STATES[state]
    try:
        m = cls([I, 16], [16, I], 10, **kw, **extra)
    except NotImplementedError:
        return None
    m.train(training)
    if p is not None:
        m.drop.p = p
    assert not training or m.drop.p > 0 or p == 0.0
    return m


def _diffusion(name, mean_type, scale):
    if name == "GaussianDiffusion":
        return gdmcf_amd.GaussianDiffusion(mean_type, "linear-var", scale, 0.001, 0.01, T, "cpu")
    d = gdmcf_amd.GaussianDiffusionDiscrete(mean_type, "linear-var", scale, 0.001, 0.01, T, "cpu", CatOneHot=True)
    d.indexIn = name == "Discrete+indexIn"
    return d


def _drives(d, m):
    """Whether p_sample of this diffusion accepts the model at all (the checks it makes ahead of any route)."""
    if not d.CatOneHot:
        return isinstance(m, gdmcf_amd.DNN)
    try:
        d._onehot_model(m)
    except (TypeError, NotImplementedError):
        return False
    return True


def _csr(values=None):
    m = sp.csr_matrix((np.random.default_rng(0).random((6, I)) < 0.2).astype(np.float64))
    if values is not None:
        m.data[:] = values
    return DeviceCSR(m, "cpu")


def enumeration():
    """(key, diffusion, model) of every entry: the full product, less the states a constructor refuses and the pairs p_sample
    refuses."""
    for name, mt, scale in itertools.product(DIFFUSIONS, (ModelMeanType.START_X, ModelMeanType.EPSILON), (0.01, 0.0)):
        d = _diffusion(name, mt, scale)
        for backbone, state in itertools.product(BACKBONES, STATES):
            m = _model(backbone, state)
            if m is not None and _drives(d, m):
                yield f"{backbone}/{state}/{name}/{mt.name}/{scale}", d, m


def rows_of_calls():
    """The row objects the calls name: matrices for recommend, and p_sample's batches of them."""
    binary, valued, other = _csr(), _csr(2.0), _csr()
    ids = torch.arange(3)
    batches = dict(dense=torch.zeros(3, I), binary=binary.batch(ids), valued=valued.batch(ids))
    return dict(binary=binary, valued=valued, other=other), batches


def test_the_enumeration_covers_every_backbone_and_state():
    keys = [k for k, _, _ in enumeration()]
    assert len(keys) == len(set(keys))
    for backbone in BACKBONES:
        for state in STATES:  # nothing drops out silently: only the states a constructor is known to refuse
            assert any(k.startswith(f"{backbone}/{state}/") for k in keys) is ((backbone, state) not in REFUSED), (backbone, state)
    for name in DIFFUSIONS:
        assert any(f"/{name}/" in k for k in keys)


def test_every_route_is_the_recorded_one():
    from gdmcf_amd import reverse_route
    from gdmcf_amd.recommend import route_of
    with open(TABLE) as fh:
        table = json.load(fh)
    csrs, batches = rows_of_calls()
    seen = 0
    for key, d, m in enumeration():
        assert key in table, f"{key}: not in the recorded table"
        want = table[key]
        got = []
        for latent, steps, rows, noise, capture in P_SAMPLE_CALLS:
            p = reverse_route.plan(d, m, batches[rows], steps, noise, capture, reverse_route.latent_mode(latent))
            assert p.route in ("item", "latent") and p.keep_sparse in (False, True)
            got.append(("L" if p.keep_sparse else "l") if p.route == "latent" else ("I" if p.keep_sparse else "i"))
        assert "".join(got) == want["p_sample"], (key, "".join(got), want["p_sample"])
        got = []
        for latent, mask, steps, rows, noise in RECOMMEND_CALLS:
            masks = dict(none=(), rows=(csrs["other"], csrs[rows]), other=(csrs["other"],))[mask]
            route = route_of(d, m, csrs[rows], steps, noise, extended=latent == "extended", masks=masks)
            got.append({"item": "i", "latent": "l", "latent-csr": "c"}[route])
        assert "".join(got) == want["recommend"], (key, "".join(got), want["recommend"])
        seen += 1
    assert seen == len(table)  # and nothing recorded that the enumeration no longer reaches
