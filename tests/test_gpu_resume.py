"""GPU (-m gpu): a checkpointed run resumes bit for bit, on every backbone and through every random stream.

`run` trains a few steps, saves with checkpoint.save_checkpoint, trains on; a second set of freshly built objects loads the
file and runs the same continuation.  Everything the two leave behind is compared with torch.equal / == -- no tolerance
anywhere in this file.  No randomness is injected (timesteps, noise, dropout, class draws are the library's own, in-kernel),
so a stream position or seed the checkpoint does not carry shows as different bits.  Every case also runs its reference twice
(the kernels claim a fixed order) and proves that it bites: a continuation that loads the checkpoint and then puts the one
counter under test back to 0 (or changes the seed) must give different losses or evaluation outputs -- a case whose stream
never took part could not fail (the "stale operands cannot pass" idiom of tests/test_gpu_latent.py)."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gdmcf_amd
from gdmcf_amd import ModelMeanType, checkpoint

DEV = "cuda:0"
T, U, EMB = 5, 301, 10
SEED = 7  # torch's seed of every reference run: what the diffusion's draws and a fresh engine are keyed on
X0, EPS = ModelMeanType.START_X, ModelMeanType.EPSILON
COUNTERS = ("_ts_calls", "_q_calls", "_randn_calls", "_noise_calls")


# ---- rows ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(I):
    """U users x I items from a fixed CPU generator: the dense matrix, the same rows resident as CSR, and the user ids of
    the batches (distinct within a batch: they index the embedding tables too)."""
    import scipy.sparse as sp
    from gdmcf_amd.data_utils import DeviceCSR
    g = torch.Generator().manual_seed(0)
    full = (torch.rand(U, I, generator=g) < 0.05).float()
    dcsr = DeviceCSR(sp.csr_matrix(full.numpy().astype(np.float64)), DEV)
    assert dcsr.values is None
    order = [torch.randperm(U, generator=g) for _ in range(8)]
    return SimpleNamespace(full=full, dcsr=dcsr, order=order)


def _rows(I, ids, rows):
    data = _data(I)
    return data.dcsr.batch(ids) if rows == "csr" else data.full[ids].to(DEV)


# ---- objects ------------------------------------------------------------------------------------------------------------------
def _continuous(mean_type, scale=0.01):
    return gdmcf_amd.GaussianDiffusion(mean_type, "linear-var", scale, 0.001, 0.01, T, DEV)


def _discrete(mean_type, index_in=False):
    d = gdmcf_amd.GaussianDiffusionDiscrete(mean_type, "linear-var", 0.01, 0.001, 0.01, T, DEV, CatOneHot=True)
    d.indexIn = index_in
    return d


def _objects(model, diffusion, fuse=False):
    m = model.to(DEV).train()
    o = gdmcf_amd.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    if fuse:
        o.fuse_into_backward(m, min_numel=1)
        assert o._fused_ids
    return SimpleNamespace(m=m, d=diffusion, o=o)


def build_dnn(mean_type, I=515, hid=64, scale=0.01):
    return lambda: _objects(gdmcf_amd.DNN([I, hid], [hid, I], EMB), _continuous(mean_type, scale))


def build_onehot(mean_type, I=257, hid=48):
    return lambda: _objects(gdmcf_amd.DNNOneHot([I, hid], [hid, I], EMB), _discrete(mean_type))


def build_embedding(I=257, hid=48):
    return lambda: _objects(gdmcf_amd.DNNOneHotEmbedding([I, hid], [hid, I], EMB, item_num=I, user_num=U), _discrete(X0, True))


def build_gcn(I=257, hid=48):
    def build():
        model = gdmcf_amd.DNNOneHotEmbeddingGCN([I, hid], [hid, I], EMB, item_num=I, user_num=U)
        with torch.no_grad():
            model.sumW.fill_(0.6)  # the GCN branch carries weight
        return _objects(model, _discrete(X0, True), fuse=True)
    return build


def build_cat(mean_type, csr_rows=False, I=515, hid=48):
    return lambda: _objects(gdmcf_amd.DNNCat([I, hid], [hid, I], EMB, csr_rows=csr_rows), _discrete(mean_type))


# ---- steps --------------------------------------------------------------------------------------------------------------------
def eager_steps(I, B, rows="dense", index=False):
    """step_fn of the plain loop: zero_grad -> training_losses(reweight=True) -> mean -> backward -> step on batch k; the step
    returns the per-row losses.  (A step_fn is a context manager over the objects and the phase -- "before" the save, "after"
    it in the reference run, "resumed" -- that yields step(k).)"""
    @contextlib.contextmanager
    def step_fn(objs, phase):
        def step(k):
            ids = _data(I).order[k][:B]
            objs.o.zero_grad()
            loss = objs.d.training_losses(objs.m, _rows(I, ids, rows), True, **(dict(index=ids) if index else {}))["loss"]
            loss.mean().backward()
            objs.o.step()
            assert loss.shape == (B,) and bool(torch.isfinite(loss).all())
            return loss.detach().clone()
        yield step
    return step_fn


def _state(objs, **more):
    """Everything a run leaves behind."""
    m, d, o = objs.m, objs.d, objs.o
    rec = dict(more)
    rec["params"] = {k: p.detach().clone() for k, p in m.named_parameters()}
    rec["moments"] = {k: (o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone(), int(o.state[p]["step"]))
                      for k, p in m.named_parameters() if o.state.get(p)}
    assert rec["moments"]
    rec["Lt_history"], rec["Lt_count"] = d.Lt_history.clone(), d.Lt_count.clone()
    rec["engine"] = (int(m.engine.seed), int(m.engine.offset))
    rec["counters"] = {name: int(getattr(d, name, 0)) for name in COUNTERS}
    return rec


def _same(a, b, where="run"):
    """a == b through dicts, sequences, tensors (torch.equal) and numbers; the path of the first difference otherwise."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for n, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{n}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, (where, a, b)


def _differs(a, b):
    try:
        _same(a, b)
    except AssertionError:
        return True
    return False


def set_attr(target, name, value=0):
    """A mutation for `bite`: after loading, objs.<target>.<name> = value (a counter back to 0, a seed to another value)."""
    def mutate(objs):
        obj = getattr(objs, target)
        obj = obj.engine if name in ("offset", "seed") and target == "m" else obj
        assert getattr(obj, name, value) != value, f"{name} is {value} in the checkpoint already: nothing to put back"
        setattr(obj, name, value)
    mutate.__name__ = name
    return mutate


def run(build, step_fn, n_before, n_after, tmp_path, *, eval_fn=None, reseed=None, bite=(), extra=None):
    """The reference run twice (equal to itself), the resumed run (equal to the reference), one more continuation per entry
    of `bite` (mutate(objs) after loading: must differ from the reference in a loss or an evaluation output; an entry
    (mutate, outputs) names the evaluation outputs that must each differ).  extra = (save(objs) -> what goes into the
    checkpoint's `extra`, load(objs, extra)): state the caller owns.  Returns the reference's record."""
    cuda_rng = torch.cuda.get_rng_state()
    cpu_rng, seed_was = torch.get_rng_state(), torch.initial_seed()
    try:
        def reference(path):
            torch.manual_seed(SEED)
            objs = build()
            with step_fn(objs, "before") as step:
                before = [step(k) for k in range(n_before)]
            eval_before = eval_fn(objs) if eval_fn is not None else None
            checkpoint.save_checkpoint(path, objs.m, objs.d, objs.o, epoch=n_before,
                                       extra=extra[0](objs) if extra is not None else None)
            saved = _state(objs)
            with step_fn(objs, "after") as step:
                losses = [step(k) for k in range(n_before, n_before + n_after)]
            evals = eval_fn(objs) if eval_fn is not None else None
            return _state(objs, losses=losses, evals=evals), dict(before=before, eval_before=eval_before, saved=saved)

        def resumed(path, mutate=None):
            objs = build()
            epoch, ext = checkpoint.load_checkpoint(path, objs.m, objs.d, objs.o)
            assert epoch == n_before
            if extra is not None:
                extra[1](objs, ext)
            if mutate is not None:
                mutate(objs)
            with step_fn(objs, "resumed") as step:
                losses = [step(k) for k in range(n_before, n_before + n_after)]
            evals = eval_fn(objs) if eval_fn is not None else None
            return _state(objs, losses=losses, evals=evals)

        ref, head = reference(tmp_path / "ck.pt")
        again, head_again = reference(tmp_path / "ck_again.pt")
        _same(head, head_again, "reference twice, up to the save")
        _same(ref, again, "reference twice")
        if reseed is not None:
            torch.manual_seed(reseed)
        _same(ref, resumed(tmp_path / "ck.pt"), "resumed")
        assert bite, "every case names the stream it is about"
        for entry in bite:
            mutate, outputs = entry if isinstance(entry, tuple) else (entry, None)
            got = resumed(tmp_path / "ck.pt", mutate)
            if outputs is None:
                assert _differs(ref["losses"], got["losses"]) or _differs(ref["evals"], got["evals"]), mutate.__name__
            for n in outputs or ():
                assert _differs(ref["evals"][n], got["evals"][n]), (mutate.__name__, n)
        return ref
    finally:
        torch.manual_seed(seed_was)
        torch.set_rng_state(cpu_rng)
        torch.cuda.set_rng_state(cuda_rng)


# ---- the training streams: engine.offset, _ts_calls, _randn_calls, the draw seed ----------------------------------------------
OFFSET, TS, RANDN = set_attr("m", "offset"), set_attr("d", "_ts_calls"), set_attr("d", "_randn_calls")
DRAW_SEED = set_attr("d", "_draw_seed", 12345)

CASES = {
    # 1: the eps target's normals (stream 4) are drawn through _randn_calls
    "dnn-eps": (build_dnn(EPS), eager_steps(515, 32), (RANDN,), None),
    # 2: CSR rows on the sparse route
    "dnn-x0-csr": (build_dnn(X0), eager_steps(515, 32, "csr"), (OFFSET, TS), None),
    # 3: the one-hot backbone: three engine positions and two timestep draws per step
    "onehot-x0-dense": (build_onehot(X0), eager_steps(257, 40), (OFFSET, TS), None),
    "onehot-x0-csr": (build_onehot(X0), eager_steps(257, 40, "csr"), (OFFSET, TS), None),
    # 4
    "onehot-eps": (build_onehot(EPS), eager_steps(257, 40), (RANDN,), None),
    # 5: the embedding backbone (default ntxent) from CSR rows and the users' ids
    "embedding-x0-csr": (build_embedding(), eager_steps(257, 40, "csr", index=True), (OFFSET, TS), None),
    # 6: the GCN backbone with every fusable weight updated inside the backward pass
    "gcn-x0-fused": (build_gcn(), eager_steps(257, 40, index=True), (OFFSET, TS), None),
    # 7: DNNCat, dense rows and (opt-in) CSR rows
    "cat-x0-dense": (build_cat(X0), eager_steps(515, 32), (OFFSET, TS), None),
    "cat-x0-csr": (build_cat(X0, csr_rows=True), eager_steps(515, 32, "csr"), (OFFSET, TS), None),
    # 8
    "cat-eps": (build_cat(EPS), eager_steps(515, 32), (RANDN,), None),
    # 9: the resuming process is seeded differently: the draws stay keyed on the seed the run was saved with
    "dnn-eps-reseeded": (build_dnn(EPS), eager_steps(515, 32), (DRAW_SEED,), 999),
    "onehot-x0-reseeded": (build_onehot(X0), eager_steps(257, 40), (DRAW_SEED,), 999),
}


@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_bit_exact(case, tmp_path):
    build, step_fn, bite, reseed = CASES[case]
    ref = run(build, step_fn, 2, 2, tmp_path, bite=bite, reseed=reseed)
    assert ref["counters"]["_ts_calls"] >= 4 and ref["engine"][1] >= 4 and int(ref["Lt_count"].sum()) > 0
    if RANDN in bite:
        assert ref["counters"]["_randn_calls"] == 4  # one draw of the target per step


# ---- the evaluation side ------------------------------------------------------------------------------------------------------
def test_resume_continues_the_sampling_noise_of_an_evaluation(tmp_path):
    """Case 10: p_sample(sampling_noise=True) between training steps draws the reverse loop's normals (stream 7) through
    _randn_calls; an evaluation after the resume must see the draws the uninterrupted run saw."""
    I, B = 515, 32
    x = _data(I).full[_data(I).order[6][:B]].to(DEV)

    def eval_fn(objs):
        objs.m.eval()
        out = objs.d.p_sample(objs.m, x, T // 2, sampling_noise=True).clone()
        objs.m.train()
        return [out]

    ref = run(build_dnn(X0), eager_steps(I, B), 2, 2, tmp_path, eval_fn=eval_fn, bite=(RANDN,))
    assert ref["counters"]["_randn_calls"] == 2 * (T - 1)  # every reverse step but the last one draws


def test_resume_continues_the_discrete_draws_of_an_evaluation(tmp_path):
    """Case 11: the embedding backbone's reverse loop advances the degree-guided graph at every step (offset base 2^42 +
    _noise_calls), apply_noise by name draws at 2^41 + _noise_calls, q_sample (by name, and x_T inside p_sample) at 2^40 +
    _q_calls.  Putting _noise_calls back must change both the graph and apply_noise's classes; _q_calls both q_sample's rows and
    the loop's result."""
    I, B = 257, 40
    ids = _data(I).order[6][:B]
    x = _data(I).full[ids].to(DEV)
    onehot = torch.nn.functional.one_hot(x.long(), num_classes=2).float()
    ts = (torch.arange(B) % T).to(DEV)

    def eval_fn(objs):
        objs.m.eval()
        out = objs.d.p_sample(objs.m, x, T, index=ids).clone()
        graph = objs.d.last_graph.clone()
        classes = objs.d.apply_noise(ts, onehot)
        noised = objs.d.q_sample(x, ts).clone()
        objs.m.train()
        assert 0 < int(graph.sum()) < graph.numel()
        return [out, graph, classes, noised]

    ref = run(build_embedding(I), eager_steps(I, B, index=True), 2, 2, tmp_path, eval_fn=eval_fn,
              bite=((set_attr("d", "_noise_calls"), (1, 2)), (set_attr("d", "_q_calls"), (0, 3))))
    assert ref["counters"]["_noise_calls"] == 2 * (T + 1) and ref["counters"]["_q_calls"] == 4


# ---- the graphed step ---------------------------------------------------------------------------------------------------------
def graphed_steps(I, B, graph_phases):
    """step_fn over row ids of the resident CSR matrix: in `graph_phases` the steps run through a graph.GraphedTrainStep that is
    closed when the phase ends (the save comes after close()), elsewhere through the eager DataParallelStep the graph captures.
    A step returns the batch's mean loss."""
    from gdmcf_amd.graph import GraphedTrainStep
    from gdmcf_amd.parallel import DataParallelStep
    dcsr, order = _data(I).dcsr, _data(I).order

    @contextlib.contextmanager
    def step_fn(objs, phase):
        if phase in graph_phases:
            # before the save: three eager calls, the capture, one replay; resumed: one eager call, then the capture
            with GraphedTrainStep(objs.d, objs.m, objs.o, dcsr, B, warmup=3 if phase == "before" else 1) as gstep:
                yield lambda k: gstep(order[k][:B]).clone()
                assert isinstance(gstep.graph, torch.cuda.CUDAGraph), gstep.capture_error
        else:
            eager = DataParallelStep(objs.d, objs.m, objs.o)
            yield lambda k: eager(dcsr.batch(order[k][:B]), True).clone()
    return step_fn


def test_resume_after_a_graphed_step_was_closed(tmp_path):
    """Case 12: five calls of a GraphedTrainStep (warmup=3), close(), save, two eager steps.  The counters close() hands back are
    what the checkpoint carries: the run equals seven eager steps, and fresh objects that load the file and open a new
    GraphedTrainStep (one eager call, then capture and replay) continue it bit for bit."""
    I, B = 515, 32
    build = build_dnn(X0, scale=0.1)
    ref = run(build, graphed_steps(I, B, ("before", "resumed")), 5, 2, tmp_path, bite=(OFFSET, TS))
    eager = run(build, graphed_steps(I, B, ()), 5, 2, tmp_path, bite=(OFFSET, TS))
    _same(ref, eager, "graphed vs eager")
    assert ref["engine"][1] == 7 and ref["counters"]["_ts_calls"] == 7
    assert {step for _, _, step in ref["moments"].values()} == {7}


# ---- the whole loop -----------------------------------------------------------------------------------------------------------
def test_resume_of_the_driver_loop_with_the_loaders_generator_in_extra(tmp_path):
    """Case 13: driver.train_one_epoch(shuffle=True, generator=g, sparse=True), one epoch, save with the generator's state in
    `extra`, a second epoch.  The shuffling generator is the caller's: restored from `extra` the second epoch is the same epoch
    (loss sum and every parameter); started over it is another one."""
    from gdmcf_amd import driver
    I, B = 515, 32
    dcsr = _data(I).dcsr

    def build():
        objs = build_dnn(X0)()
        objs.g = torch.Generator().manual_seed(9)
        return objs

    @contextlib.contextmanager
    def epochs(objs, phase):
        def epoch(k):
            total, count = driver.train_one_epoch(objs.d, objs.m, objs.o, dcsr, B, DEV, shuffle=True, generator=objs.g, sparse=True)
            assert count == U // B
            return total
        yield epoch

    def start_over(objs):
        objs.g.manual_seed(9)

    ref = run(build, epochs, 1, 1, tmp_path, bite=(start_over,),
              extra=(lambda objs: {"loader": objs.g.get_state()}, lambda objs, extra: objs.g.set_state(extra["loader"])))
    assert ref["engine"][1] == 2 * (U // B)
