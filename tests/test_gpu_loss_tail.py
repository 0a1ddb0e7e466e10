"""GPU (-m gpu): the float64 loss tail of csrc/loss_tail.hip (gdmcf_row_loss_finish_f64 / _mean_f64) through the C ABI, bit for bit
against tests/glue_ref.py: row_loss restates the kernel's multiplications and divisions one by one, kernel_mean its summation order
(256 strided partial sums, a butterfly per wave, the four waves in order), and the Lt-history FIFO is the oracle's serial loop.
Batches below, at and above the 256 threads (where the loops stride), the small and the production history (88 KB of LDS, which the
mean's partial sums share with the FIFO update), every optional pointer present and absent, update_history 0 and 1."""
import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from oracle import gdmcf_oracle as O
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH_IDS = [f"T{t}-H{h}" for t, h in R.LOSS_TH]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _history(T, H, seed):
    rng = np.random.default_rng([seed, T, H])
    return rng.random((T, H)), rng.integers(0, H + 1, T).astype(np.int64)  # every slot holds something, live or not


def _finish(case, T, H, hist, cnt, update, alpha=True, gradcoef=True, rowscale_mean=True, loss_mean=True, plain=False):
    """One launch; returns {name: numpy result} of the outputs that were asked for (each behind its canaries)."""
    lib = _lib.load()
    rowsum, rowdiv, al, ts, weight, pt = case
    B = len(rowsum)
    ins = [_dev(x) for x in (rowsum, rowdiv, al, ts, weight, pt)]
    outs = dict(lu=R.seat(1, B, B, DEV, dtype=torch.float64), loss=R.seat(1, B, B, DEV, dtype=torch.float64),
                gradcoef=R.seat(1, B, B, DEV), rowscale_mean=R.seat(1, B, B, DEV),
                loss_mean=R.seat(1, 1, 1, DEV, dtype=torch.float64))
    asked = dict(lu=True, loss=True, gradcoef=gradcoef, rowscale_mean=rowscale_mean and not plain, loss_mean=loss_mean and not plain)

    def p(name):
        return outs[name][1].data_ptr() if asked[name] else None

    args = [ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr() if alpha else None, ins[3].data_ptr(), ins[4].data_ptr(),
            ins[5].data_ptr(), B, T, H, hist.data_ptr(), cnt.data_ptr(), update, p("lu"), p("loss"), p("gradcoef")]
    if plain:
        _lib.check(lib.gdmcf_row_loss_finish_f64(*args, _lib.stream_ptr()))
    else:
        _lib.check(lib.gdmcf_row_loss_finish_mean_f64(*args, p("loss_mean"), p("rowscale_mean"), _lib.stream_ptr()))
    torch.cuda.synchronize()
    res = {}
    for name, (buf, view) in outs.items():
        n = view.shape[1]
        assert R.canary_intact(buf, 1, n, n), name
        if asked[name]:
            res[name] = view.cpu().numpy()[0]
        else:
            assert bool(torch.isnan(view).all()), name  # an output that was not asked for is not written
    return res


def _assert_rows(res, case, alpha):
    rowsum, rowdiv, al, ts, weight, pt = case
    lu, loss, gc, rsm = R.row_loss(rowsum, rowdiv, al if alpha else None, ts, weight, pt)
    assert np.array_equal(res["lu"], lu) and np.array_equal(res["loss"], loss)
    if "gradcoef" in res:
        assert res["gradcoef"].dtype == np.float32 and np.array_equal(res["gradcoef"], gc)
    if "rowscale_mean" in res:
        assert np.array_equal(res["rowscale_mean"], rsm)
    if "loss_mean" in res:
        assert res["loss_mean"][0] == R.kernel_mean(loss), (res["loss_mean"][0], R.kernel_mean(loss), R.kernel_mean(loss, "pairs"))
    return lu


@pytest.mark.parametrize("T,H", R.LOSS_TH, ids=TH_IDS)
@pytest.mark.parametrize("B", R.LOSS_B)
def test_optional_outputs_without_history_update(B, T, H):
    """update_history = 0 with alpha / gradcoef / rowscale_mean / loss_mean present and absent: every row and the mean bit for bit,
    Lt_history and Lt_count unchanged bit for bit; gdmcf_row_loss_finish_f64 gives the same rows as the _mean entry."""
    case = R.loss_case(B, T, seed=B)
    hist0, cnt0 = _history(T, H, B)
    hbuf, hist = R.seat(T, H, H, DEV, hist0, dtype=torch.float64)
    cbuf, cnt = R.seat(1, T, T, DEV, cnt0, dtype=torch.int64)
    for opts in (dict(), dict(alpha=False, rowscale_mean=False), dict(gradcoef=False, rowscale_mean=False, loss_mean=False),
                 dict(alpha=False, loss_mean=False), dict(plain=True), dict(plain=True, alpha=False, gradcoef=False)):
        res = _finish(case, T, H, hist, cnt, 0, **opts)
        _assert_rows(res, case, opts.get("alpha", True))
        assert np.array_equal(hist.cpu().numpy(), hist0) and np.array_equal(cnt.cpu().numpy()[0], cnt0), opts
        assert R.canary_intact(hbuf, T, H, H) and R.canary_intact(cbuf, 1, T, T)


@pytest.mark.parametrize("T,H", R.LOSS_TH, ids=TH_IDS)
@pytest.mark.parametrize("B", R.LOSS_B)
def test_history_update_with_the_mean(B, T, H):
    """update_history = 1 with loss_mean given (the partial sums and the FIFO update share the LDS): three launches on one history,
    the second with every row on one timestep (deep overflow); rows and mean bit for bit, Lt_history and Lt_count equal to the
    oracle's serial row-by-row update of the reference's loss_unscaled, slots that are not live included."""
    od = O.GaussianDiffusion(O.ModelMeanType.START_X, "linear", 0.1, 0.001, 0.01, T, history_num_per_term=H)
    hist0, cnt0 = _history(T, H, B + 1)
    od.Lt_history.copy_(torch.from_numpy(hist0))
    od.Lt_count.copy_(torch.from_numpy(cnt0))
    hbuf, hist = R.seat(T, H, H, DEV, hist0, dtype=torch.float64)
    cbuf, cnt = R.seat(1, T, T, DEV, cnt0, dtype=torch.int64)
    for rnd in range(3):
        case = R.loss_case(B, T, seed=100 * rnd + B, same_ts=rnd == 1)
        opts = (dict(), dict(alpha=False, rowscale_mean=False), dict(gradcoef=False, rowscale_mean=False))[rnd]
        res = _finish(case, T, H, hist, cnt, 1, **opts)
        lu = _assert_rows(res, case, opts.get("alpha", True))
        od.update_history(torch.from_numpy(case[3]), torch.from_numpy(lu))
        assert np.array_equal(cnt.cpu().numpy()[0], od.Lt_count.numpy()), rnd
        assert np.array_equal(hist.cpu().numpy(), od.Lt_history.numpy()), rnd
        assert R.canary_intact(hbuf, T, H, H) and R.canary_intact(cbuf, 1, T, T)
    assert not np.array_equal(od.Lt_history.numpy(), hist0)


def test_history_update_without_the_mean():
    """update_history = 1 through gdmcf_row_loss_finish_f64 (no loss_mean: the LDS is the FIFO update's alone)."""
    B, (T, H) = 400, R.LOSS_TH[0]
    od = O.GaussianDiffusion(O.ModelMeanType.START_X, "linear", 0.1, 0.001, 0.01, T, history_num_per_term=H)
    hbuf, hist = R.seat(T, H, H, DEV, od.Lt_history.numpy(), dtype=torch.float64)
    cbuf, cnt = R.seat(1, T, T, DEV, od.Lt_count.numpy(), dtype=torch.int64)
    case = R.loss_case(B, T, seed=9)
    lu = _assert_rows(_finish(case, T, H, hist, cnt, 1, plain=True), case, True)
    od.update_history(torch.from_numpy(case[3]), torch.from_numpy(lu))
    assert np.array_equal(cnt.cpu().numpy()[0], od.Lt_count.numpy()) and np.array_equal(hist.cpu().numpy(), od.Lt_history.numpy())
    assert R.canary_intact(hbuf, T, H, H) and R.canary_intact(cbuf, 1, T, T)
