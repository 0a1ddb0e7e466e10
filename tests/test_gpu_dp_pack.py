"""GPU (-m gpu): the data-parallel exchange helpers of csrc/dp_exchange.hip (gdmcf_dp_pack_f64 / gdmcf_dp_unpack_f64) through the C
ABI.  Every rank of a world packs into a NaN-filled buffer, which must then hold exactly: the small gradients as doubles in table
order, zeros in the other ranks' (ts, loss) slices, the rank's own pairs interleaved.  The ranks' buffers are summed (what the
all-reduce does) and unpacked: the gradients are the float32 of the sums -- small integers, so every sum is exact -- and ts_all /
loss_unscaled_all come out in rank order.  Tables: none, sixteen entries with empty ones (one of them a NULL pointer), and one
gradient longer than the 1024 x 256 threads of the grid."""
import ctypes

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLES = {
    "none": ((), 7),
    "sixteen": ((1, 0, 5, 256, 0, 3, 1000, 7, 2, 0, 64, 1, 9, 31, 4, 255), 5),
    "grid-stride": ((300000,), 33),
}
NULL_ENTRY = 1  # of "sixteen": count 0 and no pointer at all (entries 4 and 9 have count 0 and a pointer)


def _table(seated, counts, name):
    """Host arrays (pointers, counts) of a gradient table, as the entries take them."""
    ptrs = [None if (name == "sixteen" and k == NULL_ENTRY) else v.data_ptr() for k, (_, v) in enumerate(seated)]
    return (ctypes.c_void_p * max(len(counts), 1))(*ptrs), (ctypes.c_int64 * max(len(counts), 1))(*counts)


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name", list(TABLES))
def test_pack_sum_unpack(name, world):
    lib = _lib.load()
    counts, B = TABLES[name]
    n, n_small = len(counts), sum(counts)
    assert n <= 16 and (name != "grid-stride" or n_small + 2 * world * B > 1024 * 256)
    total = n_small + 2 * world * B
    rng = np.random.default_rng([len(name), world])
    flats, all_grads, all_ts, all_lu = [], [], [], []
    for rank in range(world):
        grads = [rng.integers(-8, 9, max(c, 1)).astype(np.float32) for c in counts]  # (an empty entry still gets a buffer)
        ts = rng.integers(0, 1000, B).astype(np.int64)
        lu = rng.random(B)
        seated = [R.seat(1, len(g), len(g), DEV, g) for g in grads]
        gp, gc = _table(seated, counts, name)
        d_ts, d_lu = torch.from_numpy(ts).to(DEV), torch.from_numpy(lu).to(DEV)
        fbuf, flat = R.seat(1, total, total, DEV, dtype=torch.float64)
        _lib.check(lib.gdmcf_dp_pack_f64(ctypes.addressof(gp) if n else None, ctypes.addressof(gc) if n else None, n,
                                         d_ts.data_ptr(), d_lu.data_ptr(), B, rank, world, flat.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        pairs = np.zeros((world, B, 2))
        pairs[rank, :, 0], pairs[rank, :, 1] = ts, lu
        want = np.concatenate([g[:c].astype(np.float64) for g, c in zip(grads, counts)] + [pairs.ravel()])
        assert np.array_equal(flat.cpu().numpy()[0], want), rank
        assert R.canary_intact(fbuf, 1, total, total)
        assert all(np.array_equal(v.cpu().numpy()[0], g) for (_, v), g in zip(seated, grads))  # the inputs are as before
        flats.append(flat)
        all_grads.append(grads)
        all_ts.append(ts)
        all_lu.append(lu)
    summed = flats[0].clone()
    for f in flats[1:]:
        summed += f
    summed = summed.contiguous()
    # unpack: every gradient buffer starts as NaN where it is to be written, a canary elsewhere
    outs = [R.seat(1, max(c, 1), max(c, 1), DEV) for c in counts]
    for (buf, v), c in zip(outs, counts):
        if c == 0:
            v.fill_(R.CANARY)
    gp, gc = _table(outs, counts, name)
    tbuf, ts_all = R.seat(1, world * B, world * B, DEV, dtype=torch.int64)
    lbuf, lu_all = R.seat(1, world * B, world * B, DEV, dtype=torch.float64)
    _lib.check(lib.gdmcf_dp_unpack_f64(summed.data_ptr(), ctypes.addressof(gp) if n else None, ctypes.addressof(gc) if n else None,
                                       n, B, world, ts_all.data_ptr(), lu_all.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, ((buf, v), c) in enumerate(zip(outs, counts)):
        want = np.sum([all_grads[r][k][:c].astype(np.float64) for r in range(world)], axis=0).astype(np.float32)
        assert c == 0 or np.array_equal(v.cpu().numpy()[0], want), k
        assert R.canary_intact(buf, 1, c, max(c, 1)) if c else bool((buf == R.CANARY).all()), k
    assert np.array_equal(ts_all.cpu().numpy()[0], np.concatenate(all_ts))
    assert np.array_equal(lu_all.cpu().numpy()[0], np.concatenate(all_lu))
    assert R.canary_intact(tbuf, 1, world * B, world * B) and R.canary_intact(lbuf, 1, world * B, world * B)
