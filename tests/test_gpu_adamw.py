"""GPU (-m gpu): the fused multi-tensor AdamW of csrc/adamw.hip through the C ABI, against torch.optim.AdamW's element update in
float64 (tests/glue_ref.py: adam64) inside bounds derived there -- tensors shorter and longer than one 4096-element block, the last
1-3 elements, the hand-over between the tensors of a table with empty tensors in it, the scalar path of pointers that are not
16-byte aligned, and the bf16 shadow stores where a group of four crosses shadow rows.  Two bit-equalities between library results
are asserted because csrc/common.h promises them: unaligned == aligned, and adamw_bf16s == adamw.  The measured size of the step
term's error stands in the docstrings of test_single_tensor and test_step_term_from_a_zero_parameter."""
import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER_IDS = [f"step{h['step']}-lr{h['lr']}" for h in R.ADAM_HYPERS]


def _seat_state(numel, seed, offset):
    """[(buf, view)] x 4 for p, g, m, v of adam_state(numel, seed), each `offset` floats into a buffer of its own (offset 0:
    16-byte aligned, as the allocator hands it out; 1: four bytes past)."""
    state = R.adam_state(numel, seed)
    seated = [R.seat(1, numel, numel, DEV, x, offset=offset) for x in state]
    assert all((v.data_ptr() & 15) == 4 * offset for _, v in seated)
    return state, seated


def _launch(lib, rows, total_blocks, hyper, shadow_table=None):
    """rows: [(p, g, m, v pointers or 0, numel, first_block)]."""
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 6).to(DEV)
    h = hyper
    args = (len(rows), total_blocks, h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"], h["grad_scale"],
            _lib.stream_ptr())
    if shadow_table is None:
        _lib.check(lib.gdmcf_adamw_f32(table.data_ptr(), *args))
    else:
        _lib.check(lib.gdmcf_adamw_bf16s_f32(table.data_ptr(), shadow_table.data_ptr(), *args))
    torch.cuda.synchronize()


def _check_against_float64(state, seated, hyper, what):
    """p, m, v inside their bounds, g and every canary untouched.  Returns the share of the step term in p's error."""
    p0, g0, m0, v0 = state
    numel = len(p0)
    p64, m64, v64, term, _ = R.adam64(p0, g0, m0, v0, **hyper)
    bp, bm, bv = R.adam_bounds(p0, g0, m0, v0, **hyper)
    got = [v.cpu().double().numpy()[0] for _, v in seated]
    err_p = np.abs(got[0] - p64)
    print(f"adamw {what}: p {float((err_p / bp).max()):.3f}, m {float((np.abs(got[2] - m64) / bm).max()):.3f}, "
          f"v {float((np.abs(got[3] - v64) / bv).max()):.3f} of the bound; "
          f"p against 2u|p| + c|term| alone: {float((err_p / R.adam_bound_p_as_first_stated(p0, g0, m0, v0, **hyper)).max()):.3f}")
    assert (err_p <= bp).all(), what
    assert (np.abs(got[2] - m64) <= bm).all(), what
    assert (np.abs(got[3] - v64) <= bv).all(), what
    assert np.array_equal(seated[1][1].cpu().numpy()[0], g0), what
    for buf, view in seated:
        offset = (view.data_ptr() - buf.data_ptr()) // 4
        assert R.canary_intact(buf, 1, numel, numel, offset=offset), what
    rest = bp - R.ADAM_C * np.abs(term)
    return float(((err_p - rest) / np.abs(term)).max())  # (negative: the other terms already cover the error)


@pytest.mark.parametrize("hyper", R.ADAM_HYPERS, ids=HYPER_IDS)
@pytest.mark.parametrize("numel", R.ADAM_NUMELS)
def test_single_tensor(numel, hyper):
    """One tensor per launch, 16-byte aligned (vector path, scalar tail of 1-3 elements) and four bytes past (scalar path all the
    way): each inside the float64 bounds, the two bit-identical.

    Measured on an MI355X, largest (|p - p64| - everything but the step term's share of the bound) / |step term| over the 24
    cases: 5.9e-8, at 12 293 elements and step 100000 (the bound allows ADAM_C = 1e-6; csrc/common.h documents ~3e-7).  The largest
    error was 0.95 of the bound; against 2u |p| + ADAM_C |step term| alone it was 1.06 (12 293 elements, step 3) -- the two terms
    glue_ref.adam_bounds adds are needed on the device as they are for float32 arithmetic on the host."""
    lib = _lib.load()
    blocks = -(-numel // R.ADAM_BLOCK)
    results = []
    for offset in (0, 1):
        state, seated = _seat_state(numel, 1, offset)
        _launch(lib, [[v.data_ptr() for _, v in seated] + [numel, 0]], blocks, hyper)
        share = _check_against_float64(state, seated, hyper, f"numel {numel} offset {offset}")
        print(f"adamw step-term share numel {numel} step {hyper['step']} offset {offset}: {share:.3e}")
        results.append([v.cpu() for _, v in seated])
    for a, b in zip(*results):
        assert torch.equal(a, b)  # the element function's rounding does not depend on the path


@pytest.mark.parametrize("hyper", R.ADAM_HYPERS, ids=HYPER_IDS)
def test_step_term_from_a_zero_parameter(hyper):
    """p = 0 and exp_avg = 0 before the step (the state of a first step): the result is minus the step term and m = (1 - beta1) g
    cannot cancel, so |p - p64| / |step term| is the step's own relative error -- hardware reciprocal and square root, the float32
    scalars, the roundings of m and v -- with no rounding of a parameter beside it.

    Measured on an MI355X over 12 293 elements, step 3 / 1 / 100000: largest 2.76e-7 / 3.03e-7 / 3.12e-7 (99.9th percentile
    2.1e-7 / 2.5e-7 / 2.7e-7) -- the ~3e-7 of csrc/common.h, just above it in two of the three, a third of ADAM_C."""
    lib = _lib.load()
    numel = 12293
    p, g, m, v = R.adam_state(numel, 5)
    state = (np.zeros_like(p), g, np.zeros_like(m), v)
    seated = [R.seat(1, numel, numel, DEV, x) for x in state]
    _launch(lib, [[t.data_ptr() for _, t in seated] + [numel, 0]], -(-numel // R.ADAM_BLOCK), hyper)
    _check_against_float64(state, seated, hyper, "zero parameter")
    p64, _, _, term, _ = R.adam64(*state, **hyper)
    rel = np.abs(seated[0][1].cpu().double().numpy()[0] - p64) / np.abs(term)
    print(f"adamw step term alone, step {hyper['step']}: max {rel.max():.3e}, 99.9th percentile {np.quantile(rel, 0.999):.3e}")


@pytest.mark.parametrize("hyper", R.ADAM_HYPERS, ids=HYPER_IDS)
def test_table_with_empty_tensors(hyper):
    """Every size in one table with an empty tensor (pointers 0, numel 0) first, in the middle and last: the block search of
    adamw_kernel takes the LAST tensor whose first_block is not above the block index, so an empty tensor -- which shares its
    first_block with its successor, or with the grid's end -- is never picked.  Each tensor inside the float64 bounds; two runs from
    the same state bit-identical."""
    lib = _lib.load()
    numels = (0,) + R.ADAM_NUMELS[:4] + (0,) + R.ADAM_NUMELS[4:] + (0,)
    first, total = R.adam_table(numels)
    assert total == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 4 and first[-1] == total and first[0] == first[1] == 0
    runs = []
    for _ in range(2):
        tensors, rows = [], []
        for k, (n, fb) in enumerate(zip(numels, first)):
            if n == 0:
                rows.append([0, 0, 0, 0, 0, fb])
                continue
            state, seated = _seat_state(n, 2 + k, 0)
            tensors.append((state, seated))
            rows.append([v.data_ptr() for _, v in seated] + [n, fb])
        _launch(lib, rows, total, hyper)
        for state, seated in tensors:
            _check_against_float64(state, seated, hyper, f"table, numel {len(state[0])}")
        runs.append([v.cpu() for _, seated in tensors for _, v in seated])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


SHADOWED = ((5, 1), (7, 3), (9, 37), (64, 64), (33, 130))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
def test_bf16_shadows(offset):
    """gdmcf_adamw_bf16s_f32 on five 2-D parameters and a 1-D tensor without a shadow (entry (0, 1, 0)): the float32 results equal
    gdmcf_adamw_f32's from the same state bit for bit, the shadow holds the updated parameter rounded to nearest even over
    [rows, cols) and is still zero everywhere else.  cols = 1 and 3 put several shadow rows into one group of four, cols = 37 and 130
    put the 8-byte store on 2-byte aligned addresses and groups across a row end; the unaligned run takes the scalar path.  The
    shadow table is built by hand from the layout of include/gdmcf_hip.h: nothing is registered."""
    lib = _lib.load()
    hyper = R.ADAM_HYPERS[0]
    shapes = SHADOWED + ((1000, None),)
    numels = [r * (c or 1) for r, c in shapes]
    first, total = R.adam_table(numels)

    def run(with_shadows):
        tensors, rows, srows, shadows = [], [], [], []
        for k, ((r, c), n, fb) in enumerate(zip(shapes, numels, first)):
            state, seated = _seat_state(n, 20 + k, offset)
            tensors.append((state, seated))
            rows.append([v.data_ptr() for _, v in seated] + [n, fb])
            if c is None:
                srows.append([0, 1, 0])
                continue
            sh = torch.zeros((r + 63) // 64 * 64, (c + 63) // 64 * 64, dtype=torch.bfloat16, device=DEV)
            shadows.append(sh)
            srows.append([sh.data_ptr(), c, sh.stride(0)])
        stab = torch.tensor(srows, dtype=torch.int64).to(DEV) if with_shadows else None
        _launch(lib, rows, total, hyper, shadow_table=stab)
        return tensors, shadows

    plain, _ = run(False)
    tensors, shadows = run(True)
    for (state, seated), (_, seated_plain) in zip(tensors, plain):
        _check_against_float64(state, seated, hyper, f"bf16s, numel {len(state[0])}")
        assert all(torch.equal(a.cpu(), b.cpu()) for (_, a), (_, b) in zip(seated, seated_plain))
    for (r, c), (_, seated), sh in zip(SHADOWED, tensors, shadows):
        p = seated[0][1].cpu().reshape(r, c)
        want = torch.zeros(sh.shape, dtype=torch.bfloat16)
        want[:r, :c] = p.to(torch.bfloat16)  # round to nearest even
        assert torch.equal(sh.cpu().view(torch.int16), want.view(torch.int16)), (r, c)
