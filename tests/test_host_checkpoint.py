"""CPU: what checkpoint.diffusion_state / load_diffusion_state carry -- every draw counter of gaussian_diffusion.py and the
seed its draws are keyed on -- on a stand-in object (no GPU, no kernels), the format from before the counters were complete,
and a tripwire for a counter added later and forgotten in the checkpoint."""
import inspect
import re
from types import SimpleNamespace

import torch

from gdmcf_amd import checkpoint, gaussian_diffusion

# attribute of the diffusion object -> key of the saved state.  A new `self._*_calls` counter needs a line here AND in
# checkpoint.py (test_every_draw_counter_of_the_diffusion_is_saved).
SAVED_AS = {"_ts_calls": "ts_calls", "_q_calls": "q_calls", "_randn_calls": "randn_calls", "_noise_calls": "noise_calls"}


def _stand_in(**attrs):
    """The attributes the two functions read and write, nothing else."""
    obj = SimpleNamespace(Lt_history=torch.zeros(3, 2, dtype=torch.float64), Lt_count=torch.zeros(3, dtype=torch.int64),
                          _draw_seed=None, **attrs)
    obj.draw_seed = lambda: obj._draw_seed if obj._draw_seed is not None else 7
    return obj


def test_round_trip_carries_every_counter_and_the_seed():
    src = _stand_in(_ts_calls=11, _q_calls=12, _randn_calls=13, _noise_calls=14)
    src.Lt_history.copy_(torch.arange(6, dtype=torch.float64).reshape(3, 2) + 0.5)
    src.Lt_count.copy_(torch.tensor([2, 1, 2]))
    src._draw_seed = (1 << 62) + 5
    state = checkpoint.diffusion_state(src)
    assert all(not isinstance(v, torch.Tensor) or v.device.type == "cpu" for v in state.values())
    src.Lt_history.zero_()  # (the state holds copies)
    dst = _stand_in()
    checkpoint.load_diffusion_state(dst, state)
    assert torch.equal(dst.Lt_history, torch.arange(6, dtype=torch.float64).reshape(3, 2) + 0.5) and dst.Lt_history.dtype == torch.float64
    assert torch.equal(dst.Lt_count, torch.tensor([2, 1, 2])) and dst.Lt_count.dtype == torch.int64
    assert (dst._ts_calls, dst._q_calls, dst._randn_calls, dst._noise_calls) == (11, 12, 13, 14)
    assert dst._draw_seed == (1 << 62) + 5 and dst.draw_seed() == (1 << 62) + 5
    # an object that never loaded anything saves the seed its draws use now, and counters it never touched as 0
    fresh = checkpoint.diffusion_state(_stand_in())
    assert fresh["seed"] == 7 and all(fresh[key] == 0 for key in SAVED_AS.values())


def test_state_from_before_the_counters_were_complete_still_loads():
    old = {"Lt_history": torch.full((3, 2), 0.25, dtype=torch.float64), "Lt_count": torch.tensor([1, 0, 2]),
           "ts_calls": 5, "q_calls": 3}
    dst = _stand_in(_ts_calls=90, _q_calls=91, _randn_calls=92, _noise_calls=93)
    dst._draw_seed = 1234  # (as left by an earlier load)
    checkpoint.load_diffusion_state(dst, old)
    assert (dst._ts_calls, dst._q_calls) == (5, 3)
    assert (dst._randn_calls, dst._noise_calls) == (0, 0)
    assert dst._draw_seed is None and dst.draw_seed() == 7
    assert torch.equal(dst.Lt_history, old["Lt_history"]) and torch.equal(dst.Lt_count, old["Lt_count"])


def test_draw_seed_is_torchs_seed_until_a_checkpoint_sets_one():
    d = gaussian_diffusion.GaussianDiffusion(gaussian_diffusion.ModelMeanType.START_X, "linear-var", 0.0, 0.001, 0.01, 5, "cpu")
    was = torch.initial_seed()
    try:
        torch.manual_seed(21)
        assert d._draw_seed is None and d.draw_seed() == 21
        torch.manual_seed((1 << 63) + 9)  # masked to 63 bits, as the draws always were
        assert d.draw_seed() == 9
        state = checkpoint.diffusion_state(d)
        assert state["seed"] == 9
        torch.manual_seed(22)
        checkpoint.load_diffusion_state(d, state)
        assert d.draw_seed() == 9
    finally:
        torch.manual_seed(was)


def test_every_draw_counter_of_the_diffusion_is_saved():
    source = inspect.getsource(gaussian_diffusion)
    assigned = set(re.findall(r"self\.(_\w+_calls)\s*=(?!=)", source))
    assert assigned, "the pattern no longer finds the counters"
    assert assigned == set(SAVED_AS), "a draw counter of gaussian_diffusion.py that SAVED_AS (and checkpoint.py) does not know"
    values = {name: 100 + n for n, name in enumerate(sorted(assigned))}
    state = checkpoint.diffusion_state(_stand_in(**values))
    for name, key in SAVED_AS.items():
        assert state.get(key) == values[name], name
    dst = _stand_in()
    checkpoint.load_diffusion_state(dst, state)
    assert {name: getattr(dst, name) for name in assigned} == values
