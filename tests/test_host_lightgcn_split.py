"""CPU (-m "not gpu"): gdmcf_amd.lightgcn after its split by concern -- every name that could be imported from it is still there
and is the object of its home module; spmm_schedule.pick_generation chooses the SpMM kernel generation by the rule
LightGCN.get_A_tilda applied inline."""
import importlib

import pytest

from gdmcf_amd import lightgcn
from gdmcf_amd.spmm_schedule import SPMM_SLICE_MB, pick_generation

# dir(gdmcf_amd.lightgcn) before the split, without dunder names and imported modules, and where each name lives now
HOME = {
    "lightgcn": ["LightGCN", "_PropagateMean", "normalized_bipartite_csr"],
    "spmm_schedule": ["SPMM_CHUNK", "SPMM_COST_PIECE", "SPMM_COST_ROW", "SPMM_HOT_MB", "SPMM_MISS_W", "SPMM_NT", "SPMM_PIECE",
                      "SPMM_SHORT", "SPMM_SLICE_MB", "SPMM_SMAX", "SPMM_WAVES", "spmm_bundle_plan", "spmm_plan", "spmm_stream_pack"],
    "lightgcn_eval": ["_check_Ks", "_history_rows", "get_metrics", "get_metrics_at", "hits_from_ranks", "ranking_terms"],
    "bpr": ["BPRTrainer", "_bpr_grad", "_bpr_loss", "_bpr_operands", "_bpr_order", "_bpr_sample", "bpr_loss", "bpr_loss_grad",
            "bpr_reg_grad_", "sample_bpr_batch", "sample_bpr_items"],
}


def test_lightgcn_still_exposes_every_name_from_its_home_module():
    assert sum(len(v) for v in HOME.values()) == 34
    for module, names in HOME.items():
        home = importlib.import_module("gdmcf_amd." + module)
        for name in names:
            assert hasattr(lightgcn, name), name
            assert getattr(lightgcn, name) is getattr(home, name), (module, name)
            if callable(getattr(home, name)):
                assert getattr(home, name).__module__ == "gdmcf_amd." + module, (module, name)


N_FIT = int(SPMM_SLICE_MB * 1e6 // (64 * 4 / 8))  # the most nodes whose eighth of a 64-wide float32 table fits the slice


@pytest.mark.parametrize("n_nodes,d,nnz,env,want", [
    (1000, 20, 5000, "auto", "1"),        # 5 lanes per row: no power-of-two lane groups
    (1000, 7, 5000, "auto", "1"),         # not even whole 16-byte slices
    (N_FIT, 64, 5000, "auto", "3"),       # N * d * 4 / 8 <= SPMM_SLICE_MB * 1e6
    (N_FIT + 1, 64, 5000, "auto", "1"),   # just above it
    (1000, 64, 0, "auto", "1"),           # nothing to schedule
    (1000, 64, 0, "3", "1"),
    (1000, 64, 5000, "2", "2"),           # forced, fitting width
    (N_FIT + 1, 64, 5000, "3", "3"),
    (1000, 64, 5000, "1", "1"),
    (1000, 20, 5000, "3", "1"),           # forced, but the width does not fit
    (1000, 20, 5000, "2", "1"),
])
def test_pick_generation(n_nodes, d, nnz, env, want):
    assert N_FIT * 64 * 4 / 8 <= SPMM_SLICE_MB * 1e6 < (N_FIT + 1) * 64 * 4 / 8
    assert pick_generation(n_nodes, d, nnz, env) == want
