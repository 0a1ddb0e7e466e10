"""gdmcf_amd -- MI355X-native (gfx950) hot path of GDMCF: the per-batch forward/reverse Gaussian
diffusion path behind the reference's own Python API.  See DESIGN.md / include/gdmcf_hip.h."""
from . import _lib  # noqa: F401
from .DNN import DNN, timestep_embedding  # noqa: F401
from .gaussian_diffusion import GaussianDiffusion, GaussianDiffusionDiscrete, ModelMeanType  # noqa: F401
from .optim import FusedAdamW  # noqa: F401
from .evaluate_utils import computeTopNAccuracy, computeTopNAccuracy_device, masked_topk, print_results, score_rank, score_topk  # noqa: F401
from .bpr import BPRTrainer  # noqa: F401
from .lightgcn import LightGCN  # noqa: F401
from .onehot import DNNOneHot  # noqa: F401
from .cat import DNNCat  # noqa: F401
from .onehot_embedding import DNNOneHotEmbedding, nt_xent_loss_grad  # noqa: F401
from .onehot_gcn import DNNOneHotEmbeddingGCN  # noqa: F401
from . import checkpoint, data_utils, driver, parallel  # noqa: F401
from .recommend import rank_targets, recommend, score_candidates  # noqa: F401  (the function shadows its module's name in the package: `gdmcf_amd.recommend(...)`)

__all__ = ["DNN", "timestep_embedding", "GaussianDiffusion", "GaussianDiffusionDiscrete", "ModelMeanType", "FusedAdamW", "computeTopNAccuracy",
           "computeTopNAccuracy_device", "masked_topk", "score_topk", "score_rank", "print_results", "LightGCN", "BPRTrainer", "DNNOneHot", "DNNCat", "DNNOneHotEmbedding", "DNNOneHotEmbeddingGCN", "nt_xent_loss_grad", "recommend", "score_candidates", "rank_targets"]
