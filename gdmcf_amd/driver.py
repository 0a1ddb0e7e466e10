"""The training / evaluation loop surface of the reference driver (reference main.py:267-351), restated
on top of the HIP path.  Host glue only: batches in, metrics out.

* `train_one_epoch`  = main.py:327-351 (the body that is dead code behind a stray `continue` in the
  shipped file): zero_grad -> training_losses -> mean -> backward -> step per batch.
* `evaluate`         = main.py:267-310: p_sample -> history mask -> top-N -> computeTopNAccuracy.
  The reference moves a dense [B, I] row block to the device per batch and masks with
  `prediction[his_data.nonzero()] = -inf`; here the history stays CSR and the mask is applied inside the
  top-k kernel.  `sparse=True` hands p_sample the rows as a CsrBatch as well: with sampling_steps == 0 the first layers of the
  reverse loop then gather the rows' weight rows instead of multiplying a dense batch (routes: DESIGN 4.9).
"""
import numpy as np
import torch

from . import evaluate_utils, reverse_route
from .data_utils import DeviceBatchLoader, DeviceCSR
from .evaluate_utils import masked_topk
from .parallel import DataParallelStep


def dense_rows(csr, rows, device):
    """float32 dense [len(rows), n_items] block of a scipy CSR matrix, on `device` (what DataDiffusion +
    DataLoader deliver in the reference, data_utils.py:216-226)."""
    return torch.from_numpy(np.asarray(csr[rows].todense(), dtype=np.float32)).to(device)


def train_one_epoch(diffusion, model, optimizer, train_csr, batch_size, device, reweight=True, shuffle=True,
                    drop_last=True, generator=None, step=None, sparse=False, graph_step=None):
    """One pass over the users of `train_csr`.  Returns (sum of batch losses, number of batches), the two
    numbers the reference prints per epoch (main.py:377).  sparse=True hands `training_losses` the rows as a CsrBatch
    (bit-identical, no densify launch); graph_step = a graph.GraphedTrainStep over the same matrix replays the whole
    step from one hipGraph per batch (drop_last is then forced: the captured batch size is fixed)."""
    model.train()
    loader = DeviceBatchLoader(train_csr, batch_size, shuffle=shuffle, drop_last=drop_last or graph_step is not None,
                               device=device, generator=generator, sparse=sparse, ids_only=graph_step is not None)
    step = step or (None if graph_step is not None else DataParallelStep(diffusion, model, optimizer))
    total, count = None, 0
    with_index = bool(getattr(diffusion, "indexIn", False))  # embedding backbones need the users' ids (main.py:346)
    for batch, index in loader:
        if graph_step is not None:
            loss = graph_step(index)
        else:
            loss = step(batch, reweight, index=index) if with_index else step(batch, reweight)
        total = loss if total is None else total + loss
        count += 1
    return (float(total) if total is not None else 0.0), count


@torch.no_grad()
def evaluate(diffusion, model, data_csr, data_te, mask_his, topN, sampling_steps, sampling_noise, batch_size,
             device, sparse=False, latent=False, recommend=False, candidates=None, ranks=False):
    """Precision / Recall / NDCG / MRR @topN exactly as reference main.py:267-310.

    data_csr: rows fed to p_sample (the reference feeds the training rows); data_te: ground-truth CSR;
    mask_his: CSR of interactions to exclude from the ranking.  sparse=True: p_sample receives each batch as a
    data_utils.CsrBatch (never densified where the reverse loop takes sparse rows; densified inside p_sample otherwise).
    latent=True / "extended": passed to p_sample -- the reverse loop in the first hidden layer's space where it can run there
    (routes: DESIGN 4.9); composes with sparse=True.  "extended" is also passed to gdmcf_amd.recommend with recommend=True.
    recommend=True: each batch's list comes from gdmcf_amd.recommend with mask_his as a DeviceCSR -- uploaded once
    per call, or passed through when it already is one -- so no batch slices a matrix on the host; `sparse` is then ignored and
    of `latent` only the value "extended" matters (recommend picks its own route, `diffusion.last_recommend_route`).
    candidates (with recommend=True only): [n_users, C], row u the items user u is ranked within (gdmcf_amd.recommend's
    `candidates`: a retriever's output, an allow-list, the sampled-negatives protocol's one held-out item among sampled ones).
    ranks=True (with recommend=True, without candidates): no lists at all -- gdmcf_amd.rank_targets gives the catalogue rank of
    every ground-truth item and evaluate_utils.rank_metrics_device the metrics from them: the same return value, with topN no
    longer bounded by the top-k's k."""
    if candidates is not None and not recommend:
        raise ValueError("driver.evaluate: candidates needs recommend=True")
    if ranks and (not recommend or candidates is not None):
        raise ValueError("driver.evaluate: ranks=True needs recommend=True and takes no candidates")
    model.eval()
    extended = {} if reverse_route.latent_mode(latent) in (None, "base") else dict(latent=latent)  # (recommend's default: True)
    n = mask_his.shape[0]
    predict_items = []
    dcsr = data_csr if isinstance(data_csr, DeviceCSR) else DeviceCSR(data_csr, device)
    if recommend:
        from .recommend import recommend as recommend_fn
        mask = mask_his if isinstance(mask_his, DeviceCSR) else DeviceCSR(mask_his, device)
        if ranks:
            from .recommend import rank_targets
            gt = data_te.tocsr().astype(np.float32, copy=True)  # (the ground truth as computeTopNAccuracy_device reads it)
            gt.eliminate_zeros()
            got = rank_targets(diffusion, model, dcsr, np.arange(n), DeviceCSR(gt, device), mask=mask, sampling_steps=sampling_steps,
                               sampling_noise=sampling_noise, batch_size=batch_size, **extended)
            return evaluate_utils.rank_metrics_device(got, topN)
        lists = recommend_fn(diffusion, model, dcsr, np.arange(n), topN[-1], mask=mask, sampling_steps=sampling_steps,
                             sampling_noise=sampling_noise, batch_size=batch_size,  # (the same batches, made inside)
                             **extended, **(dict(candidates=candidates) if candidates is not None else {}))
        return evaluate_utils.computeTopNAccuracy_device(data_te, lists, topN)
    for lo in range(0, n, batch_size):
        rows = np.arange(lo, min(lo + batch_size, n))
        batch = dcsr.batch(torch.from_numpy(rows)) if sparse else dcsr.rows(torch.from_numpy(rows))
        kw = dict(index=torch.from_numpy(rows)) if getattr(diffusion, "indexIn", False) else {}
        if latent:
            kw["latent"] = latent
        prediction = diffusion.p_sample(model, batch, sampling_steps, sampling_noise, **kw)
        indptr, cols = evaluate_utils.csr_rows_to_device(mask_his, rows, device)
        predict_items.append(masked_topk(prediction, topN[-1], indptr, cols))
    # the ranked lists never leave the device; the metric terms per user are computed there too
    return evaluate_utils.computeTopNAccuracy_device(data_te, torch.cat(predict_items), topN)
