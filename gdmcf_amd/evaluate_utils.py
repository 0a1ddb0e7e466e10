"""Evaluation helpers with the reference's interface (reference evaluate_utils.py:6-69) plus the
device-side history-mask + top-k used by main.py:296-301."""
import math

import numpy as np

import torch

from . import _lib


def masked_topk(prediction, k, mask_indptr=None, mask_indices=None, return_values=False):
    """Top-k item indices per row after setting the user's history to -inf (reference main.py:299-301).

    prediction: float32 [B, I] on the GPU (not modified).  The history mask is CSR: `mask_indptr`
    int64 [B+1], `mask_indices` int32 column ids.  Scores come back in descending order; ties are
    broken by the LOWEST item index (torch.topk leaves tie order unspecified)."""
    _lib.require_gpu(prediction, "prediction")
    lib = _lib.load()
    pred = prediction if (prediction.dtype == torch.float32 and prediction.stride(-1) == 1) else \
        prediction.float().contiguous()
    B, I = pred.shape
    if not 1 <= k <= I:
        raise AssertionError("selected index k out of range")
    dev = pred.device
    ip = ix = None
    if mask_indptr is not None:
        ip = mask_indptr.to(device=dev, dtype=torch.int64).contiguous()
        ix = mask_indices.to(device=dev, dtype=torch.int32).contiguous()
        assert ip.numel() == B + 1, "mask_indptr must have B+1 entries"
    idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    val = torch.empty(B, k, dtype=torch.float32, device=dev) if return_values else None
    _lib.check(lib.gdmcf_topk_masked_f32(pred.data_ptr(), pred.stride(0), B, I, _lib.ptr(ip), _lib.ptr(ix), k,
                                         idx.data_ptr(), _lib.ptr(val), _lib.stream_ptr()))
    return (val, idx) if return_values else idx


def _score_operands(what, user_emb, item_emb, mask_indptr, mask_indices, user_ids, check_ids, also_gpu=()):
    """The operands score_topk and score_rank (`what`: the caller, for the error texts) share, as their entries take them:
    (ue, ie, ids, n_rows, ip, ix) -- both tables float32 with unit column stride, `user_ids` int64 (range-checked against ue
    when `check_ids`: one synchronising copy) or None, the number of ranked rows, the mask CSR int64 / int32 or (None, None).
    Everything must be on the GPU, the (tensor, name) pairs of `also_gpu` included."""
    _lib.require_gpu(user_emb, "user embeddings")
    _lib.require_gpu(item_emb, "item embeddings")
    for t, name in (*also_gpu, (mask_indptr, "mask_indptr"), (mask_indices, "mask_indices"), (user_ids, "user_ids")):
        if t is not None:
            _lib.require_gpu(t, name)
    prep = lambda t: t if (t.dtype == torch.float32 and t.stride(-1) == 1) else t.float().contiguous()
    ue, ie = prep(user_emb.detach()), prep(item_emb.detach())
    assert ue.dim() == 2 and ie.dim() == 2 and ue.shape[1] == ie.shape[1], "user_emb [U, d] and item_emb [I, d] must share d"
    dev = ue.device
    ids = None
    if user_ids is not None:
        ids = user_ids.to(device=dev, dtype=torch.int64).contiguous()
        if check_ids and ids.numel():
            lo, hi = torch.aminmax(ids)  # (one synchronising copy)
            lo, hi = torch.stack((lo, hi)).tolist()
            if not (0 <= lo and hi < ue.shape[0]):
                raise IndexError(f"{what}: user_ids out of range")
    n_rows = ids.numel() if ids is not None else ue.shape[0]
    ip = ix = None
    if mask_indptr is not None:
        ip = mask_indptr.to(device=dev, dtype=torch.int64).contiguous()
        ix = mask_indices.to(device=dev, dtype=torch.int32).contiguous()
    return ue, ie, ids, n_rows, ip, ix


def score_topk(user_emb, item_emb, k, mask_indptr=None, mask_indices=None, user_ids=None, return_values=False, check_ids=True):
    """masked_topk(user_emb[user_ids] @ item_emb.T, k, mask_indptr, mask_indices) without the score matrix (reference
    lightGCN.py:75-90: the product, the dense -inf mask of the training interactions and torch.topk): one fused kernel,
    gdmcf_score_topk_f32, keeps the scores on chip.

    user_emb float32 [U, d], item_emb float32 [I, d] on the GPU; `user_ids` (int64, optional) picks the rows of user_emb,
    otherwise every row is ranked.  The CSR mask has one row per RANKED row (`mask_indptr` int64 [n_rows + 1], `mask_indices`
    int32 item ids).  Same return convention, tie rule (lowest item index first) and degenerate-row convention (masked
    items count as -inf) as masked_topk.  `check_ids=False` skips the range check of `user_ids` (a device-to-host
    synchronisation): for callers that built the ids on the host and know them to lie in [0, U)."""
    ue, ie, ids, n_rows, ip, ix = _score_operands("score_topk", user_emb, item_emb, mask_indptr, mask_indices, user_ids, check_ids)
    lib = _lib.load()
    dev = ue.device
    I, d = ie.shape
    if not 1 <= k <= I:
        raise AssertionError("selected index k out of range")
    assert ip is None or ip.numel() == n_rows + 1, "mask_indptr must have one entry per ranked row plus one"
    idx = torch.empty(n_rows, k, dtype=torch.int64, device=dev)
    val = torch.empty(n_rows, k, dtype=torch.float32, device=dev) if return_values else None
    if n_rows == 0:
        return (val, idx) if return_values else idx
    nbytes = int(lib.gdmcf_score_topk_ws_bytes(n_rows, I, d, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _lib.check(lib.gdmcf_score_topk_f32(ue.data_ptr(), ue.stride(0), _lib.ptr(ids), n_rows, ie.data_ptr(), ie.stride(0), I, d,
                                        _lib.ptr(ip), _lib.ptr(ix), k, idx.data_ptr(), _lib.ptr(val), _lib.ptr(ws), nbytes,
                                        _lib.stream_ptr()))
    return (val, idx) if return_values else idx


def score_rank(user_emb, item_emb, tgt_indptr, tgt_indices, mask_indptr=None, mask_indices=None, user_ids=None, G=None,
               return_live=False, check_ids=True):
    """The exact catalogue rank of named items per ranked row, without the score matrix: the counterpart of score_topk for
    held-out targets (gdmcf_score_rank_f32: the same fused product, counting instead of selecting).  ranks[r, j] is the number
    of items that precede target j of row r in score_topk's order (descending score, equal scores in ascending item index,
    masked items as -inf at the end by index) -- the place the item has in score_topk(..., k = n_items)'s list, for any
    catalogue size.  -1 for a target outside [0, n_items) and for the columns past a row's length.

    Tensors as score_topk's; the target CSR (`tgt_indptr` int64 [n_rows + 1], `tgt_indices` int32, required) and the mask CSR
    have one row per RANKED row; rows may be unsorted and hold repeats.  `G`: the number of columns; target entries past G are
    not ranked.  G=None takes the longest target row (at least 1), which costs ONE DEVICE-TO-HOST READ of `tgt_indptr`: callers
    that know G pass it.  Returns int32 [n_rows, G] on the device, and with `return_live` also n_live int32 [n_rows], the
    number of unmasked items of each row.  `check_ids` as in score_topk."""
    if tgt_indptr is None or tgt_indices is None:
        raise ValueError("score_rank: tgt_indptr and tgt_indices are required")
    if (mask_indptr is None) != (mask_indices is None):
        raise ValueError("score_rank: mask_indptr and mask_indices go together")
    ue, ie, ids, n_rows, ip, ix = _score_operands("score_rank", user_emb, item_emb, mask_indptr, mask_indices, user_ids, check_ids,
                                                  also_gpu=((tgt_indptr, "tgt_indptr"), (tgt_indices, "tgt_indices")))
    lib = _lib.load()
    dev = ue.device
    I, d = ie.shape
    tp = tgt_indptr.to(device=dev, dtype=torch.int64).contiguous()
    tx = tgt_indices.to(device=dev, dtype=torch.int32).contiguous()
    assert tp.numel() == n_rows + 1, "tgt_indptr must have one entry per ranked row plus one"
    assert ip is None or ip.numel() == n_rows + 1, "mask_indptr must have one entry per ranked row plus one"
    if G is None:
        G = max(int((tp[1:] - tp[:-1]).max()), 1) if n_rows else 1  # (the one host read)
    G = int(G)
    if G < 1:
        raise AssertionError("score_rank: G must be at least 1")
    ranks = torch.empty(n_rows, G, dtype=torch.int32, device=dev)
    live = torch.empty(n_rows, dtype=torch.int32, device=dev) if return_live else None
    if n_rows == 0:
        return (ranks, live) if return_live else ranks
    if tx.numel() == 0:
        tx = torch.zeros(1, dtype=torch.int32, device=dev)  # (a pointer for the entry; no row reads it)
    nbytes = int(lib.gdmcf_score_rank_ws_bytes(n_rows, I, d, G))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.gdmcf_score_rank_f32(ue.data_ptr(), ue.stride(0), _lib.ptr(ids), n_rows, ie.data_ptr(), ie.stride(0), I, d,
                                        _lib.ptr(ip), _lib.ptr(ix), tp.data_ptr(), tx.data_ptr(), G, ranks.data_ptr(),
                                        ranks.stride(0), _lib.ptr(live), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    return (ranks, live) if return_live else ranks


def csr_rows_to_device(csr, rows, device):
    """(indptr int64, indices int32) device tensors for `csr[rows]` (a scipy CSR history matrix)."""
    sub = csr[rows]
    return (torch.from_numpy(sub.indptr.astype("int64")).to(device),
            torch.from_numpy(sub.indices.astype("int32")).to(device))


def computeTopNAccuracy(GroundTruth, predictedIndices, topN):
    """Precision / Recall / NDCG / MRR @N with the reference's exact conventions: users with an
    empty ground truth add nothing to the sums but still count in the divisor; 4-decimal rounding."""
    precision, recall, NDCG, MRR = [], [], [], []
    n_users = len(predictedIndices)
    for N in topN:
        sum_p = sum_r = sum_n = sum_m = 0
        for i in range(n_users):
            gt = GroundTruth[i]
            if len(gt) == 0:
                continue
            gt_set = set(gt)
            hits, dcg, idcg, mrr, left, first = 0, 0.0, 0.0, 0.0, len(gt), True
            pred = predictedIndices[i]
            for j in range(N):
                if pred[j] in gt_set:
                    dcg += 1.0 / math.log2(j + 2)
                    if first:
                        mrr = 1.0 / (j + 1.0)
                        first = False
                    hits += 1
                if left > 0:
                    idcg += 1.0 / math.log2(j + 2)
                    left -= 1
            sum_p += hits / N
            sum_r += hits / len(gt)
            sum_n += (dcg / idcg) if idcg != 0 else 0
            sum_m += mrr
        precision.append(round(sum_p / n_users, 4))
        recall.append(round(sum_r / n_users, 4))
        NDCG.append(round(sum_n / n_users, 4))
        MRR.append(round(sum_m / n_users, 4))
    return precision, recall, NDCG, MRR


def computeTopNAccuracy_device(ground_truth_csr, predicted_idx, topN):
    """computeTopNAccuracy with the per-user work on the MI355X (gdmcf_topn_metrics_f64): `ground_truth_csr` is a
    scipy CSR (one row per predicted user), `predicted_idx` an int64 device tensor [U, >= max(topN)] as masked_topk
    returns it.  The per-user terms are bit-identical to the Python loop; they are added up in user order on the
    host, so the rounded results equal computeTopNAccuracy's (the reference's) exactly."""
    import ctypes
    from . import _lib
    _lib.require_gpu(predicted_idx, "predicted indices")
    topN = [int(n) for n in topN]
    if topN != sorted(set(topN)) or not topN:
        raise ValueError("topN must be ascending and non-empty")
    gt = ground_truth_csr.tocsr().astype(np.float32, copy=True)
    gt.eliminate_zeros()
    gt.sort_indices()
    U = gt.shape[0]
    pred = predicted_idx if predicted_idx.dtype == torch.int64 else predicted_idx.to(torch.int64)
    if pred.stride(-1) != 1:
        pred = pred.contiguous()
    assert pred.shape[0] == U and pred.shape[1] >= topN[-1], "one prediction row per ground-truth row, >= max(topN) items"
    dev = pred.device
    indptr = torch.from_numpy(gt.indptr.astype(np.int64)).to(dev)
    indices = torch.from_numpy(gt.indices.astype(np.int32)).to(dev)
    out = torch.empty(U, len(topN), 4, dtype=torch.float64, device=dev)
    tn = (ctypes.c_int * len(topN))(*topN)
    _lib.check(_lib.load().gdmcf_topn_metrics_f64(pred.data_ptr(), pred.stride(0), U, indptr.data_ptr(), indices.data_ptr(),
                                                  tn, len(topN), out.data_ptr(), _lib.stream_ptr()))
    terms = out.cpu().numpy()
    sums = np.add.accumulate(terms, axis=0)[-1]  # sequential float64 additions in user order, as the reference's loop
    res = [[round(float(sums[k, m]) / U, 4) for k in range(len(topN))] for m in range(4)]
    return res[0], res[1], res[2], res[3]


def _check_topN(topN):
    topN = [int(n) for n in topN]
    if topN != sorted(set(topN)) or not topN or topN[0] < 1:
        raise ValueError("topN must be ascending, non-empty and >= 1")
    return topN


def rank_metrics(ranks, topN):
    """computeTopNAccuracy from RANKS instead of lists, in plain Python: ranks[u] holds the 0-based catalogue rank of each of
    user u's ground-truth items (gdmcf_amd.rank_targets; negative entries = no item there).  |GT| is the number of non-negative
    entries, a hit below N an entry < N; the hits are taken in ascending rank, so every sum receives the terms of the
    reference's loop over the list the ranks came from, in its order: the same rounded results.  Cut-offs are bounded by no
    list length; users without ground truth add nothing but count in the divisor."""
    topN = _check_topN(topN)
    precision, recall, NDCG, MRR = [], [], [], []
    n_users = len(ranks)
    for N in topN:
        sum_p = sum_r = sum_n = sum_m = 0
        for i in range(n_users):
            gt = sorted(int(r) for r in ranks[i] if int(r) >= 0)
            if len(gt) == 0:
                continue
            hits, dcg, idcg, mrr = 0, 0.0, 0.0, 0.0
            for r in gt:
                if r >= N:
                    break
                dcg += 1.0 / math.log2(r + 2)
                if hits == 0:
                    mrr = 1.0 / (r + 1.0)
                hits += 1
            for j in range(min(N, len(gt))):
                idcg += 1.0 / math.log2(j + 2)
            sum_p += hits / N
            sum_r += hits / len(gt)
            sum_n += (dcg / idcg) if idcg != 0 else 0
            sum_m += mrr
        precision.append(round(sum_p / n_users, 4))
        recall.append(round(sum_r / n_users, 4))
        NDCG.append(round(sum_n / n_users, 4))
        MRR.append(round(sum_m / n_users, 4))
    return precision, recall, NDCG, MRR


RANK_METRICS_GROUP = 8  # cut-offs per gdmcf_rank_metrics_f64 call


def rank_metrics_terms(ranks, topN):
    """The per-user terms [U, len(topN), 4] (float64, on the device; precision / recall / NDCG / MRR) of gdmcf_rank_metrics_f64
    for int32 device ranks [U, G], the cut-offs in groups of RANK_METRICS_GROUP."""
    import ctypes
    _lib.require_gpu(ranks, "ranks")
    topN = _check_topN(topN)
    if ranks.dim() != 2 or ranks.shape[1] < 1:
        raise ValueError("ranks is [n_users, G >= 1]")
    r = ranks if ranks.dtype == torch.int32 else ranks.to(torch.int32)
    if r.stride(-1) != 1:
        r = r.contiguous()
    U, G = r.shape
    out = torch.empty(U, len(topN), 4, dtype=torch.float64, device=r.device)
    if U == 0:
        return out
    for lo in range(0, len(topN), RANK_METRICS_GROUP):
        grp = topN[lo:lo + RANK_METRICS_GROUP]
        part = out if len(grp) == len(topN) else torch.empty(U, len(grp), 4, dtype=torch.float64, device=r.device)
        _lib.check(_lib.load().gdmcf_rank_metrics_f64(r.data_ptr(), r.stride(0), U, G, (ctypes.c_int * len(grp))(*grp), len(grp),
                                                      part.data_ptr(), _lib.stream_ptr()))
        if part is not out:
            out[:, lo:lo + len(grp)] = part
    return out


def rank_metrics_device(ranks, topN):
    """rank_metrics with the per-user work on the MI355X (gdmcf_rank_metrics_f64): `ranks` an int32 device tensor [U, G] as
    gdmcf_amd.rank_targets returns it for the ground truth as targets.  The per-user terms carry the bits of
    gdmcf_topn_metrics_f64 on the lists the ranks came from; they are added up in user order on the host and rounded exactly
    as computeTopNAccuracy_device does, so the four lists equal its (and the reference's) -- for any cut-offs, also above the
    item count."""
    topN = _check_topN(topN)
    terms = rank_metrics_terms(ranks, topN).cpu().numpy()
    U = terms.shape[0]
    sums = np.add.accumulate(terms, axis=0)[-1]  # sequential float64 additions in user order, as the reference's loop
    res = [[round(float(sums[k, m]) / U, 4) for k in range(len(topN))] for m in range(4)]
    return res[0], res[1], res[2], res[3]


def print_results(loss, valid_result, test_result):
    """output the evaluation results."""
    if loss is not None:
        print("[Train]: loss: {:.4f}".format(loss))
    for tag, res in (("Valid", valid_result), ("Test", test_result)):
        if res is not None:
            print("[{}]: Precision: {} Recall: {} NDCG: {} MRR: {}".format(
                tag, *["-".join(str(x) for x in res[i]) for i in range(4)]))
