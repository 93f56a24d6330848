"""Float64 reference for rankings deeper than ten (``ihg_score_topk_deep``, ``RawGnn.top_items(u, q, k)``, ``Metrics`` at extra cutoffs), for
``tests/test_topk_deep_host.py`` / ``test_topk_deep.py``.  Not a test module; torch on the CPU only.

    scores   HEM scores of every (pair, item) in float64, either head (``Models/PredictionLayers.py:35-43``)
    ranking  a stable descending sort: higher score first, equal scores by lower item id (the kernels' order)
    metrics  HR@K / NDCG@K / MAP@K: the reference's ``Helpers/Metrics.py:60-109`` with every 10 read as K - the cap is ``min(len(truth), K)``, ranks are taken
             within the first K, the logarithms run as far as K needs

The reference hard-codes ten (``Metrics.py:60-63``), so no golden fixture can be produced for any other cutoff: what ties this file to the reference is its K = 10
case, which ``tests/test_topk_deep_host.py`` holds equal to the pinned ``oracle.ihgnn_ref.ranking_metrics``.
"""
import math

import numpy as np
import torch

EPS = 1e-8


def all_item_scores(features, users, queries, query_row0, item_row0, bias, lam=0.5, cosine=False):
    """``[C, I]`` float64 scores of ``C`` (user, query) pairs against every item (``features`` / ``bias`` of any float type)."""
    f = features.double()
    users, queries = (torch.as_tensor(np.asarray(v)).long() for v in (users, queries))
    items = f[item_row0:]
    m = lam * f[queries + query_row0] + (1 - lam) * f[users]
    if cosine:
        m = m / m.norm(dim=1, keepdim=True).clamp_min(EPS)
        items = items / items.norm(dim=1, keepdim=True).clamp_min(EPS)
    return m @ items.t() + bias.double()


def ranking(scores, k):
    """The first ``k`` of a stable descending sort of a score vector (or of every row of a matrix)."""
    return torch.sort(scores, dim=-1, descending=True, stable=True).indices[..., :k]


def metrics_from_top(top, truth, flags=None, cutoff=10):
    """``(HR@K, NDCG@K, MAP@K)`` from a ranked item list (best first; only its first K entries count); ``flags=None``: every relevance 1."""
    top = [int(t) for t in top][:cutoff]
    cap = min(len(truth), cutoff)
    if flags is None:
        hits = [top.index(t) for t in truth if t in top]
        dcg = sum(math.log(2, r + 2) for r in hits)
        idcg = sum(math.log(2, r) for r in range(2, 2 + cap))
    else:
        pairs = [(top.index(t), f) for t, f in zip(truth, flags) if t in top]
        hits = [p for p, _ in pairs]
        dcg = sum(math.log(2, r + 2) * (2 ** f - 1) for r, f in pairs)
        idcg = sum(math.log(2, r + 2) * (2 ** f - 1) for r, f in enumerate(sorted((f for _, f in pairs), reverse=True)))
    hr = len(hits) / cap
    ap = 0.0 if not hits else sum(j / (r + 1) for r, j in zip(hits, range(1, len(hits) + 1))) / len(hits)
    return hr, dcg / idcg, ap


def ranking_metrics(scores, truth, flags=None, cutoff=10):
    """``metrics_from_top`` of the stable descending sort of ``scores`` over all items."""
    return metrics_from_top(ranking(scores, cutoff).tolist(), truth, flags, cutoff)
