"""Float64 restatement of the reference's cosine-similarity HEM head (``Gs.Prediction.use_cosine_similarity``, ``Models/PredictionLayers.py:38-40``) and of a whole
``RawGnn`` with it, for ``tests/test_cosine_head_host.py`` / ``test_cosine_head.py`` and the generator of fixture F14.  Not a test module; torch on the CPU only.
The layers, the embeddings and the hypergraph tensors are the oracle's (``oracle/ihgnn_ref.py``, through ``tests/query_transform_reference.py``), which scores with
the dot product only: this file puts the other head behind them.

    a = [X_0 | .. | X_L][item]          m = lam a[query] + (1 - lam) a[user]          eps = 1e-8
    na = max(||a||, eps)   nm = max(||m||, eps)   c = (a . m) / (na nm)   score = c + items_bias[item]            torch.cosine_similarity
    dc/da = m / (na nm) - c a / (na ||a||)                dc/dm = a / (na nm) - c m / (nm ||m||)                  second terms 0 for a zero row

torch clamps the VALUE of the norm outside autograd and differentiates the unclamped norm (``d||a||/da = a / ||a||``, 0 at ``a = 0``): wherever ``||a|| >= eps`` the
second term is the familiar ``c a / na^2``; a row with ``0 < ||a|| < eps`` keeps it with ``na ||a||`` in the denominator (checked against autograd in
``tests/test_cosine_head_host.py``).
"""
import numpy as np
import torch
import torch.nn.functional as F

import query_transform_reference as qref
from oracle import ihgnn_ref as ref

EPS = 1e-8
t64 = qref.t64


def cosine(a, m):
    """``c`` of every row pair, written out (no call of ``torch.cosine_similarity``: this is the statement it is checked against)."""
    na, nm = a.norm(dim=1).clamp_min(EPS), m.norm(dim=1).clamp_min(EPS)
    return (a * m).sum(1) / (na * nm)


def hem_cosine(user, query, item, bias, lam=0.5):
    """Scores of ``[B, D]`` row sets; ``bias`` already gathered to ``[B]``."""
    return cosine(item, lam * query + (1 - lam) * user) + bias


def row_gradients(user, query, item, ds, lam=0.5):
    """``(rowgrad_user, rowgrad_query, rowgrad_item)`` of ``sum_r ds[r] score[r]``, ``[B, D]`` each, from the closed forms above (not from autograd)."""
    a, m = item, lam * query + (1 - lam) * user
    ra, rm = a.norm(dim=1, keepdim=True), m.norm(dim=1, keepdim=True)
    na, nm = ra.clamp_min(EPS), rm.clamp_min(EPS)
    c = (a * m).sum(1, keepdim=True) / (na * nm)
    unit = lambda x, r: torch.where(r > 0, x / r.clamp_min(1e-300), torch.zeros_like(x))
    dc_da = m / (na * nm) - c / na * unit(a, ra)
    dc_dm = a / (na * nm) - c / nm * unit(m, rm)
    ds = ds.reshape(-1, 1)
    return ds * (1 - lam) * dc_dm, ds * lam * dc_dm, ds * dc_da


def all_item_scores(features, users, queries, query_row0, item_row0, bias, lam=0.5):
    """``[C, I]`` scores of ``C`` (user, query) pairs against every item: what ``forward(u * ones(I), q * ones(I), None)`` gives per pair (``RawGnn.py:124-137``)."""
    users, queries = (torch.as_tensor(np.asarray(v)).long() for v in (users, queries))
    items = features[item_row0:]
    m = lam * features[queries + query_row0] + (1 - lam) * features[users]
    return (m / m.norm(dim=1, keepdim=True).clamp_min(EPS)) @ (items / items.norm(dim=1, keepdim=True).clamp_min(EPS)).t() + bias


def model_features(sd, triples, counts, bag_input, bag_offsets, kind, layer_count, order):
    """``[N, d (L + 1)]`` float64 features of a mean-transform RawGnn from a state dict in the reference's key space."""
    U, Q, I = (int(c) for c in counts[:3])
    g = ref.HyperGraph(np.asarray(triples), U, Q, I, dtype=torch.float64)
    return torch.cat(qref.model_features(sd, g, bag_input, bag_offsets, kind, layer_count, order, None), 1)


def model_step(sd_np, triples, counts, bag_input, bag_offsets, kind, layer_count, order, u, q, i, flags, lr=1e-3, lam=0.5):
    """One training step with the cosine head in float64: ``dict(scores, loss, grads {key: tensor}, adam {key: tensor})`` - ``adam``: the parameters after one Adam step
    (torch's defaults, as the reference's driver).  ``bag_input`` holds table rows (word id + 1)."""
    U, Q, I = (int(c) for c in counts[:3])
    sd = {k: t64(v).clone().requires_grad_(True) for k, v in sd_np.items()}
    f = model_features(sd, triples, counts, bag_input, bag_offsets, kind, layer_count, order)
    u, q, i = (torch.as_tensor(np.asarray(v)).long() for v in (u, q, i))
    scores = hem_cosine(f[u], f[q + U], f[i + U + Q], sd['prediction_layer.items_bias'][i], lam)
    loss = F.binary_cross_entropy_with_logits(scores, t64(flags))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    params = [v.detach().clone().requires_grad_(True) for v in sd.values()]
    opt = torch.optim.Adam(params, lr, weight_decay=0)
    for p, k in zip(params, sd):
        p.grad = grads[k].clone()
    opt.step()
    return dict(scores=scores.detach(), loss=float(loss.detach()), grads=grads, adam={k: p.detach() for k, p in zip(sd, params)})


def model_all_item_scores(sd_np, triples, counts, bag_input, bag_offsets, kind, layer_count, order, users, queries, lam=0.5):
    """``[C, I]`` float64 scores of the model's (user, query) pairs against every item."""
    U, Q, I = (int(c) for c in counts[:3])
    sd = {k: t64(v) for k, v in sd_np.items()}
    with torch.no_grad():
        f = model_features(sd, triples, counts, bag_input, bag_offsets, kind, layer_count, order)
        return all_item_scores(f, users, queries, U, U + Q, sd['prediction_layer.items_bias'], lam)
