"""Float64 restatement of the Srrl baseline (reference ``Models/Srrl.py``, ``Models/CommonLayers.py:7-26``, ``Helpers/TrainTestHelper.py:160-257``) for
``tests/test_srrl_host.py`` / ``test_srrl_kernels.py`` / ``test_srrl_model.py`` and the generator of fixture F15.  Not a test module; torch and numpy on the CPU only.

The block every module of the model is made of, on one concatenated row ``x`` of width K:

    n      = max(|x|_2, eps),  eps = 1e-12                      F.normalize's clamp
    x^     = x / n
    y      = act(W x^ + b),  act = identity or LeakyReLU(0.01)
    dz     = dy * (y > 0 ? 1 : 0.01)                            (LeakyReLU; the sign of y is the sign of the pre-activation)
    dW     = sum_rows dz x^T,  db = sum_rows dz,  dx^ = W^T dz
    dx     = (dx^ - x^ (x^ . dx^)) / n      where |x| >= eps    autograd of x / clamp_min(|x|, eps): the clamp passes the norm's gradient
    dx     = dx^ / eps                      below it            ... and blocks it here

Error bounds (``u = 2^-24``, one rounding of fp32): a sum of n products formed in ANY order (each product fused into its add or rounded once) sits within
``n u sum|terms|`` of the exact sum - no term passes through more than n roundings - and ``(n + c) u sum|terms|`` when the operands carry c roundings of their own.
The bounds below are of that form; every c is counted where it is used.  The backward takes the forward's stored inverse norms as an INPUT (the kernel reads them
from memory and the restatement is handed the same numbers), so there ``x^ = x inv`` carries one rounding, not the norm's.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12
SLOPE = 0.01
U = 2.0 ** -24


def t64(a):
    return a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()


# ------------------------------------------------------------------------------------------------ the block, per entry (numpy float64)
def cat_rows(a, idx_a, rep_a, b=None, idx_b=None, rep_b=1):
    """``[R, K]`` float64: row r = cat(a[idx_a[r // rep_a]], b[idx_b[r // rep_b]]); an index of ``None`` is the identity."""
    def rows(t, idx, rep):
        t = np.asarray(t, np.float64)
        t = t if idx is None else t[np.asarray(idx)]
        return np.repeat(t, rep, axis=0)
    x = rows(a, idx_a, rep_a)
    return x if b is None else np.concatenate([x, rows(b, idx_b, rep_b)], axis=1)


def block_forward(x, w, bias, normalize=True, leaky=False):
    """-> ``dict(y, inv, xhat, bound, bound_inv)``: ``bound`` per output entry, ``bound_inv`` per row.  The inverse norm: K squares summed in any order (K u on the
    sum, K / 2 on its root), the root and the reciprocal of the clamped norm (2 u; below eps the fp32 constant and the reciprocal, 2 u as well): ``(K / 2 + 2) u inv``.
    An output: its K products summed in some order (K u), the scale applied to the sum (K / 2 + 2 for the inverse norm, 1 for the multiply), the bias add (1), the
    activation's multiply by the fp32 slope (2: the constant's rounding and the product's): ``(K + K / 2 + 6) u (sum|w x^| + |b|)``."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float64)
    norm = np.sqrt((x * x).sum(1))
    inv = 1.0 / np.maximum(norm, EPS) if normalize else np.ones(x.shape[0])
    xhat = x * inv[:, None]
    z = xhat @ w.T + b
    y = np.where(z > 0, z, SLOPE * z) if leaky else z
    K = x.shape[1]
    bound = (K + K / 2 + 6) * U * (np.abs(xhat) @ np.abs(w).T + np.abs(b))
    return dict(y=y, inv=inv, xhat=xhat, norm=norm, bound=bound, bound_inv=(K / 2 + 2) * U * inv)


def block_backward(x, w, dy, y, normalize=True, leaky=False, inv=None):
    """Gradients of the block for the cotangent ``dy`` and the stored output ``y`` (which decides the activation's slope, as in the kernel):
    ``dict(dw, dbias, dx, bound_dw, bound_dbias, bound_dx)``.  ``inv``: the stored inverse norms, an input of the backward (default: exact).  Bounds, with R rows, K columns, m outputs:
    dz carries 2 u under LeakyReLU (the fp32 slope and the multiply), x^ = x inv 1 u.
    dw: R products in any order of a dz and an x^ entry -> ``(R + 3) u sum_r |dz x^|``; dbias: R terms of dz -> ``(R + 2) u sum_r |dz|``;
    dx^_k: m products of a dz -> ``(m + 2) u A_k`` with ``A = |W|^T |dz|``;  dot = x^ . dx^: K products of an x^ (1) and a dx^ (m + 2) ->
    ``(K + m + 3) u S`` with ``S = sum_j |x^_j| A_j``;  dx_k = (dx^_k - x^_k dot) inv: dx^_k's own m + 2, the product x^_k dot (x^_k 1, dot K + m + 3, the multiply 1),
    the subtraction (1) and the scale (1) on both parts -> ``u inv ((m + 4) A_k + (K + m + 7) |x^_k| S)``;  below eps dx_k = dx^_k / eps: dx^_k's m + 2, the fp32
    constant 1 / eps and the multiply (2) -> ``(m + 4) u A_k / eps``."""
    x, w, dy, y = (np.asarray(t, np.float64) for t in (x, w, dy, y))
    R, K = x.shape
    m = w.shape[0]
    norm = np.sqrt((x * x).sum(1))
    if inv is None:
        inv = 1.0 / np.maximum(norm, EPS) if normalize else np.ones(R)
    inv = np.asarray(inv, np.float64)
    xhat = x * inv[:, None]
    dz = dy * np.where(y > 0, 1.0, SLOPE) if leaky else dy
    dw = dz.T @ xhat
    dbias = dz.sum(0)
    dxhat = dz @ w
    A = np.abs(dz) @ np.abs(w)
    if normalize:
        above = (norm >= EPS)[:, None]
        dot = (xhat * dxhat).sum(1, keepdims=True)
        dx = np.where(above, (dxhat - xhat * dot) * inv[:, None], dxhat / EPS)
        bound_dx = np.where(above, U * inv[:, None] * ((m + 4) * A + (K + m + 7) * np.abs(xhat) * (np.abs(xhat) * A).sum(1, keepdims=True)), (m + 4) * U * A / EPS)
    else:
        dx, bound_dx = dxhat, (m + 2) * U * A
    return dict(dw=dw, dbias=dbias, dx=dx, bound_dw=(R + 3) * U * (np.abs(dz).T @ np.abs(xhat)), bound_dbias=(R + 2) * U * np.abs(dz).sum(0), bound_dx=bound_dx)


def group_sum(rows, bound, rep):
    """Row gradients of a repeated source: the ``rep`` consecutive rows of a group added -> (sum, bound): the rows' own bounds plus the ``rep`` terms' sum, ``rep`` u of their magnitudes."""
    rows, bound = np.asarray(rows, np.float64), np.asarray(bound, np.float64)
    g = rows.reshape(-1, rep, rows.shape[1])
    return g.sum(1), bound.reshape(g.shape).sum(1) + rep * U * np.abs(g).sum(1)


def rows_dot(x, y, rep=1):
    """-> (s, bound): ``s[r] = sum_c x[r, c] y[r // rep, c]``, ``width`` products in some order: ``width u sum|terms|``."""
    x, y = np.asarray(x, np.float64), np.repeat(np.asarray(y, np.float64), rep, axis=0)
    return (x * y).sum(1), x.shape[1] * U * np.abs(x * y).sum(1)


def rows_dot_backward(ds, x, y, rep=1):
    """-> (dx, dy, bound_dx, bound_dy): one product per dx entry (1 u), ``rep`` products per dy entry (``rep`` u)."""
    ds, x, y = (np.asarray(t, np.float64) for t in (ds, x, y))
    dx = ds[:, None] * np.repeat(y, rep, axis=0)
    terms = (ds[:, None] * x).reshape(-1, rep, x.shape[1])
    return dx, terms.sum(1), U * np.abs(dx), rep * U * np.abs(terms).sum(1)


def kg_loss(pos, neg, weight=None):
    """The KG loss of ``Helpers/TrainTestHelper.py:185-201`` -> ``dict(loss, dpos, dneg)`` in float64 (torch's ``logsigmoid`` and autograd)."""
    p, n = t64(pos).clone().requires_grad_(True), t64(neg).clone().requires_grad_(True)
    positive, negative = F.logsigmoid(p), F.logsigmoid(-n).mean(dim=1)
    if weight is None:
        loss = (-positive.mean() - negative.mean()) / 2
    else:
        w = t64(weight)
        loss = (-(w * positive).sum() / w.sum() - (w * negative).sum() / w.sum()) / 2
    loss.backward()
    return dict(loss=float(loss.detach()), dpos=p.grad.numpy(), dneg=n.grad.numpy())


def topk(scores, k):
    """-> (items [C, k] int64, scores [C, k]): best first, equal scores in ascending item id, ``-1`` / ``-inf`` beyond the row's entries."""
    scores = np.asarray(scores)
    C, I = scores.shape
    items, best = np.full((C, k), -1, np.int64), np.full((C, k), -np.inf, np.float64)
    for c in range(C):
        order = np.lexsort((np.arange(I), -scores[c].astype(np.float64)))[:k]
        items[c, :len(order)], best[c, :len(order)] = order, scores[c][order]
    return items, best


# ------------------------------------------------------------------------------------------------ the model (torch float64, autograd)
def _linear(sd, key, x):
    return x @ sd[key + '.weight'].t() + sd[key + '.bias']


def aggregation(sd, name, x):
    return F.leaky_relu(_linear(sd, name + '.aggregation.0', F.normalize(x, dim=-1)), SLOPE)


def mlp(sd, name, x):
    return _linear(sd, name + '.mlp.2', F.leaky_relu(_linear(sd, name + '.mlp.0', F.normalize(x, dim=-1)), SLOPE))


def query_rows(sd, bag_input, bag_offsets):
    """``[Q, d]``: the KG's bag means (``bag_input`` holds table rows, word id + 1)."""
    return F.embedding_bag(torch.as_tensor(np.asarray(bag_input)).long(), sd['KG.embedding_bag_vocabulary.weight'], torch.as_tensor(np.asarray(bag_offsets)).long(), mode='mean')


def kg_scores(sd, bags, sample, mode, positive_mode):
    """``Srrl.trainkg``: ``[B, 1]`` / ``[B, k]``.  ``sample`` as the reference's (long tensors)."""
    if positive_mode:
        positive, items2, users2, queries2 = sample
        scored_ids = positive[:, 2:3]
    else:
        positive, scored_ids, items2, users2, queries2 = sample
    U_, I_, Q_ = sd['KG.embedding_user.weight'][1:], sd['KG.embedding_item.weight'][1:], query_rows(sd, *bags)
    u, q, i = U_[positive[:, 0]].unsqueeze(1), Q_[positive[:, 1]].unsqueeze(1), I_[positive[:, 2]].unsqueeze(1)
    scored = I_[scored_ids.long()]
    k = scored.shape[1]
    if mode == 'tail-company-batch':
        other = I_[items2[:, 0]].unsqueeze(1) if positive_mode else i.expand(-1, k, -1)
        scored = aggregation(sd, 'kg_aggre_tail', torch.cat([scored, other], -1))
        context = mlp(sd, 'kg_mlp_pre', torch.cat([u, q], -1))
    elif mode == 'head-company-batch':
        head = aggregation(sd, 'kg_aggre_head', torch.cat([u, U_[users2[:, 0]].unsqueeze(1)], -1))
        context = mlp(sd, 'kg_mlp_pre', torch.cat([head, q], -1))
    else:
        query = aggregation(sd, 'kg_aggre_query', torch.cat([q, Q_[queries2[:, 0]].unsqueeze(1)], -1))
        context = mlp(sd, 'kg_mlp_pre', torch.cat([u, query], -1))
    return (scored * context).sum(2)


def ps_scores(sd, bags, users, queries, items, kg_loss_on=True):
    """``Srrl.forward``; ``items=None``: all items (row r of users / queries against item r)."""
    Q_ = query_rows(sd, *bags)
    items = torch.arange(sd['PS.embedding_item.weight'].shape[0] - 1) if items is None else items
    u, i, q = sd['PS.embedding_user.weight'][1:][users], sd['PS.embedding_item.weight'][1:][items], Q_[queries]
    if kg_loss_on:
        u = aggregation(sd, 'g_u', torch.cat([u, sd['KG.embedding_user.weight'][1:][users].detach()], -1))
        i = aggregation(sd, 'g_i', torch.cat([i, sd['KG.embedding_item.weight'][1:][items].detach()], -1))
    uq = mlp(sd, 'ps_mlp_uq', torch.cat([u, q], -1))
    ui = mlp(sd, 'ps_mlp_ui', torch.cat([u, i], -1))
    return mlp(sd, 'ps_mlp_pred', torch.cat([uq, ui], -1)).squeeze(-1)


def _leaves(sd_np):
    return {k: t64(v).clone().requires_grad_(True) for k, v in sd_np.items()}


def _finish(sd, loss, lr):
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else None) for k, v in sd.items()}
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr, weight_decay=0)
    for k, p in params.items():
        p.grad = None if grads[k] is None else grads[k].clone()
    opt.step()
    return grads, {k: p.detach() for k, p in params.items()}


def kg_step(sd_np, bags, positive, negative, weight, tails, heads, queries, mode, uni_weight=False, lr=1e-3):
    """One KG step in float64 -> ``dict(pos, neg, loss, grads, adam)``; ``grads[k]`` is ``None`` for a parameter the step does not reach (Adam leaves it alone)."""
    sd = _leaves(sd_np)
    long = lambda t: torch.as_tensor(np.asarray(t)).long()
    positive, negative, tails, heads, queries = (long(t) for t in (positive, negative, tails, heads, queries))
    neg = kg_scores(sd, bags, (positive, negative, tails, heads, queries), mode, False)
    pos = kg_scores(sd, bags, (positive, tails, heads, queries), mode, True)
    ln, lp = F.logsigmoid(-neg).mean(dim=1), F.logsigmoid(pos).squeeze(1)
    if uni_weight:
        loss = (-lp.mean() - ln.mean()) / 2
    else:
        w = t64(weight)
        loss = (-(w * lp).sum() / w.sum() - (w * ln).sum() / w.sum()) / 2
    grads, adam = _finish(sd, loss, lr)
    return dict(pos=pos.detach(), neg=neg.detach(), loss=float(loss.detach()), grads=grads, adam=adam)


def ps_step(sd_np, bags, users, queries, items, labels, kg_loss_on=True, lr=1e-3):
    """One PS step in float64 -> ``dict(scores, loss, grads, adam)``."""
    sd = _leaves(sd_np)
    long = lambda t: torch.as_tensor(np.asarray(t)).long()
    scores = ps_scores(sd, bags, long(users), long(queries), long(items), kg_loss_on)
    loss = F.binary_cross_entropy_with_logits(scores, t64(labels))
    grads, adam = _finish(sd, loss, lr)
    return dict(scores=scores.detach(), loss=float(loss.detach()), grads=grads, adam=adam)


def all_item_scores(sd_np, bags, users, queries, kg_loss_on=True):
    """``[C, I]``: every pair against every item."""
    sd = {k: t64(v) for k, v in sd_np.items()}
    n_items = sd['PS.embedding_item.weight'].shape[0] - 1
    with torch.no_grad():
        return torch.stack([ps_scores(sd, bags, torch.full((n_items,), int(u)), torch.full((n_items,), int(q)), None, kg_loss_on) for u, q in zip(users, queries)])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))
