"""Float64 restatement of the reference's query transform (``Gs.Query.transform == 'activation'``, ``Models/EmbeddingLayers.py:40-44, 76-91``) and of a whole
``RawGnn`` with it, for ``tests/test_query_transform_host.py`` / ``test_query_transform.py`` and the generator of fixture F13.  Not a test module; torch on the CPU
only.  The layers, the HEM head and the hypergraph tensors are the oracle's (``oracle/ihgnn_ref.py``), which has no query transform: this file adds it in front.

    m[q] = mean of the word rows of query q (0 for an empty bag)        nn.EmbeddingBag(mode='mean')
    z[q] = m[q] W^T + b                                                 nn.Linear(d, d)
    y[q] = act(z[q]),  act in {ReLU, Tanh}                              Gs.Query.transform_activation()
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ihgnn_ref as ref

ACTIVATIONS = {'relu': torch.relu, 'tanh': torch.tanh}
W_KEY, B_KEY = 'embeddings.query_transform.0.weight', 'embeddings.query_transform.0.bias'


def t64(a):
    return a.detach().cpu().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()


def bag_means(w_vocab, bag_input, bag_offsets):
    """``[Q, d]`` means of the word rows per bag, 0 for an empty bag; ``bag_input`` holds table rows (word id + 1)."""
    bag_input, bag_offsets = torch.as_tensor(np.asarray(bag_input)).long(), torch.as_tensor(np.asarray(bag_offsets)).long()
    if bag_input.numel() == 0:
        return torch.zeros(bag_offsets.shape[0], w_vocab.shape[1], dtype=w_vocab.dtype) + 0 * w_vocab[:1].sum()        # (no words at all: zeros, still a function of the table)
    return F.embedding_bag(bag_input, w_vocab, bag_offsets, mode='mean')


def query_rows(w_vocab, bag_input, bag_offsets, wq, bq, act):
    """``(m, z, y)`` of every query."""
    m = bag_means(w_vocab, bag_input, bag_offsets)
    z = m @ wq.t() + bq
    return m, z, ACTIVATIONS[act](z)


def longest_bag(bag_input, bag_offsets):
    ends = np.append(np.asarray(bag_offsets, np.int64), len(np.asarray(bag_input).reshape(-1)))
    return int(np.diff(ends).max()) if len(ends) > 1 else 0


def kink_threshold(m, wq, bq, longest):
    """``tau[q, j] = (d + longest bag + 8) 2^-23 (sum_k |m[q,k] W[j,k]| + |b[j]|)``: the worst-case rounding of an fp32 evaluation of ``z[q, j]`` (a mean of
    ``longest`` rows, a ``d``-term dot product, the bias add, a few roundings of slack), from the float64 operands alone.  Where ``|z| < tau`` the sign of an fp32
    ``z`` - the ReLU mask bit - is not determined by the inputs."""
    d = wq.shape[0]
    return (d + longest + 8) * 2.0 ** -23 * (m.abs() @ wq.abs().t() + bq.abs())


def model_features(sd, g, bag_input, bag_offsets, kind, layer_count, order, act):
    """``[X0, X1, .., XL]`` of a RawGnn (``Models/RawGnn.py:110-122``) from a float64 state dict in the reference's key space; ``act`` None: the mean transform."""
    users, items = sd['embeddings.embedding_user.weight'][1:], sd['embeddings.embedding_item.weight'][1:]
    if act is None:
        queries = bag_means(sd['embeddings.embedding_bag_vocabulary.weight'], bag_input, bag_offsets)
    else:
        queries = query_rows(sd['embeddings.embedding_bag_vocabulary.weight'], bag_input, bag_offsets, sd[W_KEY], sd[B_KEY], act)[2]
    x = torch.cat([users, queries, items])
    outs = [x]
    for l in range(layer_count):
        wt, bt = sd[f'gnn_{l}.feature_transform.weight'], sd[f'gnn_{l}.feature_transform.bias']
        if kind == 'ihgnn':
            x = ref.ihgnn_layer(x, g, wt, bt, sd[f'gnn_{l}.feature_interactor.aggregation.weight'], sd[f'gnn_{l}.feature_interactor.aggregation.bias'],
                                order if (l == 0 or order == 1) else 1)                     # RawGnn.py:76-78: only layer 0 keeps the requested order
        else:
            x = ref.hgcn_layer(x, g, wt, bt)
        outs.append(x)
    return outs


def model_scores(sd, g, bag_input, bag_offsets, kind, layer_count, order, act, u, q, i, lam=0.5):
    f = torch.cat(model_features(sd, g, bag_input, bag_offsets, kind, layer_count, order, act), 1)
    u, q, i = (torch.as_tensor(np.asarray(v)).long() for v in (u, q, i))
    return ref.hem_score(f[u], f[q + g.user_count], f[i + g.user_count + g.query_count], sd['prediction_layer.items_bias'][i], lam)


def model_step(sd_np, triples, counts, bag_input, bag_offsets, kind, layer_count, order, act, u, q, i, flags, lr=1e-3):
    """One training step in float64: ``dict(scores, loss, grads {key: tensor}, adam {key: tensor}, min_margin)`` - ``adam``: the parameters after one Adam step
    (torch's defaults, as the reference's driver); ``min_margin``: the smallest ``|z| - tau`` over the query pre-activations (``kink_threshold``)."""
    U, Q, I = (int(c) for c in counts[:3])
    g = ref.HyperGraph(np.asarray(triples), U, Q, I, dtype=torch.float64)
    sd = {k: t64(v).clone().requires_grad_(True) for k, v in sd_np.items()}
    scores = model_scores(sd, g, bag_input, bag_offsets, kind, layer_count, order, act, u, q, i)
    loss = F.binary_cross_entropy_with_logits(scores, t64(flags))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    params = [v.detach().clone().requires_grad_(True) for v in sd.values()]
    opt = torch.optim.Adam(params, lr, weight_decay=0)
    for p, k in zip(params, sd):
        p.grad = grads[k].clone()
    opt.step()
    margin = None
    if act is not None:
        with torch.no_grad():
            m, z, _ = query_rows(sd['embeddings.embedding_bag_vocabulary.weight'], bag_input, bag_offsets, sd[W_KEY], sd[B_KEY], act)
            margin = float((z.abs() - kink_threshold(m, sd[W_KEY], sd[B_KEY], longest_bag(bag_input, bag_offsets))).min())
    return dict(scores=scores.detach(), loss=float(loss.detach()), grads=grads, adam={k: p.detach() for k, p in zip(sd, params)}, min_margin=margin)


def fixture_error(z, prefix, got):
    """Largest deviation of ``got`` from what F13 keeps under ``prefix`` (whole: ``.full``; else every 8th row ``.rows8`` and the float64 row / column sums), relative to
    the kept tensor's largest magnitude - for the sums: to the largest sum of magnitudes of a row / column, which is what their rounding scales with."""
    g = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)

    def rel(a, b, scale=None):
        return float(np.abs(a - b).max() / max(np.abs(b).max() if scale is None else scale, 1e-30))
    if prefix + '.full' in z.files:
        return rel(g, z[prefix + '.full'].astype(np.float64))
    return max(rel(g[::8], z[prefix + '.rows8'].astype(np.float64)), rel(g.sum(1), z[prefix + '.rowsum'], np.abs(g).sum(1).max()),
               rel(g.sum(0), z[prefix + '.colsum'], np.abs(g).sum(0).max()))


def fixture_state(z, tag):
    """The initial parameters of model case ``tag`` (shared by its two activations) as ``{key: numpy}``."""
    pre = f'{tag}.sd.'
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def adam_allowance(g64, p64, bar, lr=1e-3, eps=1e-8):
    """Per entry, how far a parameter after Adam's FIRST step may sit from the float64 step when its gradient holds ``bar`` (relative to the gradient's largest
    magnitude).  The first step moves an entry by ``u(g) = lr g / (|g| + eps)`` (``m_hat = g``, ``v_hat = g^2``), which is steep where ``|g|`` is within a few orders
    of ``eps``: ``u' = lr eps / (|g| + eps)^2``.  ``u`` is monotone, so a gradient error of at most ``delta = bar max|g|`` moves the step by at most
    ``max |u(g +- delta) - u(g)|`` - from the float64 gradient alone - on top of ``bar max|p|`` for the parameter itself."""
    g = np.asarray(g64.detach().cpu().numpy() if torch.is_tensor(g64) else g64, np.float64)
    p = np.asarray(p64.detach().cpu().numpy() if torch.is_tensor(p64) else p64, np.float64)

    def u(x):
        return lr * x / (np.abs(x) + eps)
    delta = bar * np.abs(g).max()
    return bar * np.abs(p).max() + np.maximum(np.abs(u(g + delta) - u(g)), np.abs(u(g - delta) - u(g)))


def adam_excess(got, g64, p64, bar):
    """Largest ``|got - p64| / adam_allowance`` over the entries (<= 1: inside what the gradient's bar allows)."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    p = np.asarray(p64.detach().cpu().numpy() if torch.is_tensor(p64) else p64, np.float64)
    return float((np.abs(got - p) / adam_allowance(g64, p64, bar)).max())


def fixture_adam_excess(z, prefix, g64, p64, bar):
    """The entries F13 keeps of a stepped parameter (whole, or every 8th row) against the float64 step, as a multiple of ``adam_allowance``."""
    if prefix + '.full' in z.files:
        return adam_excess(z[prefix + '.full'], g64, p64, bar)
    g = np.asarray(g64.detach().cpu().numpy() if torch.is_tensor(g64) else g64, np.float64)
    p = np.asarray(p64.detach().cpu().numpy() if torch.is_tensor(p64) else p64, np.float64)
    return float((np.abs(z[prefix + '.rows8'].astype(np.float64) - p[::8]) / adam_allowance(g, p, bar)[::8]).max())
