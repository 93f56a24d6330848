"""Float64 restatement of the GRU query encoder (``Gs.Query.transform == 'gru'``) and of a whole ``RawGnn`` behind it, for ``tests/test_query_gru_host.py`` /
``test_query_gru.py``.  Not a test module; torch on the CPU only.  The reference project names a recurrent query model and raises for it, so there is no fixture: the
yardstick is ``torch.nn.GRU`` in float64, which ``test_query_gru_host.py`` holds this restatement against.  The layers, the HEM head and the hypergraph tensors are the
oracle's (``oracle/ihgnn_ref.py``); the Adam allowance is the activation transform's (``query_transform_reference``).

For query q with word rows x_1 .. x_T of the vocabulary table, in the order of ``bag_input``, and h_0 = 0:

    r_t = sigmoid(W_ir x_t + b_ir + W_hr h_{t-1} + b_hr)
    z_t = sigmoid(W_iz x_t + b_iz + W_hz h_{t-1} + b_hz)
    n_t = tanh(W_in x_t + b_in + r_t * (W_hn h_{t-1} + b_hn))
    h_t = (1 - z_t) * n_t + z_t * h_{t-1}                              X0[query q] = h_T; T = 0: the zero row
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ihgnn_ref as ref
from query_transform_reference import adam_allowance, adam_excess, t64  # noqa: F401  (re-exported for the tests)

KEYS = tuple(f'embeddings.query_transform.{name}' for name in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'))
TILED = (32, 64, 128, 256)


def bag_bounds(bag_input, bag_offsets):
    """``[Q + 1]`` ends of the bags in ``bag_input``."""
    return np.append(np.asarray(bag_offsets, np.int64).reshape(-1), np.asarray(bag_input).reshape(-1).shape[0])


def ordered_product(x, w):
    """``x @ w.T`` summed over k in ascending order, one term at a time: appending zero columns to both operands appends exact zeros to every sum and changes no bit
    (a library product blocks its sums by the operands' sizes, so there the padded and the plain result may differ in the last place)."""
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=x.dtype)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * w[:, k]
    return acc


def gru_rows(w_vocab, bag_input, bag_offsets, w_ih, w_hh, b_ih, b_hh, product=lambda x, w: x @ w.t(), lanes=None):
    """``[Q, d]``: the last hidden state per bag; ``bag_input`` holds table rows (word id + 1).  All bags advance together, a finished bag keeps its state.
    ``product(x, w)``: how ``x w^T`` is evaluated.  ``lanes``: sigmoid and tanh are evaluated on rows padded to that many columns - torch's vectorised loops and their
    scalar tails differ in the last place, so a bitwise comparison of two widths puts every unit at the same place of the same loop."""
    def at(fn, v):
        return fn(v) if lanes is None else fn(F.pad(v, (0, lanes - v.shape[1])).contiguous())[:, :v.shape[1]]
    words = torch.as_tensor(np.asarray(bag_input)).long().reshape(-1)
    ends = bag_bounds(bag_input, bag_offsets)
    starts, lens = torch.from_numpy(ends[:-1]), torch.from_numpy(np.diff(ends))
    d = w_vocab.shape[1]
    h = torch.zeros(len(lens), d, dtype=w_vocab.dtype) + 0 * w_vocab[:1].sum()        # (no words at all: zeros, still a function of the table)
    for t in range(int(lens.max()) if len(lens) else 0):
        live = torch.nonzero(lens > t).reshape(-1)
        x, hp = w_vocab[words[starts[live] + t]], h[live]
        gi, gh = product(x, w_ih) + b_ih, product(hp, w_hh) + b_hh
        r = at(torch.sigmoid, gi[:, :d] + gh[:, :d])
        z = at(torch.sigmoid, gi[:, d:2 * d] + gh[:, d:2 * d])
        n = at(torch.tanh, gi[:, 2 * d:] + r * gh[:, 2 * d:])
        h = h.index_copy(0, live, (1 - z) * n + z * hp)
    return h


def torch_gru_rows(gru, w_vocab, bag_input, bag_offsets):
    """The same rows from a ``torch.nn.GRU(d, d, batch_first=True)`` module, run bag by bag."""
    words = torch.as_tensor(np.asarray(bag_input)).long().reshape(-1)
    ends = bag_bounds(bag_input, bag_offsets)
    rows = []
    for b in range(len(ends) - 1):
        if ends[b + 1] == ends[b]:
            rows.append(torch.zeros(w_vocab.shape[1], dtype=w_vocab.dtype))
        else:
            rows.append(gru(w_vocab[words[ends[b]:ends[b + 1]]][None])[1][0, 0])
    return torch.stack(rows) if rows else torch.zeros(0, w_vocab.shape[1], dtype=w_vocab.dtype)


def padded_width(d):
    return next(w for w in TILED if w >= d)


def pad_operands(w_vocab, w_ih, w_hh, b_ih, b_hh, width):
    """The five operands with zero columns / rows appended up to ``width``, every gate's block in the top-left of its own zero block."""
    d = w_vocab.shape[1]
    p = width - d
    return (F.pad(w_vocab, (0, p)), F.pad(w_ih.reshape(3, d, d), (0, p, 0, p)).reshape(3 * width, width), F.pad(w_hh.reshape(3, d, d), (0, p, 0, p)).reshape(3 * width, width),
            F.pad(b_ih.reshape(3, d), (0, p)).reshape(-1), F.pad(b_hh.reshape(3, d), (0, p)).reshape(-1))


def bags(lengths, vocab, seed):
    """``(bag_input, bag_offsets)`` with the given bag lengths, words drawn from table rows ``1 .. vocab``."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if len(lengths) else np.zeros(0, np.int64)
    return rng.integers(1, vocab + 1, int(lengths.sum())).astype(np.int64), offsets


def ragged_lengths(q, longest=None):
    """Bags of 0 .. 6 words with every 7th empty (one of ``longest`` words in the middle when asked for)."""
    lens = np.array([0 if k % 7 == 0 else 1 + (k * 5) % 6 for k in range(q)], np.int64)
    if longest is not None:
        lens[q // 2] = longest
    return lens


def operands(d, vocab, seed, dtype=torch.float64):
    """A word table ``[vocab + 1, d]`` and GRU parameters at torch's default scale ``U(-1/sqrt(d), 1/sqrt(d))``."""
    gen = torch.Generator().manual_seed(seed)
    k = d ** -0.5

    def uniform(*shape):
        return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1) * k).to(dtype)
    table = (torch.rand(vocab + 1, d, generator=gen, dtype=torch.float64) - 0.5).to(dtype)
    return table, uniform(3 * d, d), uniform(3 * d, d), uniform(3 * d), uniform(3 * d)


def model_features(sd, g, bag_input, bag_offsets, kind, layer_count, order):
    """``[X0, X1, .., XL]`` of a RawGnn (``Models/RawGnn.py:110-122``) with the GRU query rows, from a float64 state dict."""
    users, items = sd['embeddings.embedding_user.weight'][1:], sd['embeddings.embedding_item.weight'][1:]
    queries = gru_rows(sd['embeddings.embedding_bag_vocabulary.weight'], bag_input, bag_offsets, *(sd[k] for k in KEYS))
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


def model_scores(sd, g, bag_input, bag_offsets, kind, layer_count, order, u, q, i, lam=0.5):
    f = torch.cat(model_features(sd, g, bag_input, bag_offsets, kind, layer_count, order), 1)
    u, q, i = (torch.as_tensor(np.asarray(v)).long() for v in (u, q, i))
    return ref.hem_score(f[u], f[q + g.user_count], f[i + g.user_count + g.query_count], sd['prediction_layer.items_bias'][i], lam)


def model_step(sd_np, triples, counts, bag_input, bag_offsets, kind, layer_count, order, u, q, i, flags, lr=1e-3):
    """One training step in float64: ``dict(scores, loss, grads {key: tensor}, adam {key: tensor})`` - ``adam``: the parameters after one Adam step (torch's defaults,
    as the reference's driver)."""
    U, Q, I = (int(c) for c in counts[:3])
    g = ref.HyperGraph(np.asarray(triples), U, Q, I, dtype=torch.float64)
    sd = {k: t64(v).clone().requires_grad_(True) for k, v in sd_np.items()}
    scores = model_scores(sd, g, bag_input, bag_offsets, kind, layer_count, order, u, q, i)
    loss = F.binary_cross_entropy_with_logits(scores, t64(flags))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items()}
    params = [v.detach().clone().requires_grad_(True) for v in sd.values()]
    opt = torch.optim.Adam(params, lr, weight_decay=0)
    for p, k in zip(params, sd):
        p.grad = grads[k].clone()
    opt.step()
    return dict(scores=scores.detach(), loss=float(loss.detach()), grads=grads, adam={k: p.detach() for k, p in zip(sd, params)})
