"""``RawGnn.search`` and ``python -m ihgnn_amd.Search`` on the GPU.

The feature is what the model itself would compute for a query appended to ``queries_multihot.txt`` with no interaction, so the first verdict needs no tolerance:
the synthetic dataset HAS such queries - four extra bags, one of them empty, that no triple names - and ``model.search(users, words=their bags)`` must equal
``model.top_items(users, their indices)`` bit for bit, for every layer kind, at a tiled and a padded width, over a layout with and without the isolated nodes, with
and without the query transform, under both heads.  Everything else is held against the float64 reference of ``tests/search_reference.py`` within
``ranking_reference``'s per-score bound, or against ``top_items`` itself where a filter only removes items."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import search_reference as S

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, Q_TRAIN, EXTRA, I, V, E = 40, 12, 4, 90, 30, 400
LAM = 0.5


def dev():
    return torch.device('cuda:0')


class settings:
    """``Gs.Query`` and the head set for the block, put back after it."""

    def __init__(self, transform='mean', cosine=False):
        self.new = (transform, nn.Tanh, bool(cosine))

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old = (Gs.Query.transform, Gs.Query.transform_activation, Gs.Prediction.use_cosine_similarity)
        Gs.Query.transform, Gs.Query.transform_activation, Gs.Prediction.use_cosine_similarity = self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Query.transform, Gs.Query.transform_activation, Gs.Prediction.use_cosine_similarity = self.old


def workload():
    """40 users, 12 training queries + 4 queries with words and NO interaction (the second of them with no word either), 90 items; a third of the users and items in no
    hyperedge, so a compact layout has something to leave out."""
    from ihgnn_amd import synth
    w = synth.draw(U, Q_TRAIN + EXTRA, I, V, E, seed=5)
    rng = np.random.default_rng(8)
    live_u, live_i = rng.choice(U, 2 * U // 3, replace=False), rng.choice(I, 2 * I // 3, replace=False)
    w.triples = np.stack([rng.choice(live_u, E), rng.integers(0, Q_TRAIN, E), rng.choice(live_i, E)], 1).astype(np.int64)
    ends = np.append(w.bag_offsets[1:], len(w.bag_words))
    bags = [w.bag_words[a:b].tolist() for a, b in zip(w.bag_offsets, ends)]
    bags[Q_TRAIN + 1] = []
    w.bag_words = np.asarray([x for b in bags for x in b], np.int64)
    w.bag_offsets = np.cumsum([0] + [len(b) for b in bags[:-1]]).astype(np.int64)
    return w, bags


def dataset(w, pairwise=False):
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.Graph import Pps2DGraph, PpsHyperGraph
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples,
                                    graph_type=Pps2DGraph if pairwise else PpsHyperGraph, device=dev())


def model(ds, kind, order, emb, layers=2, seed=3):
    from ihgnn_amd.Models import GCNLayer, HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    torch.manual_seed(seed)
    m = RawGnn(dev(), ds, emb, {'ihgnn': IHGNNLayer, 'hgcn': HGCNLayer, 'gcn': GCNLayer}[kind], layers, order, False, HemPredictionLayer, LAM).to(dev())
    with torch.no_grad():
        m.save_features_for_test()
    return m


def flat(bags):
    return np.asarray([x for b in bags for x in b], np.int64), np.cumsum([0] + [len(b) for b in bags[:-1]]).astype(np.int64)


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize('transform', ['mean', 'activation'])
@pytest.mark.parametrize('compact', ['0', '1'])
@pytest.mark.parametrize('kind,order', [('ihgnn', 1), ('ihgnn', 3), ('hgcn', 1), ('gcn', 1)])
def test_unseen_query_equals_an_isolated_query_node(kind, order, compact, transform, monkeypatch):
    """``search`` by the bags of the dataset's interaction-free queries == ``top_items`` by their indices, bitwise, at emb 32 and at 96 (computed at 128), both heads,
    k = 10 (``top_items`` answers from ``ihg_score_topk``) and k = 50 (from ``ihg_score_topk_deep``)."""
    from ihgnn_amd import layout as layout_mod
    monkeypatch.setattr(layout_mod, 'COMPACT_NODES', compact)
    w, bags = workload()
    extra = list(range(Q_TRAIN, Q_TRAIN + EXTRA))
    pairs = [(c % U, extra[c % EXTRA]) for c in range(2 * EXTRA + 1)]
    users, queries = (torch.tensor(v, dtype=torch.int64) for v in zip(*pairs))
    words, offsets = flat([bags[q] for q in queries.tolist()])
    for emb in (32, 96):
        with settings(transform):
            ds = dataset(w, pairwise=kind == 'gcn')
            m = model(ds, kind, order, emb)
        if kind != 'gcn':
            assert bool(getattr(ds.hypergraph.layout, 'compact', False)) == (compact == '1')
        assert m.compute_width == (32 if emb == 32 else 128) and m._saved_output_feature.shape[1] == 3 * emb
        assert float(m._saved_output_feature[U + Q_TRAIN:U + Q_TRAIN + EXTRA, emb:].abs().max()) == 0.0      # isolated: zero above layer 0 (what the feature rests on)
        for cosine in (False, True):
            with settings(transform, cosine):
                for k in (10, 50):
                    got = m.search(users, words=words, offsets=offsets, k=k)
                    want = m.top_items(users, queries, k)
                    assert tuple(got[0].shape) == (len(pairs), k) and same_bits(got, want), f'{kind} order {order} emb {emb} compact {compact} {transform} cosine {cosine} k {k}'


def test_search_without_cached_features_and_k_beyond_the_catalogue():
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    users, queries = torch.tensor([1, 2, 3]), torch.tensor([Q_TRAIN, Q_TRAIN + 1, Q_TRAIN + 3])
    words, offsets = flat([bags[q] for q in queries.tolist()])
    cached = m.search(users, words=words, offsets=offsets, k=128)
    assert tuple(cached[0].shape) == (3, I) and same_bits(cached, m.top_items(users, queries, 128))          # k is capped at item_count
    m.clear_saved_feature()
    assert same_bits(m.search(users, words=words, offsets=offsets, k=128), cached)
    with pytest.raises(ValueError):
        m.search(users, words=words, offsets=offsets, k=129)
    with pytest.raises(ValueError):
        m.search(torch.tensor([1, 2, U]), words=words, offsets=offsets)


@pytest.mark.parametrize('transform', ['mean', 'activation'])
def test_training_query_by_its_own_bag(transform):
    """A bag that equals a training query's words: its layer-0 row IS that query's X0 row, bit for bit, and it is scored as an unseen query all the same - the float64
    reference of 'that query with zero rows above layer 0' within the bound - which is NOT what ``top_items`` returns for the query."""
    w, bags = workload()
    with settings(transform):
        ds = dataset(w)
        m = model(ds, 'ihgnn', 3, 32)
        f = m._saved_output_feature
        qs = [0, 5, Q_TRAIN - 1]
        words, offsets = flat([bags[q] for q in qs])
        rows = m.embeddings.embed_bags(words, offsets).detach()
        assert torch.equal(rows.view(torch.int32), f[U + torch.tensor(qs, device=f.device), :32].contiguous().view(torch.int32))
        users = torch.tensor([0, 7, 9])
        for cosine in (False, True):
            with settings(transform, cosine):
                got = m.search(users, words=words, offsets=offsets, k=20)
                base = S.case_from_features('own bag', f, users, torch.tensor(qs), U, U + Q_TRAIN + EXTRA, m.prediction_layer.items_bias, LAM)
                case = S.SearchCase(base, ext=rows.cpu().numpy())
                S.masked_float_verdict(got[1], got[0], case, 20, cosine, f'own bag {transform} cosine {cosine}')
                seen = m.top_items(users, torch.tensor(qs), 20)
                assert not torch.equal(got[1], seen[1])                     # the trained query has rows above layer 0


@pytest.mark.parametrize('cosine', [False, True])
def test_anonymous_users_against_the_head_without_a_user(cosine):
    """``users = -1``: ``HemPredictionLayer.forward(None, q, items)`` (``PredictionLayers.py:25``: ``mixed = query_feature``) restated in float64 on dense scores."""
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'hgcn', 1, 32)
    f = m._saved_output_feature.double().cpu()
    bias = m.prediction_layer.items_bias.detach().double().cpu()
    users = torch.tensor([-1, 4, -1, -1, 11, -1, 0, -1])
    queries = torch.tensor([0, 3, Q_TRAIN, 7, 2, Q_TRAIN + 1, 9, 11])
    items = f[U + Q_TRAIN + EXTRA:]
    q = f[U + queries]
    mixed = torch.where((users < 0)[:, None], q, LAM * q + (1 - LAM) * f[users.clamp_min(0)])
    dense = (torch.cosine_similarity(items[None, :, :], mixed[:, None, :], dim=2, eps=1e-8) if cosine else mixed @ items.t()) + bias
    base = S.case_from_features('anonymous', f, users.clamp_min(0), queries, U, U + Q_TRAIN + EXTRA, bias, LAM)
    case = S.SearchCase(base, anon=(users < 0).numpy())
    assert torch.allclose(case.scores64(cosine), dense, rtol=1e-12, atol=1e-12)
    with settings('mean', cosine):
        for k in (10, 90):
            got = m.search(users, queries=queries, k=k)
            S.masked_float_verdict(got[1], got[0], case, k, cosine, f'anonymous cosine {cosine} k {k}')
        # by words: the anonymous user of an unseen query
        words, offsets = flat([bags[Q_TRAIN], bags[Q_TRAIN + 1]])
        got = m.search(torch.tensor([-1, -1]), words=words, offsets=offsets, k=10)
        want = m.search(torch.tensor([-1, -1]), queries=torch.tensor([Q_TRAIN, Q_TRAIN + 1]), k=10)
        assert same_bits(got, want)


@pytest.mark.parametrize('cosine', [False, True])
def test_candidates_as_mask_and_as_ids_and_against_the_filtered_ranking(cosine):
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    users, queries = torch.tensor([0, 1, 2, 3, 4]), torch.tensor([0, 1, 2, Q_TRAIN, 5])
    rng = np.random.default_rng(2)
    with settings('mean', cosine):
        full = m.top_items(users, queries, I)                              # I = 90 <= 128: every item ranked
        for mask in (rng.random(I) < 0.3, S.mask_pattern('last_partial_word', I), S.mask_pattern('none', I), S.mask_pattern('all', I)):
            ids = torch.from_numpy(np.flatnonzero(mask)[::-1].copy())
            for k in (10, 40):
                by_mask = m.search(users, queries=queries, k=k, candidates=torch.from_numpy(mask))
                by_ids = m.search(users, queries=queries, k=k, candidates=ids.to(dev()))
                assert same_bits(by_mask, by_ids)
                want_s, want_i = S.filtered_prefix(full[1], full[0], mask, k)
                assert torch.equal(by_mask[0].cpu(), want_i) and torch.equal(by_mask[1].cpu().view(torch.int32), want_s.view(torch.int32))
        with pytest.raises(ValueError):
            m.search(users, queries=queries, candidates=torch.tensor([0, I]))


def test_self_connections_are_refused():
    from ihgnn_amd.Helpers.Graph import Pps2DGraph
    w, bags = workload()
    ds = dataset(w, pairwise=True)
    ds._graph2d = Pps2DGraph.from_triples(ds.pos_triples, ds.node_count, ds.user_count, ds.query_count, True, dev())
    m = model(ds, 'gcn', 1, 32)
    assert float(m._saved_output_feature[U + Q_TRAIN, 32:].abs().max()) > 0   # an isolated node's layer outputs are NOT zero here
    with pytest.raises(NotImplementedError):
        m.search(torch.tensor([0]), queries=torch.tensor([0]))


def test_command_line_prints_the_models_ranking(tmp_path):
    """``python -m ihgnn_amd.Search`` in a fresh child process on a written dataset and a saved checkpoint: its lines are ``model.search``'s ranking."""
    from ihgnn_amd import Search, synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    w, bags = workload()
    paths = synth.write_files(w, str(tmp_path / 'Data' / 'tiny'))
    ds = GraphDataset(paths['fn_graph_info'], paths['fn_queries_multihot'], paths['fn_train_data'], PpsHyperGraph, 10, 0, dev())
    torch.manual_seed(1)
    m = RawGnn(dev(), ds, 32, IHGNNLayer, 1, 3, False, HemPredictionLayer, Gs.lambda_muq_for_hem).to(dev())
    checkpoint = tmp_path / 'checkpoint_test'
    torch.save({'model': m.state_dict(), 'epoch_count': 0}, str(checkpoint))
    (tmp_path / 'candidates.txt').write_text('\n'.join(str(i) for i in range(0, I, 3)) + '\n')
    searches = [(3, [1, 2, 5]), (-1, [7]), (0, []), (-1, bags[0]), (39, [29, 0, 0])]
    text = ''.join(f'{u}\t{" ".join(map(str, ws))}\n' for u, ws in searches)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for extra, candidates in ((['--candidates', str(tmp_path / 'candidates.txt'), '--cosine'], torch.arange(0, I, 3)),):     # one child process: both flags at once
        done = subprocess.run([sys.executable, '-m', 'ihgnn_amd.Search', '--ds', 'tiny', '--gnn', 'IHGNN', '--gnns', '1', '--fo', '3', '--emb', '32', '--device', '0',
                               '--cp', str(checkpoint), '--k', '7'] + extra, input=text, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
        assert done.returncode == 0, done.stderr[-2000:]
        words, offsets = flat([ws for _, ws in searches])
        with settings('mean', bool(extra)), torch.no_grad():
            m.save_features_for_test()
            items, scores = m.search(torch.tensor([u for u, _ in searches]), words=words, offsets=offsets, k=7, candidates=candidates)
            m.clear_saved_feature()
        want = [Search.format_answer(a, b) for a, b in zip(items.cpu().tolist(), scores.cpu().tolist())]
        assert done.stdout.splitlines() == want and all(len(line.split()) == 7 for line in want)
