"""GPU: rankings deeper than ten - ``ihg_score_topk_deep`` (csrc/eval.hip: the deep instantiations of ``score_topk_kernel`` + ``merge_deep_kernel``),
``ops.score_topk_deep`` / ``ops.score_topk`` with k > 10, ``RawGnn.top_items(u, q, k)`` and the evaluation loop with ``Gs.Evaluation.extra_cutoffs`` - against float64
scores and a stable descending sort (``tests/topk_reference.py``), against exactly known rankings, and against the k <= 10 entry points bit for bit.

Bar: RTOL = 1e-5 of the reference scores' largest magnitude, as ``tests/test_gpu_parity.py::test_score_topk_matches_oracle``."""
import math

import numpy as np
import pytest
import torch

import topk_reference as tref

pytestmark = pytest.mark.gpu

RTOL = 1e-5
U, Q = 50, 20


def dev():
    return torch.device('cuda:0')


def rel(a, b):
    a, b = (x.detach().cpu().double().numpy() for x in (a, b))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def draw(dim, n_items, n_pairs):
    gen = torch.Generator().manual_seed(dim + n_items)
    feats = torch.randn(U + Q + n_items, dim, generator=gen) / np.sqrt(dim)
    bias = torch.randn(n_items, generator=gen)
    users = torch.randint(0, U, (n_pairs,), generator=gen)
    queries = torch.randint(0, Q, (n_pairs,), generator=gen)
    return feats, bias, users, queries


def deep(feats, users, queries, bias, k, cosine=False):
    from ihgnn_amd import ops
    return ops.score_topk_deep(feats.to(dev()), users.to(dev()), queries.to(dev()), U, U + Q, bias.to(dev()), 0.5, k, cosine=cosine)


def pass_bound(k, n_items):
    return math.ceil(min(k, n_items) / 10)


# ---------------------------------------------------------------------------------------------
# 1: against float64
# ---------------------------------------------------------------------------------------------
def check_against_float64(dim, n_items, n_pairs, cosine):
    feats, bias, users, queries = draw(dim, n_items, n_pairs)
    want = tref.all_item_scores(feats, users, queries, U, U + Q, bias, 0.5, cosine)                   # once for the three depths
    for k in (11, 50, 128):
        items, scores, passes = deep(feats, users, queries, bias, k, cosine)
        items, scores, passes = items.cpu().long(), scores.cpu(), passes.cpu()
        assert tuple(items.shape) == tuple(scores.shape) == (n_pairs, k)
        kk = min(k, n_items)
        assert (items[:, kk:] == -1).all()                                                            # fewer items than k: the tail of ihg_score_topk
        assert 1 <= passes.min().item() and passes.max().item() <= pass_bound(k, n_items), passes
        for c in range(n_pairs):
            order = tref.ranking(want[c], kk)
            got, got_scores = items[c, :kk], scores[c, :kk]
            assert rel(got_scores, want[c][order]) <= RTOL
            assert rel(want[c][got], want[c][order]) <= RTOL                                          # the kernel's items ARE the best k (up to fp32 near-ties)
            assert len(set(got.tolist())) == kk and got.min().item() >= 0 and got.max().item() < n_items
            gap = (want[c][order][:-1] - want[c][order][1:]).abs().min().item() if kk > 1 else 1.0
            if gap > 1e-4 * want[c].abs().max().item():                                               # no near-tie among the top k: same items in the same order
                assert got.tolist() == order.tolist()
    return passes


@pytest.mark.parametrize('dim,n_items,n_pairs', [(64, 257, 5), (64, 4100, 5), (128, 7, 3), (36, 31, 40), (192, 70001, 3), (1264, 530, 37), (625, 300, 70), (624, 300, 70)])
def test_deep_topk_matches_float64(dim, n_items, n_pairs):
    """16 lists with k > 10 x lists / 2 (a second pass on random data, asserted); several item slices with items off the 32-tile; fewer items than k (-1 tail); pairs
    off the block; 1,024 lists (the merge's largest candidate set); one pair tile (1264, 625) and two (624)."""
    passes = check_against_float64(dim, n_items, n_pairs, False)
    if (dim, n_items) == (64, 257):
        assert passes.max().item() > 1                                                                # (k = 128, the last depth run)


@pytest.mark.parametrize('dim,n_items,n_pairs', [(64, 257, 5), (625, 300, 70)])
def test_deep_topk_cosine_matches_float64(dim, n_items, n_pairs):
    check_against_float64(dim, n_items, n_pairs, True)


# ---------------------------------------------------------------------------------------------
# 2: exact and adversarial - zero user and query rows: every accumulator is 0 and score == bias exactly, under either head
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cosine', [False, True])
@pytest.mark.parametrize('n_items', [4100, 257])
def test_deep_topk_exact_rankings(n_items, cosine):
    k, dim, n_pairs = 128, 64, 5
    feats, _, users, queries = draw(dim, n_items, n_pairs)
    feats[:U + Q] = 0
    ids = torch.arange(n_items, dtype=torch.float32)
    bound = pass_bound(k, n_items)
    # descending in item id: the first k items, every pass finds its winners in the first tiles of the first lists
    items, scores, passes = deep(feats, users, queries, -ids, k, cosine)
    assert items.cpu().tolist() == [list(range(k))] * n_pairs
    assert torch.equal(scores.cpu(), (-ids[:k]).expand(n_pairs, k))                                   # bit-equal to the bias
    assert 1 < passes.max().item() <= bound
    # ascending: the winners sit in the last, partial tile
    items, scores, passes = deep(feats, users, queries, ids, k, cosine)
    assert items.cpu().tolist() == [list(range(n_items - 1, n_items - 1 - k, -1))] * n_pairs
    assert torch.equal(scores.cpu(), ids[-k:].flip(0).expand(n_pairs, k))
    assert passes.max().item() <= bound
    # constant: everything ties, ascending item id decides
    items, scores, passes = deep(feats, users, queries, torch.full((n_items,), 0.25), k, cosine)
    assert items.cpu().tolist() == [list(range(k))] * n_pairs
    assert (scores.cpu() == 0.25).all()
    assert passes.max().item() <= bound


# ---------------------------------------------------------------------------------------------
# 3: consistency with the k <= 10 entry points, both heads
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cosine', [False, True])
@pytest.mark.parametrize('dim,n_items,n_pairs', [(64, 4100, 37), (700, 300, 70)])
def test_deep_topk_agrees_with_the_top10_entry_points(dim, n_items, n_pairs, cosine):
    from ihgnn_amd import ops
    feats, bias, users, queries = draw(dim, n_items, n_pairs)
    args = (feats.to(dev()), users.to(dev()), queries.to(dev()), U, U + Q, bias.to(dev()), 0.5)
    for k in (10, 3):
        items, scores = ops.score_topk(*args, k, cosine=cosine)
        d_items, d_scores, passes = ops.score_topk_deep(*args, k, cosine=cosine)
        assert torch.equal(items, d_items) and torch.equal(scores.view(torch.int32), d_scores.view(torch.int32))
        assert (passes == 1).all()
    i128, s128, _ = ops.score_topk_deep(*args, 128, cosine=cosine)
    i50, s50, _ = ops.score_topk_deep(*args, 50, cosine=cosine)
    assert torch.equal(i128[:, :50], i50) and torch.equal(s128[:, :50].contiguous().view(torch.int32), s50.view(torch.int32))
    again_i, again_s, _ = ops.score_topk_deep(*args, 128, cosine=cosine)
    assert torch.equal(again_i, i128) and torch.equal(again_s.view(torch.int32), s128.view(torch.int32))
    routed_i, routed_s = ops.score_topk(*args, 50, cosine=cosine)                                       # ops.score_topk with k > 10: the deep call
    assert torch.equal(routed_i, i50) and torch.equal(routed_s.view(torch.int32), s50.view(torch.int32))


def test_deep_topk_in_a_stream_capture():
    """No host read, no allocation by the library, a fixed launch sequence: a recorded call replays with new inputs in place and returns what the eager call returns
    (a case that takes more than one pass)."""
    from ihgnn_amd import ops
    feats, bias, users, queries = draw(64, 257, 5)
    f, b, u, q = feats.to(dev()), bias.to(dev()), users.to(dev()), queries.to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.score_topk_deep(f, u, q, U, U + Q, b, 0.5, 128)                                           # warm-up: allocator, the kernels' LDS attribute
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        items, scores, passes = ops.score_topk_deep(f, u, q, U, U + Q, b, 0.5, 128)
    b.copy_(-torch.arange(257, dtype=torch.float32))                                                  # new inputs, in place: the sorted-bias case
    f[:U + Q] = 0
    graph.replay()
    torch.cuda.synchronize()
    got = (items.clone(), scores.clone(), passes.clone())
    want = ops.score_topk_deep(f, u, q, U, U + Q, b, 0.5, 128)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert got[0].cpu().tolist() == [list(range(128))] * 5 and got[2].max().item() > 1


# ---------------------------------------------------------------------------------------------
# 4: the model
# ---------------------------------------------------------------------------------------------
def build_model(ds, kind, L, order, d):
    from ihgnn_amd.Models import HGCNLayer, HemPredictionLayer, IHGNNLayer, RawGnn
    return RawGnn(dev(), ds, d, IHGNNLayer if kind == 'ihgnn' else HGCNLayer, L, order, False, HemPredictionLayer, 0.5).to(dev())


def test_top_items_ranks_a_hundred():
    """``top_items(u, q, 100)`` against the dense ``score_all_items`` + a stable sort; the profile names the deep call; 129 is refused by name of the limit."""
    from ihgnn_amd import ops, profiler, synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(60, 20, 150, 30, 800, seed=31)
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())
    torch.manual_seed(2)
    m = build_model(ds, 'ihgnn', 2, 3, 50)
    users = torch.arange(40, device=dev()) % w.user_count
    queries = torch.arange(40, device=dev()) % w.query_count
    with torch.no_grad():
        m.save_features_for_test()
        profiler.start()
        items, scores = m.top_items(users, queries, 100)
        profiler.stop()
        assert 'score_topk_deep' in profiler.summary()
        dense = m.score_all_items(users, queries)
        with pytest.raises(ValueError, match=str(ops.score_topk_max_k())):
            m.top_items(users, queries, 129)
        m.clear_saved_feature()
    assert ops.score_topk_max_k() == 128 and tuple(items.shape) == (40, 100)
    order = torch.sort(dense, dim=1, descending=True, stable=True).indices[:, :100]
    assert rel(scores, torch.gather(dense, 1, order)) <= RTOL
    assert rel(torch.gather(dense, 1, items.long()), torch.gather(dense, 1, order)) <= RTOL
    assert all(len(set(row)) == 100 for row in items.tolist())


# ---------------------------------------------------------------------------------------------
# 5: the evaluation loop
# ---------------------------------------------------------------------------------------------
def test_evaluation_with_extra_cutoffs(tmp_path):
    """``test_and_get_avg_metrics`` with cutoffs {20, 100}: one deep ranking per chunk; every cutoff's metrics equal the float64 reference's metrics of the dense
    scores (per log, see below), the averages are their means, and the @10 triple equals, as floats, that of a run without cutoffs."""
    from ihgnn_amd import profiler, synth
    from ihgnn_amd.Dataset import GraphDataset, TestSearchLogDataLoader
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Helpers.Metrics import Metrics
    from ihgnn_amd.Helpers.TrainTestHelper import test_and_get_avg_metrics
    w = synth.draw(80, 25, 120, 30, 900, seed=12, eval_logs=60)
    paths = synth.write_files(w, str(tmp_path))
    ds = GraphDataset(paths['fn_graph_info'], paths['fn_queries_multihot'], paths['fn_train_data'], PpsHyperGraph, 10, 0, dev())
    loader = TestSearchLogDataLoader(paths['fn_test_data'], ds, dev())
    torch.manual_seed(1)
    m = build_model(ds, 'ihgnn', 2, 3, 32)
    assert Gs.Evaluation.extra_cutoffs == ()
    _, plain, _ = test_and_get_avg_metrics(m, ds, loader)
    assert plain.extra == {}
    cutoffs = (20, 100)
    try:
        Gs.Evaluation.extra_cutoffs = cutoffs
        profiler.start()
        _, avg, _ = test_and_get_avg_metrics(m, ds, loader)
        profiler.stop()
        summary = profiler.summary()
    finally:
        Gs.Evaluation.extra_cutoffs = ()
    assert summary['score_topk_deep']['launches'] == 1 and 'score_topk' not in summary                # ONE ranking, at the largest cutoff
    assert (avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10) == (plain.HitRatio_at10, plain.NDCG_at10, plain.MAP_at10)
    assert sorted(avg.extra) == list(cutoffs)
    # per log: the three metrics depend on the ranking only through the ranks of the truth items, and a truth item whose score no other item comes near (1e-4 of the
    # largest score, ten times the bar on the scores) has the same rank in the kernel's ranking and in the float64 sort of the dense scores: on such logs the
    # metrics must be EQUAL at every cutoff.  Truth sets are a few items among 120, so nearly every log is such a log; at least 80 % must be.
    uq = torch.tensor([(lg[0], lg[1]) for lg in loader.logs], device=dev())
    with torch.no_grad():
        m.save_features_for_test()
        items, _ = m.top_items(uq[:, 0], uq[:, 1], 100)
        dense = m.score_all_items(uq[:, 0], uq[:, 1]).cpu().double()
        m.clear_saved_feature()
    items = items.cpu().tolist()
    sums = {c: np.zeros(3) for c in (10,) + cutoffs}
    clear_logs = 0
    for n, (_, _, truth, flags, all1) in enumerate(loader.logs):
        near = 1e-4 * dense[n].abs().max().item()
        clear = True
        for t in truth:
            d = (dense[n] - dense[n][t]).abs()
            d[t] = float('inf')
            clear = clear and d.min().item() > near
        clear_logs += clear
        for c in sums:
            got = Metrics.from_top_indices(items[n], truth, flags, all1, c)
            if clear:
                np.testing.assert_allclose((got.HitRatio_at10, got.NDCG_at10, got.MAP_at10), tref.ranking_metrics(dense[n], truth, None if all1 else flags, c), atol=1e-12)
            sums[c] += (got.HitRatio_at10, got.NDCG_at10, got.MAP_at10)
    print(f'metrics compared on {clear_logs} of {len(loader.logs)} logs')
    assert clear_logs >= 0.8 * len(loader.logs), (clear_logs, len(loader.logs))
    np.testing.assert_allclose((avg.HitRatio_at10, avg.NDCG_at10, avg.MAP_at10), sums[10] / len(loader.logs), atol=1e-9)
    for c in cutoffs:
        np.testing.assert_allclose(avg.extra[c], sums[c] / len(loader.logs), atol=1e-9)
