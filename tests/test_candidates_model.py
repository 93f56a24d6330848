"""Per-search candidate lists through the model on the GPU: ``RawGnn.search(candidate_lists=)``, ``RawGnn.top_items(candidate_lists=)``, ``RawGnn.score_candidates``, the
evaluation loop under ``Gs.Evaluation.sampled_candidates`` and ``python -m ihgnn_amd.Search --shortlists``.  The list kernels sum in plain float32, so their scores are
not the bits of the whole-catalogue kernels: every ranking here is held against a float64 restatement over ``propagate()``'s own feature matrix
(``tests/candidates_reference.py``: the derived per-score bound, per-search ``allowed``), and a call WITHOUT the keyword is held bitwise against ``ops.search_topk``."""
import io
import types

import numpy as np
import pytest
import torch

import candidates_reference as CR
import search_reference as S
from test_exclude_model import _logs, seen_mask
from test_search_model import I, LAM, Q_TRAIN, EXTRA, U, dataset, dev, flat, model, same_bits, settings, workload

pytestmark = pytest.mark.gpu
ITEM_ROW0 = U + Q_TRAIN + EXTRA


def raw_lists(n, seed, longest=2 * I):
    """Raw shortlists: any order, repeats; every fourth empty, one of every item, one of a single item."""
    rng = np.random.default_rng(seed)
    runs = [[] if c % 4 == 3 else rng.integers(0, I, size=int(rng.integers(1, longest))).tolist() for c in range(n)]
    runs[0] = list(range(I - 1, -1, -1))
    if n > 1:
        runs[1] = [I - 1, I - 1]
    return runs, (torch.from_numpy(np.cumsum([0] + [len(r) for r in runs]).astype(np.int64)), torch.from_numpy(np.asarray([i for r in runs for i in r], np.int64)))


@pytest.mark.parametrize('cosine', [False, True])
def test_search_with_shortlists_against_the_float64_restatement(cosine):
    """By query index and by words, with anonymous users, with ``candidates=`` and ``exclude_seen=True`` besides, at k = 10 and k = 90, raw lists on the host and on the
    device and prepared lists: the float verdict under the derived bound, and one ranking whichever way the lists arrive."""
    from ihgnn_amd import ops
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    f = m._saved_output_feature
    ptr, seen = ds.user_item_lists
    busiest = int(np.argmax(np.diff(ptr)))
    n = 37
    users = torch.arange(n) % U
    users[[2, 9]] = -1
    users[4] = busiest
    queries = torch.arange(n) % Q_TRAIN
    runs, lists = raw_lists(n, seed=2)
    some = np.random.default_rng(4).random(I) < 0.6
    words, offsets = flat([bags[q] for q in queries.tolist()])
    anon = (users < 0).numpy()
    base = S.case_from_features('shortlists', f, torch.where(users < 0, 0, users), queries, U, ITEM_ROW0, m.prediction_layer.items_bias, LAM)
    with settings('mean', cosine):
        ext = m.embeddings.embed_bags(words, offsets).detach().float().cpu().numpy()
        for k in (10, 90):
            for by_words in (False, True):
                how = dict(words=words, offsets=offsets) if by_words else dict(queries=queries)
                for candidates, exclude_seen in ((None, False), (some, False), (None, True), (some, True)):
                    excl = [seen[ptr[u]:ptr[u + 1]] if exclude_seen and u >= 0 else [] for u in users.tolist()]
                    case = CR.CandidateCase(base, runs, lists=excl, ext=ext if by_words else None, anon=anon, mask=candidates)
                    got = m.search(users, k=k, candidate_lists=lists, candidates=None if candidates is None else torch.from_numpy(candidates), exclude_seen=exclude_seen, **how)
                    what = f'search(candidate_lists=) k {k} cosine {cosine} words {by_words} candidates {candidates is not None} exclude_seen {exclude_seen}'
                    assert 0 < CR.float_verdict(got[1], got[0], case, k, cosine, what) <= 1
            got = m.search(users, queries=queries, k=k, candidate_lists=lists)
            assert same_bits(got, m.search(users, queries=queries, k=k, candidate_lists=(lists[0].to(dev()), lists[1].to(dev()))))
            assert same_bits(got, m.search(users, queries=queries, k=k, candidate_lists=ops.candidate_lists(lists[0], lists[1], I)))
            assert same_bits(got, m.search(users, queries=queries, k=k, candidate_lists=(lists[0].numpy(), lists[1].numpy())))
            assert got[0][0].tolist()[:min(k, I)] != [-1] * min(k, I) and got[0][1].tolist() == [I - 1] + [-1] * (k - 1) and bool((got[0][3] == -1).all())
            explicit = (torch.tensor([0, 2] + [2] * (n - 1)), torch.tensor([0, I - 1]))
            both = m.search(users, queries=queries, k=k, candidate_lists=lists, exclude=explicit)
            assert I - 1 not in both[0][0].tolist() and 0 not in both[0][0].tolist() and same_bits((both[0][1:], both[1][1:]), (got[0][1:], got[1][1:]))
        with pytest.raises(ValueError, match='candidate'):
            m.search(users, queries=queries, candidate_lists=(lists[0][:-1], lists[1]))
        with pytest.raises(ValueError, match='candidate'):
            m.search(users, queries=queries, candidate_lists=(torch.tensor([0] * n + [1]), torch.tensor([I])))
        with pytest.raises(ValueError, match='return_list_scores'):
            m.search(users, queries=queries, return_list_scores=True)


@pytest.mark.parametrize('cosine', [False, True])
def test_top_items_and_score_candidates_against_the_restatement(cosine):
    from ihgnn_amd import ops
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'hgcn', 1, 32)
    f = m._saved_output_feature
    n = 33
    users, queries = torch.arange(n) % U, torch.arange(n) % Q_TRAIN
    runs, lists = raw_lists(n, seed=6)
    base = S.case_from_features('lists', f, users, queries, U, ITEM_ROW0, m.prediction_layer.items_bias, LAM)
    with settings('mean', cosine):
        case = CR.CandidateCase(base, runs)
        for k in (10, 50):
            got = m.top_items(users, queries, k, candidate_lists=lists)
            CR.float_verdict(got[1], got[0], case, k, cosine, f'top_items(candidate_lists=) k {k} cosine {cosine}')
            assert same_bits(got, m.search(users, queries=queries, k=k, candidate_lists=lists))
        excl = [[] if c % 2 else runs[c][:3] for c in range(n)]
        excl_lists = (torch.from_numpy(np.cumsum([0] + [len(r) for r in excl]).astype(np.int64)), torch.tensor([i for r in excl for i in r], dtype=torch.int64))
        got = m.top_items(users, queries, 10, candidate_lists=lists, exclude=excl_lists)
        CR.float_verdict(got[1], got[0], CR.CandidateCase(base, runs, lists=excl), 10, cosine, f'top_items(candidate_lists=, exclude=) cosine {cosine}')
        ptr, items, scores = m.score_candidates(users, queries=queries, candidate_lists=lists)
        want_ptr, want_items, total = case.cand_csr()
        assert ptr.cpu().tolist() == want_ptr.tolist() and items.dtype == torch.int32 and items.cpu().tolist() == want_items[:total].tolist() and scores.dtype == torch.float32
        assert 0 < CR.all_scores_verdict(scores, case, cosine, f'score_candidates cosine {cosine}') <= 1
        top = m.search(users, queries=queries, k=50, candidate_lists=lists)
        ranked = CR.ranking_of_floats(scores, case, 50)
        assert torch.equal(top[1].cpu().view(torch.int32), ranked[0].view(torch.int32)) and torch.equal(top[0].cpu(), ranked[1])     # the ranking is that of these very floats
        by_words = m.score_candidates(users[:3], words=np.asarray(bags[Q_TRAIN] + bags[Q_TRAIN + 2], np.int64), offsets=np.asarray([0, len(bags[Q_TRAIN]), len(bags[Q_TRAIN])], np.int64),
                                      candidate_lists=(lists[0][:4], lists[1][:int(lists[0][3])]))
        assert by_words[0].numel() == 4 and by_words[2].numel() == int(by_words[0][-1]) == by_words[1].numel()


@pytest.mark.parametrize('cosine', [False, True])
def test_without_the_keyword_the_call_is_the_whole_catalogue_one(cosine):
    """``search`` without ``candidate_lists`` returns the bits of ``ops.search_topk`` called directly, with and without a mask and ``exclude_seen``; ``top_items``
    those of ``ops.score_topk``."""
    from ihgnn_amd import ops
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    f, head = m._saved_output_feature, m.prediction_layer
    users, queries = torch.tensor([0, -1, 5, 7, 39, -1, 12]), torch.tensor([0, 1, 2, 3, 4, 5, 6])
    some = torch.from_numpy(np.random.default_rng(4).random(I) < 0.5)
    with settings('mean', cosine):
        for k in (10, 40):
            for candidates in (None, some):
                want = ops.search_topk(f, users, U, ITEM_ROW0, head.items_bias, head.lambda_muq, k, queries=queries, candidates=candidates, cosine=cosine)
                assert same_bits(m.search(users, queries=queries, k=k, candidates=candidates), want[:2])
                want = ops.search_topk(f, users, U, ITEM_ROW0, head.items_bias, head.lambda_muq, k, queries=queries, candidates=candidates, cosine=cosine,
                                       exclude=ds.user_item_lists_on(dev()), exclude_rows=users)
                assert same_bits(m.search(users, queries=queries, k=k, candidates=candidates, exclude_seen=True), want[:2])
            plain = torch.tensor([0, 3, 5, 7, 39, 2, 12])
            assert same_bits(m.top_items(plain, queries, k), ops.score_topk(f, plain, queries, U, ITEM_ROW0, head.items_bias, head.lambda_muq, k, cosine=cosine))


def _float64_rankings(m, ds, logs, sets, k, cosine, filter_seen):
    """Per log the float64 ranking of its set (minus, under ``filter_seen``, its user's training items that are not its own positives), and the proof that the list
    kernels' float32 ranking can only be this one: every gap between neighbours among the first ``k + 1`` ranks exceeds the two scores' bounds together."""
    f = m._saved_output_feature
    users = torch.tensor([log[0] for log in logs])
    queries = torch.tensor([log[1] for log in logs])
    base = S.case_from_features('logs', f, users, queries, U, ITEM_ROW0, m.prediction_layer.items_bias, LAM)
    excl = None
    if filter_seen:
        ptr, seen = ds.user_item_lists
        excl = [[int(x) for x in seen[ptr[log[0]]:ptr[log[0] + 1]] if int(x) not in set(log[2])] for log in logs]
    case = CR.CandidateCase(base, sets, lists=excl)
    s64, bound, allowed = case.scores64(cosine).numpy(), CR.score_bound(case, cosine), case.allowed()
    rankings = []
    for c in range(len(logs)):
        ids = np.flatnonzero(allowed[c])
        order = ids[np.lexsort((ids, -s64[c, ids]))][:k + 1]
        gaps = s64[c, order[:-1]] - s64[c, order[1:]]
        assert np.all(gaps > bound[c, order[:-1]] + bound[c, order[1:]]), f'log {c}: a float64 gap among the first {k + 1} ranks is inside the bounds - choose another seed'
        rankings.append(order[:k].tolist() + [-1] * (k - len(order[:k])))
    return rankings


@pytest.mark.parametrize('cosine', [False, True])
@pytest.mark.parametrize('cutoffs', [(), (20, 50)])
def test_sampled_evaluation_equals_the_float64_ranking_of_each_logs_set(cutoffs, cosine, monkeypatch):
    """``test_and_get_avg_metrics`` under ``Gs.Evaluation.sampled_candidates = 30``: the averages equal ``Metrics.at_cutoffs`` over the float64 ranking of each log's own
    set - exactly, because on this fixture no float64 gap at or above a cutoff is inside the bounds (asserted); two evaluations give identical lines; ``filter_seen``
    composes; without the setting the averages are those of plain ``top_items``."""
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.IOHelper import IOHelper
    from ihgnn_amd.Helpers.Metrics import Metrics
    from ihgnn_amd.Helpers.TrainTestHelper import sampled_candidate_set, test_and_get_avg_metrics as evaluate
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    logs = _logs(ds)
    loader = types.SimpleNamespace(logs=logs, device=dev())
    k = max((10,) + cutoffs)
    drawn = 30
    sets = [sampled_candidate_set(i, log[2], I, drawn, 0) for i, log in enumerate(logs)]
    assert all(len(s) == drawn + len(log[2]) and set(log[2]) <= set(s.tolist()) for s, log in zip(sets, logs))

    def triple(x):
        return [x.HitRatio_at10, x.NDCG_at10, x.MAP_at10] + [v for c in cutoffs for v in x.extra[c]]

    def average(rankings):
        total = Metrics()
        for row, (u, q, positives, flags, all_1) in zip(rankings, logs):
            total.add_to_self(Metrics.at_cutoffs(row, positives, flags, all_1, cutoffs))
        return total.divide_and_get_new(len(logs))

    printed = []
    old = (Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs, Gs.Evaluation.sampled_candidates, Gs.Evaluation.candidate_seed, Gs.Prediction.use_cosine_similarity)
    monkeypatch.setattr(IOHelper, 'LogPrint', staticmethod(lambda *a, **kw: printed.append(' '.join(str(x) for x in a))))
    try:
        Gs.Evaluation.extra_cutoffs, Gs.Prediction.use_cosine_similarity, Gs.Evaluation.candidate_seed = cutoffs, cosine, 0
        Gs.Evaluation.sampled_candidates = drawn
        _, sampled, _ = evaluate(m, ds, loader)
        first = list(printed)
        del printed[:]
        _, again, _ = evaluate(m, ds, loader)
        metric_lines = lambda lines: [line for line in lines if 'evaluation done' not in line]      # (the first line carries the seconds)
        assert metric_lines(first) == metric_lines(printed) and triple(sampled) == triple(again)
        assert any(f'each ranked among its own items and {drawn} sampled ones' in line for line in first)
        Gs.Evaluation.filter_seen = True
        _, both, _ = evaluate(m, ds, loader)
        Gs.Evaluation.filter_seen = False
        Gs.Evaluation.sampled_candidates = 0
        del printed[:]
        _, plain, _ = evaluate(m, ds, loader)
        assert not any('sampled' in line for line in printed)
        Gs.Evaluation.sampled_candidates = I
        with pytest.raises(ValueError, match='sampled_candidates'):
            evaluate(m, ds, loader)
    finally:
        Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs, Gs.Evaluation.sampled_candidates, Gs.Evaluation.candidate_seed, Gs.Prediction.use_cosine_similarity = old
    with torch.no_grad(), settings('mean', cosine):
        m.save_features_for_test()
        want_sampled = average(_float64_rankings(m, ds, logs, sets, k, cosine, False))
        want_both = average(_float64_rankings(m, ds, logs, sets, k, cosine, True))
        want_plain = average([m.top_items(torch.tensor([u]), torch.tensor([q]), k)[0][0].tolist() for u, q, *_ in logs])
    assert triple(sampled) == pytest.approx(triple(want_sampled), rel=1e-12, abs=0)
    assert triple(both) == pytest.approx(triple(want_both), rel=1e-12, abs=0)
    assert triple(plain) == pytest.approx(triple(want_plain), rel=1e-12, abs=0)
    assert triple(sampled) != triple(plain) and sampled.HitRatio_at10 >= plain.HitRatio_at10     # (a positive among 30 drawn items ranks no lower than among all 90)


def test_srrl_refuses_sampled_evaluation():
    from ihgnn_amd import Main
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    with pytest.raises(NotImplementedError, match='eval_candidates'):
        Main.check_srrl_settings(parse_args(['--model', 'Srrl', '--eval_candidates', '99']), 1)


def test_search_command_line_with_shortlists(tmp_path, monkeypatch):
    """``Search.main(['--shortlists', ...], lines=, out=)`` on three lines, one of them with an empty shortlist: its lines are ``model.search(candidate_lists=)``'s
    ranking, every answer inside its line's shortlist; ``--exclude_seen`` composes."""
    from ihgnn_amd import Search, synth
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Graph import PpsHyperGraph
    from ihgnn_amd.Helpers.IOHelper import IOHelper
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    w, bags = workload()
    paths = synth.write_files(w, str(tmp_path / 'Data' / 'tiny'))
    ds = GraphDataset(paths['fn_graph_info'], paths['fn_queries_multihot'], paths['fn_train_data'], PpsHyperGraph, 10, 0, dev())
    torch.manual_seed(1)
    m = RawGnn(dev(), ds, 32, IHGNNLayer, 1, 3, False, HemPredictionLayer, Gs.lambda_muq_for_hem).to(dev())
    checkpoint = tmp_path / 'checkpoint_test'
    torch.save({'model': m.state_dict(), 'epoch_count': 0}, str(checkpoint))
    ptr, seen = ds.user_item_lists
    busiest = int(np.argmax(np.diff(ptr)))
    mine = seen[ptr[busiest]:ptr[busiest + 1]].tolist()
    searches = [(busiest, [1, 2, 5], mine[:3] + [0, 89, 44, 44, 17]), (-1, [7], []), (3, bags[0], list(range(40, 10, -1)))]
    lines = [f'{u}\t{" ".join(map(str, ws))}\t{" ".join(map(str, ids))}\n' for u, ws, ids in searches]
    argv = ['--ds', 'tiny', '--gnn', 'IHGNN', '--gnns', '1', '--fo', '3', '--emb', '32', '--device', '0', '--cp', str(checkpoint), '--k', '20', '--shortlists']
    monkeypatch.chdir(tmp_path)
    for holder, name in ((Gs, 'embedding_size'), (Gs, 'graph_completeness'), (IOHelper, 'quiet')):       # what Search.build_model assigns, put back after the test
        monkeypatch.setattr(holder, name, getattr(holder, name))
    with settings('mean', False):
        out, unseen = io.StringIO(), io.StringIO()
        assert Search.main(argv, lines=lines, out=out) == 0 and Search.main(argv + ['--exclude_seen'], lines=lines, out=unseen) == 0
        words, offsets = flat([ws for _, ws, _ in searches])
        shortlists = (np.cumsum([0] + [len(ids) for *_, ids in searches]), np.asarray([i for *_, ids in searches for i in ids], np.int64))
        with torch.no_grad():
            m.save_features_for_test()
            items, scores = m.search(torch.tensor([u for u, *_ in searches]), words=words, offsets=offsets, k=20, candidate_lists=shortlists)
            m.clear_saved_feature()
    want = [Search.format_answer(a, b) for a, b in zip(items.cpu().tolist(), scores.cpu().tolist())]
    got, filtered = out.getvalue().splitlines(), unseen.getvalue().splitlines()
    assert got == want and got[1] == '' and len(got) == 3
    answered = [[int(pair.split(':')[0]) for pair in line.split()] for line in got]
    assert sorted(answered[0]) == sorted(set(searches[0][2])) and answered[1] == []
    assert set(answered[2]) <= set(range(11, 41)) and len(answered[2]) == 20
    kept = [int(pair.split(':')[0]) for pair in filtered[0].split()]
    assert sorted(kept) == sorted(set(searches[0][2]) - set(mine)) and filtered[1] == ''
