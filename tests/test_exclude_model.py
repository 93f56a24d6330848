"""Per-search exclusion lists through the model on the GPU: ``RawGnn.search(exclude_seen=)`` / ``(exclude=)``, ``RawGnn.top_items(exclude=)``, the evaluation loop under
``Gs.Evaluation.filter_seen`` and ``python -m ihgnn_amd.Search --exclude_seen``.  Exclusion only removes items from a ranking whose scores it does not touch, so every
verdict but one is BITWISE against a call the parent already had: the same search under the candidate mask ``~seen`` of its user.  ``top_items(exclude=)`` is also held
against the float64 reference of ``tests/exclude_reference.py`` within ``ranking_reference``'s per-score bound."""
import io
import types

import numpy as np
import pytest
import torch

import exclude_reference as E
import search_reference as S
from test_search_model import I, LAM, Q_TRAIN, EXTRA, U, dataset, dev, flat, model, same_bits, settings, workload

pytestmark = pytest.mark.gpu


def seen_mask(ds, user):
    ptr, items = ds.user_item_lists
    mask = np.ones(ds.item_count, bool)
    if user >= 0:
        mask[items[ptr[user]:ptr[user + 1]]] = False
    return mask


@pytest.mark.parametrize('cosine', [False, True])
def test_exclude_seen_equals_the_users_own_candidate_mask(cosine):
    """``search(exclude_seen=True)``: the row of every search equals, bitwise, the one-search call with ``candidates = ~seen`` of its user - by query index and by
    words, with anonymous users (who exclude nothing), with ``candidates`` besides, at k = 10 and at k = 90 = every item (the tail begins where the user's unseen items
    end)."""
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    ptr, _ = ds.user_item_lists
    busiest, idle = int(np.argmax(np.diff(ptr))), int(np.argmin(np.diff(ptr)))
    assert np.diff(ptr)[busiest] > 10 and np.diff(ptr)[idle] == 0         # (a third of the users are in no hyperedge)
    users = torch.tensor([busiest, -1, idle, 3, busiest, 7, -1, 12, 39])
    queries = torch.tensor([0, 1, 2, Q_TRAIN, 5, 6, Q_TRAIN + 1, 8, 9])
    words, offsets = flat([bags[q] for q in queries.tolist()])
    some = torch.from_numpy(np.random.default_rng(4).random(I) < 0.5)
    with settings('mean', cosine):
        for k in (10, 90):
            for how in (dict(queries=queries), dict(words=words, offsets=offsets)):
                for candidates in (None, some):
                    got = m.search(users, k=k, candidates=candidates, exclude_seen=True, **how)
                    for c, user in enumerate(users.tolist()):
                        mask = torch.from_numpy(seen_mask(ds, user)) & (some if candidates is not None else True)
                        one = {key: value[c:c + 1] for key, value in how.items()} if 'queries' in how else dict(words=np.asarray(bags[int(queries[c])], np.int64), offsets=np.zeros(1, np.int64))
                        want = m.search(users[c:c + 1], k=k, candidates=mask, **one)
                        assert same_bits((got[0][c:c + 1], got[1][c:c + 1]), want), f'search {c} (user {user}) k {k} cosine {cosine} {sorted(how)} candidates {candidates is not None}'
                    assert same_bits((got[0][[1, 6]], got[1][[1, 6]]), tuple(t[[1, 6]] for t in m.search(users, k=k, candidates=candidates, **how)))       # nobody logged in
        assert int((m.search(users, queries=queries, k=90, exclude_seen=True)[0][0] >= 0).sum()) == I - int(np.diff(ptr)[busiest])
        with pytest.raises(ValueError):
            m.search(users, queries=queries, exclude_seen=True, exclude=(torch.zeros(10, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
        with pytest.raises(ValueError):
            m.search(users, queries=queries, exclude=(torch.tensor([0] * 9 + [1]), torch.tensor([I])))


@pytest.mark.parametrize('cosine', [False, True])
def test_top_items_with_explicit_lists_against_the_reference(cosine):
    """``top_items(exclude=(offsets, items))`` with raw lists (shuffled, repeats, on the host or on the device): the per-pair float verdict on the model's own feature
    matrix, the bits of ``search(exclude=)``, and rows with an empty list equal ``top_items`` without lists."""
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'hgcn', 1, 32)
    rng = np.random.default_rng(6)
    users, queries = torch.arange(0, 33) % U, torch.arange(0, 33) % Q_TRAIN
    runs = [[] if c % 4 == 0 else rng.integers(0, I, size=int(rng.integers(1, 2 * I))).tolist() for c in range(33)]
    runs[1], runs[2] = list(range(I)), list(range(I - 1, 0, -1))           # every item; every item but item 0
    offsets = torch.from_numpy(np.cumsum([0] + [len(r) for r in runs]).astype(np.int64))
    items = torch.from_numpy(np.asarray([i for r in runs for i in r], np.int64))
    f = m._saved_output_feature
    with settings('mean', cosine):
        for k in (10, 50):
            got = m.top_items(users, queries, k, exclude=(offsets, items))
            base = S.case_from_features('lists', f, users, queries, U, U + Q_TRAIN + EXTRA, m.prediction_layer.items_bias, LAM)
            E.float_verdict(got[1], got[0], E.ExcludeCase(base, runs), k, cosine, f'top_items(exclude=) k {k} cosine {cosine}')
            assert same_bits(got, m.top_items(users, queries, k, exclude=(offsets.to(dev()), items.to(dev()))))
            assert same_bits(got, m.search(users, queries=queries, k=k, exclude=(offsets, items)))
            plain = m.top_items(users, queries, k)
            assert same_bits((got[0][0::4], got[1][0::4]), (plain[0][0::4], plain[1][0::4]))
            assert bool((got[0][1] == -1).all()) and got[0][2].tolist() == [0] + [-1] * (k - 1)


def _logs(ds, n=60, seed=9):
    """Evaluation logs of the trained users: one or two interacted items each, about half of the logs with a positive that the user ALSO has in training."""
    rng = np.random.default_rng(seed)
    ptr, items = ds.user_item_lists
    active = np.flatnonzero(np.diff(ptr) > 0)
    logs = []
    for j in range(n):
        u = int(rng.choice(active))
        positives = [int(rng.integers(0, I))] + ([int(rng.choice(items[ptr[u]:ptr[u + 1]]))] if j % 2 else [])
        logs.append((u, int(rng.integers(0, Q_TRAIN)), sorted(set(positives)), None, True))
    return logs


@pytest.mark.parametrize('cutoffs', [(), (20, 50)])
def test_evaluation_under_filter_seen_equals_per_log_masked_searches(cutoffs):
    """``test_and_get_avg_metrics`` with ``Gs.Evaluation.filter_seen``: the averages equal those of one masked search per log - candidates = every item but the user's
    training items, the log's own positives put back - through the same ``Metrics``; without the flag they equal those of plain ``top_items``, as before."""
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    from ihgnn_amd.Helpers.Metrics import Metrics
    from ihgnn_amd.Helpers.TrainTestHelper import test_and_get_avg_metrics as evaluate
    w, bags = workload()
    ds = dataset(w)
    m = model(ds, 'ihgnn', 3, 32)
    logs = _logs(ds)
    loader = types.SimpleNamespace(logs=logs, device=dev())
    k = max((10,) + cutoffs)

    def average(rank):
        total = Metrics()
        for u, q, positives, flags, all_1 in logs:
            total.add_to_self(Metrics.at_cutoffs(rank(u, q, positives), positives, flags, all_1, cutoffs))
        return total.divide_and_get_new(len(logs))

    def masked(u, q, positives):
        mask = seen_mask(ds, u)
        mask[positives] = True
        return m.search(torch.tensor([u]), queries=torch.tensor([q]), k=k, candidates=torch.from_numpy(mask))[0][0].tolist()

    def triple(x):
        return [x.HitRatio_at10, x.NDCG_at10, x.MAP_at10] + [v for c in cutoffs for v in x.extra[c]]

    old = (Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs)
    try:
        Gs.Evaluation.extra_cutoffs = cutoffs
        Gs.Evaluation.filter_seen = True
        _, filtered, _ = evaluate(m, ds, loader)
        Gs.Evaluation.filter_seen = False
        _, unfiltered, _ = evaluate(m, ds, loader)
    finally:
        Gs.Evaluation.filter_seen, Gs.Evaluation.extra_cutoffs = old
    with torch.no_grad():
        m.save_features_for_test()
        want_filtered = average(masked)
        want_plain = average(lambda u, q, positives: m.top_items(torch.tensor([u]), torch.tensor([q]), k)[0][0].tolist())
    assert triple(filtered) == pytest.approx(triple(want_filtered), rel=1e-12, abs=0)
    assert triple(unfiltered) == pytest.approx(triple(want_plain), rel=1e-12, abs=0)
    assert triple(filtered) != triple(unfiltered)                          # (the protocol matters on this corpus: seen items do rank among the first ten)


def test_search_command_line_with_exclude_seen(tmp_path, monkeypatch):
    """``Search.main(argv, lines=, out=)`` with ``--exclude_seen``: its lines are ``model.search(exclude_seen=True)``'s ranking, and differ from the lines without the
    flag exactly where the user is logged in and has seen one of the items otherwise returned."""
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
    ptr, _ = ds.user_item_lists
    busiest = int(np.argmax(np.diff(ptr)))
    searches = [(busiest, [1, 2, 5]), (-1, [7]), (busiest, []), (-1, bags[0]), (int(np.argmin(np.diff(ptr))), [29, 0, 0])]
    lines = [f'{u}\t{" ".join(map(str, ws))}\n' for u, ws in searches]
    argv = ['--ds', 'tiny', '--gnn', 'IHGNN', '--gnns', '1', '--fo', '3', '--emb', '32', '--device', '0', '--cp', str(checkpoint), '--k', '80']
    monkeypatch.chdir(tmp_path)
    from ihgnn_amd.Helpers.IOHelper import IOHelper
    for holder, name in ((Gs, 'embedding_size'), (Gs, 'graph_completeness'), (IOHelper, 'quiet')):       # what Search.build_model assigns, put back after the test
        monkeypatch.setattr(holder, name, getattr(holder, name))
    with settings('mean', False):
        out, plain = io.StringIO(), io.StringIO()
        assert Search.main(argv + ['--exclude_seen'], lines=lines, out=out) == 0 and Search.main(argv, lines=lines, out=plain) == 0
        words, offsets = flat([ws for _, ws in searches])
        with torch.no_grad():
            m.save_features_for_test()
            items, scores = m.search(torch.tensor([u for u, _ in searches]), words=words, offsets=offsets, k=80, exclude_seen=True)
            m.clear_saved_feature()
    want = [Search.format_answer(a, b) for a, b in zip(items.cpu().tolist(), scores.cpu().tolist())]
    got, before = out.getvalue().splitlines(), plain.getvalue().splitlines()
    assert got == want
    assert [a == b for a, b in zip(got, before)] == [False, True, False, True, True]
    assert [len(line.split()) for line in got] == [min(80, I - int(np.diff(ptr)[u])) if u >= 0 else 80 for u, _ in searches]
