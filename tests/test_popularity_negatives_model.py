"""Popularity-weighted negatives (``GraphDataset(popularity_power=)``, ``--popularity_negatives``) on the GPU: the device loader's negatives against
``ops.sample_pool_weighted`` and the reference stream under the same keys, with and without the users' lists, the rest of the epoch unchanged, the unflagged loader's bits
kept; a two-rank split; the driver with ``--device_sampling --popularity_negatives --filter_negatives --hard_negatives 20 --loss bpr``, eager and recorded."""
import functools

import numpy as np
import pytest
import torch

import hard_negatives_reference as H
import logged_negatives_reference as L
import popularity_negatives_reference as P
from test_filter_negatives_model import BATCH, EPOCH, ITEMS, SEED, own_items, skewed
from test_loss_model import dev

pytestmark = pytest.mark.gpu

ALPHA = 0.75


def dataset(k, power=ALPHA, filtered=False):
    from ihgnn_amd.Dataset import GraphDataset
    w, triples = skewed()                                                    # 50 users, 400 items; user 0 has bought 300 of them, user 1 150
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, triples, random_negative_sample_size=k,
                                    device=dev(), filter_negatives=filtered, popularity_power=power)


def epoch_of(ds, batches=2, rank=0, world=1):
    from ihgnn_amd.Dataset import DeviceBatchLoader
    loader = DeviceBatchLoader(ds, BATCH, rank, world, seed=SEED)
    loader.set_epoch(EPOCH)
    out = []
    for b, batch in enumerate(loader):
        out.append(tuple(t.cpu() for t in batch))
        if b + 1 == batches:
            break
    return out


@functools.lru_cache(maxsize=None)
def host_table():
    """``cum`` on the host from the dataset's own weights, which are the formula of the reference on the item counts."""
    ds = dataset(10)
    counts = np.bincount(ds.pos_triples[:, 2], minlength=ITEMS)
    assert (ds.item_sampling_weights == P.dataset_weights(counts, ALPHA)).all() and ds.item_sampling_weights.max() == 2 ** 32
    return P.cum_of(ds.item_sampling_weights)


@pytest.mark.parametrize('k, filtered', [(10, False), (10, True), (20, False), (20, True)])
def test_device_batches_draw_weighted_negatives(k, filtered):
    """k = 10: the plain count; k = 20: a pool (``negative_pool`` M = 20, drawn weighted).  Both above and below the 16 draws at which the unflagged loader changes kernels."""
    from ihgnn_amd import ops
    plain, flagged_ds = dataset(k, 0.0), dataset(k, ALPHA, filtered)
    ptr, items = flagged_ds.user_item_lists
    cum = host_table()
    table = flagged_ds.item_sampling_table_on(dev())
    assert flagged_ds.item_sampling_table_on(dev()) is table                 # built and copied once
    assert table[1] == int(cum[-1]) and torch.equal(table[0].cpu(), torch.from_numpy(cum.copy()))
    lists = flagged_ds.user_item_lists_on(dev())
    unflagged, flagged = epoch_of(plain), epoch_of(flagged_ds)
    uniform = H.pool_draw if k > 16 else L.sample_negatives
    hits = 0
    for b, (old, new) in enumerate(zip(unflagged, flagged)):
        p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f = new
        n = int(p_u.shape[0])
        # the permutation, the positives and every other tensor are the unflagged epoch's
        for position in (0, 1, 2, 3, 4, 5, 7):
            assert torch.equal(old[position], new[position]), (k, b, position)
        assert torch.equal(n_u, p_u.repeat_interleave(k)) and torch.equal(n_q, p_q.repeat_interleave(k)) and int(n_f.sum()) == 0 and int(p_f.sum()) == n
        key = (SEED * 7919, (EPOCH << 32) + b)
        got = n_i.view(n, k)
        op = ops.sample_pool_weighted(*key, n, ITEMS, k, table, p_u.to(dev()) if filtered else None, lists if filtered else None,
                                      flagged_ds.max_user_items if filtered else 0, device=dev())
        assert torch.equal(got, op.cpu()), (k, b)
        want = P.pool_draw_weighted(*key, n, ITEMS, k, cum, *((p_u.numpy(), ptr, items) if filtered else ()))
        assert torch.equal(got, torch.from_numpy(want.copy())), (k, b)
        assert all(len(set(row)) == k for row in got.tolist()) and int(got.min()) >= 0 and int(got.max()) < ITEMS
        own = int(own_items(ptr, items, p_u, got.numpy()).sum())
        assert own == 0 if filtered else True
        hits += own
        # flag off: today's launches, bit for bit
        assert torch.equal(old[6].view(n, k), torch.from_numpy(uniform(*key, n, ITEMS, k).copy())), (k, b)
    assert filtered or hits > 0                                              # unfiltered, the weighted draw does fall on the users' own items


def test_unflagged_epoch_is_the_parents_launches():
    """``popularity_power = 0``: ``ihg_sample_negatives`` up to 16 draws and ``ihg_sample_pool`` beyond, called directly under the loader's keys."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    for k, name in ((10, 'ihg_sample_negatives'), (16, 'ihg_sample_negatives'), (17, 'ihg_sample_pool'), (50, 'ihg_sample_pool')):
        ds = dataset(k, 0.0)
        assert not {'_item_weights', '_item_cum', '_item_table_device'} & set(ds.__dict__)
        for b, batch in enumerate(epoch_of(ds)):
            n = int(batch[0].shape[0])
            direct = torch.empty(n, k, dtype=torch.int64, device=dev())
            assert getattr(lib, name)(SEED * 7919, (EPOCH << 32) + b, n, ITEMS, k, ops._ptr(direct), ops._stream()) == 0
            assert torch.equal(batch[6].view(n, k), direct.cpu()), (k, b)
        assert not {'_item_weights', '_item_cum', '_item_table_device'} & set(ds.__dict__)          # nothing of the weighted draw was built on the way


def test_two_ranks_draw_their_own_seeds_rows():
    k, world = 10, 2
    ds = dataset(k, ALPHA, True)
    ptr, items = ds.user_item_lists
    whole = epoch_of(dataset(k, 0.0), batches=100)
    order = torch.cat([batch[0] for batch in whole]), torch.cat([batch[2] for batch in whole])          # the epoch's permutation, as users and items
    seen = []
    for rank in range(world):
        lo = 0                                                               # (with several ranks the batches are sized evenly, not by BATCH: follow them)
        for b, batch in enumerate(epoch_of(ds, batches=2, rank=rank, world=world)):
            p_u, n_i = batch[0], batch[6]
            n = int(p_u.shape[0])
            assert torch.equal(p_u, order[0][rank::world][lo:lo + n]) and torch.equal(batch[2], order[1][rank::world][lo:lo + n]), (rank, b)
            lo += n
            want = P.pool_draw_weighted(SEED * 7919 + rank, (EPOCH << 32) + b, n, ITEMS, k, host_table(), p_u.numpy(), ptr, items)
            assert torch.equal(n_i.view(n, k), torch.from_numpy(want.copy())), (rank, b)
            seen.append(n_i)
    assert not torch.equal(seen[0], seen[2])                                 # the ranks' first batches differ: another seed


def _driver_run(tmp_path, monkeypatch, record):
    """``Main`` on a small synthetic corpus written to disk, two epochs of a few steps; the average losses of its epochs."""
    import random
    from ihgnn_amd import Main as driver, synth
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    w = synth.draw(60, 20, 400, 25, 500, eval_logs=20)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    monkeypatch.chdir(tmp_path)
    losses, drawn = [], []
    real = driver.train_and_get_avg_loss

    def watched(model, optimizer, loss_function, dataset_train, *a, **k):
        assert dataset_train.popularity_power == 0.75 and dataset_train.filter_negatives and dataset_train.rand_neg_sample_size == 20
        if not drawn:
            real_batches = dataset_train.device_batches

            def batches(*aa, **kk):
                for batch in real_batches(*aa, **kk):
                    drawn.append((batch[0].cpu().numpy(), batch[6].cpu().numpy()))
                    yield batch
            dataset_train.device_batches = batches
            drawn.append(dataset_train.user_item_lists)
        out = real(model, optimizer, loss_function, dataset_train, *a, **k)
        losses.append(out[0])
        return out
    monkeypatch.setattr(driver, 'train_and_get_avg_loss', watched)
    random.seed(11); torch.manual_seed(11)
    try:
        history = driver.main(['--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--ec', '2', '--est', '2', '--etf', '1', '--device_sampling',
                               '--popularity_negatives', '--filter_negatives', '--hard_negatives', '20', '--loss', 'bpr', '--record_step', record])
        assert Gs.Training.popularity_power == 0.75 and Gs.Training.filter_negatives is True and Gs.Training.negative_pool == 20
    finally:
        Gs.Training.loss, Gs.Training.negative_pool, Gs.Training.clip_grad_norm, Gs.Training.filter_negatives, Gs.Training.popularity_power = 'bce', 0, 0.0, False, 0.0
    (ptr, items), batches = drawn[0], drawn[1:]
    assert len(batches) >= 2
    for users, negatives in batches:                                         # what the loop trained on: 20 candidates per positive, none an item of its user
        assert negatives.shape[0] == 20 * users.shape[0] and not own_items(ptr, items, users, negatives.reshape(-1, 20)).any()
    return history, losses


def test_driver_trains_on_weighted_filtered_hard_negatives(tmp_path, monkeypatch):
    history, losses = _driver_run(tmp_path, monkeypatch, 'off')
    assert len(losses) == 2 and np.isfinite(losses).all() and min(losses) > 0
    assert history.training_step_recorded is False
    _, metrics = list(history.iter_epoch_test())[-1]
    assert np.isfinite([metrics.HitRatio_at10, metrics.NDCG_at10, metrics.MAP_at10]).all()


def test_driver_replays_the_same_run_as_a_recorded_step(tmp_path, monkeypatch):
    history, losses = _driver_run(tmp_path, monkeypatch, 'on')
    assert len(losses) == 2 and np.isfinite(losses).all() and min(losses) > 0
    assert history.training_step_recorded is True
