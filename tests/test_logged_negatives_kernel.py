"""``ihg_device_batch`` (``csrc/tail.hip``) through the C ABI and ``GraphDataset.device_batches`` / ``DeviceBatchLoader`` with logged negatives.

The kernel's generator is integer arithmetic, so every launch is held with ``torch.equal`` on the WHOLE pack to the numpy emulation of
``tests/logged_negatives_reference.py``, whose structure and statistics ``tests/test_logged_negatives_host.py`` checks on the CPU; the random entries of every row are
also compared with the prefix of the shipped ``ihg_sample_negatives`` launch under the same (seed, counter), which holds the emulation's generator to the kernel that
was there before.  The pack is a view into a sentinel-filled buffer with guards, pre-filled with a pattern no id has; every input is compared with its copy
afterwards; every launch runs twice and the two results are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import logged_negatives_reference as R
from test_attention_kernels import Guarded, Source
from test_gpu_parity import build_model, dev

pytestmark = pytest.mark.gpu


def _api():
    from ihgnn_amd import _lib, ops
    return _lib.load(), _lib, ops


def _plain(seed, counter, n, n_items, k):
    """``ihg_sample_negatives`` on the GPU -> ``[n, k]`` numpy."""
    lib, _lib, ops = _api()
    out = torch.empty(n, k, dtype=torch.int64, device=dev())
    _lib.check(lib.ihg_sample_negatives(seed, counter, n, n_items, k, ops._ptr(out), ops._stream()), 'ihg_sample_negatives')
    return out.cpu().numpy()


class Launch:
    """One corpus on the device and ``ihg_device_batch`` launches over it; ``tables=None`` passes null list pointers."""

    def __init__(self, pos, edge_ids, tables, n_items, what):
        self.pos_np, self.ids_np, self.tables_np, self.n_items, self.what = pos, np.asarray(edge_ids, np.int64), tables, int(n_items), what
        self.pos, self.ids = Source(torch.from_numpy(pos)), Source(torch.from_numpy(self.ids_np))
        self.tables = None if tables is None else [Source(torch.from_numpy(np.ascontiguousarray(t))) for t in tables]
        self.n = len(self.ids_np)

    def call(self, seed, counter, k_rand, k_logged, out, null_lists=False, null_pack=False):
        lib, _lib, ops = _api()
        lists = [None] * 3 if self.tables is None or null_lists else [ops._ptr(s.t) for s in self.tables]
        return lib.ihg_device_batch(seed, counter, ops._ptr(self.pos.t), ops._ptr(self.ids.t), self.n, *lists, self.n_items, k_rand, k_logged,
                                    None if null_pack else ops._ptr(out.arg), ops._stream())

    def output(self, k):
        return Guarded(2 * 4 * self.n * (1 + k))                            # int64 entries as pairs of floats, NaN-filled: 0x7FC000007FC00000 is no id and no flag

    def run(self, seed, counter, k_rand, k_logged):
        _, _lib, _ = _api()
        k = k_rand + k_logged
        out = self.output(k)
        rc = self.call(seed, counter, k_rand, k_logged, out)
        torch.cuda.synchronize()
        assert rc == _lib.OK, f'{self.what}: returned {rc}: {_lib.last_error()}'
        out.assert_guards(self.what)
        self.assert_sources()
        return out.view.view(torch.int64).view(4, self.n * (1 + k)).cpu()

    def assert_sources(self):
        for s in [self.pos, self.ids] + (self.tables or []):
            s.assert_unchanged(self.what)

    def check(self, seed, counter, k_rand, k_logged):
        """Two launches, bit-identical, equal to the emulation as a whole; the random entries equal to the plain sampler's prefix on the GPU."""
        k, n = k_rand + k_logged, self.n
        got, again = self.run(seed, counter, k_rand, k_logged), self.run(seed, counter, k_rand, k_logged)
        assert torch.equal(got, again), f'{self.what}: two launches differ'
        want = torch.from_numpy(R.device_batch(seed, counter, self.pos_np, self.ids_np, self.tables_np, self.n_items, k_rand, k_logged))
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f'{self.what}: {len(bad)} of {got.numel()} entries differ from the emulation, first at (row, column) {bad[0].tolist()} of [4, {n} x (1 + {k})]: '
                                 f'{int(got[tuple(bad[0])])} for {int(want[tuple(bad[0])])}')
        negs = got[2, n:].numpy().reshape(n, k)
        plain = _plain(seed, counter, n, self.n_items, k)
        if k_logged:
            pair = self.tables_np[0][self.ids_np]
            length = self.tables_np[1][pair + 1] - self.tables_np[1][pair]
        else:
            length = np.zeros(n, np.int64)
        enough = length >= k_logged
        n_random, first = np.where(enough, k_rand, k - length), np.where(enough, k_logged, 0)
        rows = np.arange(n)
        for j in range(k):
            sel = rows[j < n_random]
            assert np.array_equal(negs[sel, first[sel] + j], plain[sel, j]), f'{self.what}: random entry {j} is not the plain sampler\'s'
        return negs


def _case(n, k_logged, n_items=50, n_pairs=61, seed=0, what=''):
    """``n`` rows over ``n_pairs`` pairs with the mixed list lengths, the edge ids a shuffled subset with repeats."""
    pos, tables = R.corpus(R.list_lengths(k_logged, n_pairs), k_logged, n_items=n_items, seed=seed)
    edge_ids = np.random.default_rng([seed, n]).integers(0, n_pairs, n)
    return Launch(pos, edge_ids, tables, n_items, what or f'n={n} k_logged={k_logged} items={n_items}')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 256, 257])
def test_device_batch_row_ladder(n):
    """Around one wave and one workgroup of rows, at k_rand = k_logged = 5 and at the plain sampler's k = 10."""
    _case(n, 5).check(3, 7, 5, 5)
    _case(n, 0).check(3, 7, 10, 0)


@pytest.mark.parametrize('k_rand,k_logged', [(10, 0), (0, 1), (0, 16), (1, 3), (10, 6), (5, 5)])
def test_device_batch_count_ladder(k_rand, k_logged):
    """Every split of k, list lengths {0, 1, k_logged - 1, k_logged, k_logged + 1, 17, 1000} mixed within the launch, items repeated within the lists."""
    negs = _case(257, k_logged).check(11, (2 << 32) + 5, k_rand, k_logged)
    assert negs.min() >= 0 and negs.max() < 50


def test_device_batch_null_lists_without_logged_negatives():
    """k_logged = 0 with null list pointers: the plain sampler's launch, bit for bit, in the pack's layout."""
    pos, _ = R.corpus(np.zeros(40, np.int64), 0)
    launch = Launch(pos, np.random.default_rng(1).integers(0, 40, 100), None, 50, 'null lists')
    negs = launch.check(4, 9, 10, 0)
    assert np.array_equal(negs, _plain(4, 9, 100, 50, 10))


def test_device_batch_second_grid_stride_trip():
    """2048 x 256 + 65 rows, k_rand = k_logged = 1: the grid-stride loop goes into a second trip."""
    n = 2048 * 256 + 65
    _case(n, 1, n_items=1000, n_pairs=4099, what='second trip').check(2, 1, 1, 1)


def test_device_batch_catalogue_edges():
    """n_items = k: every all-random row is a permutation of the catalogue; n_items = 2^31 - 1: the multiply-high at the top of the id range."""
    k_rand, k_logged = 4, 3
    launch = _case(129, k_logged, n_items=7)
    negs = launch.check(6, 6, k_rand, k_logged)
    pair = launch.tables_np[0][launch.ids_np]
    empty = np.flatnonzero(launch.tables_np[1][pair + 1] == launch.tables_np[1][pair])
    assert len(empty) > 5 and all(sorted(r) == list(range(7)) for r in negs[empty].tolist())
    negs = _case(129, k_logged, n_items=2 ** 31 - 1).check(6, 6, k_rand, k_logged)
    assert negs.max() > 2 ** 30 and negs.max() < 2 ** 31 - 1


@pytest.mark.parametrize('why', ['k = 17', 'k > n_items', 'k = 0', 'null list', 'null pack'])
def test_device_batch_refusals(why):
    """``IHG_ERR_INVALID`` with a message, nothing launched: the output and the guards stay as they were.  'k = 17' runs on a catalogue of 50 items, so that only the
    limit of 16 can refuse it; 'k > n_items' is 13 of 12 items, within the 16."""
    _, _lib, _ = _api()
    n_items = 50 if why == 'k = 17' else 12
    launch = _case(65, 3, n_items=n_items)
    k_rand, k_logged = {'k = 17': (9, 8), 'k > n_items': (10, 3), 'k = 0': (0, 0), 'null list': (2, 3), 'null pack': (2, 3)}[why]
    out = launch.output(max(k_rand + k_logged, 1))
    rc = launch.call(1, 1, k_rand, k_logged, out, null_lists=why == 'null list', null_pack=why == 'null pack')
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and 'ihg_device_batch' in _lib.last_error()
    with pytest.raises(_lib.IhgnnHipError):
        _lib.check(rc, 'ihg_device_batch')
    out.assert_untouched(why)
    launch.assert_sources()
    empty = Launch(launch.pos_np, np.zeros(0, np.int64), launch.tables_np, n_items, 'n = 0')
    assert empty.call(1, 1, 2, 3, out) == _lib.OK                             # an empty batch is fine and writes nothing
    torch.cuda.synchronize()
    out.assert_untouched('n = 0')


# =============================================================================================
# GraphDataset.device_batches / DeviceBatchLoader
# =============================================================================================
def _loader_corpus(rand, nonrand):
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(60, 30, 80, 40, 1000, seed=6)
    rng = np.random.default_rng(66)
    pairs = np.unique(w.triples[:, :2], axis=0)
    counts = rng.integers(0, 7, len(pairs))                                # 0 ... 6 logged negatives per pair with a positive: both branches at nonrand = 3
    uq = np.concatenate([np.repeat(pairs, counts, axis=0), np.stack([rng.integers(0, 60, 50), rng.integers(0, 30, 50)], 1)])      # and some pairs that may have none
    neg = np.concatenate([uq, rng.integers(0, 80, (len(uq), 1))], 1)[rng.permutation(len(uq))]
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, random_negative_sample_size=rand,
                                  non_random_negative_sample_size=nonrand, device=dev(), neg_triples=neg)
    return w, ds


def test_device_batches_with_logged_negatives_cover_the_epoch_and_train():
    """nonrand = 3, rand = 4: over two ranks every positive once per epoch, the tuple layout of collate_fn, every negative row with its positive's user and query,
    items in range, every row by the rule against the host's dict - and three training epochs driven by it lower the loss."""
    from ihgnn_amd.Dataset import DeviceBatchLoader
    w, ds = _loader_corpus(4, 3)
    table = ds.neg_items_for_user_query_pair
    seen, short, full = [], 0, 0
    for rank in range(2):
        loader = DeviceBatchLoader(ds, 100, rank, 2)
        loader.set_epoch(3)
        batches = list(loader)
        assert len(batches) == len(loader) == 5
        for batch in batches:
            pu, pq, pi, pf, nu, nq, ni, nf = batch
            assert all(t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 for t in batch)
            assert len(pq) == len(pi) == len(pf) == len(pu) and len(nq) == len(ni) == len(nf) == len(nu) == 7 * len(pu)
            assert bool((pf == 1).all()) and bool((nf == 0).all())
            assert torch.equal(nu.view(-1, 7), pu[:, None].expand(-1, 7)) and torch.equal(nq.view(-1, 7), pq[:, None].expand(-1, 7))
            assert int(ni.min()) >= 0 and int(ni.max()) < 80
            for u, q, negs in zip(pu.tolist(), pq.tolist(), ni.view(-1, 7).tolist()):
                logged = table.get((u, q), [])
                if len(logged) >= 3:
                    left = list(logged)
                    for item in negs[:3]:
                        left.remove(item)                                    # three entries of the list at distinct positions
                    assert len(set(negs[3:])) == 4
                    full += 1
                else:
                    c = 7 - len(logged)
                    assert negs[c:] == logged and len(set(negs[:c])) == c
                    short += 1
            seen += torch.stack([pu, pq, pi], 1).tolist()
    assert sorted(seen) == sorted(w.triples.tolist()) and short > 50 and full > 50
    m = build_model(ds, 'ihgnn', 2, 3, 32)
    from ihgnn_amd.optim import Adam
    opt = Adam(m.parameters(), 1e-2)
    loader = DeviceBatchLoader(ds, 100)
    losses = []
    for epoch in range(3):
        loader.set_epoch(epoch)
        for pu, pq, pi, pf, nu, nq, ni, nf in loader:
            loss = m.bce_loss(torch.cat([pu, nu]), torch.cat([pq, nq]), torch.cat([pi, ni]), torch.cat([pf, nf]).float())
            loss.backward(); opt.step(); opt.zero_grad()
            losses.append(loss.item())
    assert np.mean(losses[-5:]) < np.mean(losses[:5])


def test_device_batches_on_a_corpus_without_logged_negatives():
    """nonrand = 3 asked of a corpus that logged no negative at all: every list is short, so every row is 7 random items - the plain sampler's row under the same keys."""
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import DeviceBatchLoader, GraphDataset
    w = synth.draw(60, 30, 80, 40, 300, seed=6)
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, random_negative_sample_size=4,
                                  non_random_negative_sample_size=3, device=dev())
    assert len(ds.logged_negative_lists[2]) == 0
    loader = DeviceBatchLoader(ds, 128, seed=2)
    loader.set_epoch(1)
    seen = []
    for b, (pu, pq, pi, pf, nu, nq, ni, nf) in enumerate(loader):
        n = len(pu)
        assert np.array_equal(ni.view(n, 7).cpu().numpy(), _plain(2 * 7919, (1 << 32) + b, n, 80, 7))
        assert torch.equal(nu.view(n, 7)[:, 6], pu) and torch.equal(nq.view(n, 7)[:, 0], pq) and bool((pf == 1).all()) and bool((nf == 0).all())
        seen += torch.stack([pu, pq, pi], 1).tolist()
    assert sorted(seen) == sorted(w.triples.tolist())


def test_device_batches_without_logged_negatives_are_unchanged():
    """nonrand = 0: the loader's batches for one (seed, epoch, rank) are bit for bit the earlier formula - the device permutation's slices gathered from the positives,
    ``ihg_sample_negatives`` under the keys seed * 7919 + rank and (epoch << 32) + b - whether or not the corpus has logged negatives."""
    from ihgnn_amd.Dataset import DeviceBatchLoader
    w, ds = _loader_corpus(10, 0)
    seed, epoch = 4, 2
    loader = DeviceBatchLoader(ds, 128, seed=seed)
    loader.set_epoch(epoch)
    batches = list(loader)
    gen = torch.Generator(device=dev())
    gen.manual_seed(seed * 1_000_003 + epoch)
    order = torch.randperm(len(ds), device=dev(), generator=gen)
    pos_all = torch.from_numpy(w.triples).to(dev())
    assert len(batches) == 8
    for b, (pu, pq, pi, pf, nu, nq, ni, nf) in enumerate(batches):
        pos = pos_all[order[128 * b:128 * (b + 1)]]
        n = len(pos)
        assert torch.equal(torch.stack([pu, pq, pi], 1), pos) and bool((pf == 1).all()) and bool((nf == 0).all()) and len(pf) == n and len(nf) == 10 * n
        assert torch.equal(nu, pos[:, 0].repeat_interleave(10)) and torch.equal(nq, pos[:, 1].repeat_interleave(10))
        assert np.array_equal(ni.view(n, 10).cpu().numpy(), _plain(seed * 7919, (epoch << 32) + b, n, 80, 10))
