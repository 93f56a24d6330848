"""The GRU query encoder (``Gs.Query.transform == 'gru'``) on the host: the float64 restatement against ``torch.nn.GRU``, the exactness of zero-padding, the
module's state dict and RNG draws, the flags, the new entry points' declarations and argument checks, and ``BagLayout``'s two new lists.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import query_gru_reference as gref
from conftest import GOLDEN

CPU = torch.device('cpu')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRU_SYMBOLS = ('ihg_gru_workspace_bytes', 'ihg_gru_saved_bytes', 'ihg_gru_fwd', 'ihg_gru_bwd')


def small():
    return np.load(os.path.join(GOLDEN, 'f2_small_workload.npz'))


def small_dataset():
    from ihgnn_amd.Dataset import GraphDataset
    w = small()
    U, Q, I, V = (int(x) for x in w['counts'])
    return GraphDataset.from_arrays(U, Q, I, V, w['bag_words'], w['bag_offsets'], w['triples'], device=CPU)


class query_transform:
    """``Gs.Query.transform`` set for the block, put back after it."""

    def __init__(self, transform):
        self.new = transform

    def __enter__(self):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        self.old, Gs.Query.transform = Gs.Query.transform, self.new

    def __exit__(self, *exc):
        from ihgnn_amd.Helpers.GlobalSettings import Gs
        Gs.Query.transform = self.old


def host_lengths():
    return np.concatenate([gref.ragged_lengths(20), [40]])       # 0 .. 6 words, every 7th bag empty, one of 40


@pytest.mark.parametrize('d', [8, 32, 96, 256])
def test_restatement_equals_torch_gru_with_all_five_gradients(d):
    table, w_ih, w_hh, b_ih, b_hh = gref.operands(d, 50, seed=d)
    words, offsets = gref.bags(host_lengths(), 50, seed=1)
    gru = nn.GRU(d, d, batch_first=True).double()
    with torch.no_grad():
        for p, v in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v)
    mine = [t.clone().requires_grad_(True) for t in (table, w_ih, w_hh, b_ih, b_hh)]
    theirs_table = table.clone().requires_grad_(True)
    y = gref.gru_rows(mine[0], words, offsets, *mine[1:])
    want = gref.torch_gru_rows(gru, theirs_table, words, offsets)
    assert float((y - want).detach().abs().max()) <= 1e-12
    assert float(y[0].detach().abs().max()) == 0.0                           # bag 0 is empty: the zero row
    cot = torch.rand(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5
    (y * cot).sum().backward()
    (want * cot).sum().backward()
    for got, ref_t in zip(mine, (theirs_table, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
        assert float((got.grad - ref_t.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize('d', [8, 30, 96])
def test_zero_padding_to_the_next_tiled_width_is_exact(d):
    ops5 = gref.operands(d, 50, seed=d + 1)
    words, offsets = gref.bags(host_lengths(), 50, seed=3)
    width = gref.padded_width(d)
    assert width in gref.TILED and width >= d
    padded = gref.pad_operands(*ops5, width)
    y = gref.gru_rows(ops5[0], words, offsets, *ops5[1:], product=gref.ordered_product, lanes=256)
    yp = gref.gru_rows(padded[0], words, offsets, *padded[1:], product=gref.ordered_product, lanes=256)
    assert torch.equal(yp[:, :d], y) and float(yp[:, d:].abs().max()) == 0.0
    assert float((y - gref.gru_rows(ops5[0], words, offsets, *ops5[1:])).abs().max()) <= 1e-14          # (the ordered sums are the same function)


def test_gru_model_state_dict_and_rng_draws():
    from ihgnn_amd.Helpers.GlobalSettings import Gsv
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    from ihgnn_amd.Models.EmbeddingLayers import EmbeddingLayer
    assert Gsv.gru == 'gru' and Gsv.rnn == 'rnn'
    ds, d = small_dataset(), 32
    with query_transform(Gsv.gru):
        torch.manual_seed(3)
        m = RawGnn(CPU, ds, d, IHGNNLayer, 2, 3, False, HemPredictionLayer, 0.5)
    keys = list(m.state_dict())
    assert keys[:7] == ['embeddings.embedding_user.weight', 'embeddings.embedding_item.weight', 'embeddings.embedding_bag_vocabulary.weight'] + list(gref.KEYS)
    assert [k for k in keys if 'query_transform' in k] == list(gref.KEYS)
    shapes = {k: tuple(m.state_dict()[k].shape) for k in gref.KEYS}
    assert shapes == dict(zip(gref.KEYS, ((3 * d, d), (3 * d, d), (3 * d,), (3 * d,))))
    gru = m.embeddings.query_transform
    assert isinstance(gru, nn.GRU) and (gru.num_layers, gru.bidirectional, gru.batch_first, gru.input_size, gru.hidden_size) == (1, False, True, d, d)
    # the draws: the three tables, then nn.GRU(d, d)
    with query_transform(Gsv.gru):
        torch.manual_seed(11)
        layer = EmbeddingLayer(ds, d)
        after = torch.rand(4)
    torch.manual_seed(11)
    tables = [EmbeddingLayer.create_embedding(ds.user_count + 1, d, padding_idx=0), EmbeddingLayer.create_embedding(ds.item_count + 1, d, padding_idx=0),
              EmbeddingLayer.create_embedding_bag(ds.vocab_size + 1, d)]
    twin = nn.GRU(d, d, batch_first=True)
    assert torch.equal(after, torch.rand(4))
    assert torch.equal(layer.embedding_bag_vocabulary.weight, tables[2].weight)
    for name in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0'):
        assert torch.equal(getattr(layer.query_transform, name), getattr(twin, name))
    t = layer._transform()
    assert t.kind == 'gru' and len(t.tensors) == 4 and t.tensors[0] is layer.query_transform.weight_ih_l0
    with query_transform(Gsv.mean):
        plain = EmbeddingLayer(ds, d)
    assert not hasattr(plain, 'query_transform') and plain._transform().kind == 'mean' and plain._transform().tensors == ()


def test_gru_flag_parses_and_rnn_is_still_refused():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs, Gsv
    from ihgnn_amd.Models.EmbeddingLayers import EmbeddingLayer
    a = parse_args(['--query_transform', 'gru'])
    assert a.query_transform == Gsv.gru
    with pytest.raises(SystemExit):
        parse_args(['--query_transform', 'rnn'])
    with query_transform(Gsv.mean):
        driver.apply_query_settings(a)
        assert Gs.Query.transform == Gsv.gru
    assert Gs.Query.transform == Gsv.mean
    with query_transform(Gsv.rnn):
        with pytest.raises(NotImplementedError):
            EmbeddingLayer(small_dataset(), 8)
    with pytest.raises(NotImplementedError, match='gru'):
        driver.check_srrl_settings(parse_args(['--model', 'Srrl', '--query_transform', 'gru']), 1)


def test_gru_symbols_are_declared_bound_and_exported():
    from ihgnn_amd import _lib
    header = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in GRU_SYMBOLS:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 37 and _lib.load().ihg_abi_version() == 37
    assert os.path.join(os.path.dirname(_lib.LIB_PATH), 'recurrent.hip') in __import__('ihgnn_amd.build', fromlist=['SOURCES']).SOURCES


def test_gru_entries_check_arguments_before_any_launch():
    """What the two launching entry points refuse, with which code and word (the entry's name in front), in the order dim, sizes, null pointers, alignment, workspace; and
    the sizes the two ``*_bytes`` calls answer.  Every call is refused or has nothing to do: ``ok`` is an aligned address that is never dereferenced, ``odd`` a misaligned one."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    ok, odd, INV, WS, BIG = ctypes.c_void_p(16), ctypes.c_void_p(8), _lib.ERR_INVALID, _lib.ERR_WORKSPACE, 1 << 40

    def refused(rc, code, word):
        assert rc == code and word in _lib.last_error(), (rc, _lib.last_error())

    def fwd(dim=32, table=ok, ld_table=32, ptr=ok, words=ok, n_bags=3, n_words=5, w=ok, b=ok, out=ok, ld_out=32, saved=None):
        return lib.ihg_gru_fwd(table, ld_table, ptr, words, None, n_bags, n_words, w, w, b, b, out, ld_out, saved, None, 0, dim, None)

    def bwd(dim=32, dq=ok, ld_dq=32, table=ok, ld_table=32, n_bags=3, n_words=5, rows=4, saved=ok, d_table=ok, dw=ok, ws=ok, ws_bytes=BIG):
        return lib.ihg_gru_bwd(dq, ld_dq, table, ld_table, ok, ok, None, n_bags, n_words, ok, ok, rows, ok, ok, saved, d_table, dw, dw, dw, dw, ws, ws_bytes, dim, None)

    for entry, name in ((fwd, 'ihg_gru_fwd'), (bwd, 'ihg_gru_bwd')):
        for dim in (0, 30, 96, 257):
            refused(entry(dim=dim), INV, f'{name}: dim {dim} is not one of 32 / 64 / 128 / 256')
        refused(entry(dim=96, table=None), INV, f'{name}: dim')                     # the width first
        refused(entry(n_bags=-1), INV, f'{name}: bad size')
        refused(entry(n_words=-1), INV, f'{name}: bad size')
        refused(entry(ld_table=31), INV, f'{name}: bad size')
        refused(entry(ld_table=34), INV, f'{name}: bad size')
        refused(entry(ld_table=31, table=None), INV, f'{name}: bad size')          # sizes before pointers
    refused(fwd(ld_out=31), INV, 'ihg_gru_fwd: bad size')
    refused(fwd(out=None), INV, 'ihg_gru_fwd: null bag_ptr or out')
    refused(fwd(ptr=None), INV, 'ihg_gru_fwd: null bag_ptr or out')
    refused(fwd(table=None), INV, 'ihg_gru_fwd: null table, words or parameter')
    refused(fwd(b=None), INV, 'ihg_gru_fwd: null table, words or parameter')
    refused(fwd(table=odd), INV, 'ihg_gru_fwd: table, w_ih and w_hh must be 16-byte aligned')
    refused(fwd(w=odd), INV, 'ihg_gru_fwd: table, w_ih and w_hh must be 16-byte aligned')
    assert fwd(n_bags=0, n_words=0, table=None, out=None) == _lib.OK                # nothing to do, nothing launched
    refused(bwd(ld_dq=31), INV, 'ihg_gru_bwd: bad size')
    refused(bwd(rows=-1), INV, 'ihg_gru_bwd: bad size')
    refused(bwd(dw=None), INV, 'ihg_gru_bwd: null gradient')
    refused(bwd(d_table=None), INV, 'ihg_gru_bwd: null gradient')
    refused(bwd(d_table=odd), INV, 'ihg_gru_bwd: d_table must be 16-byte aligned')
    refused(bwd(dq=None), INV, 'ihg_gru_bwd: null operand')
    refused(bwd(saved=None), INV, 'ihg_gru_bwd: null operand')
    refused(bwd(saved=odd), INV, 'ihg_gru_bwd: table and saved must be 16-byte aligned')
    refused(bwd(ws=None), WS, 'ihg_gru_bwd: workspace')
    refused(bwd(ws=odd), WS, 'ihg_gru_bwd: workspace')
    need = lib.ihg_gru_workspace_bytes(3, 5, 32)
    refused(bwd(ws_bytes=need - 4), WS, f'ihg_gru_bwd: workspace of {need - 4} bytes, {need} needed')
    refused(bwd(saved=odd, ws=None), INV, 'ihg_gru_bwd: table and saved')            # alignment before the workspace
    # sizes: any width 1 .. 256 at its tiled width; the saved state is 5 floats per word occurrence and unit
    for dim, width in ((1, 32), (30, 32), (32, 32), (96, 128), (256, 256)):
        assert lib.ihg_gru_saved_bytes(1000, dim) == 1000 * 5 * width * 4
        assert lib.ihg_gru_workspace_bytes(10, 1000, dim) == lib.ihg_gru_workspace_bytes(10, 1000, width) >= 1000 * 5 * width * 4
    for dim in (0, -1, 257):
        assert lib.ihg_gru_workspace_bytes(10, 1000, dim) == -1 and lib.ihg_gru_saved_bytes(1000, dim) == -1
    assert lib.ihg_gru_saved_bytes(26000 * 3, 128) == 26000 * 3 * 5 * 128 * 4


@pytest.mark.parametrize('case', ['ragged', 'empty', 'vocab1', 'equal'])
def test_bag_layout_length_order_and_word_positions(case):
    from ihgnn_amd import ops
    if case == 'ragged':
        lens, vocab = host_lengths(), 9
    elif case == 'empty':
        lens, vocab = np.zeros(5, np.int64), 3
    elif case == 'vocab1':
        lens, vocab = gref.ragged_lengths(12), 1
    else:
        lens, vocab = np.full(6, 3, np.int64), 7
    words, offsets = gref.bags(lens, vocab, seed=5)
    bag = ops.BagLayout(words, offsets, vocab + 1, CPU)
    assert bag.n_words == int(lens.sum())
    want = np.array(sorted(range(len(lens)), key=lambda b: -lens[b]), np.int64)      # (sorted() is stable: ties in bag order)
    if bag.length_order is None:
        assert np.array_equal(want, np.arange(len(lens))) and case in ('empty', 'equal')
    else:
        order = bag.length_order.numpy()
        assert order.dtype == np.int32 and np.array_equal(order, want)
        assert np.all(np.diff(lens[order]) <= 0) and sorted(order) == list(range(len(lens)))
    ptr, pos = bag.words_of.ptr.numpy(), bag.word_positions.numpy()
    assert ptr.shape == (vocab + 2,) and ptr[0] == 0 and ptr[-1] == len(words) and pos.dtype == np.int32
    seen = []
    for w in range(vocab + 1):
        mine = pos[ptr[w]:ptr[w + 1]]
        assert np.all(words[mine] == w) and np.all(np.diff(mine) > 0)             # this word's occurrences, in position order
        seen.extend(mine.tolist())
    assert sorted(seen) == list(range(len(words)))
