"""The per-entry source weights of the two-hop lists (``IncidenceLayout.two_hop_source_weights``) and the launch form that takes them
(``IHG_SRC_SCALE_IN_ENTRIES``), as far as they can be checked without a GPU: the weights bit for bit, the cache, the size gate and the argument checks."""
import numpy as np
import pytest
import torch

from ihgnn_amd import _lib, ops
from ihgnn_amd.layout import SOURCE_WEIGHT_SLOTS, IncidenceLayout


def _layout(seed=0, users=40, queries=9, items=50, edges=700):
    rng = np.random.default_rng(seed)
    triples = np.stack([rng.integers(0, users, edges), rng.integers(0, queries, edges), rng.integers(0, items, edges)], axis=1)
    triples[: edges // 3, 1] = 0                                        # a hub query: a split row, and many repeated (destination, source) entries
    return IncidenceLayout(triples, users, queries, items, torch.device('cpu'), heavy_threshold=64)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('scale_name', ['inv_deg', 'inv_sqrt_deg'])
def test_source_weights_are_the_kernels_products_bit_for_bit(scale_name):
    lay = _layout()
    scale = getattr(lay, scale_name)
    plain = lay.two_hop_source_weights(scale, merged=False)
    ids = lay.hop2_csr.ids.long()
    assert plain.dtype == torch.float32 and plain.shape == (lay.hop2_csr.nnz,)
    assert torch.equal(_bits(plain), _bits(scale[ids]))
    csr, weights, _ = lay.two_hop_merged()
    merged = lay.two_hop_source_weights(scale, merged=True)
    assert merged.shape == (csr.nnz,) and csr.nnz < lay.hop2_csr.nnz
    # my_w = src_scale[id]; my_w *= entry_scale[p]: one float32 product per entry, in numpy as a second opinion on torch's
    want = (scale.numpy()[csr.ids_host] * weights.numpy()).astype(np.float32)
    assert np.array_equal(merged.numpy().view(np.int32), want.view(np.int32))
    assert bool((weights > 1).any()), 'the case has no merged entry: nothing checks the product'


def test_source_weights_are_built_once_per_vector_and_rebuilt_after_an_in_place_change():
    lay = _layout(1)
    w0 = lay.two_hop_source_weights(lay.inv_deg, merged=False)
    assert lay.two_hop_source_weights(lay.inv_deg, merged=False) is w0
    assert lay.has_two_hop_source_weights(lay.inv_deg, False) and not lay.has_two_hop_source_weights(lay.inv_deg, True)
    other = lay.inv_deg.clone()
    w1 = lay.two_hop_source_weights(other, merged=False)
    assert w1 is not w0 and torch.equal(w1, w0)
    other.mul_(2.0)
    assert not lay.has_two_hop_source_weights(other, False)
    w2 = lay.two_hop_source_weights(other, merged=False)
    assert torch.equal(w2, 2.0 * w0) and lay.two_hop_source_weights(other, merged=False) is w2


def test_source_weights_cache_is_bounded():
    lay = _layout(2)
    kept = [lay.inv_deg.clone() for _ in range(SOURCE_WEIGHT_SLOTS)]
    assert all(lay.two_hop_source_weights(s, merged=False) is not None for s in kept)
    assert lay.two_hop_source_weights(lay.inv_deg.clone(), merged=False) is None          # a fifth vector: the caller keeps the per-id gather
    assert lay.two_hop_source_weights(kept[0], merged=False) is not None                  # the kept ones stay


def test_source_weights_refuse_a_vector_that_is_not_per_node():
    lay = _layout(3)
    with pytest.raises(ValueError):
        lay.two_hop_source_weights(lay.inv_deg[:-1], merged=False)
    with pytest.raises(ValueError):
        lay.two_hop_source_weights(lay.inv_deg.double(), merged=False)


def test_size_gate_keeps_the_existing_path(monkeypatch):
    lay = _layout(4)
    monkeypatch.setattr(ops, 'TWO_HOP_MERGED', False)
    nbytes = 4 * lay.hop2_csr.nnz
    assert lay.two_hop_source_weights(lay.inv_deg, False, max_bytes=nbytes - 1) is None
    assert lay.two_hop_source_weights(lay.inv_deg, False, max_bytes=nbytes) is not None
    # the gate of the launches: C3's list (13.2 M entries) and C4's (19.8 M) pass, a list of 64 M entries does not
    assert 4 * 6 * 3_300_000 <= ops.SOURCE_WEIGHTS_MAX_BYTES < 4 * 64_000_000
    csr, weights, folded = ops.two_hop_scaled_list(lay, lay.inv_deg)
    assert folded and csr is lay.hop2_csr and torch.equal(weights, lay.inv_deg[csr.ids.long()])
    monkeypatch.setattr(ops, 'SOURCE_WEIGHTS_MAX_BYTES', nbytes - 1)
    fresh = _layout(4)
    csr, weights, folded = ops.two_hop_scaled_list(fresh, fresh.inv_deg)
    assert not folded and weights is None and csr is fresh.hop2_csr
    assert not fresh.has_two_hop_source_weights(fresh.inv_deg, False)
    # the merged list is gated by ITS size
    monkeypatch.setattr(ops, 'TWO_HOP_MERGED', True)
    mcsr, mweights, _ = fresh.two_hop_merged()
    monkeypatch.setattr(ops, 'SOURCE_WEIGHTS_MAX_BYTES', 4 * mcsr.nnz)
    csr, weights, folded = ops.two_hop_scaled_list(fresh, fresh.inv_deg)
    assert folded and csr is mcsr and weights is not mweights
    # no scale, or the switch off: the list as it is
    assert ops.two_hop_scaled_list(fresh, None) == (mcsr, mweights, False)
    monkeypatch.setattr(ops, 'SOURCE_WEIGHTS', False)
    assert ops.two_hop_scaled_list(fresh, fresh.inv_deg) == (mcsr, mweights, False)


def test_flag_needs_both_scale_pointers():
    """``IHG_SRC_SCALE_IN_ENTRIES`` without a source scale or without entries is refused before any launch (runs without a GPU)."""
    lib = _lib.load()
    some = 4096                                              # a non-null address that is never dereferenced
    mode = _lib.SCALE_NONE | _lib.SRC_SCALE_IN_ENTRIES

    def call(src_scale, entry_scale):
        return lib.ihg_node_segment_sum(some, 4, some, some, None, src_scale, entry_scale, None, mode, some, 4, 3, 4, 0, None, None, 0, None, None, 0, None, None, None, None)

    for src_scale, entry_scale in ((None, some), (some, None), (None, None)):
        assert call(src_scale, entry_scale) == _lib.ERR_INVALID
        assert 'IHG_SRC_SCALE_IN_ENTRIES' in _lib.last_error()
    assert lib.ihg_node_segment_sum(None, 4, None, None, None, None, None, None, mode, None, 4, 0, 4, 0, None, None, 0, None, None, 0, None, None, None, None) == _lib.OK
