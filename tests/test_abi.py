"""The C-ABI shared library: loads, exports exactly what include/ihgnn_hip.h declares, rejects bad arguments with
an error string, and the product refuses to run without it or on CPU tensors.  No GPU kernel is launched here."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from ihgnn_amd import _lib


def declared_symbols():
    text = open(os.path.join(REPO, 'include', 'ihgnn_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(ihg_[a-z0-9_]+)\s*\(', text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.SIGNATURES)


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), f'{name} declared in include/ihgnn_hip.h but not exported'
    assert _lib.load().ihg_abi_version() == _lib.ABI_VERSION
    assert lib.ihg_ablation_build() == 0, 'the shipped library was built with an ablation switch (csrc/ablate.hpp)'


def test_widest_scored_row_is_one_number_everywhere():
    """The evaluation kernel's width limit comes from the library's LDS budget; the model's constructor check and the header quote the same number."""
    from ihgnn_amd.Models import RawGnn
    lib = _lib.load()
    assert lib.ihg_score_topk_max_dim() == RawGnn.MAX_SCORED_WIDTH
    assert f'ihg_score_topk_max_dim() = {RawGnn.MAX_SCORED_WIDTH}' in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ihgnn_hip.h')).read()
    ws = ctypes.c_void_p(16)
    # one past the limit is refused with a message that names the limit (argument checks come before any launch: runs without a GPU)
    rc = lib.ihg_score_topk(ws, 2000, RawGnn.MAX_SCORED_WIDTH + 1, 0, 0, 10, ws, ws, ws, 0.5, 1, 10, ws, ws, ws, 1 << 40, None)
    assert rc != 0 and str(RawGnn.MAX_SCORED_WIDTH) in _lib.last_error()


def test_bad_arguments_return_codes_and_messages():
    lib = _lib.load()
    assert lib.ihg_edge_gather_sum(None, 4, None, None, None, 1.0, None, None, 4, 5, 4, None) == _lib.ERR_INVALID
    assert 'null pointer' in _lib.last_error()
    assert lib.ihg_edge_gather_sum(None, 2, None, None, None, 1.0, None, None, 4, 5, 4, None) == _lib.ERR_INVALID   # ld < dim
    assert lib.ihg_node_segment_sum(None, 4, None, None, None, None, None, None, 7, None, 4, 3, 4, 0, None, None, 0, None, None, 0, None, None, None, None) == _lib.ERR_INVALID
    assert 'out_scale_mode' in _lib.last_error()
    assert lib.ihg_interact_fwd(None, 4, None, 4, None, None, 28, 1, None, 4, None, 0, 3, 4, None) == _lib.ERR_INVALID
    assert 'order' in _lib.last_error()
    assert lib.ihg_interact_fwd(None, 4, None, 4, None, None, 8, 3, None, 4, None, 0, 3, 4, None) == _lib.ERR_INVALID   # ld_w < 7*dim
    # fp32-packed product blocks (3 or 4 of them) + at d = 64 / 128 / 256 the three bf16 planes of four block slots (1.5 x 4 d^2)
    assert lib.ihg_interact_fwd_workspace_bytes(1000, 64, 2) == (3 * 64 * 64 + 6 * 64 * 64) * 4 and lib.ihg_interact_fwd_workspace_bytes(1000, 12, 3) == 0
    assert lib.ihg_interact_fwd_workspace_bytes(1000, 64, 3) == (4 * 64 * 64 + 6 * 64 * 64) * 4 and lib.ihg_interact_fwd_workspace_bytes(1000, 32, 3) == 4 * 32 * 32 * 4
    assert lib.ihg_interact_bwd_workspace_bytes(1000, 64, 3) > lib.ihg_interact_fwd_workspace_bytes(1000, 64, 3)
    # empty problems are fine and launch nothing
    assert lib.ihg_edge_gather_sum(None, 4, None, None, None, 1.0, None, None, 4, 0, 4, None) == _lib.OK
    assert lib.ihg_node_segment_sum(None, 4, None, None, None, None, None, None, 0, None, 4, 0, 4, 0, None, None, 0, None, None, 0, None, None, None, None) == _lib.OK
    with pytest.raises(_lib.IhgnnHipError, match='status -1'):
        _lib.check(_lib.ERR_INVALID, 'probe')


def test_update_tail_bad_arguments_return_invalid_and_launch_nothing():
    """The loss-and-update end of a step: every argument check answers IHG_ERR_INVALID before any launch (this runs where there is no GPU: a launch would answer
    something else), also for a bad tensor BEHIND the first 24 of an Adam call - a refused call has updated nothing."""
    from ihgnn_amd.optim import _AdamTensor
    lib = _lib.load()
    some = 4096                                              # a non-null address that is never dereferenced

    def table(entries):
        t = (_AdamTensor * len(entries))()
        for slot, (p, g, m, v, count) in zip(t, entries):
            slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq, slot.count = p, g, m, v, count
        return ctypes.cast(t, ctypes.c_void_p), t

    good = (some, some, some, some, 8)
    one, keep = table([good])
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    scalars = ctypes.c_void_p(some)
    assert lib.ihg_adam_step(one, 1, *hyper, 0, None) == _lib.ERR_INVALID                       # steps are counted from 1
    assert lib.ihg_adam_step(one, 1, *hyper, -3, None) == _lib.ERR_INVALID
    assert lib.ihg_adam_step(None, 1, *hyper, 1, None) == _lib.ERR_INVALID
    assert lib.ihg_adam_step(one, -1, *hyper, 1, None) == _lib.ERR_INVALID
    assert lib.ihg_adam_step_device_scalars(one, 1, *hyper[1:], None, None) == _lib.ERR_INVALID  # null scalars
    assert lib.ihg_adam_step_device_scalars(None, 1, *hyper[1:], scalars, None) == _lib.ERR_INVALID
    for bad in ((some, some, some, some, -1), (None, some, some, some, 8), (some, None, some, some, 8), (some, some, None, some, 8), (some, some, some, None, 8)):
        for entries in ([bad], [good] * 30 + [bad], [(None, None, None, None, 0)] * 3 + [bad]):
            ptr, keep = table(entries)
            assert lib.ihg_adam_step(ptr, len(entries), *hyper, 1, None) == _lib.ERR_INVALID, (bad, len(entries))
            assert f'tensor {len(entries) - 1}' in _lib.last_error()
            assert lib.ihg_adam_step_device_scalars(ptr, len(entries), *hyper[1:], scalars, None) == _lib.ERR_INVALID, (bad, len(entries))
    # nothing to do is fine: no tensors, or only empty ones (null pointers allowed there)
    ptr, keep = table([(None, None, None, None, 0)] * 26)
    assert lib.ihg_adam_step(ptr, 26, *hyper, 1, None) == _lib.OK and lib.ihg_adam_step(None, 0, *hyper, 1, None) == _lib.OK
    assert lib.ihg_adam_step_device_scalars(ptr, 26, *hyper[1:], scalars, None) == _lib.OK
    # BCE: 1 .. 2^24 rows
    ws = ctypes.c_void_p(some)
    assert lib.ihg_bce_with_logits(ws, ws, 0, ws, ws, None) == _lib.ERR_INVALID
    assert lib.ihg_bce_with_logits(ws, ws, (1 << 24) + 1, ws, ws, None) == _lib.ERR_INVALID
    assert lib.ihg_bce_with_logits(ws, ws, -1, ws, ws, None) == _lib.ERR_INVALID
    for k in range(4):
        args = [ws, ws, 10, ws, ws]
        args[k if k < 2 else k + 1] = None
        assert lib.ihg_bce_with_logits(*args, None) == _lib.ERR_INVALID
    # HEM scores: 1 .. 8 layer outputs, ld >= dim > 0, row stride of the gradients >= L * dim
    layers9 = (ctypes.c_void_p * 9)(*[some] * 9)
    for n_layers, ld, dim in ((9, 4, 4), (0, 4, 4), (2, 3, 4), (2, 4, 0)):
        assert lib.ihg_hem_score_fwd(layers9, n_layers, ld, dim, ws, ws, ws, 0.5, ws, 5, None) == _lib.ERR_INVALID
        assert lib.ihg_hem_score_bwd(layers9, n_layers, ld, dim, ws, ws, 1.0, 0.5, ws, 64, 5, None) == _lib.ERR_INVALID
        assert lib.ihg_hem_score_fwd_typed0(layers9, n_layers, ld, dim, None, 0, None, ws, None, ws, ws, 0.5, ws, 5, None) == _lib.ERR_INVALID
        assert lib.ihg_hem_score_bwd_typed0(layers9, n_layers, ld, dim, None, 0, None, ws, None, ws, None, 1.0, 0.5, ws, 64, 5, None) == _lib.ERR_INVALID
    assert lib.ihg_hem_score_bwd(layers9, 2, 4, 4, ws, ws, 1.0, 0.5, ws, 7, 5, None) == _lib.ERR_INVALID                   # rowgrad rows shorter than 2 x 4
    assert lib.ihg_hem_score_bwd_typed0(layers9, 2, 4, 4, None, 0, None, ws, None, ws, None, 1.0, 0.5, ws, 7, 5, None) == _lib.ERR_INVALID
    assert lib.ihg_hem_score_fwd_typed0(layers9, 2, 4, 4, layers9, 4, None, ws, None, ws, ws, 0.5, ws, 5, None) == _lib.ERR_INVALID   # typed layer 0 without its type ranges
    assert lib.ihg_hem_score_fwd(layers9, 8, 4, 4, ws, ws, ws, 0.5, ws, 0, None) == _lib.OK                                 # an empty batch launches nothing
    # every layer pointer that is read must be there: all of them, or all but slot 0 when layer 0 is typed (its three tables stand in for it)
    dot_fwd = lambda layers, l0, ld0, tb, batch: lib.ihg_hem_score_fwd_typed0(layers, 2, 4, 4, l0, ld0, tb, ws, None, ws, ws, 0.5, ws, batch, None)
    dot_bwd = lambda layers, l0, ld0, tb, batch: lib.ihg_hem_score_bwd_typed0(layers, 2, 4, 4, l0, ld0, tb, ws, None, ws, None, 1.0, 0.5, ws, 12, batch, None)
    cos_fwd = lambda layers, l0, ld0, tb, batch: lib.ihg_hem_cosine_fwd(layers, 2, 4, 4, l0, ld0, tb, ws, None, ws, ws, 0.5, ws, ws, batch, None)
    cos_bwd = lambda layers, l0, ld0, tb, batch: lib.ihg_hem_cosine_bwd(layers, 2, 4, 4, l0, ld0, tb, ws, None, ws, ws, None, 1.0, 0.5, ws, 12, batch, None)
    holes = (ctypes.c_void_p * 2)(some, None)
    first_null = (ctypes.c_void_p * 2)(None, some)
    type_begin = (ctypes.c_int64 * 4)(0, 1, 2, 3)
    for call in (lambda: lib.ihg_hem_score_fwd(holes, 2, 4, 4, ws, ws, ws, 0.5, ws, 5, None), lambda: lib.ihg_hem_score_bwd(holes, 2, 4, 4, ws, ws, 1.0, 0.5, ws, 12, 5, None),
                 lambda: dot_fwd(holes, None, 0, None, 5), lambda: dot_bwd(holes, None, 0, None, 5)):
        assert call() == _lib.ERR_INVALID and 'null layer' in _lib.last_error()
    for entry in (dot_fwd, dot_bwd, cos_fwd, cos_bwd):
        assert entry(first_null, layers9, 4, type_begin, 0) == _lib.OK
        assert entry(first_null, None, 0, None, 0) == _lib.ERR_INVALID and 'null layer' in _lib.last_error()


def _refused(rc, code, word):
    assert rc == code and word in _lib.last_error(), (rc, _lib.last_error())


def test_interact_hyperedge_entries_check_arguments_in_one_order(monkeypatch):
    """The five hyperedge-form entry points of the interactive layer: what each refuses, with which word, and which of two faults present at once is reported
    (shape support, sizes, null pointers, alignment, workspace - in that order).  ``ok`` is an aligned address that is never dereferenced, ``odd`` a misaligned one."""
    monkeypatch.delenv('IHG_INTERACT_ARITH', raising=False)
    lib = _lib.load()
    ok, odd, INV, WS = ctypes.c_void_p(16), ctypes.c_void_p(8), _lib.ERR_INVALID, _lib.ERR_WORKSPACE

    def bwd(order=3, ld_w=28, n=3, dim=4, p=ok):               # (h, ld_h, i3, w, ld_w, order, dout, ld_dout, g, dw, ld_dw, ws, bytes, n, dim, stream)
        return lib.ihg_interact_bwd(p, 4, p, p, ld_w, order, p, 4, p, None, 0, None, 0, n, dim, None)
    _refused(bwd(order=1), INV, 'order')
    _refused(bwd(ld_w=27), INV, 'bad size')
    _refused(bwd(p=None), INV, 'null pointer')
    _refused(bwd(order=1, ld_w=8, p=None), INV, 'order')      # the order is looked at first,
    _refused(bwd(ld_w=8, p=None), INV, 'bad size')             # then the sizes
    _refused(bwd(n=0, p=None), INV, 'null pointer')            # (no early return for an empty problem in the backward)
    _refused(lib.ihg_interact_bwd(ok, 4, ok, ok, 28, 3, ok, 4, ok, ok, 27, None, 0, 3, 4, None), INV, 'bad size')    # ld_dw counts only with a dw

    def fwd(order=3, ld_w=28, n=0, p=None):                    # (h, ld_h, p, ld_p, i3, w, ld_w, order, out, ld_out, ws, bytes, n, dim, stream)
        return lib.ihg_interact_fwd(p, 4, p, 4, p, p, ld_w, order, p, 4, None, 0, n, 4, None)
    assert fwd() == _lib.OK and fwd(order=2, ld_w=24) == _lib.OK       # an empty problem with valid sizes: nothing to do, before the pointers are looked at
    _refused(fwd(ld_w=27), INV, 'bad size')                    # sizes before the empty-problem return
    _refused(fwd(order=0, ld_w=8), INV, 'order')
    _refused(fwd(n=-1), INV, 'bad size')
    _refused(fwd(n=3), INV, 'null pointer')

    def reduced(dim=128, ld=128, n=5, h=ok, dh=ok, ws=ok, ws_bytes=1 << 40, dw=None, ld_dw=0):
        # (h, ld_h, i3, w, ld_w, order, dout, ld_dout, g2, dh, ld_dh, dw, ld_dw, ws, bytes, n, dim, stream)
        return lib.ihg_interact_bwd_user_reduced(h, ld, ok, ok, 7 * dim, 3, ok, ld, ok, dh, ld, dw, ld_dw, ws, ws_bytes, n, dim, None)
    _refused(reduced(dim=12, ld=12), INV, 'not supported')
    _refused(reduced(n=0), INV, 'bad size')
    _refused(reduced(dh=None), INV, 'null pointer')
    _refused(reduced(h=odd), INV, '16-byte aligned')
    _refused(reduced(ws_bytes=0), WS, 'workspace too small')
    _refused(reduced(dim=12, ld=12, n=0, dh=None), INV, 'not supported')
    _refused(reduced(n=0, dh=None, h=odd), INV, 'bad size')
    _refused(reduced(dh=None, h=odd, ws_bytes=0), INV, 'null pointer')
    _refused(reduced(ws=None, ws_bytes=0), INV, 'null pointer')        # a missing workspace is a null pointer here, not a small workspace
    _refused(reduced(h=odd, ws_bytes=0), INV, '16-byte aligned')
    _refused(reduced(dw=ok, ld_dw=7 * 128 - 1), INV, 'bad size')
    _refused(lib.ihg_interact_bwd_user_reduced(ok, 128, ok, ok, 896, 1, ok, 128, ok, ok, 128, None, 0, ok, 1 << 40, 5, 128, None), INV, 'not supported')   # a bad order too

    def planes(dim=256, n=5, rows=ok, g2=ok, ws_bytes=1 << 40):
        # (h, ld_h, i3, w, ld_w, order, planes_rows, inv_scale, g2, dh, ld_dh, ws, bytes, n, dim, stream)
        return lib.ihg_interact_bwd_user_reduced_planes(ok, dim, ok, ok, 7 * dim, 3, rows, ok, g2, ok, dim, ok, ws_bytes, n, dim, None)
    _refused(planes(dim=128), INV, 'not supported')
    _refused(planes(dim=128, n=0, rows=None), INV, 'not supported')
    _refused(planes(n=0, rows=None), INV, 'bad size')
    _refused(planes(rows=None, g2=odd), INV, 'null pointer')
    _refused(planes(g2=odd, ws_bytes=0), INV, '16-byte aligned')
    _refused(planes(rows=odd), INV, '16-byte aligned')
    _refused(planes(ws_bytes=0), WS, 'workspace too small')
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32')            # the planes are an operand of the split kernels only
    _refused(planes(), INV, 'not supported')
    monkeypatch.delenv('IHG_INTERACT_ARITH')

    def gathered(dim=32, n=5, h=ok, dout=ok, ld_dout=None, dw=None, ws_bytes=0):
        # (h, ld_h, i3, w, ld_w, order, dy, ld_dy, dy_scale, dout, ld_dout, g2, dh, ld_dh, dw, ld_dw, ws, bytes, n, dim, stream)
        return lib.ihg_interact_bwd_gathered(h, dim, ok, ok, 7 * dim, 3, ok, dim, None, dout, dim if ld_dout is None else ld_dout, ok, ok, dim, dw, 7 * dim, ok, ws_bytes, n,
                                             dim, None)
    _refused(gathered(dim=256), INV, 'not supported')
    _refused(gathered(dim=256, n=0, h=None), INV, 'not supported')
    _refused(gathered(dout=None, dw=ok), INV, 'null pointer')            # the weight step reads the stored rows
    _refused(gathered(dout=None, dw=None), WS, 'workspace too small')    # without it they need not be stored: past the null test, refused for the workspace
    _refused(gathered(dout=None, ld_dout=0), WS, 'workspace too small')  # ... and their row stride is not looked at, neither for size
    _refused(gathered(dout=None, ld_dout=34), WS, 'workspace too small')  # nor for alignment
    _refused(gathered(ld_dout=0), INV, 'bad size')
    _refused(gathered(ld_dout=34), INV, '16-byte aligned')
    _refused(gathered(dout=odd), INV, '16-byte aligned')
    _refused(gathered(n=0, h=None), INV, 'bad size')
    _refused(gathered(h=None, dout=odd), INV, 'null pointer')
    _refused(gathered(dim=128, dout=ok, dw=ok), WS, 'workspace too small')
    _refused(gathered(dim=128, ld_dout=1 << 31, dw=ok, ws_bytes=1 << 40), INV, 'strides')    # rows the weight kernel cannot address: the last check before the launch
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32')            # d = 64 / 128 gather on the split kernels only, d = 32 in fp32 either way
    _refused(gathered(dim=128), INV, 'not supported')
    _refused(gathered(dim=32), WS, 'workspace too small')


def test_interact_node_entries_check_arguments_in_one_order():
    """``ihg_node_interact_fwd`` / ``ihg_node_interact_bwd_weight``: order, type ranges, sizes, (forward: no nodes = nothing to do,) null pointers, shape support,
    workspace - in that order."""
    lib = _lib.load()
    ok, odd, INV, WS = ctypes.c_void_p(16), ctypes.c_void_p(8), _lib.ERR_INVALID, _lib.ERR_WORKSPACE
    rising, falling, empty = (ctypes.c_int64 * 4)(0, 3, 5, 9), (ctypes.c_int64 * 4)(0, 5, 3, 9), (ctypes.c_int64 * 4)(0, 0, 0, 0)

    def fwd(order=3, tb=rising, ld_w=7 * 32, dim=32, p=ok, h=None, ws_bytes=1 << 40):
        # (h, ld_h, sums, ld_sums, degree, out_scale, bias, w, ld_w, order, type_begin, out, ld_out, ws, bytes, dim, stream)
        return lib.ihg_node_interact_fwd(p if h is None else h, dim, p, 3 * dim, p, None, None, p, ld_w, order, tb, p, dim, p, ws_bytes, dim, None)

    def weight(order=3, tb=rising, ld_w=7 * 32, dim=32, p=ok, h=None, ws_bytes=1 << 40):
        # (h, ld_h, sums, ld_sums, dy, ld_dy, dy_scale, order, type_begin, dw, ld_dw, ws, bytes, dim, stream)
        return lib.ihg_node_interact_bwd_weight(p if h is None else h, dim, p, 3 * dim, p, dim, None, order, tb, p, ld_w, p, ws_bytes, dim, None)

    for entry in (fwd, weight):
        _refused(entry(order=4), INV, 'order')
        _refused(entry(tb=falling), INV, 'type_begin')
        _refused(entry(tb=None), INV, 'type_begin')
        _refused(entry(tb=(ctypes.c_int64 * 4)(1, 3, 5, 9)), INV, 'type_begin')
        _refused(entry(order=4, tb=falling, ld_w=8), INV, 'order')
        _refused(entry(tb=falling, ld_w=8, p=None), INV, 'type_begin')
        _refused(entry(ld_w=7 * 32 - 1, p=None), INV, 'bad size')
        _refused(entry(p=None), INV, 'null pointer')
        _refused(entry(p=None, dim=12, ld_w=7 * 12), INV, 'null pointer')
        _refused(entry(dim=12, ld_w=7 * 12, ws_bytes=0), INV, 'not supported')
        _refused(entry(h=odd, ws_bytes=0), INV, 'not supported')
        _refused(entry(ws_bytes=0), WS, 'workspace too small')
    assert fwd(tb=empty, p=None) == _lib.OK                     # no nodes: nothing to do, before the pointers are looked at
    _refused(fwd(tb=empty, ld_w=8, p=None), INV, 'bad size')
    _refused(weight(tb=empty, p=None), INV, 'null pointer')     # (the weight gradient has no such return)


def test_node_linear_entries_check_arguments_in_one_order(monkeypatch):
    """The seven entry points of the node-level linear maps: what each refuses, with which code and word (its own name in front), which of two faults present at once is
    reported, and where the empty-problem returns come.  Shared front of the five ``ihg_node_linear_*``: dim, ``type_begin``, leading dimensions - and at a tiled width
    with rows of whole float4s and a workspace: type ranges, workspace size, workspace alignment; everything else is the any-width kernels', which ask for none of the
    three.  Every call here is refused or has nothing to do: ``ok`` is an aligned address that is never dereferenced, ``odd`` a misaligned one."""
    monkeypatch.delenv('IHG_INTERACT_ARITH', raising=False)
    lib = _lib.load()
    ok, odd, INV, WS, BIG = ctypes.c_void_p(16), ctypes.c_void_p(8), _lib.ERR_INVALID, _lib.ERR_WORKSPACE, 1 << 40
    rising, falling, empty = (ctypes.c_int64 * 4)(0, 3, 5, 9), (ctypes.c_int64 * 4)(0, 5, 3, 9), (ctypes.c_int64 * 4)(4, 4, 4, 4)
    hollow = (ctypes.c_int64 * 4)(0, 3, 3, 9)                  # no rows of the middle type
    rows = lambda a=16, b=16, c=16: (ctypes.c_void_p * 3)(a, b, c)

    def fwd(dim=32, x=ok, ld_x=None, w=ok, ld_w=None, tb=rising, out=ok, ld_out=None, ws=ok, ws_bytes=BIG):
        # (x, ld_x, w, ld_w, w_type_stride, bias, bias_mask, bias_type_stride, type_begin, out, ld_out, ws, bytes, dim, stream)
        return lib.ihg_node_linear_fwd(x, dim if ld_x is None else ld_x, w, dim if ld_w is None else ld_w, 0, None, 0b111, 0, tb, out, dim if ld_out is None else ld_out,
                                       ws, ws_bytes, dim, None)

    def bwd_input(dim=32, x=ok, ld_x=None, w=ok, ld_w=None, tb=rising, out=ok, ld_out=None, ws=ok, ws_bytes=BIG):
        # (dout, ld_dout, w, ld_w, w_type_stride, type_begin, dx, ld_dx, ws, bytes, dim, stream)
        return lib.ihg_node_linear_bwd_input(x, dim if ld_x is None else ld_x, w, dim if ld_w is None else ld_w, 0, tb, out, dim if ld_out is None else ld_out, ws, ws_bytes, dim, None)

    def fwd_typed(dim=32, x=rows(), ld_x=None, w=ok, ld_w=None, tb=rising, out=ok, ld_out=None, ws=ok, ws_bytes=BIG):
        return lib.ihg_node_linear_fwd_typed(x, dim if ld_x is None else ld_x, w, dim if ld_w is None else ld_w, 0, None, 0b111, 0, tb, out, dim if ld_out is None else ld_out,
                                             ws, ws_bytes, dim, None)

    for name, entry in (('ihg_node_linear_fwd', fwd), ('ihg_node_linear_bwd_input', bwd_input), ('ihg_node_linear_fwd_typed', fwd_typed)):
        _refused(entry(dim=0, tb=None), INV, name + ': dim 0')
        _refused(entry(dim=-4, ld_x=-8), INV, name + ': dim -4')
        _refused(entry(tb=None, ld_x=31), INV, name + ': null pointer')
        for ld in ('ld_x', 'ld_w', 'ld_out'):
            _refused(entry(tb=falling, **{ld: 31}), INV, name + ': bad leading dimension')
        _refused(entry(tb=falling, ws_bytes=0), INV, name + ': type ranges not ascending')
        _refused(entry(ws=odd, ws_bytes=0), WS, name + ': workspace too small')
        _refused(entry(ws_bytes=int(lib.ihg_node_linear_workspace_bytes(32)) - 1), WS, name + ': workspace too small')
        _refused(entry(ws=odd, x=None), INV, name + ': workspace not 16-byte aligned')
        for operand in ('x', 'w', 'out'):
            _refused(entry(**{operand: None}), INV, name + ': null pointer')
        # the empty problem: nothing to do once the front has passed, before the operands are looked at
        assert entry(tb=empty, x=None, w=None, out=None) == _lib.OK
        assert entry(tb=empty, dim=12, x=None, ws=None, ws_bytes=0) == _lib.OK
        _refused(entry(tb=empty, ld_out=31), INV, name + ': bad leading dimension')
        _refused(entry(tb=empty, ws_bytes=0), WS, name + ': workspace too small')
        # rows for the any-width kernels (a width that is not tiled, rows that are not whole float4s, no workspace): ranges and workspace are not looked at
        _refused(entry(dim=12, tb=falling, ws=odd, ws_bytes=0, x=None), INV, name + ': null pointer')
        _refused(entry(ld_x=33, tb=falling, ws=odd, ws_bytes=0, out=None), INV, name + ': null pointer')
        _refused(entry(ws=None, ws_bytes=0, tb=falling, w=None), INV, name + ': null pointer')

    name = 'ihg_node_linear_fwd_typed'
    _refused(fwd_typed(x=rows(b=8)), INV, name + ': rows of type 1')
    _refused(fwd_typed(x=rows(a=None, b=8)), INV, name + ': rows of type 0')
    _refused(fwd_typed(x=rows(c=None), dim=12), INV, name + ': rows of type 2')          # the rows before the shape
    _refused(fwd_typed(x=rows(b=8), out=None), INV, name + ': null pointer')             # the operands before the rows
    _refused(fwd_typed(x=rows(b=8), tb=hollow, dim=12), INV, name + ': not available for this shape')     # (the rows of a type that has none are not looked at)
    _refused(fwd_typed(dim=12), INV, name + ': not available for this shape')
    _refused(fwd_typed(ld_x=33), INV, name + ': not available for this shape')
    _refused(fwd_typed(ld_out=34), INV, name + ': not available for this shape')
    _refused(fwd_typed(ws=None), INV, name + ': not available for this shape')
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32')            # typed rows at d = 128 / 256 are the split kernels'
    _refused(fwd_typed(dim=128), INV, name + ': not available for this shape')
    _refused(fwd_typed(dim=256), INV, name + ': not available for this shape')
    monkeypatch.delenv('IHG_INTERACT_ARITH')

    def weight(dim=32, dout=ok, ld_dout=None, x=ok, ld_x=None, tb=rising, dw=ok, ld_dw=None, w=ok, ld_w=None, dx=None, ld_dx=None, acc=0, ws=ok, ws_bytes=BIG):
        # (dout, ld_dout, x, ld_x, type_begin, dw, ld_dw, dw_type_stride, dbias, bias_mask, dbias_type_stride, w, ld_w, dx, ld_dx, dx_accumulate, ws, bytes, dim, stream)
        return lib.ihg_node_linear_bwd_weight(dout, dim if ld_dout is None else ld_dout, x, dim if ld_x is None else ld_x, tb, dw, dim if ld_dw is None else ld_dw, 0, None, 0b111, 0,
                                              w, dim if ld_w is None else ld_w, dx, dim if ld_dx is None else ld_dx, acc, ws, ws_bytes, dim, None)

    def weight_typed(dim=32, dout=ok, ld_dout=None, x=rows(), ld_x=None, tb=rising, dw=ok, ld_dw=None, w=ok, ld_w=None, dx=None, ld_dx=None, acc=0, ws=ok, ws_bytes=BIG):
        # (..., w, ld_w, dx_rows, ld_dx, zero_row_before_mask, ws, bytes, dim, stream): `acc` is not an argument of this one
        return lib.ihg_node_linear_bwd_weight_typed(dout, dim if ld_dout is None else ld_dout, x, dim if ld_x is None else ld_x, tb, dw, dim if ld_dw is None else ld_dw, 0, None, 0b111,
                                                    0, w, dim if ld_w is None else ld_w, dx, dim if ld_dx is None else ld_dx, 0, ws, ws_bytes, dim, None)

    for name, entry, some_dx in (('ihg_node_linear_bwd_weight', weight, ok), ('ihg_node_linear_bwd_weight_typed', weight_typed, rows())):
        _refused(entry(dim=0, tb=None), INV, name + ': dim 0')
        _refused(entry(tb=None, ld_x=31), INV, name + ': null pointer')
        for ld in ('ld_dout', 'ld_x', 'ld_dw'):
            _refused(entry(tb=falling, **{ld: 31}), INV, name + ': bad leading dimension')
        _refused(entry(tb=falling, ws_bytes=0), INV, name + ': type ranges not ascending')
        _refused(entry(ws=odd, ws_bytes=0), WS, name + ': workspace too small')
        _refused(entry(ws=odd, dout=None), INV, name + ': workspace not 16-byte aligned')
        for operand in ('dout', 'x', 'dw'):
            _refused(entry(**{operand: None}), INV, name + ': null pointer')
        _refused(entry(tb=empty, dout=None), INV, name + ': null pointer')       # (no early return for an empty problem in the weight gradient)
        _refused(entry(tb=empty, ws_bytes=0, dout=None), WS, name + ': workspace too small')
        _refused(entry(dim=12, tb=falling, ws=odd, ws_bytes=0, x=None), INV, name + ': null pointer')
        _refused(entry(dx=some_dx, w=None), INV, name + ': dx needs w')
        _refused(entry(dx=some_dx, ld_w=31), INV, name + ': dx needs w')
        _refused(entry(dx=some_dx, ld_dx=31), INV, name + ': dx needs w')
        _refused(entry(dx=some_dx, w=None, dw=None), INV, name + ': null pointer')     # the operands before the dx rule
        assert _lib.last_error().startswith(name + ':')

    name = 'ihg_node_linear_bwd_weight'
    _refused(weight(dim=64, acc=1), INV, name + ': dx_accumulate needs dx and a fused')                     # no dx
    _refused(weight(dim=12, dx=ok, acc=1), INV, name + ': dx_accumulate needs dx and a fused')              # no such kernel at this width
    _refused(weight(dim=64, dx=ok, ld_x=65, acc=1, ws_bytes=0), INV, name + ': dx_accumulate needs dx and a fused')   # ... nor for these rows; before the any-width workspace
    _refused(weight(dim=64, dx=ok, w=None, acc=1), INV, name + ': dx needs w')                              # the dx rule before the accumulate rules
    _refused(weight(dim=64, dx=ok, acc=1, dout=odd), INV, name + ': dx_accumulate needs 16-byte aligned dout and x rows')     # rows for the any-width kernels, which overwrite
    _refused(weight(dim=64, dx=ok, acc=1, x=odd), INV, name + ': dx_accumulate needs 16-byte aligned dout and x rows')
    _refused(weight(dim=32, dx=ok, acc=1, w=odd), INV, name + ': dx_accumulate at dim 32')
    _refused(weight(dim=32, dx=odd, acc=1), INV, name + ': dx_accumulate at dim 32')
    _refused(weight(dim=128, dx=odd, acc=1), INV, name + ': dx_accumulate needs 16-byte aligned dx rows')
    _refused(weight(dim=256, dx=odd, acc=1), INV, name + ': dx_accumulate needs 16-byte aligned dx rows')
    # the any-width branch asks for its own, smaller workspace - when there is no dx, before anything is launched (with a dx: tests/test_gpu_parity.py)
    _refused(weight(dim=12, ws_bytes=64), WS, name + ': workspace too small (any-width path)')
    _refused(weight(dim=12, ws_bytes=3 * 64 * (12 * 12 + 12) * 4 - 1), WS, name + ': workspace too small (any-width path)')
    _refused(weight(dim=32, ws=None, ws_bytes=BIG), WS, name + ': workspace too small (any-width path)')
    _refused(weight(dim=32, ld_x=33, ws_bytes=64), WS, name + ': workspace too small (any-width path)')
    _refused(weight(dim=32, dout=odd, ws_bytes=64), WS, name + ': workspace too small')                      # (16-byte rows of whole float4s: the front has asked for the tiled size)
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32')            # d = 128 / 256 form dx in the weight-gradient pass on the split kernels only
    _refused(weight(dim=128, dx=ok, acc=1), INV, name + ': dx_accumulate needs dx and a fused')
    _refused(weight(dim=256, dx=ok, acc=1), INV, name + ': dx_accumulate needs dx and a fused')
    monkeypatch.delenv('IHG_INTERACT_ARITH')

    name = 'ihg_node_linear_bwd_weight_typed'
    _refused(weight_typed(x=rows(b=8)), INV, name + ': rows of type 1')
    _refused(weight_typed(dx=rows(c=8)), INV, name + ': rows of type 2')
    _refused(weight_typed(dx=rows(a=None), dim=12), INV, name + ': rows of type 0')      # the rows before the shape
    _refused(weight_typed(dx=rows(a=None), w=None), INV, name + ': dx needs w')          # the dx rule before the rows
    _refused(weight_typed(x=rows(b=8), dx=rows(b=None), tb=hollow, dim=12), INV, name + ': not available for this shape')
    _refused(weight_typed(dim=12), INV, name + ': not available for this shape')
    _refused(weight_typed(ld_x=33), INV, name + ': not available for this shape')
    _refused(weight_typed(dx=rows(), ld_dx=34), INV, name + ': not available for this shape')
    _refused(weight_typed(dx=rows(), w=odd), INV, name + ': not available for this shape')         # d = 32: the one-pass kernel reads w in float4s
    _refused(weight_typed(dout=odd), INV, name + ': not available for this shape')
    _refused(weight_typed(dim=128, dout=odd), INV, name + ': not available for this shape')
    _refused(weight_typed(dim=128, x=rows(a=8), tb=(ctypes.c_int64 * 4)(0, 0, 5, 9)), INV, name + ': not available for this shape')
    _refused(weight_typed(ws=None), INV, name + ': not available for this shape')
    monkeypatch.setenv('IHG_INTERACT_ARITH', 'f32')
    _refused(weight_typed(dim=128), INV, name + ': not available for this shape')
    monkeypatch.delenv('IHG_INTERACT_ARITH')

    def act_fwd(dim=32, act=1, n=5, x=ok, ld_x=None, w=ok, ld_w=None, out=ok, ld_out=None, ws=ok, ws_bytes=BIG):
        # (x, ld_x, w, ld_w, bias, activation, out, ld_out, n_rows, ws, bytes, dim, stream)
        return lib.ihg_rows_linear_act_fwd(x, dim if ld_x is None else ld_x, w, dim if ld_w is None else ld_w, None, act, out, dim if ld_out is None else ld_out, n, ws, ws_bytes, dim, None)

    def act_bwd(dim=32, act=1, n=5, x=ok, ld_x=None, w=ok, ld_w=None, out=ok, ld_out=None, ws=ok, ws_bytes=BIG, ld_y=None, dw=ok, ld_dw=None, dx=None, ld_dx=0):
        # (dy, ld_dy, y, ld_y, x, ld_x, w, ld_w, activation, dw, ld_dw, dbias, dx, ld_dx, n_rows, ws, bytes, dim, stream): `x` stands for dy here, `out` for x
        return lib.ihg_rows_linear_act_bwd(x, dim if ld_x is None else ld_x, ok, dim if ld_y is None else ld_y, out, dim if ld_out is None else ld_out, w, dim if ld_w is None else ld_w,
                                           act, dw, dim if ld_dw is None else ld_dw, None, dx, ld_dx, n, ws, ws_bytes, dim, None)

    for name, entry in (('ihg_rows_linear_act_fwd', act_fwd), ('ihg_rows_linear_act_bwd', act_bwd)):
        _refused(entry(dim=0, act=0), INV, name + ': dim 0')
        _refused(entry(n=-1, act=0), INV, name + ': dim 32, -1 rows')
        _refused(entry(act=0, ld_x=31), INV, name + ': activation 0')
        _refused(entry(act=3), INV, name + ': activation 3')
        for ld in ('ld_x', 'ld_w', 'ld_out'):
            _refused(entry(ws=None, **{ld: 31}), INV, name + ': bad leading dimension')
        _refused(entry(ws=None, ws_bytes=0), INV, name + ': workspace null or not 16-byte aligned')
        _refused(entry(ws=odd, ws_bytes=0), INV, name + ': workspace null or not 16-byte aligned')
        _refused(entry(ws_bytes=0, x=None), WS, name + ': workspace too small')
        _refused(entry(dim=12, ws_bytes=3 * 64 * (12 * 12 + 12) * 4 - 1, x=None), WS, name + ': workspace too small')
        for operand in ('x', 'w', 'out'):
            _refused(entry(**{operand: None}), INV, name + ': null pointer')
    assert act_fwd(n=0, x=None, w=None, out=None) == _lib.OK   # no rows: nothing to do, after the front, before the operands
    _refused(act_fwd(n=0, ws_bytes=0), WS, 'ihg_rows_linear_act_fwd: workspace too small')
    name = 'ihg_rows_linear_act_bwd'
    for ld in ({'ld_y': 31}, {'ld_dw': 31}, {'dx': ok, 'ld_dx': 31}):
        _refused(act_bwd(x=None, **ld), INV, name + ': bad leading dimension')
    _refused(act_bwd(ld_y=31, ws_bytes=0), WS, name + ': workspace too small')          # its own three strides come after the shared front
    _refused(act_bwd(n=0, dw=None), INV, name + ': null pointer')                       # no rows: dw and dbias are zeroed, so dw is still asked for
    _refused(act_bwd(dw=None), INV, name + ': null pointer')


def test_gather_entries_check_arguments_in_one_order():
    """``ihg_edge_gather_sum``, ``ihg_edge_gather_sum_planes``, ``ihg_node_segment_sum``, ``ihg_node_pair_sums`` and the bag-mean pair: every refusal with its code
    and its words, the empty problem (answered before the pointers are looked at, after the sizes and the mode), and which of two faults present at once is reported.
    Every call here is refused or has nothing to do: ``ok`` is an aligned address that is never dereferenced, ``odd`` a misaligned one."""
    lib = _lib.load()
    ok, odd, INV = ctypes.c_void_p(16), ctypes.c_void_p(8), _lib.ERR_INVALID

    def k5(src=ok, ld_src=8, i3=ok, out=ok, ld_out=8, n=5, dim=8):
        # (src, ld_src, i3, node_scale, bias, alpha, edge_scale, out, ld_out, n_edges, dim, stream)
        return lib.ihg_edge_gather_sum(src, ld_src, i3, None, None, 1.0, None, out, ld_out, n, dim, None)
    for bad in (dict(n=-1), dict(dim=0), dict(dim=-8), dict(ld_src=7), dict(ld_out=7)):
        _refused(k5(**bad), INV, 'ihg_edge_gather_sum: bad size (E=')
    _refused(k5(n=0, ld_out=7, src=None), INV, 'ihg_edge_gather_sum: bad size')           # the sizes before the empty problem
    assert k5(n=0, src=None, i3=None, out=None) == _lib.OK
    for operand in ('src', 'i3', 'out'):
        _refused(k5(**{operand: None}), INV, 'ihg_edge_gather_sum: null pointer')

    def planes(src=ok, ld_src=256, i3=ok, rows=ok, inv=ok, n=5, dim=256):
        # (src, ld_src, i3, node_scale, edge_scale, planes, inv_scale, n_edges, dim, stream)
        return lib.ihg_edge_gather_sum_planes(src, ld_src, i3, None, None, rows, inv, n, dim, None)
    for bad in (dict(dim=128, ld_src=128), dict(ld_src=252), dict(ld_src=258), dict(dim=128, ld_src=128, n=-1, src=None)):
        _refused(planes(**bad), INV, 'ihg_edge_gather_sum_planes: shape not supported')
    _refused(planes(n=-1, src=None), INV, 'ihg_edge_gather_sum_planes: bad size')
    assert planes(n=0, src=None, i3=None, rows=None, inv=None) == _lib.OK
    for bad in (dict(src=None), dict(i3=None), dict(rows=None), dict(inv=None), dict(src=odd), dict(rows=odd)):
        _refused(planes(**bad), INV, 'ihg_edge_gather_sum_planes: null or unaligned pointer')

    NONE, MUL, DIV, ACC, ONCE, IN_ENTRIES = _lib.SCALE_NONE, _lib.SCALE_MULTIPLY, _lib.SCALE_DIVIDE, _lib.SCALE_ACCUMULATE, _lib.SRC_READ_ONCE, _lib.SRC_SCALE_IN_ENTRIES
    plan_pointers = ('seg_begin', 'seg_end', 'heavy_rows', 'heavy_segptr', 'partials')

    def k7(src=ok, ld_src=8, rowptr=ok, ids=ok, src_scale=None, entry_scale=None, out_scale=None, mode=NONE, out=ok, ld_out=8, n=5, dim=8, threshold=0, seg_begin=None,
           seg_end=None, n_segments=0, heavy_rows=None, heavy_segptr=None, n_heavy=0, partials=None):
        # (src, ld_src, rowptr, ids, row_order, src_scale, entry_scale, out_scale, mode, out, ld_out, n_rows, dim, heavy_threshold, seg_begin, seg_end, n_segments,
        #  heavy_rows, heavy_segptr, n_heavy, partials, self_weight, src_mask, stream)
        return lib.ihg_node_segment_sum(src, ld_src, rowptr, ids, None, src_scale, entry_scale, out_scale, mode, out, ld_out, n, dim, threshold, seg_begin, seg_end, n_segments,
                                        heavy_rows, heavy_segptr, n_heavy, partials, None, None, None)
    split = dict(threshold=2, seg_begin=ok, seg_end=ok, n_segments=3, heavy_rows=ok, heavy_segptr=ok, n_heavy=1, partials=ok)
    name = 'ihg_node_segment_sum'
    for bad in (dict(n=-1), dict(dim=0), dict(ld_src=7), dict(ld_out=7), dict(n_segments=-1), dict(n_heavy=-1), dict(split, n_segments=-1)):
        _refused(k7(**bad), INV, name + ': bad size')
    _refused(k7(ld_src=7, mode=7, n=0), INV, name + ': bad size')                          # the sizes first,
    for mode in (3, 7, 0x1000, 0x200 | MUL, MUL, DIV, MUL | ACC, DIV | ONCE | IN_ENTRIES):
        _refused(k7(mode=mode), INV, name + f': bad out_scale_mode {mode}')               # (MULTIPLY / DIVIDE: without an out_scale)
        _refused(k7(mode=mode, n=0, src=None), INV, name + ': bad out_scale_mode')        # then the mode, also where there are no rows,
    for mode, scale in ((NONE, None), (MUL, ok), (DIV | ACC | ONCE | IN_ENTRIES, ok), (NONE | ACC, None)):
        assert k7(mode=mode, out_scale=scale, n=0, src=None, rowptr=None, ids=None, out=None) == _lib.OK      # then the empty problem, before the pointers
    for operand in ('src', 'rowptr', 'ids', 'out'):
        _refused(k7(**{operand: None}), INV, name + ': null pointer')
        _refused(k7(**dict(split, seg_end=None, mode=IN_ENTRIES, **{operand: None})), INV, name + ': null pointer')     # the operands before the plan
    for pointer in plan_pointers:
        _refused(k7(**dict(split, **{pointer: None})), INV, name + ': incomplete split-row plan')
    _refused(k7(**dict(split, threshold=0)), INV, name + ': incomplete split-row plan')
    _refused(k7(**dict(split, threshold=-2)), INV, name + ': incomplete split-row plan')
    _refused(k7(**dict(split, partials=None, mode=IN_ENTRIES)), INV, name + ': incomplete split-row plan')         # the plan before the entry scales
    for scales in (dict(), dict(src_scale=ok), dict(entry_scale=ok)):
        _refused(k7(mode=IN_ENTRIES, **scales), INV, name + ': IHG_SRC_SCALE_IN_ENTRIES needs src_scale and entry_scale')
        _refused(k7(**dict(split, mode=IN_ENTRIES | MUL | ACC, out_scale=ok, **scales)), INV, name + ': IHG_SRC_SCALE_IN_ENTRIES needs')

    def pairs(h=ok, ld_h=8, ptr=ok, ids=ok, out=ok, ld_out=24, n=5, dim=8, threshold=0, seg_begin=None, seg_end=None, n_segments=0, heavy_rows=None, heavy_segptr=None,
              n_heavy=0, partials=None):
        # (h, ld_h, pair_ptr, pair_ids, row_order, out, ld_out, n_rows, dim, heavy_threshold, seg_begin, seg_end, n_segments, heavy_rows, heavy_segptr, n_heavy, partials,
        #  pair_weight, stream)
        return lib.ihg_node_pair_sums(h, ld_h, ptr, ids, None, out, ld_out, n, dim, threshold, seg_begin, seg_end, n_segments, heavy_rows, heavy_segptr, n_heavy, partials,
                                      None, None)
    name = 'ihg_node_pair_sums'
    for bad in (dict(n=-1), dict(dim=0), dict(dim=6, ld_h=8, ld_out=24), dict(ld_h=4), dict(ld_h=10), dict(ld_out=23), dict(ld_out=26), dict(n_segments=-1), dict(n_heavy=-1),
                dict(n=0, ld_out=23, h=None)):
        _refused(pairs(**bad), INV, name + ': bad size (rows=')
    assert pairs(n=0, h=None, ptr=None, ids=None, out=None) == _lib.OK
    for bad in (dict(h=None), dict(ptr=None), dict(ids=None), dict(out=None), dict(h=odd), dict(out=odd), dict(split, out=odd, seg_end=None)):
        _refused(pairs(**bad), INV, name + ': null or unaligned pointer')
    for pointer in plan_pointers:
        _refused(pairs(**dict(split, **{pointer: None})), INV, name + ': incomplete split-row plan')
    _refused(pairs(**dict(split, threshold=0)), INV, name + ': incomplete split-row plan')
    _refused(pairs(**dict(split, partials=odd)), INV, name + ': incomplete split-row plan')        # unaligned partials

    def bag_fwd(table=ok, ld_table=8, ptr=ok, words=ok, bag_len=ok, out=ok, ld_out=8, n=5, dim=8):
        return lib.ihg_bag_mean_fwd(table, ld_table, ptr, words, bag_len, out, ld_out, n, dim, None)

    def bag_bwd(table=ok, ld_table=8, ptr=ok, words=ok, bag_len=ok, out=ok, ld_out=8, n=5, dim=8):      # (dout, ld_dout, word_ptr, word_bags, inv_len, dtable, ld_dtable, rows, dim)
        return lib.ihg_bag_mean_bwd(table, ld_table, ptr, words, bag_len, out, ld_out, n, dim, None)
    _refused(bag_fwd(bag_len=None), INV, 'ihg_bag_mean_fwd: null bag_len')
    _refused(bag_bwd(bag_len=None), INV, 'ihg_bag_mean_bwd: null inv_len')
    _refused(bag_fwd(bag_len=None, dim=0), INV, 'ihg_bag_mean_fwd: null bag_len')         # its own vector first
    _refused(bag_bwd(bag_len=None, dim=0), INV, 'ihg_bag_mean_bwd: null inv_len')
    for entry in (bag_fwd, bag_bwd):                                                      # the rest are K7's answers, under K7's name
        for bad in (dict(n=-1), dict(dim=0), dict(ld_table=7), dict(ld_out=7), dict(n=0, ld_out=7)):
            _refused(entry(**bad), INV, 'ihg_node_segment_sum: bad size')
        assert entry(n=0, table=None, ptr=None, words=None, out=None) == _lib.OK
        for operand in ('table', 'ptr', 'words', 'out'):
            _refused(entry(**{operand: None}), INV, 'ihg_node_segment_sum: null pointer')
    _refused(bag_fwd(n=0, bag_len=None), INV, 'ihg_node_segment_sum: bad out_scale_mode 2')        # no bags and no lengths: the divide mode without its vector
    assert bag_bwd(n=0, bag_len=None) == _lib.OK                                          # (the backward's vector scales the sources: no mode to refuse)


def test_plan_arguments_of_the_gather_and_attention_calls():
    """``ops._plan_args``: for a ``Csr`` with split rows and for one without, the arguments ``node_segment_sum_raw``, ``node_pair_sums_raw`` and (with ``seg_row``) the
    attention calls pass for the plan - written out here as those calls listed them one by one."""
    import numpy as np
    from ihgnn_amd import ops
    from ihgnn_amd.layout import Csr, CsrRows
    lengths = [1, 5, 0, 2, 4, 3]
    ptr = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=ptr[1:])
    ids = np.arange(int(ptr[-1])) % 7
    split = Csr(ptr, ids, torch.device('cpu'), heavy_threshold=2, heavy_chunk=2)
    plain = Csr(ptr, ids, torch.device('cpu'), heavy_threshold=0)
    assert split.n_heavy == 3 and split.n_segments == 3 + 2 + 2 and plain.n_heavy == 0

    def values(args):
        return tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)

    def listed(csr, seg_row):
        heavy = csr.n_heavy > 0
        address = lambda t: t.data_ptr() if heavy else None
        front = (csr.heavy_threshold if heavy else 0, address(csr.seg_begin), address(csr.seg_end))
        back = (csr.n_segments if heavy else 0, address(csr.heavy_rows), address(csr.heavy_segptr), csr.n_heavy)
        return front + ((address(csr.seg_row),) if seg_row else ()) + back

    for csr in (split, plain):
        assert values(ops._plan_args(csr)) == listed(csr, False) and len(ops._plan_args(csr)) == 7
        assert values(ops._split_row_args(csr)) == values(ops._gat_plan(csr)) == values(ops._plan_args(csr, seg_row=True)) == listed(csr, True)
    assert values(ops._plan_args(split)) == (2, split.seg_begin.data_ptr(), split.seg_end.data_ptr(), 7, split.heavy_rows.data_ptr(), split.heavy_segptr.data_ptr(), 3)
    assert values(ops._split_row_args(plain)) == (0, None, None, None, 0, None, None, 0) and values(ops._plan_args(plain)) == (0, None, None, 0, None, None, 0)
    assert values(ops._plan_args(CsrRows(split, 1, 3))) == (0, None, None, 0, None, None, 0)      # a slice of rows: summed in place, no plan


def test_node_linear_workspace_bytes_arithmetic():
    """``ihg_node_linear_workspace_bytes``: packed weights ``[3, d, d]``, 256 weight slabs ``[3, d, d]`` with their bias parts ``[3, d]``, and at d = 128 / 256 the two-byte
    weight planes (three per weight) - at a tiled width; elsewhere the 64 row-slab partials of the any-width weight gradient."""
    lib = _lib.load()
    for d in (12, 32, 128, 256):
        if d in (32, 64, 128, 256):
            floats = 3 * d * d + 3 * 256 * (d * d + d) + ((3 * 3 * d * d) // 2 if d >= 128 else 0)
        else:
            floats = 3 * 64 * (d * d + d)
        assert int(lib.ihg_node_linear_workspace_bytes(d)) == 4 * floats
    assert int(lib.ihg_node_linear_workspace_bytes(0)) == -1 and int(lib.ihg_node_linear_workspace_bytes(-32)) == -1
    # every width's workspace holds the any-width partials too (unaligned rows at a tiled width take that branch)
    for d in (32, 64, 128, 256):
        assert int(lib.ihg_node_linear_workspace_bytes(d)) >= 4 * 3 * 64 * (d * d + d)


def test_interactive_layer_workspace_bytes_arithmetic():
    """The four workspaces of the interactive layer: each ``*_workspace_bytes`` is the sum of the regions include/ihgnn_hip.h names for it, in floats, and the number the
    library returned before the layouts were written as one function each (recorded from that build)."""
    lib = _lib.load()
    recorded = {   # (dim, order): forward, backward, node-level forward, node-level weight gradient
        (32, 2): (12288, 10002496, 86016, 6291456), (32, 3): (16384, 12107840, 86016, 8388608),
        (64, 2): (147456, 25577472, 394752, 12582912), (64, 3): (163840, 33982464, 394752, 16777216),
        (128, 2): (589824, 51447808, 1575936, 25165824), (128, 3): (655360, 68290560, 1575936, 33554432),
        (256, 2): (2359296, 28575744, 6297600, 25165824), (256, 3): (2621440, 37226496, 6297600, 33554432),
        (12, 2): (0, 0, 0, 0), (12, 3): (0, 0, 0, 0)}
    for (d, order), expected in recorded.items():
        got = (int(lib.ihg_interact_fwd_workspace_bytes(1000, d, order)), int(lib.ihg_interact_bwd_workspace_bytes(1000, d, order)),
               int(lib.ihg_node_interact_fwd_workspace_bytes(d)), int(lib.ihg_node_interact_bwd_weight_workspace_bytes(d, order)))
        assert got == expected, (d, order)
        if d == 12:
            continue
        blocks = 3 if order == 2 else 4
        fragments = blocks * d * d
        planes = 6 * d * d if d >= 64 else 0
        fwd = fragments + planes
        slabs = {32: 512, 64: 512, 128: 256, 256: 32}[d]
        ranges = 2048 if d == 32 else 256
        member_image = planes if d >= 64 else 1024 * blocks + 16 + 2048 * 320
        assert d < 64 or 4 * d * d + 8 * d <= planes                    # what the member kernel's planes, scales and inverses take of the region
        bwd = fragments + slabs * fragments + 2 * ranges * d + 2 * ranges * d + 2 * ranges + member_image
        node_fwd = 3 * 7 * 1024 if d == 32 else 24 * d * d + 3 * d + 3 * d
        node_weight = {32: 512, 64: 256, 128: 128, 256: 32}[d] * d * blocks * d
        assert got == (4 * fwd, 4 * bwd, 4 * node_fwd, 4 * node_weight), (d, order)
    # the sizes do not depend on the number of hyperedges
    assert int(lib.ihg_interact_bwd_workspace_bytes(1, 128, 3)) == int(lib.ihg_interact_bwd_workspace_bytes(10 ** 9, 128, 3)) == recorded[(128, 3)][1]


def test_missing_library_is_a_hard_error(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libihgnn_hip.so')
    with pytest.raises(_lib.IhgnnHipError, match='no CPU or PyTorch fallback'):
        _lib.load()


def test_ops_refuse_cpu_tensors():
    from ihgnn_amd import ops
    from ihgnn_amd.layout import IncidenceLayout
    import numpy as np
    lay = IncidenceLayout(np.array([[0, 0, 0], [1, 0, 1]]), 2, 1, 2, torch.device('cpu'))
    with pytest.raises(_lib.IhgnnHipError, match='no CPU path'):
        ops.edge_gather_sum(torch.zeros(5, 4), lay)
    with pytest.raises(_lib.IhgnnHipError, match='no CPU path'):
        ops.node_segment_sum(torch.zeros(2, 4), lay)


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, 'ihgnn_amd')):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.cpp', '.h')):
                assert 'oracle' not in open(os.path.join(root, fn)).read(), f'{fn} mentions the oracle'


def test_header_is_plain_c():
    """include/ihgnn_hip.h is the contract for non-Python callers: it must compile as C99 and as C++ on its own."""
    import shutil
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ihgnn_hip.h')
    for compiler, lang in (('gcc', ['-x', 'c', '-std=c99']), ('g++', ['-x', 'c++'])):
        if shutil.which(compiler) is None:
            pytest.skip(f'{compiler} not installed')
        proc = subprocess.run([compiler, '-fsyntax-only', '-Wall', '-Werror'] + lang + [header], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
