"""The aggregation kernels of ``csrc/aggregate.hip``, each launch on its own: K5 ``ihg_edge_gather_sum`` and its fp16-plane form, K7 ``ihg_node_segment_sum`` (plain, masked
and read-once instances, the split-row finish), ``ihg_node_pair_sums`` and the bag mean built on K7.

Structural cases run on EXACT inputs (small integers, power-of-two scales) and must equal the float64 reference bit for bit - a dropped, doubled, misplaced or
mis-weighted entry cannot hide; one float case per kernel instance is held per element to ``(n + 4) 2^-24 sum |terms|`` and prints its worst ``error / bound``.  The
cases, the references and both verdicts are in ``tests/aggregate_reference.py`` (guarded on the CPU by ``tests/test_aggregate_host.py``).  Every written tensor is a view
into a sentinel-filled buffer - guard rows in front and behind, the columns beyond ``dim`` - and every source is compared with its copy after the launch.
"""
import copy

import numpy as np
import pytest
import torch

import aggregate_reference as R
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

GUARD = 3                                # sentinel rows in front of and behind every payload
SENTINEL = 12345.678


def _rng(*key):
    return np.random.default_rng([ord(k) if isinstance(k, str) else int(k) for k in key])


def _to(t):
    return None if t is None else t.to(dev())


class Padded:
    """A ``[rows, dim]`` view in geometry (a) - (d) of ``aggregate_reference.geometry_of`` into a sentinel-filled ``[GUARD + rows + GUARD, ld]`` buffer on the device."""

    def __init__(self, payload, geometry):
        rows, dim = payload if isinstance(payload, tuple) else payload.shape
        ld, col0 = R.geometry_of(dim, geometry)
        self.buf = torch.full((GUARD + rows + GUARD, ld), SENTINEL, dtype=torch.float32, device=dev())
        self.view = self.buf[GUARD:GUARD + rows, col0:col0 + dim]
        self.rows, self.dim, self.col0 = rows, dim, col0
        if not isinstance(payload, tuple):
            self.view.copy_(payload)
        if geometry in ('a', 'b') and dim % 4 == 0:
            assert (self.view.data_ptr() % 16 == 0 or rows == 0) and ld % 4 == 0
        elif geometry == 'd':
            assert (self.view.data_ptr() % 16 == 4 or rows == 0) and ld % 4 == 0
        elif geometry == 'c':
            assert ld % 4 != 0
        self.before = self.buf.clone()

    def assert_unchanged(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), f'{what}: a source was written'

    def assert_guards(self, what):
        c = self.buf.clone()
        c[GUARD:GUARD + self.rows, self.col0:self.col0 + self.dim] = SENTINEL
        assert bool((c == SENTINEL).all()), f'{what}: memory around the output (guard rows, columns beyond dim) was written'

    def assert_untouched(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before.view(torch.int32)), f'{what}: a refused call wrote into its output'


def _verdict(got, ref, exact, what):
    if exact:
        R.assert_exact(got, ref, what)
        return 0.0
    return R.assert_within_float_bound(got, ref, what)


# =============================================================================================
# K5  ihg_edge_gather_sum
# =============================================================================================
def _k5_run(dim, geometry, i3, on, exact, rng, what, bias_off=0, n_nodes=41):
    from ihgnn_amd import ops
    src_cpu, kw = R.k5_case(dim, i3, on, exact, rng, n_nodes)
    ref = R.edge_gather_reference(src_cpu, i3, **kw)
    if exact:
        R.assert_exact_condition(ref, what)
    src, out = Padded(src_cpu, geometry), Padded((i3.shape[0], dim), geometry)
    bias = None
    if on:
        bias_buf = torch.full((dim + 12,), SENTINEL, dtype=torch.float32, device=dev())
        bias = bias_buf[4 + bias_off: 4 + bias_off + dim]
        bias.copy_(kw['bias'])
        assert bias.data_ptr() % 16 == 4 * bias_off
    ops.edge_gather_sum_raw(src.view, _to(i3), _to(kw.get('node_scale')), bias, kw.get('alpha', 1.0), out=out.view, edge_scale=_to(kw.get('edge_scale')))
    torch.cuda.synchronize()
    worst = _verdict(out.view.cpu(), ref, exact, what)
    out.assert_guards(what)
    src.assert_unchanged(what)
    return worst


@pytest.mark.parametrize('geometry', ['a', 'b', 'c', 'd', 'e'])
@pytest.mark.parametrize('dim', R.ALL_DIMS)
def test_edge_gather_sum_exact(dim, geometry):
    """Hyperedge counts around a wave's share (0, 1, EPW - 1, EPW, EPW + 1, 3 EPW + 2), runs of equal users of 1 ... 7 hyperedges and a hyperedge of one node three times,
    with ``node_scale``, ``bias``, ``alpha`` and ``edge_scale`` all off and all on, in every geometry ((e): only the bias off 16-byte alignment): bit for bit."""
    bias_off, geo = (1, 'b') if geometry == 'e' else (0, geometry)
    g = R.group_lanes(dim, 1 if geometry == 'e' else R.vec_of(dim, geo))
    rng = _rng(5, dim, geometry)
    for on in ((True,) if geometry == 'e' else (False, True)):
        for n_edges in R.k5_edge_counts(g):
            i3 = torch.from_numpy(rng.integers(0, 41, (n_edges, 3)).astype(np.int32))
            _k5_run(dim, geo, i3, on, True, rng, f'K5 dim {dim} geometry {geometry} E {n_edges} options {on}', bias_off)
        _k5_run(dim, geo, R.reuse_i3(41), on, True, rng, f'K5 dim {dim} geometry {geometry} runs of equal users, options {on}', bias_off)


@pytest.mark.parametrize('dim,geometry', [(256, 'a'), (100, 'c')])
def test_edge_gather_sum_float(dim, geometry):
    rng = _rng(6, dim)
    i3 = torch.from_numpy(np.sort(rng.integers(0, 41, (1003, 3)), axis=0).astype(np.int32))
    _k5_run(dim, geometry, i3, True, False, rng, f'K5 dim {dim} geometry {geometry}')


def _device_ints(shape, gen, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=gen, device=dev()).float()


def _device_scales(n, gen):
    return torch.ldexp(torch.ones(n, device=dev()), torch.randint(-1, 3, (n,), generator=gen, device=dev()))


@pytest.mark.parametrize('dim,n_edges,geometry', [(3, (1 << 20) + 21, 'a'), (256, 196608 + 5, 'b')])
def test_edge_gather_sum_second_trip(dim, n_edges, geometry):
    """More hyperedges than one grid of waves takes in one trip (65,536 waves x EPW): the id prefetch of the NEXT trip matters from here on.  Reference and comparison
    on the device."""
    from ihgnn_amd import ops
    g = R.group_lanes(dim, R.vec_of(dim, geometry))
    assert n_edges > R.MAX_WAVES * R.k5_epw(g)
    gen = torch.Generator(device=dev()).manual_seed(dim)
    n_nodes = 1000
    i3 = torch.randint(0, n_nodes, (n_edges, 3), generator=gen, device=dev(), dtype=torch.int32)
    i3[:, 0] = torch.sort(i3[:, 0]).values                                               # users in runs, as the layout numbers them
    src = Padded(_device_ints((n_nodes, dim), gen), geometry)
    out = Padded((n_edges, dim), geometry)
    node_scale, edge_scale, bias = _device_scales(n_nodes, gen), _device_scales(n_edges, gen), _device_ints((dim,), gen)
    ops.edge_gather_sum_raw(src.view, i3, node_scale, bias, 0.5, out=out.view, edge_scale=edge_scale)
    torch.cuda.synchronize()
    ref = R.edge_gather_reference(src.view, i3, node_scale, bias, 0.5, edge_scale)
    R.assert_exact_condition(ref, f'K5 second trip dim {dim}')
    R.assert_exact(out.view, ref, f'K5 second trip dim {dim}')
    out.assert_guards(f'K5 second trip dim {dim}')
    src.assert_unchanged(f'K5 second trip dim {dim}')


# =============================================================================================
# ihg_edge_gather_sum_planes (d = 256)
# =============================================================================================
def _planes_launch(src_view, i3, node_scale, edge_scale, planes, inv):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    ld_src = int(src_view.stride(0))
    rc = lib.ihg_edge_gather_sum_planes(ops._ptr(src_view), ld_src, ops._ptr(i3), ops._ptr(node_scale), ops._ptr(edge_scale), ops._ptr(planes), ops._ptr(inv),
                                        int(i3.shape[0]), 256, ops._stream())
    torch.cuda.synchronize()
    return rc


def _planes_buffers(n_edges):
    planes = Padded((n_edges, 256), 'a')
    inv_buf = torch.full((8 + n_edges + 8,), SENTINEL, dtype=torch.float32, device=dev())
    return planes, inv_buf, inv_buf[8:8 + n_edges]


@pytest.mark.parametrize('geometry', ['a', 'b'])
@pytest.mark.parametrize('scaled', [False, True])
def test_edge_gather_sum_planes_exact(scaled, geometry):
    """E = 1 ... 5 (partial groups of four hyperedges) and runs of equal users, with and without ``edge_scale``: the inverse scale and both fp16 planes of every row
    are those of the numpy emulation applied to the EXACT row."""
    from ihgnn_amd import _lib
    from split_emulation import split_two_fp16
    rng = _rng(7, scaled, geometry)
    for i3 in [torch.from_numpy(rng.integers(0, 41, (e, 3)).astype(np.int32)) for e in (1, 2, 3, 4, 5)] + [R.reuse_i3(41)]:
        what = f'planes E {i3.shape[0]} edge_scale {scaled} geometry {geometry}'
        n_edges = int(i3.shape[0])
        src_cpu = R.features(rng, 41, 256, True)
        src_cpu[i3[0].long()] = 0                                                        # the first hyperedge's row is all zeros
        node_scale = R.scales(rng, 41, True)
        edge_scale = R.scales(rng, n_edges, True) if scaled else None
        ref = R.edge_gather_reference(src_cpu, i3, node_scale, None, 1.0, edge_scale)
        R.assert_exact_condition(ref, what)
        src = Padded(src_cpu, geometry)
        planes, inv_buf, inv = _planes_buffers(n_edges)
        assert _planes_launch(src.view, _to(i3), _to(node_scale), _to(edge_scale), planes.view, inv) == _lib.OK, what
        want = ref.want.numpy().astype(np.float32)
        expo = np.clip(((np.abs(want).max(1).view(np.uint32) >> 23) & 0xff).astype(np.int64), 27, 227)      # scale_up_for: the row's largest magnitude to [2^13, 2^14)
        want_inv = np.ldexp(1.0, expo - 13 - 127).astype(np.float32)
        hi, lo = split_two_fp16((want / want_inv[:, None]).astype(np.float32))
        halves = planes.view.cpu().view(torch.float16).view(n_edges, 2, 256).float().numpy()
        np.testing.assert_array_equal(inv.cpu().numpy(), want_inv, err_msg=what)
        np.testing.assert_array_equal(halves[:, 0], hi.astype(np.float32), err_msg=what)
        np.testing.assert_array_equal(halves[:, 1], lo.astype(np.float32), err_msg=what)
        assert (halves[0] == 0).all()
        planes.assert_guards(what)
        assert bool((inv_buf[:8] == SENTINEL).all()) and bool((inv_buf[8 + n_edges:] == SENTINEL).all()), f'{what}: memory around inv_scale was written'
        src.assert_unchanged(what)


@pytest.mark.parametrize('geometry', ['c', 'd'])
def test_edge_gather_sum_planes_refuses_unaligned_sources(geometry):
    from ihgnn_amd import _lib
    rng = _rng(8, geometry)
    i3 = torch.from_numpy(rng.integers(0, 41, (5, 3)).astype(np.int32))
    src = Padded(R.features(rng, 41, 256, True), geometry)
    planes, inv_buf, inv = _planes_buffers(5)
    inv_before = inv_buf.clone()
    assert _planes_launch(src.view, _to(i3), None, None, planes.view, inv) == _lib.ERR_INVALID
    planes.assert_untouched(f'planes geometry {geometry}')
    assert torch.equal(inv_buf, inv_before)


def test_edge_gather_sum_planes_second_trip():
    """E = 262,144 + 3 > 65,536 waves x 4 hyperedges: the same split done with torch on the device (fp16 round-to-nearest-even twice)."""
    from ihgnn_amd import _lib
    n_edges, n_nodes = 262144 + 3, 1000
    assert n_edges > R.MAX_WAVES * R.K5_UPLANES
    gen = torch.Generator(device=dev()).manual_seed(11)
    i3 = torch.randint(0, n_nodes, (n_edges, 3), generator=gen, device=dev(), dtype=torch.int32)
    i3[:, 0] = torch.sort(i3[:, 0]).values
    src = Padded(_device_ints((n_nodes, 256), gen), 'b')
    node_scale, edge_scale = _device_scales(n_nodes, gen), _device_scales(n_edges, gen)
    planes, inv_buf, inv = _planes_buffers(n_edges)
    assert _planes_launch(src.view, i3, node_scale, edge_scale, planes.view, inv) == _lib.OK
    ref = R.edge_gather_reference(src.view, i3, node_scale, None, 1.0, edge_scale)
    R.assert_exact_condition(ref, 'planes second trip')
    want = ref.want.float()
    expo = ((want.abs().amax(1).view(torch.int32) >> 23) & 0xff).clamp(27, 227)
    want_inv = torch.ldexp(torch.ones_like(inv), expo - 140)
    scaled = want / want_inv[:, None]
    hi = scaled.half()
    lo = (scaled - hi.float()).half()
    halves = planes.view.view(torch.float16).view(n_edges, 2, 256)
    assert torch.equal(inv, want_inv) and torch.equal(halves[:, 0], hi) and torch.equal(halves[:, 1], lo)
    planes.assert_guards('planes second trip')
    assert bool((inv_buf[:8] == SENTINEL).all()) and bool((inv_buf[8 + n_edges:] == SENTINEL).all())
    src.assert_unchanged('planes second trip')


# =============================================================================================
# K7  ihg_node_segment_sum
# =============================================================================================
def _csr(ptr, ids, heavy_threshold, heavy_chunk=None):
    from ihgnn_amd.layout import Csr
    return Csr(ptr, ids, dev(), heavy_threshold=heavy_threshold, heavy_chunk=heavy_chunk)


def _without_order(csr):
    other = copy.copy(csr)
    other.row_order = None
    return other


def _k7_launch(src_cpu, kw, csr, geometry, what, rows=None, read_once=False, row_range=None):
    """One launch into a padded output (pre-filled with ``acc_in`` when the case accumulates); masked source rows hold NaN.  Returns the payload (CPU)."""
    from ihgnn_amd import ops
    src_cpu = src_cpu.clone()
    mask = kw.get('src_mask')
    if mask is not None:
        src_cpu[mask == 0] = float('nan')
    acc_in = kw.get('acc_in')
    n_rows, dim = len(csr.ptr_host) - 1, src_cpu.shape[1]
    src, out = Padded(src_cpu, geometry), Padded(acc_in if acc_in is not None else (n_rows, dim), geometry)
    target, out_scale, launch_csr = out.view, _to(kw.get('out_scale')), csr
    if row_range is not None:
        b, e = row_range
        launch_csr, target, out_scale = csr.row_slice(b, e), out.view[b:e], None if out_scale is None else out_scale[b:e]
    ops.node_segment_sum_raw(src.view, launch_csr, _to(kw.get('src_scale')), out_scale, kw.get('mode', 0), out=target, entry_scale=_to(kw.get('entry_scale')),
                             self_weight=_to(kw.get('self_weight')), rows=_to(rows), src_mask=_to(mask), accumulate=acc_in is not None, read_once=read_once)
    torch.cuda.synchronize()
    out.assert_guards(what)
    src.assert_unchanged(what)
    return out.view.cpu()


def _k7_check(src_cpu, kw, csr, geometry, exact, what, written=None, **launch):
    """Launch and verdict.  ``written`` (bool per row): only these rows are computed, the others must keep what the output held (the sentinel, or ``acc_in``)."""
    ref = R.segment_sum_reference(src_cpu, torch.from_numpy(csr.ptr_host), torch.from_numpy(csr.ids_host), **kw)
    if exact:
        R.assert_exact_condition(ref, what)
    got = _k7_launch(src_cpu, kw, csr, geometry, what, **launch)
    if written is not None:
        kept = kw['acc_in'].double() if 'acc_in' in kw else torch.full_like(ref.want, float(torch.tensor(SENTINEL, dtype=torch.float32)))
        assert torch.equal(got[~written], kept[~written].float()), f'{what}: a row that is neither listed nor split was written'
        got, ref = got[written], R.Ref(ref.want[written], ref.mag[written], ref.peak[written], ref.n[written])
    assert bool(torch.isfinite(got).all()), f'{what}: a masked (NaN) source row reached the result'
    return got, _verdict(got, ref, exact, what)


def _light_csr(dim, geometry, rng, n_src=None):
    g = R.group_lanes(dim, R.vec_of(dim, geometry))
    lengths = R.light_lengths(g, rng)
    n_src = n_src or len(lengths) + 5
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    return _csr(ptr, ids, 0), n_src, lengths


@pytest.mark.parametrize('geometry', R.GEOMETRIES)
@pytest.mark.parametrize('dim', R.ALL_DIMS)
def test_node_segment_sum_light_rows_exact(dim, geometry):
    """Row lengths at the lane-group and unroll boundaries (0, 1, G - 1, G, G + 1, 7 ... 9, 15 ... 17, 2 G + 3, 200; a 200-entry row between empty ones), walked in file
    order and in the layout's order by decreasing length: both exact, hence bitwise equal."""
    rng = _rng(9, dim, geometry)
    csr, n_src, _ = _light_csr(dim, geometry, rng)
    assert csr.row_order is not None and csr.n_heavy == 0
    for options in ((), R.K7_ALL_ON):
        src, kw = R.k7_case(csr.ptr_host, csr.ids_host, n_src, dim, options, True, rng)
        what = f'K7 light rows dim {dim} geometry {geometry} options {options}'
        ordered, _ = _k7_check(src, kw, csr, geometry, True, what)
        in_file_order, _ = _k7_check(src, kw, _without_order(csr), geometry, True, what + ', file order')
        assert torch.equal(ordered, in_file_order)


OPTION_SETS = [('src_scale',), ('entry_scale',), (), ('mode1',), ('mode2',), ('self_weight',), ('accumulate',), ('src_scale', 'entry_scale', 'mode2', 'self_weight', 'accumulate')]


@pytest.mark.parametrize('geometry', ['a', 'd'])
@pytest.mark.parametrize('dim', [16, 100, 256])
def test_node_segment_sum_options_exact(dim, geometry):
    """Each option alone against the independent sum, then all together; ``read_once`` (the non-temporal instance) bitwise the plain one."""
    rng = _rng(10, dim, geometry)
    csr, n_src, _ = _light_csr(dim, geometry, rng)
    for options in OPTION_SETS:
        src, kw = R.k7_case(csr.ptr_host, csr.ids_host, n_src, dim, options, True, rng)
        what = f'K7 dim {dim} geometry {geometry} options {options}'
        if 'mode2' in options:
            assert bool((kw['out_scale'] == 0).any())
        plain, _ = _k7_check(src, kw, csr, geometry, True, what)
        once, _ = _k7_check(src, kw, csr, geometry, True, what + ', read_once', read_once=True)
        assert torch.equal(plain, once)


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('dim', [16, 100, 256])
def test_node_segment_sum_row_subset_exact(dim, accumulate):
    """``rows=``: the listed rows and the plan's split rows are written (a split row that is also listed once), every other row keeps what it held."""
    rng = _rng(12, dim, accumulate)
    g = R.group_lanes(dim, R.vec_of(dim, 'b'))
    lengths = R.light_lengths(g, rng)
    n_src = len(lengths) + 5
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = _csr(ptr, ids, 150, 32)                                                        # the 200-entry rows are split: seven segments
    heavy = np.flatnonzero(np.diff(ptr) > 150)
    assert csr.n_heavy == len(heavy) == 3
    light = np.flatnonzero(np.diff(ptr) <= 150)
    listed = np.concatenate([rng.permutation(light)[: len(light) // 3], heavy[:1]]).astype(np.int32)
    written = torch.zeros(len(lengths), dtype=torch.bool)
    written[torch.from_numpy(np.concatenate([listed, heavy]).astype(np.int64))] = True
    assert 0 < int(written.sum()) < len(lengths) - 5
    options = ('src_scale', 'mode1', 'self_weight') + (('accumulate',) if accumulate else ())
    src, kw = R.k7_case(ptr, ids, n_src, dim, options, True, rng)
    _k7_check(src, kw, csr, 'b', True, f'K7 rows= dim {dim} accumulate {accumulate}', written=written, rows=torch.from_numpy(listed))


@pytest.mark.parametrize('listed', [0.02, 0.5])
@pytest.mark.parametrize('dim', [16, 100, 256])
def test_node_segment_sum_source_mask_exact(dim, listed):
    """The masked instance: unlisted source rows hold NaN and must not be fetched (by id, or as a row's own ``self_weight`` term); one row's ids are all unlisted."""
    rng = _rng(13, dim, int(listed * 100))
    for geometry in ('a', 'c'):
        csr, n_src, lengths = _light_csr(dim, geometry, rng, n_src=400)
        dead_row = lengths.index(17)
        for options in (('src_mask',), ('src_mask', 'self_weight'), R.K7_ALL_ON):
            src, kw = R.k7_case(csr.ptr_host, csr.ids_host, n_src, dim, options, True, rng, listed=listed, dead_row=dead_row)
            share = float(kw['src_mask'].float().mean())
            assert 0 < share < 2 * listed + 0.02
            what = f'K7 masked dim {dim} geometry {geometry} listed {share:.3f} options {options}'
            got, _ = _k7_check(src, kw, csr, geometry, True, what)
            if options == ('src_mask',):
                assert bool((got[dead_row] == 0).all())


LADDER_OPTIONS = [(), ('self_weight', 'src_scale'), ('src_mask', 'self_weight'), ('accumulate', 'mode1'), ('mode2', 'entry_scale'), R.K7_ALL_ON]


@pytest.mark.parametrize('dim,geometry', [(d, 'b') for d in R.ALL_DIMS] + [(16, 'd'), (100, 'c'), (256, 'c'), (320, 'a'), (8, 'a')])
def test_node_segment_sum_split_rows_exact(dim, geometry):
    """Rows of GROUPS - 1 ... 33 GROUPS + 3 segments (two entries each; one odd row; light rows of 0 ... 2 entries): every trip count of the finish kernel's 16-deep loop,
    4-deep loop and tail, its epilogue with every option; exact, and bitwise repeatable."""
    rng = _rng(14, dim, geometry)
    g = R.group_lanes(dim, R.vec_of(dim, geometry))
    lengths = R.ladder_lengths(g, rng)
    n_src = len(lengths) + 5
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = _csr(ptr, ids, 2, 2)
    counts = np.diff(csr.heavy_segptr.cpu().numpy())
    assert sorted(counts) == sorted(R.ladder_segment_counts(g) + [6]) and counts.max() == 33 * R.finish_groups(g) + 3
    for options in LADDER_OPTIONS:
        src, kw = R.k7_case(ptr, ids, n_src, dim, options, True, rng)
        what = f'K7 split rows dim {dim} geometry {geometry} options {options}'
        first, _ = _k7_check(src, kw, csr, geometry, True, what)
        again, _ = _k7_check(src, kw, csr, geometry, True, what + ' (again)')
        assert torch.equal(first, again)


@pytest.mark.parametrize('dim', [16, 100, 256])
def test_node_segment_sum_capped_segments_exact(dim, monkeypatch):
    """At most ``HEAVY_MAX_SEGMENTS`` segments per row: a 101-entry row gets seven segments of 14 and one of 3."""
    from ihgnn_amd import layout
    monkeypatch.setattr(layout, 'HEAVY_MAX_SEGMENTS', 8)
    rng = _rng(15, dim)
    lengths = [1, 101, 2, 0, 7, 2]
    ptr, ids = R.csr_from_lengths(lengths, 11, rng)
    csr = _csr(ptr, ids, 2, 2)
    assert (csr.seg_end - csr.seg_begin).tolist() == [14] * 7 + [3] + [2, 2, 2, 1]
    for options in ((), R.K7_ALL_ON):
        src, kw = R.k7_case(ptr, ids, 11, dim, options, True, rng)
        _k7_check(src, kw, csr, 'b', True, f'K7 capped segments dim {dim} options {options}')


@pytest.mark.parametrize('dim', [16, 100, 256])
def test_node_segment_sum_row_slice_exact(dim):
    """``Csr.row_slice``: a bumped row pointer and output pointer; the slice's long rows are summed in place by the light kernel; rows outside the slice keep the sentinel."""
    rng = _rng(16, dim)
    g = R.group_lanes(dim, R.vec_of(dim, 'b'))
    lengths = R.ladder_lengths(g, rng)
    n_src, n = len(lengths) + 5, len(lengths)
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = _csr(ptr, ids, 2, 2)
    src, kw = R.k7_case(ptr, ids, n_src, dim, ('src_scale', 'entry_scale', 'mode1'), True, rng)
    longest = int(np.argmax(lengths))
    for b, e in ((0, n), (3, n - 2), (longest, longest + 1)):
        written = torch.zeros(n, dtype=torch.bool)
        written[b:e] = True
        _k7_check(src, kw, csr, 'b', True, f'K7 row slice [{b}, {e}) dim {dim}', written=written, row_range=(b, e))


@pytest.mark.parametrize('dim,geometry', [(16, 'a'), (100, 'c'), (256, 'b')])
def test_node_segment_sum_float(dim, geometry):
    """One float case per instance (plain, read-once, masked; light and split rows): per element within (n + 4) 2^-24 sum |terms|."""
    rng = _rng(17, dim)
    g = R.group_lanes(dim, R.vec_of(dim, geometry))
    lengths = R.light_lengths(g, rng) + [600, 1200, 4230]
    n_src = 300
    ptr, ids = R.csr_from_lengths(lengths, n_src, rng)
    csr = _csr(ptr, ids, 256, 16)
    assert csr.n_heavy == 3
    worst = {}
    for name, options, launch in (('plain', ('src_scale', 'entry_scale', 'mode1', 'self_weight', 'accumulate'), {}),
                                  ('read_once', ('src_scale', 'mode2'), dict(read_once=True)), ('masked', R.K7_ALL_ON, {})):
        src, kw = R.k7_case(ptr, ids, n_src, dim, options, False, rng)
        _, worst[name] = _k7_check(src, kw, csr, geometry, False, f'K7 {name} dim {dim} geometry {geometry}', **launch)
    assert max(worst.values()) > 0


@pytest.mark.parametrize('dim,n_rows,geometry', [(16, (1 << 20) + 40, 'a'), (256, 65536 + 9, 'b')])
def test_node_segment_sum_second_trip(dim, n_rows, geometry):
    """More rows than one grid of waves takes in one trip (65,536 waves x 64 / G rows), rows of 0 ... 3 entries; reference and comparison on the device."""
    from ihgnn_amd import ops
    g = R.group_lanes(dim, R.vec_of(dim, geometry))
    assert n_rows > R.MAX_WAVES * (R.WAVE // g)
    rng = _rng(18, dim)
    n_src = 1000
    ptr, ids = R.csr_from_lengths(rng.integers(0, 4, n_rows), n_src, rng)
    csr = _csr(ptr, ids, 0)
    gen = torch.Generator(device=dev()).manual_seed(dim)
    src, out = Padded(_device_ints((n_src, dim), gen), geometry), Padded((n_rows, dim), geometry)
    src_scale, out_scale, entry_scale = _device_scales(n_src, gen), _device_scales(n_rows, gen), _device_ints((len(ids),), gen, 1, 5)
    ops.node_segment_sum_raw(src.view, csr, src_scale, out_scale, 1, out=out.view, entry_scale=entry_scale)
    torch.cuda.synchronize()
    ref = R.segment_sum_reference(src.view, csr.ptr, csr.ids, src_scale, entry_scale, out_scale, 1)
    what = f'K7 second trip dim {dim}'
    R.assert_exact_condition(ref, what)
    R.assert_exact(out.view, ref, what)
    out.assert_guards(what)
    src.assert_unchanged(what)


# =============================================================================================
# ihg_node_pair_sums
# =============================================================================================
def _pair_sums(h, csr, out, pair_weight, dim):
    """The library call of ``ops.node_pair_sums_raw`` on a hand-built pair list; returns the status."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    heavy = csr.n_heavy > 0
    p = ops._ptr
    rc = lib.ihg_node_pair_sums(p(h), ops._ld(h), p(csr.ptr), p(csr.ids), p(csr.row_order), p(out), ops._ld(out), csr.n_rows, dim,
                                csr.heavy_threshold if heavy else 0, p(csr.seg_begin) if heavy else None, p(csr.seg_end) if heavy else None,
                                csr.n_segments if heavy else 0, p(csr.heavy_rows) if heavy else None, p(csr.heavy_segptr) if heavy else None, csr.n_heavy,
                                p(csr.partials(3 * dim)) if heavy else None, p(pair_weight), ops._stream())
    torch.cuda.synchronize()
    return rc


def _pair_check(h_cpu, csr, pair_weight, geometry, exact, what):
    from ihgnn_amd import _lib
    dim = h_cpu.shape[1]
    ref = R.pair_sums_reference(h_cpu, torch.from_numpy(csr.ptr_host), torch.from_numpy(csr.ids_host), pair_weight)
    if exact:
        R.assert_exact_condition(ref, what, bits=0)
    h, out = Padded(h_cpu, geometry), Padded((csr.n_rows, 3 * dim), geometry)
    assert _pair_sums(h.view, csr, out.view, _to(pair_weight), dim) == _lib.OK, what
    got = out.view.cpu()
    worst = _verdict(got, ref, exact, what)
    out.assert_guards(what)
    h.assert_unchanged(what)
    return got, worst


def _pair_csrs(dim, rng):
    g = R.group_lanes(dim, 4)
    light = [2 * k for k in rng.permutation([0, 1, g // 2, g // 2 + 1, 0, 3, g, 2 * g + 1, 100])]
    ladder = R.pair_ladder_lengths(g, rng)
    n_src = 37
    return g, n_src, _csr(*R.csr_from_lengths(light, n_src, rng), 0), _csr(*R.csr_from_lengths(ladder, n_src, rng), 2, 2)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('dim', [8, 16, 32, 64, 128, 256])
def test_node_pair_sums_exact(dim, weighted):
    """``S_a | S_b | S_ab`` over hand-built pair lists: rows of 0, 1, G / 2, G / 2 + 1 ... pairs, and the split-row ladder with one pair per segment (the finish over
    3 d columns, ``gridDim.y >= 3`` from d = 16 x 4 lanes up), contiguous and as column slices; the ladder bitwise repeatable."""
    rng = _rng(19, dim, weighted)
    g, n_src, light, ladder = _pair_csrs(dim, rng)
    counts = np.diff(ladder.heavy_segptr.cpu().numpy())
    assert sorted(counts) == sorted(R.ladder_segment_counts(g)) and light.n_heavy == 0
    assert bool(((ladder.seg_end - ladder.seg_begin) == 2).all())
    for geometry in ('a', 'b'):
        for name, csr in (('light rows', light), ('ladder', ladder)):
            h = R.features(rng, n_src, dim, True)
            pw = R.weights(rng, len(csr.ids_host) // 2, True) if weighted else None
            what = f'pair sums {name} dim {dim} weighted {weighted} geometry {geometry}'
            first, _ = _pair_check(h, csr, pw, geometry, True, what)
            if name == 'ladder':
                again, _ = _pair_check(h, csr, pw, geometry, True, what + ' (again)')
                assert torch.equal(first, again)


@pytest.mark.parametrize('geometry', ['c', 'd'])
@pytest.mark.parametrize('dim', [16, 256])
def test_node_pair_sums_refuses_unaligned_operands(dim, geometry):
    from ihgnn_amd import _lib
    rng = _rng(20, dim, geometry)
    _, n_src, light, ladder = _pair_csrs(dim, rng)
    for csr in (light, ladder):
        for bad_h, bad_out in ((True, False), (False, True), (True, True)):
            h, out = Padded(R.features(rng, n_src, dim, True), geometry if bad_h else 'b'), Padded((csr.n_rows, 3 * dim), geometry if bad_out else 'b')
            assert _pair_sums(h.view, csr, out.view, None, dim) == _lib.ERR_INVALID
            out.assert_untouched(f'pair sums dim {dim} geometry {geometry}')


@pytest.mark.parametrize('dim,weighted', [(64, False), (256, True)])
def test_node_pair_sums_float(dim, weighted):
    rng = _rng(21, dim)
    g = R.group_lanes(dim, 4)
    lengths = [2 * k for k in [0, 1, g // 2 + 1, 100, 3] + R.ladder_segment_counts(g)]
    n_src = 300
    csr = _csr(*R.csr_from_lengths(lengths, n_src, rng), 2, 2)
    h = R.features(rng, n_src, dim, False)
    pw = R.weights(rng, len(csr.ids_host) // 2, False) if weighted else None
    _, worst = _pair_check(h, csr, pw, 'b', False, f'pair sums dim {dim} weighted {weighted}')
    assert worst > 0


def test_node_pair_sums_second_trip():
    """65,536 + 7 rows of one pair at d = 256 (one row per wave): a second trip of the grid-stride loop; on the device."""
    from ihgnn_amd import _lib
    dim, n_rows, n_src = 256, 65536 + 7, 1000
    assert n_rows > R.MAX_WAVES * (R.WAVE // R.group_lanes(dim, 4))
    rng = _rng(22)
    csr = _csr(*R.csr_from_lengths([2] * n_rows, n_src, rng), 0)
    gen = torch.Generator(device=dev()).manual_seed(22)
    h, out = Padded(_device_ints((n_src, dim), gen), 'b'), Padded((n_rows, 3 * dim), 'b')
    pw = _device_ints((n_rows,), gen, 1, 5)
    assert _pair_sums(h.view, csr, out.view, pw, dim) == _lib.OK
    ref = R.pair_sums_reference(h.view, csr.ptr, csr.ids, pw)
    R.assert_exact_condition(ref, 'pair sums second trip', bits=0)
    R.assert_exact(out.view, ref, 'pair sums second trip')
    out.assert_guards('pair sums second trip')
    h.assert_unchanged('pair sums second trip')


# =============================================================================================
# bag mean (ops.bag_mean: K7 in divide mode forward, K7 over the transposed lists backward)
# =============================================================================================
BAG_WORDS = 50                           # table rows 1 ... 50 are words, row 0 is the padding row that no bag holds
EVERYWHERE = 7                           # the word that every one of the 5,000 bags holds


def _bags(rng, special, common):
    """Bags of the ``special`` lengths (three of each) in front of and behind 5,000 bags of the ``common`` lengths that all hold word ``EVERYWHERE``."""
    lens = list(special) * 3
    lens = lens[: len(lens) // 2] + [int(x) for x in rng.choice(common, 5000)] + lens[len(lens) // 2:]
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    words = rng.integers(1, BAG_WORDS + 1, int(ptr[-1]))
    first = len(special) * 3 // 2
    words[ptr[first:first + 5000]] = EVERYWHERE
    return ptr, words


def _bag_run(dim, ptr, words, exact, rng, what):
    """Forward and backward through ``ops.bag_mean``; the forward once more through the same launch into a padded output.  Returns the worst error / bound (float)."""
    from ihgnn_amd import ops
    n_bags = len(ptr) - 1
    bag = ops.BagLayout(words, ptr[:-1], BAG_WORDS + 1, dev())
    assert bag.words_of.n_heavy == 0 and int(np.diff(bag.words_of.ptr_host).max()) >= 5000      # a long transposed row, no split plan
    table_cpu, dout_cpu = R.features(rng, BAG_WORDS + 1, dim, exact), R.features(rng, n_bags, dim, exact)
    table = Padded(table_cpu, 'b')
    leaf = table.view.detach().requires_grad_(True)
    got = ops.bag_mean(leaf, bag)
    got.backward(_to(dout_cpu))
    padded = Padded((n_bags, dim), 'b')
    with torch.no_grad():
        ops._query_rows_forward(table.view, bag, None, None, 0, padded.view)
    torch.cuda.synchronize()
    assert torch.equal(padded.view, got)
    padded.assert_guards(what)
    table.assert_unchanged(what)
    t_ptr, t_words, lens = torch.from_numpy(ptr), torch.from_numpy(words), torch.from_numpy(np.diff(ptr))
    fwd = R.segment_sum_reference(table_cpu, t_ptr, t_words, out_scale=lens.float(), mode=2)
    bwd = R.bag_mean_backward_reference(dout_cpu, t_ptr, t_words, BAG_WORDS + 1)
    got, grad = got.detach().cpu(), leaf.grad.cpu()
    assert bool((got[lens == 0] == 0).all()) and bool((grad[0] == 0).all()), f'{what}: an empty bag or the padding row is not zero'
    if exact:
        total = R.segment_sum_reference(table_cpu, t_ptr, t_words)
        R.assert_exact_condition(total, what, bits=0)
        R.assert_mean_of_exact_sum(got, total.want, lens, what)
        R.assert_exact_condition(bwd, what, bits=6)                                      # 1 / len down to 1 / 64
        R.assert_exact(grad, bwd, what + ', backward')
        return 0.0
    return max(R.assert_within_float_bound(got, fwd, what + ', forward'), R.assert_within_float_bound(grad, bwd, what + ', backward'))


@pytest.mark.parametrize('dim', [8, 100, 128, 256])
def test_bag_mean_exact(dim):
    """Bags of 0, 1, 2, 4, 64 words (powers of two: 1 / len is exact) and one word in 5,000 bags: every mean is ``float32(exact sum / len)`` or its neighbour, the
    gradient of the table is exact, an empty bag gives zeros and takes no part in the gradient, the padding row's gradient is zero."""
    rng = _rng(23, dim)
    ptr, words = _bags(rng, (0, 1, 2, 4, 64), (1, 2, 4))
    _bag_run(dim, ptr, words, True, rng, f'bag mean dim {dim}')


@pytest.mark.parametrize('dim', [8, 100, 128, 256])
def test_bag_mean_float(dim):
    """Bags of 0, 1, 2, 3, 64 words: forward and backward per element within (n + 4) 2^-24 sum |terms|."""
    rng = _rng(24, dim)
    ptr, words = _bags(rng, (0, 1, 2, 3, 64), (1, 2, 3))
    assert _bag_run(dim, ptr, words, False, rng, f'bag mean dim {dim}') > 0


def test_bag_mean_of_exact_inputs_with_odd_lengths():
    """Lengths 3, 5, 6, 7 on exact inputs: the division is IEEE (no fast-math), every mean within one float of ``exact sum / len``."""
    from ihgnn_amd import ops
    rng = _rng(25)
    ptr, words = _bags(rng, (0, 3, 5, 6, 7), (3, 5, 7))
    bag = ops.BagLayout(words, ptr[:-1], BAG_WORDS + 1, dev())
    table = R.features(rng, BAG_WORDS + 1, 100, True)
    got = ops.bag_mean(_to(table), bag).cpu()
    total = R.segment_sum_reference(table, torch.from_numpy(ptr), torch.from_numpy(words))
    R.assert_exact_condition(total, 'bag mean, odd lengths', bits=0)
    R.assert_mean_of_exact_sum(got, total.want, torch.from_numpy(np.diff(ptr)), 'bag mean, odd lengths')


@pytest.mark.parametrize('dim', [8, 100])
def test_bag_mean_entries_are_k7_launches(dim):
    """``ihg_bag_mean_fwd`` / ``ihg_bag_mean_bwd`` through the binding, bags of 0, 1, 2, 3, 64, 4, 0 words: bit for bit what ``node_segment_sum_raw`` gives for the same
    operands - the bags divided by ``bag_len`` forward, the transposed lists with ``src_scale = inv_len`` backward (dim 100: 25 float4 columns on 32 lanes)."""
    from ihgnn_amd import _lib, ops
    from ihgnn_amd.ops import _ld, _ptr, _stream
    rng = _rng(26, dim)
    lens = np.array([0, 1, 2, 3, 64, 4, 0])
    ptr = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    words = rng.integers(1, BAG_WORDS + 1, int(ptr[-1]))
    bag = ops.BagLayout(words, ptr[:-1], BAG_WORDS + 1, dev())
    lib = _lib.load()
    table, dout = _to(R.features(rng, BAG_WORDS + 1, dim, False)), _to(R.features(rng, len(lens), dim, False))
    means = torch.full((len(lens), dim), float('nan'), device=dev())
    _lib.check(lib.ihg_bag_mean_fwd(_ptr(table), _ld(table), _ptr(bag.bags.ptr), _ptr(bag.bags.ids), _ptr(bag.bag_len), _ptr(means), _ld(means), len(lens), dim, _stream()),
               'ihg_bag_mean_fwd')
    grad = torch.full((BAG_WORDS + 1, dim), float('nan'), device=dev())
    _lib.check(lib.ihg_bag_mean_bwd(_ptr(dout), _ld(dout), _ptr(bag.words_of.ptr), _ptr(bag.words_of.ids), _ptr(bag.inv_len), _ptr(grad), _ld(grad), BAG_WORDS + 1, dim,
                                    _stream()), 'ihg_bag_mean_bwd')
    assert bag.bags.n_heavy == 0 and bag.words_of.n_heavy == 0
    want_means = ops.node_segment_sum_raw(table, bag.bags, None, bag.bag_len, _lib.SCALE_DIVIDE)
    want_grad = ops.node_segment_sum_raw(dout, bag.words_of, bag.inv_len, None, _lib.SCALE_NONE)
    torch.cuda.synchronize()
    empty = torch.from_numpy(lens == 0)
    assert bool(torch.isfinite(means).all()) and bool((means.cpu()[empty] == 0).all()) and bool((means.cpu()[~empty] != 0).any()) and bool(torch.isfinite(grad).all())
    assert torch.equal(means, want_means) and torch.equal(grad, want_grad)
