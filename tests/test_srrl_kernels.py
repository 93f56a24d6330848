"""The kernels of the Srrl baseline (``csrc/srrl.hip``) through the C ABI, per entry against float64 (``tests/srrl_reference.py``) with the any-order bounds derived
there, into NaN-prefilled buffers with guard rows and exact-size workspaces; ``dW`` / ``dbias`` bitwise across two runs; the top-k exactly.

Row counts: the any-width kernels stage 16 rows per workgroup trip, the matrix-core kernels (K = 64 / 128, aligned rows) 128 / 64 in the forward and 32 in the backward,
so 0 / 1 / 15 / 16 / 17 / 33 / 65 / 129 cover the empty problem, partial tiles, full ones and the tails after them.  One past a single trip of a grid: the any-width forward
holds 2048 workgroups (32768 rows) and both backwards 64 (1024 rows any-width, 2048 on the matrix cores); the matrix-core forward 1024 (131072 rows at K = 64, 65536 at
K = 128)."""
import ctypes

import numpy as np
import pytest
import torch

import srrl_reference as sref
from ihgnn_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 2
TINY = float(np.finfo(np.float32).tiny)
ROW_LADDER = (0, 1, 15, 16, 17, 33, 65, 129, 1025, 2049, 32769)


def dev():
    return torch.device('cuda:0')


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Out:
    """``[rows, cols]`` of a NaN-filled ``[GUARD + rows + GUARD, ld]`` device buffer; ``check()``: every payload entry written, nothing around it."""

    def __init__(self, rows, cols, ld=None):
        self.rows, self.cols, self.ld = rows, cols, cols if ld is None else ld
        self.buf = torch.full((GUARD + rows + GUARD, self.ld), float('nan'), dtype=torch.float32, device=dev())
        self.view = self.buf[GUARD:GUARD + rows, :cols]
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + GUARD * self.ld * 4)

    def check(self, what, written=True):
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + self.rows:]).all() and np.isnan(b[:, self.cols:]).all(), f'{what}: memory around the output was written'
        got = b[GUARD:GUARD + self.rows, :self.cols]
        assert np.isnan(got).all() if not written else not np.isnan(got).any(), f'{what}: {"written" if not written else "entries left unwritten"}'
        return got.astype(np.float64)


def table(rng, rows, width, misaligned=False):
    """A source table on the device: float32 ``[rows, width]``; ``misaligned``: on a base 4 bytes past a 16-byte boundary with an odd row stride."""
    host = (rng.standard_normal((rows, width)) * 10 ** rng.uniform(-1, 1, (rows, 1))).astype(np.float32)
    if not misaligned:
        return host, torch.from_numpy(host).to(dev())
    ld = width + 1 + (width % 2)                                         # odd
    flat = torch.full((1 + max(rows, 1) * ld,), float('nan'), dtype=torch.float32, device=dev())
    view = flat[1:1 + rows * ld].view(rows, ld)[:, :width]
    view.copy_(torch.from_numpy(host))
    assert (rows == 0 or view.data_ptr() % 16 == 4) and ld % 2 == 1
    return host, view


def ld_of(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def index_vector(rng, kind, groups, table_rows):
    if kind == 'none':
        return None
    idx = rng.permutation(table_rows)[:groups] if kind == 'perm' else np.full(groups, min(2, table_rows - 1))
    return idx.astype(np.int64)


class Block:
    """One case of the block: sources, weight, bias on the device and as float64."""

    def __init__(self, rows, wa, wb, m, normalize=True, leaky=True, idx_a='none', idx_b='none', rep_a=1, rep_b=1, bias=True, misaligned=False, special=False, seed=0):
        rng = np.random.default_rng(1000 * seed + 7 * rows + wa + m)
        self.rows, self.wa, self.wb, self.m, self.normalize, self.leaky, self.rep_a, self.rep_b = rows, wa, wb, m, normalize, leaky, rep_a, rep_b
        ga, gb = rows // rep_a, rows // rep_b
        assert ga * rep_a == rows and gb * rep_b == rows
        na, nb = (ga if idx_a == 'none' else ga + 3), (gb if idx_b == 'none' else gb + 3)
        self.a_host, self.a = table(rng, na, wa, misaligned)
        self.b_host, self.b = table(rng, nb, wb, misaligned) if wb else (None, None)
        if special:                                                      # one zero row and one of norm 1e-13: F.normalize's eps branch
            assert idx_a == idx_b == 'none' and rep_a == rep_b and ga >= 6
            for host, dev_t in ((self.a_host, self.a), (self.b_host, self.b)):
                if host is not None:
                    host[3] = 0.0
            cat5 = np.concatenate([self.a_host[5]] + ([self.b_host[5]] if wb else [])).astype(np.float64)
            scale = 1e-13 / np.sqrt((cat5 * cat5).sum())
            for host, dev_t in ((self.a_host, self.a), (self.b_host, self.b)):
                if host is not None:
                    host[5] = (host[5] * scale).astype(np.float32)
                    dev_t.copy_(torch.from_numpy(host))
        self.idx_a_host, self.idx_b_host = index_vector(rng, idx_a, ga, na), index_vector(rng, idx_b, gb, nb) if wb else None
        self.idx_a = None if self.idx_a_host is None else torch.from_numpy(self.idx_a_host).to(dev())
        self.idx_b = None if self.idx_b_host is None else torch.from_numpy(self.idx_b_host).to(dev())
        K = wa + wb
        self.K = K
        self.w_host = (rng.standard_normal((m, K)) / np.sqrt(K)).astype(np.float32)
        self.bias_host = (rng.standard_normal(m) * 0.1).astype(np.float32) if bias else None
        self.w = torch.from_numpy(self.w_host).to(dev())
        self.bias = None if self.bias_host is None else torch.from_numpy(self.bias_host).to(dev())
        self.x = sref.cat_rows(self.a_host, self.idx_a_host, rep_a, self.b_host, self.idx_b_host, rep_b) if rows else np.zeros((0, K))
        self.rng = rng

    def sources(self):
        a = (ptr(self.a), ld_of(self.a), self.wa, ptr(self.idx_a), self.rep_a)
        b = (ptr(self.b), ld_of(self.b), self.wb, ptr(self.idx_b), self.rep_b) if self.wb else (None, 0, 0, None, 1)
        return a + b

    def act(self):
        return _lib.ACT_LEAKY_RELU if self.leaky else _lib.ACT_NONE

    def forward(self, ld_out=None):
        lib = _lib.load()
        out, inv = Out(self.rows, self.m, ld_out), Out(1, self.rows)
        rc = lib.ihg_cat_linear_fwd(*self.sources(), ptr(self.w), self.K, ptr(self.bias), self.m, int(self.normalize), self.act(), out.ptr, out.ld,
                                    inv.ptr if self.normalize else None, self.rows, stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return out.check('out'), inv.check('inv_norm', written=self.normalize)[0]

    def backward(self, dy, y, inv, skip_a=False, skip_b=False):
        """-> (dw, dbias, da, db) as float64 (None where skipped), checked for guards and for bitwise equal dw / dbias across two runs."""
        lib = _lib.load()
        runs = []
        dy_d, y_d = torch.from_numpy(dy).to(dev()), torch.from_numpy(y).to(dev())
        inv_d = torch.from_numpy(inv.astype(np.float32)).to(dev()) if self.normalize else None
        ws_bytes = int(lib.ihg_cat_linear_workspace_bytes(self.rows, self.K, self.m))
        for _ in range(2):
            ws = torch.full((max(ws_bytes // 4, 4) + 4,), float('nan'), dtype=torch.float32, device=dev())
            dw, dbias = Out(self.m, self.K), Out(1, self.m)
            da = None if skip_a else Out(self.rows // self.rep_a, self.wa)
            db = None if skip_b or not self.wb else Out(self.rows // self.rep_b, self.wb)
            rc = lib.ihg_cat_linear_bwd(ptr(dy_d), self.m, ptr(y_d), self.m, *self.sources(), ptr(inv_d), ptr(self.w), self.K, self.m, int(self.normalize), self.act(),
                                        dw.ptr, self.K, dbias.ptr if self.bias is not None else None, None if da is None else da.ptr, self.wa, None if db is None else db.ptr,
                                        self.wb, self.rows, ptr(ws), ws_bytes, stream())
            assert rc == 0, _lib.last_error()
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws[ws_bytes // 4:]).all()), 'the workspace was written beyond its size'
            runs.append((dw.check('dw'), dbias.check('dbias', written=self.bias is not None)[0], None if da is None else da.check('da'), None if db is None else db.check('db')))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1], equal_nan=True), 'dw / dbias differ between two runs'
        return runs[0]


def inside(got, want, bound, what):
    excess = np.abs(got - want) - (bound + TINY)
    assert (excess <= 0).all(), f'{what}: off by {np.abs(got - want).max():.3e}, {excess.max():.3e} beyond its bound at {np.unravel_index(excess.argmax(), excess.shape)}'


def check_block(case, skip_a=False, skip_b=False, ld_out=None, zero_y=True):
    fwd = sref.block_forward(case.x, case.w_host, case.bias_host, case.normalize, case.leaky)
    out, inv = case.forward(ld_out)
    inside(out, fwd['y'], fwd['bound'], 'out')
    if case.normalize:
        inside(inv, fwd['inv'], fwd['bound_inv'], 'inv_norm')
    # the backward: a cotangent of its own, y as the forward rounded it with some exact zeros (the slope of a zero is 0.01), the kernel's stored inverse norms
    rng = case.rng
    dy = rng.standard_normal((case.rows, case.m)).astype(np.float32)
    y = out.astype(np.float32)
    if zero_y and y.size:
        y[rng.random(y.shape) < 0.1] = 0.0
    dw, dbias, da, db = case.backward(dy, y, inv.astype(np.float32), skip_a, skip_b)
    ref = sref.block_backward(case.x, case.w_host, dy, y, case.normalize, case.leaky, inv if case.normalize else None)
    if case.rows == 0:
        assert not dw.any() and (case.bias is None or not dbias.any())
        return
    inside(dw, ref['dw'], ref['bound_dw'], 'dw')
    if case.bias is not None:
        inside(dbias, ref['dbias'], ref['bound_dbias'], 'dbias')
    for got, lo, hi, rep, name in ((da, 0, case.wa, case.rep_a, 'da'), (db, case.wa, case.K, case.rep_b, 'db')):
        if got is None:
            continue
        want, bound = sref.group_sum(ref['dx'][:, lo:hi], ref['bound_dx'][:, lo:hi], rep)
        inside(got, want, bound, name)


@pytest.mark.parametrize('rows', ROW_LADDER)
def test_block_row_ladder(rows):
    """d = 32: the Aggregation shape (K = 64 -> 32) over the row ladder, with the eps rows where there are six rows - on the matrix cores, and from misaligned sources
    on the any-width kernels."""
    check_block(Block(rows, 32, 32, 32, special=rows >= 6))
    check_block(Block(rows, 32, 32, 32, special=rows >= 6, misaligned=True, seed=8))


@pytest.mark.parametrize('rows,wa,wb,m', [(131073, 32, 32, 32), (65537, 64, 64, 64), (65537, 128, 0, 1)])
def test_block_past_a_single_trip_of_the_matrix_core_forward(rows, wa, wb, m):
    check_block(Block(rows, wa, wb, m, special=True, seed=9))


@pytest.mark.parametrize('wa,wb,m', [(32, 32, 64), (32, 32, 1), (64, 64, 64), (64, 64, 128), (64, 64, 1), (12, 12, 24), (128, 128, 256), (128, 128, 1), (17, 7, 5)])
def test_block_widths(wa, wb, m):
    """K in {64, 128} with m in {1, d, 2d} (d = 32, 64), and the widths beside them: 24, 256, an odd pair."""
    check_block(Block(33, wa, wb, m, special=True, seed=1))


@pytest.mark.parametrize('normalize,leaky', [(True, False), (False, True), (False, False)])
def test_block_switches(normalize, leaky):
    check_block(Block(33, 32, 32, 32, normalize=normalize, leaky=leaky, special=normalize, seed=2))
    check_block(Block(17, 64, 0, 1, normalize=normalize, leaky=leaky, bias=False, seed=2))        # MLP's second Linear: one source


@pytest.mark.parametrize('idx_a,idx_b', [('perm', 'perm'), ('equal', 'none'), ('none', 'equal'), ('perm', 'equal')])
def test_block_index_vectors(idx_a, idx_b):
    check_block(Block(33, 32, 32, 32, idx_a=idx_a, idx_b=idx_b, seed=3))
    check_block(Block(17, 64, 0, 64, idx_a=idx_a, seed=3))


@pytest.mark.parametrize('groups', (1, 2, 4, 103))
@pytest.mark.parametrize('rep_a,rep_b', [(1, 10), (10, 1), (10, 10)])
def test_block_repeat_factors(groups, rep_a, rep_b):
    """rep = 10: the k negatives of a positive; 103 groups = 1030 rows, past a single trip of the backward's grid.  A repeated source with an index vector too."""
    check_block(Block(10 * groups, 32, 32, 32, rep_a=rep_a, rep_b=rep_b, idx_a='perm' if rep_a > 1 else 'none', idx_b='equal' if rep_b > 1 and groups > 1 else 'none', seed=4))


@pytest.mark.parametrize('skip_a,skip_b', [(True, False), (False, True), (True, True)])
def test_block_skipped_source_gradients(skip_a, skip_b):
    check_block(Block(33, 32, 32, 32, seed=5), skip_a=skip_a, skip_b=skip_b)
    check_block(Block(40, 32, 32, 32, rep_a=10, seed=5), skip_a=skip_a, skip_b=skip_b)


@pytest.mark.parametrize('wa,wb,m', [(32, 32, 32), (12, 12, 24), (128, 128, 32)])
def test_block_misaligned_sources_and_a_wider_output(wa, wb, m):
    """Sources 4 bytes past a 16-byte boundary with an odd row stride, and an output that is a column window (ld_out > m)."""
    check_block(Block(33, wa, wb, m, misaligned=True, special=True, seed=6), ld_out=m + 3)


def test_block_workspace_and_refusals_on_the_device():
    lib = _lib.load()
    case = Block(17, 32, 32, 32, seed=7)
    out, inv = case.forward()
    dy = torch.ones(17, 32, device=dev())
    y, inv_d = torch.from_numpy(out.astype(np.float32)).to(dev()), torch.from_numpy(inv.astype(np.float32)).to(dev())
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=dev())
    dw = Out(32, 64)
    args = lambda nbytes: (ptr(dy), 32, ptr(y), 32, *case.sources(), ptr(inv_d), ptr(case.w), 64, 32, 1, case.act(), dw.ptr, 64, None, None, 32, None, 32, 17, ptr(ws), nbytes, stream())
    assert lib.ihg_cat_linear_bwd(*args(int(lib.ihg_cat_linear_workspace_bytes(17, 64, 32)) - 4)) == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    dw.check('dw', written=False)                                        # a refused call has written nothing


# ------------------------------------------------------------------------------------------------ row dots
@pytest.mark.parametrize('rep', (1, 10))
@pytest.mark.parametrize('groups', (0, 1, 15, 16, 17, 33, 52430))
def test_rows_dot(groups, rep):
    """The same ladder (in groups), the last one past a single trip of the grid (2048 workgroups x 256 rows) at rep = 10."""
    lib = _lib.load()
    if rep == 1 and groups == 52430:
        groups = 2048 * 256 + 1
    rng = np.random.default_rng(groups + rep)
    rows, width = groups * rep, 32 if groups < 1000 else 8
    x, y = rng.standard_normal((rows, width)).astype(np.float32), rng.standard_normal((groups, width)).astype(np.float32)
    ds = rng.standard_normal(rows).astype(np.float32)
    xd, yd, dsd = (torch.from_numpy(t).to(dev()) for t in (x, y, ds))
    s, dx, dy = Out(1, rows), Out(rows, width, width + 2), Out(groups, width)
    assert lib.ihg_rows_dot_fwd(ptr(xd), width, ptr(yd), width, rep, s.ptr, rows, width, stream()) == 0, _lib.last_error()
    assert lib.ihg_rows_dot_bwd(ptr(dsd), ptr(xd), width, ptr(yd), width, rep, dx.ptr, dx.ld, dy.ptr, width, rows, width, stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    want, bound = sref.rows_dot(x, y, rep)
    inside(s.check('s')[0], want, bound, 's')
    wdx, wdy, bdx, bdy = sref.rows_dot_backward(ds, x, y, rep)
    inside(dx.check('dx'), wdx, bdx, 'dx')
    inside(dy.check('dy'), wdy, bdy, 'dy')
    only_dy = Out(groups, width)                                         # either gradient alone
    assert lib.ihg_rows_dot_bwd(ptr(dsd), ptr(xd), width, ptr(yd), width, rep, None, 0, only_dy.ptr, width, rows, width, stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(only_dy.check('dy'), dy.check('dy'))


# ------------------------------------------------------------------------------------------------ the KG loss
@pytest.mark.parametrize('weighted', (True, False))
@pytest.mark.parametrize('k', (1, 10))
@pytest.mark.parametrize('batch', (1, 16, 100, 300))
def test_kg_loss(batch, k, weighted):
    """B in {1, 16, 100} and one batch past a single trip of the workgroup (256 rows); scores at +-40 for logsigmoid's tails.  Bounds: every logsigmoid / sigmoid is a
    few library roundings (expf, log1pf, a division: 8 u), the weight sum and the weighted sums add B (+ k) terms in some order."""
    lib = _lib.load()
    rng = np.random.default_rng(batch + k)
    pos, neg = (rng.standard_normal(batch) * 3).astype(np.float32), (rng.standard_normal((batch, k)) * 3).astype(np.float32)
    pos[0], neg[0, 0] = 40.0, -40.0
    if batch > 1:
        pos[1], neg[1, k - 1] = -40.0, 40.0
    weight = np.sqrt(1 / rng.integers(4, 9, batch)).astype(np.float32) if weighted else None
    pd, nd = torch.from_numpy(pos).to(dev()), torch.from_numpy(neg).to(dev())
    wd = None if weight is None else torch.from_numpy(weight).to(dev())
    loss, dpos, dneg = Out(1, 1), Out(1, batch), Out(batch, k, k + 1)
    results = []
    for _ in range(2):
        assert lib.ihg_kg_loss(ptr(pd), ptr(nd), k, ptr(wd), batch, k, loss.ptr, dpos.ptr, dneg.ptr, dneg.ld, stream()) == 0, _lib.last_error()
        torch.cuda.synchronize()
        results.append((loss.check('loss')[0, 0], dpos.check('dpos')[0], dneg.check('dneg')))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    ref = sref.kg_loss(pos, neg, weight)
    w = np.ones(batch) if weight is None else weight.astype(np.float64)
    lp = np.minimum(pos.astype(np.float64), 0) - np.log1p(np.exp(-np.abs(pos.astype(np.float64))))
    ln = np.minimum(-neg.astype(np.float64), 0) - np.log1p(np.exp(-np.abs(neg.astype(np.float64))))
    magnitude = ((w * np.abs(lp)).sum() + (w * np.abs(ln).mean(1)).sum()) / w.sum() / 2
    assert abs(results[0][0] - ref['loss']) <= (2 * batch + k + 16) * sref.U * magnitude + TINY
    inside(results[0][1], ref['dpos'], (batch + 16) * sref.U * np.abs(ref['dpos']), 'dpos')
    inside(results[0][2], ref['dneg'], (batch + 16) * sref.U * np.abs(ref['dneg']), 'dneg')


# ------------------------------------------------------------------------------------------------ top-k over dense rows
def run_topk(scores, k, ld=None):
    lib = _lib.load()
    C, I = scores.shape
    ld = I if ld is None else ld
    buf = torch.full((C, ld), float('nan'), dtype=torch.float32, device=dev())      # a NaN beyond a row's entries must not be ranked
    buf[:, :I] = torch.from_numpy(scores)
    items = torch.full((GUARD + C + GUARD, k), -7, dtype=torch.int64, device=dev())
    best = Out(C, k)
    assert lib.ihg_rows_topk(ptr(buf), ld, C, I, k, ctypes.c_void_p(items.data_ptr() + GUARD * k * 8), best.ptr, stream()) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((items[:GUARD] == -7).all()) and bool((items[GUARD + C:] == -7).all())
    return items[GUARD:GUARD + C].cpu().numpy(), best.check('top scores')


@pytest.mark.parametrize('k', (1, 10, 11, 128))
@pytest.mark.parametrize('n_items', (3, 10, 11, 257, 1000))
def test_rows_topk_exact_with_ties(n_items, k):
    """Integer-valued scores with many ties (about 12 distinct values); 257 items: one past a single trip of the workgroup's 256 threads.  Exact, -1 / -inf beyond I."""
    rng = np.random.default_rng(n_items * 131 + k)
    scores = rng.integers(-6, 6, (5, n_items)).astype(np.float32)
    scores[1] = 2.0                                                      # one row all equal: ascending item ids
    want_items, want_scores = sref.topk(scores, k)
    for ld in (None, n_items + 5):
        items, best = run_topk(scores, k, ld)
        assert np.array_equal(items, want_items)
        assert np.array_equal(best, want_scores)


def test_rows_topk_more_rows_than_workgroups():
    rng = np.random.default_rng(9)
    scores = rng.integers(-3, 3, (2049, 11)).astype(np.float32)          # the grid holds 2048 workgroups: row 2048 is a second trip
    items, best = run_topk(scores, 10)
    want_items, want_scores = sref.topk(scores, 10)
    assert np.array_equal(items, want_items) and np.array_equal(best, want_scores)


def test_rows_topk_ties_rank_as_score_topk_ranks_them():
    """A constructed tie case through both rankers: zero features, so every pair's score of an item is its integer-valued bias."""
    from ihgnn_amd import ops
    users_n, queries_n, items_n = 3, 2, 40
    bias = torch.tensor([float(v % 4) for v in range(items_n)], device=dev())
    features = torch.zeros(users_n + queries_n + items_n, 32, device=dev())
    users, queries = torch.tensor([0, 2], device=dev()), torch.tensor([1, 0], device=dev())
    theirs, their_scores = ops.score_topk(features, users, queries, users_n, users_n + queries_n, bias, 0.5, k=10)
    mine, my_scores = ops.rows_topk(bias.repeat(2, 1), 10)
    assert theirs.cpu().tolist() == mine.cpu().tolist() == [[3, 7, 11, 15, 19, 23, 27, 31, 35, 39]] * 2
    assert torch.equal(their_scores, my_scores)
