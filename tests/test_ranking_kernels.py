"""The evaluation ranking of ``csrc/eval.hip``, each entry point on its own through the C ABI: ``ihg_score_topk``, ``ihg_score_topk_cosine`` and ``ihg_score_topk_deep``
under both heads (``score_prepare_kernel``, ``score_topk_kernel<PB, COSINE, DEEP>``, ``merge_topk_kernel``, ``deep_init_kernel``, ``merge_deep_kernel``).

Every returned (score, item) is held against the float64 scores of all items (``tests/ranking_reference.py``): *exact cases* - integer operands, power-of-two row
scales, rows of power-of-two norm for the cosine head, ``ensure_exact`` on every (pair, item) - must EQUAL the stable ranking and the float32 of its scores, with the
winners placed list by list from the restated launch geometry (more than ten in ONE list, one per list, ties across lane halves, waves and item slices, ties on the
deep boundary) and the deep entry's ``passes`` equal to the emulation's; *float cases* meet the per-score bound and the ranking verdict derived there.
``tests/test_ranking_host.py`` holds the emulation to the same verdicts and shows that each way of being wrong fails them.

``features`` is a column slice of a wider, sentinel-filled matrix (16-byte aligned rows and an odd ``ld`` in turn), ``item_row0 > query_row0 > 0``; the outputs are
views into sentinel buffers, pre-filled so that an unwritten slot shows; the workspace is exactly as long as the library asks, with a guard behind it, and every call
runs twice - over a workspace of all-ones bytes (fp16 NaN planes, NaN ``aux``) and over one whose bytes read as finite values - and must come back bitwise equal: what
the kernels never wrote (the last tile's rows past ``n_items``) must not reach a result.  Every source is compared with its copy after the launch."""
import numpy as np
import pytest
import torch

import ranking_reference as R
from test_aggregate_kernels import Padded
from test_attention_kernels import Guarded, Source
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

GUARD = 64
INT_GUARD, INT_FILL = -123456, -777
WORST = {}                               # entry point and head -> worst |s - s64| / bound of the float cases (recorded in DESIGN.md section 5)
K_PLAIN = (1, 3, 10)
K_DEEP = (1, 10, 11, 20, 21, 50, 128)
WIDTHS = (1, 7, 8, 9, 15, 16, 17, 32, 48, 64, 80, 100, 150, 624, 625, 1263, 1264)
HEADS = [False, True]


@pytest.fixture(scope='module', autouse=True)
def _report_worst_ratios():
    yield
    for name in sorted(WORST):
        print(f'worst error / bound: {name}: {WORST[name]:.3f}')


class GuardedInts:
    """An ``[n]`` int32 view into a buffer of ``INT_GUARD``, the payload pre-filled with ``INT_FILL``."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((GUARD + self.n + GUARD,), INT_GUARD, dtype=torch.int32, device=dev())
        self.view = self.buf[GUARD:GUARD + self.n]
        self.view.fill_(INT_FILL)

    def assert_guards(self, what):
        assert bool((self.buf[:GUARD] == INT_GUARD).all()) and bool((self.buf[GUARD + self.n:] == INT_GUARD).all()), f'{what}: memory around an int output was written'


class Workspace:
    """Exactly ``n_bytes`` (256-byte aligned) of ``fill`` bytes between two guards of 0x5A bytes."""

    def __init__(self, n_bytes, fill):
        self.n = int(n_bytes)
        self.buf = torch.full((256 + self.n + 256,), 0x5A, dtype=torch.uint8, device=dev())
        self.view = self.buf[256:256 + self.n]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    def assert_guards(self, what):
        assert bool((self.buf[:256] == 0x5A).all()) and bool((self.buf[256 + self.n:] == 0x5A).all()), f'{what}: the kernels wrote past the workspace the library asks for'


class Operands:
    """The sources of a case on the device."""

    def __init__(self, case, geometry):
        self.case = case
        self.features = Padded(case.features, geometry)
        self.users, self.queries, self.bias = Source(case.users), Source(case.queries), Source(case.bias)
        assert int(self.features.view.stride(0)) > case.dim and case.item_row0 > case.query_row0 > 0

    def assert_unchanged(self, what):
        for src in (self.features, self.users, self.queries, self.bias):
            src.assert_unchanged(what)


def _launch(x, k, cosine, deep, fill, what):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    c = x.case
    n_bytes = int(lib.ihg_score_topk_deep_workspace_bytes(c.n_pairs, c.n_items, c.dim, k) if deep else lib.ihg_score_topk_workspace_bytes(c.n_pairs, c.n_items, c.dim))
    assert n_bytes == (R.deep_workspace_bytes if deep else R.workspace_bytes)(c.n_pairs, c.n_items, c.dim)
    ws = Workspace(n_bytes, fill)
    scores, items, passes = Guarded(c.n_pairs * k), GuardedInts(c.n_pairs * k), GuardedInts(c.n_pairs)
    args = (ops._ptr(x.features.view), int(x.features.view.stride(0)), c.dim, c.query_row0, c.item_row0, c.n_items, ops._ptr(x.bias.t), ops._ptr(x.users.t), ops._ptr(x.queries.t),
            c.lam, c.n_pairs, k, ops._ptr(scores.view), ops._ptr(items.view), ops._ptr(ws.view), n_bytes)
    if deep:
        rc = lib.ihg_score_topk_deep(*args, int(cosine), ops._ptr(passes.view), ops._stream())
    else:
        rc = (lib.ihg_score_topk_cosine if cosine else lib.ihg_score_topk)(*args, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.OK, f'{what}: returned {rc}: {_lib.last_error()}'
    for t in (scores, items, passes, ws):
        t.assert_guards(what)
    x.assert_unchanged(what)
    if not deep:
        assert bool((passes.view == INT_FILL).all())
    return scores.view.view(c.n_pairs, k).clone(), items.view.view(c.n_pairs, k).clone(), passes.view.clone() if deep else None


def _call(x, k, cosine, deep, what):
    """One call twice - over a workspace of all-ones bytes (NaN) and over one of 0x3C bytes (finite fp16 planes and ``aux``) - bitwise equal."""
    first = _launch(x, k, cosine, deep, 0xFF, what)
    second = _launch(x, k, cosine, deep, 0x3C, what + ' (second run)')
    assert torch.equal(first[0].view(torch.int32), second[0].view(torch.int32)) and torch.equal(first[1], second[1]), f'{what}: two runs differ (the workspace\'s old bytes reach the result)'
    assert not deep or torch.equal(first[2], second[2]), f'{what}: the pass counts of two runs differ'
    return first


def _entry(cosine, deep):
    return ('ihg_score_topk_deep' if deep else 'ihg_score_topk') + (' cosine' if cosine else ' dot product')


def _check(case, k, cosine, deep, geometry='b', x=None):
    """One case through one entry: the exact or the float verdict; returns the outputs."""
    what = f'{case.name} k={k} {_entry(cosine, deep)} geometry {geometry}'
    x = Operands(case, geometry) if x is None else x
    scores, items, passes = _call(x, k, cosine, deep, what)
    if case.exact:
        R.ensure_exact(case, cosine)
        R.assert_exact(scores, items, case, k, cosine, what)
        if deep:
            want = R.emulate(case, k, cosine, True, scores=case.scores64(cosine).float().numpy())[2]
            assert np.array_equal(passes.cpu().numpy(), want), f'{what}: passes {passes.tolist()} != {want.tolist()}'
    else:
        WORST[_entry(cosine, deep)] = max(WORST.get(_entry(cosine, deep), 0.0), R.float_verdict(scores, items, case, k, cosine, what))
        if deep:
            p = passes.cpu().numpy()
            assert np.all((1 <= p) & (p <= R.max_passes(k, case.n_items))), f'{what}: passes {p.tolist()}'
    return scores, items, passes


def _designs(cosine):
    return R.COSINE_EXACT_DESIGNS if cosine else R.EXACT_DESIGNS


def _rotate(cosine, j, n_pairs, n_items, dim):
    designs = [d for d in _designs(cosine) if d != 'identity']
    return R.exact_case(designs[j % len(designs)], n_pairs, n_items, dim, cosine, R.LAMS_EXACT[j % 2])


@pytest.mark.parametrize('cosine', HEADS)
def test_width_ladder_exact(cosine):
    """Widths around one k-step, 2 - 5 k-steps (the prefetch ring of 4 and one step beyond), 100 and 150, 624 | 625 (two pair tiles -> one) and 1263, 1264: the designs
    in rotation over 5 pairs x 70 items, plain and deep; under the dot product also ``identity`` (item c = the one-hot row of column c, so score c names column c:
    every column of every k-step, and the zero padding behind ``dim``)."""
    for j, dim in enumerate(WIDTHS):
        case = _rotate(cosine, j, 5, 70, dim)
        x = Operands(case, 'bc'[j % 2])
        _check(case, K_PLAIN[j % 3], cosine, False, 'bc'[j % 2], x)
        _check(case, K_DEEP[j % 7], cosine, True, 'bc'[j % 2], x)
        if not cosine:
            ident = R.exact_case('identity', 3, dim, dim, False, R.LAMS_EXACT[j % 2])
            xi = Operands(ident, 'cb'[j % 2])
            _check(ident, 10, False, False, 'cb'[j % 2], xi)
            _check(ident, 128, False, True, 'cb'[j % 2], xi)
            assert R.eval_ksteps(dim) * 16 >= dim


@pytest.mark.parametrize('cosine', HEADS)
def test_pairs_ladder_exact(cosine):
    """Pairs around one and two pair tiles of a workgroup (two tiles at d = 48, one at d = 625) and a third workgroup: pairs past the end repeat the last one and
    write nothing."""
    for j, (n_pairs, dim) in enumerate([(p, 48) for p in (1, 31, 32, 33, 63, 64, 65, 129)] + [(p, 625) for p in (1, 32, 33, 65)]):
        assert R.eval_pair_tiles(dim) == (2 if dim == 48 else 1)
        case = _rotate(cosine, j + 3, n_pairs, 100, dim)
        x = Operands(case, 'cb'[j % 2])
        _check(case, K_PLAIN[j % 3], cosine, False, 'cb'[j % 2], x)
        _check(case, K_DEEP[(j + 2) % 7], cosine, True, 'cb'[j % 2], x)


ITEMS = (1, 7, 10, 11, 31, 32, 33, 255, 256, 257, 2016, 2017, 4100)


@pytest.mark.parametrize('design,cosine', [(d, False) for d in R.EXACT_DESIGNS if d != 'identity'] + [(d, True) for d in R.COSINE_EXACT_DESIGNS])
def test_items_ladder_exact(design, cosine):
    """Every design at item counts around the list length, one tile, eight tiles (one per wave, below that waves with empty runs) and nine, the step from one item
    slice to two (2016 | 2017 at 5 pairs x d = 64) and four slices: k = 10 and the deep k in rotation."""
    for j, n_items in enumerate(ITEMS):
        case = R.exact_case(design, 5, n_items, 64, cosine, R.LAMS_EXACT[j % 2])
        x = Operands(case, 'bc'[j % 2])
        _check(case, 10, cosine, False, 'bc'[j % 2], x)
        _check(case, K_DEEP[2 + j % 5], cosine, True, 'bc'[j % 2], x)


@pytest.mark.parametrize('cosine', HEADS)
@pytest.mark.parametrize('design', ['one_list_dec', 'one_list_inc', 'tie_at_boundary', 'row_scales'])
def test_deep_k_ladder_exact(design, cosine):
    """k = 1, 10, 11, 20, 21, 50, 128 on 2016 items in one slice (a list holds 128): with the winners in ONE list every k needs all its ``ceil(k / 10)`` passes, each
    of which ranks exactly ten; ``tie_at_boundary`` has them in ONE list too, in a shuffled id order, with ranks 10 | 11, 20 | 21, ... bit-equal, so the boundary
    that every pass leaves falls inside a tie (``test_ranking_host.py`` holds both properties of the case).  Each shorter k is a prefix of k = 128, and k <= 10 is
    bitwise the plain entry."""
    case = R.exact_case(design, 5, 2016, 64, cosine)
    x = Operands(case, 'b')
    full = _check(case, 128, cosine, True, 'b', x)
    in_one_list = design != 'row_scales'
    if in_one_list:
        assert bool((full[2] == 13).all())
    for k in K_DEEP[:-1]:
        scores, items, passes = _check(case, k, cosine, True, 'b', x)
        assert torch.equal(items, full[1][:, :k]) and torch.equal(scores.view(torch.int32), full[0][:, :k].view(torch.int32)), f'{case.name}: k={k} is no prefix of k=128'
        if in_one_list:
            assert bool((passes == R.max_passes(k, 2016)).all())
        if k <= 10:
            plain = _check(case, k, cosine, False, 'b', x)
            assert torch.equal(plain[1], items) and torch.equal(plain[0].view(torch.int32), scores.view(torch.int32)), f'{case.name}: deep k={k} is not the plain entry'


@pytest.mark.parametrize('cosine', HEADS)
def test_merge_limit_of_1024_lists_exact(cosine):
    """65,505 items x d = 16 x 8 pairs: 64 item slices, 1,024 partial lists - all the deep merge holds (65,504 items: 63 slices).  One winner per list, and a
    bit-equal score in both lane halves, in tiles of different waves and in the first and the last slice."""
    assert R.eval_slices(8, 65505, 16) == 64 and R.eval_slices(8, 65504, 16) == 63
    for design, n_items, k in (('one_per_list', 65505, 128), ('tied_across', 65505, 21), ('one_per_list', 65504, 50)):
        case = R.exact_case(design, 8, n_items, 16, cosine)
        x = Operands(case, 'b')
        _check(case, k, cosine, True, 'b', x)
        _check(case, 10, cosine, False, 'b', x)


FLOAT_SHAPES = ((5, 257, 48), (33, 300, 100), (3, 70, 625), (2, 40, 1264), (5, 2017, 64), (65, 33, 17))


@pytest.mark.parametrize('cosine', HEADS)
@pytest.mark.parametrize('design', R.FLOAT_DESIGNS)
def test_float_cases_meet_the_bound_and_the_ranking_verdict(design, cosine):
    """``randn`` rows, rows of the significand the split loses most on (one-sided), rows with entries down to 2^-17 of their largest; lam = 0, 0.3, 1: every returned
    score within its bound of the float64 score of ITS item, the order and the ids as the verdict of ``ranking_reference.float_verdict`` states - no case left out."""
    for j, (n_pairs, n_items, dim) in enumerate(FLOAT_SHAPES):
        case = R.float_case(design, n_pairs, n_items, dim, R.LAMS_FLOAT[j % 3])
        x = Operands(case, 'bc'[j % 2])
        _check(case, K_PLAIN[(j + 2) % 3], cosine, False, 'bc'[j % 2], x)
        _check(case, K_DEEP[3 + j % 4], cosine, True, 'bc'[j % 2], x)
