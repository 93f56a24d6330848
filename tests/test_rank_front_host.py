"""The shared host front of the six ranking entry points (``csrc/ranking.hpp``), where there is no GPU: the workspace sizes the layout functions add up to, the
same refusal for the same bad argument whichever entry point it is given to, the order in which refusals are reported, and the empty call.  Every call here answers
before a launch: an answer at all means that nothing was launched, and the addresses are never dereferenced."""
import ctypes
import itertools

import pytest

P = ctypes.c_void_p(4096)                                                  # non-null, 16-byte aligned
PLAIN, DEEP, SEARCH, LISTS = ('ihg_score_topk', 'ihg_score_topk_cosine'), ('ihg_score_topk_deep',), ('ihg_search_topk',), ('ihg_search_topk_excluding', 'ihg_search_candidates')
ENTRIES = PLAIN + DEEP + SEARCH + LISTS
TAKES_QUERY_ROWS = SEARCH + LISTS
K_RANGE = {name: 'k <= 10' if name in PLAIN else '1 <= k <= 128' for name in ENTRIES}

# (n_pairs, n_items, dim) -> the bytes of ihg_score_topk / _deep / ihg_search_topk / _excluding _workspace_bytes, the same for every k of 1, 10, 11, 128; and
# (n_pairs, total) -> ihg_search_candidates_workspace_bytes for every such k and every dim below.  Taken from a build of the commit before the layout functions, whose
# four size functions each added "what the next one appends" to the previous one's answer.
CATALOGUE = {
    (1, 1, 8): (3584, 3600, 3616, 3632),
    (1, 1, 64): (9728, 9744, 9760, 9776),
    (1, 1, 624): (81408, 81424, 81440, 81456),
    (1, 1, 640): (83456, 83472, 83488, 83504),
    (1, 1, 1264): (163328, 163344, 163360, 163376),
    (1, 31, 8): (3584, 3600, 3616, 3632),
    (1, 31, 64): (9728, 9744, 9760, 9776),
    (1, 31, 624): (81408, 81424, 81440, 81456),
    (1, 31, 640): (83456, 83472, 83488, 83504),
    (1, 31, 1264): (163328, 163344, 163360, 163376),
    (1, 1000, 8): (75008, 75024, 75040, 75056),
    (1, 1000, 64): (271616, 271632, 271648, 271664),
    (1, 1000, 624): (2565376, 2565392, 2565408, 2565424),
    (1, 1000, 640): (2630912, 2630928, 2630944, 2630960),
    (1, 1000, 1264): (5186816, 5186832, 5186848, 5186864),
    (1, 120000, 8): (8721920, 8721936, 8721952, 8721968),
    (1, 120000, 64): (31761920, 31761936, 31761952, 31761968),
    (1, 120000, 624): (300561920, 300561936, 300561952, 300561968),
    (1, 120000, 640): (308241920, 308241936, 308241952, 308241968),
    (1, 120000, 1264): (607761920, 607761936, 607761952, 607761968),
    (5, 1, 8): (8704, 8784, 8800, 8832),
    (5, 1, 64): (14848, 14928, 14944, 14976),
    (5, 1, 624): (86528, 86608, 86624, 86656),
    (5, 1, 640): (88576, 88656, 88672, 88704),
    (5, 1, 1264): (168448, 168528, 168544, 168576),
    (5, 31, 8): (8704, 8784, 8800, 8832),
    (5, 31, 64): (14848, 14928, 14944, 14976),
    (5, 31, 624): (86528, 86608, 86624, 86656),
    (5, 31, 640): (88576, 88656, 88672, 88704),
    (5, 31, 1264): (168448, 168528, 168544, 168576),
    (5, 1000, 8): (80128, 80208, 80224, 80256),
    (5, 1000, 64): (276736, 276816, 276832, 276864),
    (5, 1000, 624): (2570496, 2570576, 2570592, 2570624),
    (5, 1000, 640): (2636032, 2636112, 2636128, 2636160),
    (5, 1000, 1264): (5191936, 5192016, 5192032, 5192064),
    (5, 120000, 8): (9049600, 9049680, 9049696, 9049728),
    (5, 120000, 64): (32089600, 32089680, 32089696, 32089728),
    (5, 120000, 624): (300889600, 300889680, 300889696, 300889728),
    (5, 120000, 640): (308569600, 308569680, 308569696, 308569728),
    (5, 120000, 1264): (608089600, 608089680, 608089696, 608089728),
    (33, 1, 8): (44544, 45072, 45088, 45232),
    (33, 1, 64): (50688, 51216, 51232, 51376),
    (33, 1, 624): (122368, 122896, 122912, 123056),
    (33, 1, 640): (124416, 124944, 124960, 125104),
    (33, 1, 1264): (204288, 204816, 204832, 204976),
    (33, 31, 8): (44544, 45072, 45088, 45232),
    (33, 31, 64): (50688, 51216, 51232, 51376),
    (33, 31, 624): (122368, 122896, 122912, 123056),
    (33, 31, 640): (124416, 124944, 124960, 125104),
    (33, 31, 1264): (204288, 204816, 204832, 204976),
    (33, 1000, 8): (115968, 116496, 116512, 116656),
    (33, 1000, 64): (312576, 313104, 313120, 313264),
    (33, 1000, 624): (2606336, 2606864, 2606880, 2607024),
    (33, 1000, 640): (2671872, 2672400, 2672416, 2672560),
    (33, 1000, 1264): (5227776, 5228304, 5228320, 5228464),
    (33, 120000, 8): (11343360, 11343888, 11343904, 11344048),
    (33, 120000, 64): (34383360, 34383888, 34383904, 34384048),
    (33, 120000, 624): (303183360, 303183888, 303183904, 303184048),
    (33, 120000, 640): (310863360, 310863888, 310863904, 310864048),
    (33, 120000, 1264): (610383360, 610383888, 610383904, 610384048),
    (4096, 1, 8): (5245184, 5310720, 5310736, 5327120),
    (4096, 1, 64): (5251328, 5316864, 5316880, 5333264),
    (4096, 1, 624): (5323008, 5388544, 5388560, 5404944),
    (4096, 1, 640): (5325056, 5390592, 5390608, 5406992),
    (4096, 1, 1264): (5404928, 5470464, 5470480, 5486864),
    (4096, 31, 8): (5245184, 5310720, 5310736, 5327120),
    (4096, 31, 64): (5251328, 5316864, 5316880, 5333264),
    (4096, 31, 624): (5323008, 5388544, 5388560, 5404944),
    (4096, 31, 640): (5325056, 5390592, 5390608, 5406992),
    (4096, 31, 1264): (5404928, 5470464, 5470480, 5486864),
    (4096, 1000, 8): (5316608, 5382144, 5382160, 5398544),
    (4096, 1000, 64): (5513216, 5578752, 5578768, 5595152),
    (4096, 1000, 624): (7806976, 7872512, 7872528, 7888912),
    (4096, 1000, 640): (7872512, 7938048, 7938064, 7954448),
    (4096, 1000, 1264): (10428416, 10493952, 10493968, 10510352),
    (4096, 120000, 8): (50583040, 50648576, 50648592, 50664976),
    (4096, 120000, 64): (73623040, 73688576, 73688592, 73704976),
    (4096, 120000, 624): (342423040, 342488576, 342488592, 342504976),
    (4096, 120000, 640): (329131520, 329197056, 329197072, 329213456),
    (4096, 120000, 1264): (628651520, 628717056, 628717072, 628733456),
}
CANDIDATES = {
    (1, 0): 32,
    (1, 5): 64,
    (1, 1000): 4032,
    (5, 0): 128,
    (5, 5): 160,
    (5, 1000): 4128,
    (33, 0): 800,
    (33, 5): 832,
    (33, 1000): 4800,
    (4096, 0): 98320,
    (4096, 5): 98352,
    (4096, 1000): 102320,
}
N_PAIRS, N_ITEMS, DIMS, KS, TOTALS = (1, 5, 33, 4096), (1, 31, 1000, 120000), (8, 64, 624, 640, 1264), (1, 10, 11, 128), (0, 5, 1000)


@pytest.fixture(scope='module')
def lib():
    from ihgnn_amd import _lib
    return _lib.load()


def call(lib, name, *, features=P, ld=2000, dim=64, n_items=1000, k=10, n_pairs=1, queries=P, query_rows=None, ld_q=0, q_dim=0, excl=(P, P, None, 1), space=P,
         nbytes=1 << 40):
    """One call of ``name`` with good arguments except the ones given; an entry takes the groups it has."""
    head = (features, ld, dim, 0, 0, n_items, P, P, queries)
    sources = (query_rows, ld_q, q_dim, None) if name in TAKES_QUERY_ROWS else ()
    lists = tuple(excl) if name in LISTS else ()
    if name == 'ihg_search_candidates':
        lists += (P, P, None, max(n_pairs, 1), 5)                          # cand_ptr, cand_items, cand_row, n_cand_rows, total
    ranked = (0.5, n_pairs, k, P, P) + ((None,) if name == 'ihg_search_candidates' else ())
    tail = (None,) if name in PLAIN else (0, None, None)                   # stream | cosine, passes, stream
    return getattr(lib, name)(*head, *sources, *lists, *ranked, space, nbytes, *tail)


def test_workspace_sizes_are_those_of_the_four_function_chain(lib):
    assert set(CATALOGUE) == set(itertools.product(N_PAIRS, N_ITEMS, DIMS)) and set(CANDIDATES) == set(itertools.product(N_PAIRS, TOTALS))
    for (n_pairs, n_items, dim), want in CATALOGUE.items():
        assert lib.ihg_score_topk_workspace_bytes(n_pairs, n_items, dim) == want[0], (n_pairs, n_items, dim)
        for k in KS:
            got = tuple(getattr(lib, f'ihg_{name}_workspace_bytes')(n_pairs, n_items, dim, k) for name in ('score_topk_deep', 'search_topk', 'search_topk_excluding'))
            assert got == want[1:], (n_pairs, n_items, dim, k)
    for (n_pairs, total), want in CANDIDATES.items():
        for dim, k in itertools.product(DIMS, KS):
            assert lib.ihg_search_candidates_workspace_bytes(n_pairs, total, dim, k) == want, (n_pairs, total, dim, k)


BOTH, NEITHER = dict(queries=P, query_rows=P, ld_q=64, q_dim=64), dict(queries=None, query_rows=None)
# (the bad argument, the entries that have it, the text after the entry's name)
REFUSALS = [(dict(k=0), ENTRIES, None), (dict(k=129), ENTRIES, None),
            (BOTH, TAKES_QUERY_ROWS, ': exactly one of queries and query_rows'), (NEITHER, TAKES_QUERY_ROWS, ': exactly one of queries and query_rows'),
            (dict(queries=None, query_rows=P, ld_q=128, q_dim=65), TAKES_QUERY_ROWS, ': 1 <= q_dim <= dim and ld_q >= q_dim'),
            (dict(queries=None, query_rows=P, ld_q=31, q_dim=32), TAKES_QUERY_ROWS, ': 1 <= q_dim <= dim and ld_q >= q_dim'),
            (dict(excl=(P, None, None, 1)), LISTS, ': excl_ptr and excl_items go together'), (dict(excl=(None, P, None, 1)), LISTS, ': excl_ptr and excl_items go together'),
            (dict(excl=(None, None, P, 1)), LISTS, ': excl_row without lists'),
            (dict(features=None), ENTRIES, ': null pointer'),
            (dict(space=ctypes.c_void_p(4100)), ENTRIES, ': workspace too small')]


def test_the_same_bad_argument_is_refused_alike_by_every_entry_that_has_it(lib):
    from ihgnn_amd import _lib
    for bad, entries, text in REFUSALS:
        for name in entries:
            want = _lib.ERR_WORKSPACE if 'space' in bad and name in PLAIN + DEEP else _lib.ERR_INVALID      # the score entries' own code for the workspace; the search entries': invalid
            assert call(lib, name, **bad) == want, (name, bad)
            assert _lib.last_error() == name + (text or f': bad size ({K_RANGE[name]})'), (name, bad)


def test_a_bad_size_is_reported_before_a_bad_query_source_and_that_before_a_bad_list(lib):
    from ihgnn_amd import _lib
    bad_list = dict(excl=(P, None, None, 1))
    for name in ENTRIES:
        later = dict(features=None, nbytes=0)
        if name in TAKES_QUERY_ROWS:
            later.update(NEITHER)
        if name in LISTS:
            later.update(bad_list)
        assert call(lib, name, k=129, **later) == _lib.ERR_INVALID and _lib.last_error() == f'{name}: bad size ({K_RANGE[name]})'
        if name in TAKES_QUERY_ROWS:
            assert call(lib, name, **later) == _lib.ERR_INVALID and _lib.last_error() == name + ': exactly one of queries and query_rows'
        if name in LISTS:
            assert call(lib, name, features=None, nbytes=0, **bad_list) == _lib.ERR_INVALID and _lib.last_error() == name + ': excl_ptr and excl_items go together'
        assert call(lib, name, features=None, nbytes=0) == _lib.ERR_INVALID and _lib.last_error() == name + ': null pointer'       # ... and a null pointer before the workspace


def test_an_empty_call_with_good_arguments_is_ok_for_every_entry(lib):
    from ihgnn_amd import _lib
    for name in ENTRIES:
        assert call(lib, name, n_pairs=0) == _lib.OK, name
        assert call(lib, name, n_pairs=0, features=None, space=None, nbytes=0) == _lib.OK, name                  # before the null-pointer and workspace tests
        assert call(lib, name, n_pairs=0, k=0) == _lib.ERR_INVALID, name                                         # a bad size with nothing to do is still bad
