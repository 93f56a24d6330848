"""Every branch of the catalogue launch routine and its dispatch (``csrc/eval.hip``: ``catalogue_launch<COSINE, DEEP, SEARCH, EXCL>`` out of one table) at the smallest
shapes that reach them, through the C ABI: the entry points are held against each other BITWISE where the kernels' comments promise one expression and one item
order, so no tolerance is involved.  ``dim`` 64 / 640 give two pair tiles per workgroup and one (the switch is at 624); 33 pairs are a full pair tile and one pair;
1,000 items are a partial last item tile and more than one wave run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_USERS, N_QUERIES, N_ITEMS, N_PAIRS = 50, 40, 1000, 33


def _run(lib, name, case, k, cosine=False, lists=None):
    """One call of ``ihg_<name>`` on ``case`` -> (items, scores, passes); ``lists`` = (ptr, items) of ``ihg_search_topk_excluding`` or a pair of ``None``."""
    from ihgnn_amd import _lib, ops
    features, bias, users, queries = case
    dim, dev = int(features.shape[1]), features.device
    scores, items = torch.empty(N_PAIRS, k, dtype=torch.float32, device=dev), torch.empty(N_PAIRS, k, dtype=torch.int32, device=dev)
    passes = torch.full((N_PAIRS,), -1, dtype=torch.int32, device=dev)
    plain = name in ('score_topk', 'score_topk_cosine')
    size = lib.ihg_score_topk_workspace_bytes(N_PAIRS, N_ITEMS, dim) if plain else getattr(lib, f'ihg_{name}_workspace_bytes')(N_PAIRS, N_ITEMS, dim, k)
    space = torch.empty(int(size) // 4, dtype=torch.float32, device=dev)
    head = (ops._ptr(features), ops._ld(features), dim, N_USERS, N_USERS + N_QUERIES, N_ITEMS, ops._ptr(bias), ops._ptr(users), ops._ptr(queries))
    sources = (None, 0, 0, None) if name.startswith('search') else ()
    excl = (ops._ptr(lists[0]), ops._ptr(lists[1]), None, N_PAIRS if lists[0] is not None else 0) if lists is not None else ()
    tail = (ops._stream(),) if plain else (int(cosine), ops._ptr(passes), ops._stream())
    _lib.check(getattr(lib, 'ihg_' + name)(*head, *sources, *excl, 0.3, N_PAIRS, k, ops._ptr(scores), ops._ptr(items), ops._ptr(space), space.numel() * 4, *tail), 'ihg_' + name)
    return items, scores, passes


def _same(got, want, parts=3):
    return all(torch.equal(g, w) for g, w in list(zip(got, want))[:parts])


def test_the_entry_points_agree_bitwise_wherever_they_launch_the_same_arithmetic():
    from ihgnn_amd import _lib
    lib, dev = _lib.load(), torch.device('cuda:0')
    for dim in (64, 640):
        _check_width(lib, dev, dim)


def _check_width(lib, dev, dim):
    gen = torch.Generator().manual_seed(dim)
    features = torch.randn(N_USERS + N_QUERIES + N_ITEMS, dim, generator=gen).to(dev)                   # users | queries | items
    bias = torch.randn(N_ITEMS, generator=gen).to(dev)
    case = (features, bias, torch.randint(0, N_USERS, (N_PAIRS,), generator=gen).to(dev), torch.randint(0, N_QUERIES, (N_PAIRS,), generator=gen).to(dev))
    no_runs = (torch.zeros(N_PAIRS + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))      # 33 empty runs (and the one-entry dummy)
    for cosine in (False, True):
        plain = _run(lib, 'score_topk_cosine' if cosine else 'score_topk', case, 10)
        assert bool((plain[0] >= 0).all()) and bool((plain[1][:, :-1] >= plain[1][:, 1:]).all())         # (a ranking at all: ten items, best first)
        assert _same(_run(lib, 'score_topk_deep', case, 10, cosine), plain, 2), f'dim {dim}, cosine {cosine}: deep at k = 10 differs from the plain call'
        deep = _run(lib, 'score_topk_deep', case, 25, cosine)
        search = _run(lib, 'search_topk', case, 25, cosine)
        assert _same(search, deep), f'dim {dim}, cosine {cosine}: a search by index with no mask and no anonymous user differs from the deep call'
        assert _same(_run(lib, 'search_topk_excluding', case, 25, cosine, (None, None)), search), f'dim {dim}, cosine {cosine}: excluding with null lists differs from the search'
        assert _same(_run(lib, 'search_topk_excluding', case, 25, cosine, no_runs), search), f'dim {dim}, cosine {cosine}: excluding 33 empty runs differs from the search'
