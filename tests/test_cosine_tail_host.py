"""No GPU: the reference of the cosine batch tail (``tests/update_tail_reference.py``: ``hem_cosine_reference`` and its counted bounds) held to its own conditions -
a plain float32 numpy evaluation in the kernels' order stays inside every bound on the shapes ``tests/test_cosine_tail_kernels.py`` runs, the edge rows come out as
stated, the closed-form gradients are torch's, and the bounds notice a wrong kernel."""
import numpy as np
import pytest
import torch

import update_tail_reference as R

LAYERS, DIMS, BATCHES, LAMBDAS, FORMS = (1, 2, 5, 8), (1, 7, 33, 64, 100, 256), (1, 63, 65), (0.0, 0.3, 1.0), ('one', 'upper', 'typed')


def scales_of(form):
    """(host ``grad_scale``, device scalar): float32(1 / 3) on the host; 0.75 x 3 / 128 with the second factor on the device (an exact product)."""
    return (R.f32(1.0 / 3.0), None) if form == 'one' else (0.75, 3.0 / 128.0)


def reference_of(case, form, lam):
    scale, device_scale = scales_of(form)
    ds = case['dscores'].astype(np.float64) * scale * (1.0 if device_scale is None else device_scale)
    want = R.hem_cosine_reference([x.astype(np.float64) for x in case['layers']], case['rows'], case['rows_upper'], case['items'], case['bias'].astype(np.float64), lam, ds)
    return want, ds


@pytest.mark.parametrize('n_layers', LAYERS)
def test_float32_evaluation_in_the_kernels_order_stays_inside_the_counted_bounds(n_layers):
    worst = np.zeros(3)
    for i, dim in enumerate(DIMS):
        for j, batch in enumerate(BATCHES):
            for k, form in enumerate(FORMS):
                lam = LAMBDAS[(i + j + k) % 3]
                case = R.cosine_tail_case(n_layers, dim, batch, form, i + k)
                want, ds = reference_of(case, form, lam)
                got = R.hem_cosine_float32(case['layers'], case['rows'], case['rows_upper'], case['items'], case['bias'], lam, case['dscores'], *scales_of(form))
                worst = np.maximum(worst, R.assert_cosine_tail_within_bounds(*got, want, ds, f'L = {n_layers}, d = {dim}, B = {batch}, {form}, lam = {lam}'))
    print(f'worst error / bound of the float32 evaluation, L = {n_layers}: scores {worst[0]:.3f}, stats {worst[1]:.3f}, row gradients {worst[2]:.3f}')
    assert (worst > 0).all()


def test_edge_rows_are_what_their_names_say():
    for form in FORMS:
        case = R.cosine_tail_case(5, 33, 63, form, 0)
        want, ds = reference_of(case, form, 0.3)
        edge = {name: r for r, name in enumerate(case['edges'])}
        stats, grads, bound = want['stats'], want['grads'], want['grad_bound']
        z = edge['zero_item']                                               # a = 0: the score is the bias, dc/dm is exactly 0, dc/da = m / (eps |m|) is finite
        assert stats[z, 1] == 0 and want['score'][z] == case['bias'][case['items'][z]] and want['score_bound'][z] == R.U * abs(want['score'][z])
        assert (grads[:2, z] == 0).all() and (bound[:2, z] == 0).all() and np.isfinite(grads[2, z]).all() and np.abs(grads[2, z]).max() > 0
        z = edge['zero_mixed']
        assert stats[z, 2] == 0 and (grads[2, z] == 0).all() and (bound[2, z] == 0).all() and np.abs(grads[0, z]).max() > 0
        t = edge['tiny_item']                                               # 0 < |a| < 1e-8: the clamped value divides, the unclamped norm is differentiated
        assert 0 < np.sqrt(stats[t, 1]) < R.COSINE_EPS and np.isfinite(grads[:, t]).all()
        if form != 'one':
            up = case['rows_upper']
            assert up[2 * 63 + edge['item_isolated']] == -1 and up[edge['user_and_query_isolated']] == -1 and up[63 + edge['user_and_query_isolated']] == -1
            xu, xq, a = R.hem_cosine_rows(case['layers'], case['rows'], up, 63)
            assert (a[edge['item_isolated'], 33:] == 0).all() and np.abs(a[edge['item_isolated'], :33]).min() > 0
            r = edge['user_and_query_isolated']
            assert (xu[r, 33:] == 0).all() and (xq[r, 33:] == 0).all() and stats[r, 2] > 0


def test_closed_form_gradients_are_autograd_of_torch_cosine_similarity():
    case = R.cosine_tail_case(2, 33, 65, 'upper', 1)
    want, ds = reference_of(case, 'upper', 0.3)
    lam = R.f32(0.3)
    xu, xq, a = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in R.hem_cosine_rows([x.astype(np.float64) for x in case['layers']], case['rows'],
                                                                                                     case['rows_upper'], 65))
    score = torch.cosine_similarity(a, lam * xq + (1 - lam) * xu, dim=1, eps=R.COSINE_EPS) + torch.tensor(case['bias'].astype(np.float64))[case['items']]
    (score * torch.tensor(ds)).sum().backward()
    ordinary = np.array([e not in ('zero_item', 'zero_mixed', 'tiny_item') for e in case['edges']] + [True] * (65 - len(case['edges'])))
    np.testing.assert_allclose(score.detach().numpy()[ordinary], want['score'][ordinary], rtol=1e-12, atol=1e-14)
    for k, x in enumerate((xu, xq, a)):
        np.testing.assert_allclose(x.grad.numpy()[ordinary], want['grads'][k][ordinary], rtol=1e-10, atol=1e-14)


def test_the_bounds_notice_a_wrong_kernel():
    case = R.cosine_tail_case(5, 100, 65, 'upper', 2)
    want, ds = reference_of(case, 'upper', 0.3)
    args = (case['rows'], case['rows_upper'], case['items'], case['bias'], 0.3, case['dscores'], *scales_of('upper'))
    good = R.hem_cosine_float32(case['layers'], *args)
    R.assert_cosine_tail_within_bounds(*good, want, ds)

    def fails(score, stats, rowgrad):
        try:
            R.assert_cosine_tail_within_bounds(score, stats, rowgrad, want, ds)
        except AssertionError:
            return True
        return False

    dropped = [x.copy() for x in case['layers']]
    dropped[4][:, 99] = 0                                                   # the last column of the last layer left out of the sums
    assert fails(*R.hem_cosine_float32(dropped, *args))
    skipped = R.hem_cosine_float32(case['layers'], case['rows'], np.where(case['rows_upper'] < 0, 0, case['rows_upper']), *args[2:])      # an isolated node read as row 0
    assert fails(*skipped)
    score, stats, rowgrad = (x.copy() for x in good)
    stats[:, [1, 2]] = stats[:, [2, 1]]                                     # |a|^2 and |m|^2 swapped
    assert fails(score, stats, rowgrad)
    score, stats, rowgrad = (x.copy() for x in good)
    rowgrad[[0, 1]] = rowgrad[[1, 0]]                                       # the user's and the query's rows swapped (lam = 0.3)
    assert fails(score, stats, rowgrad)
    score, stats, rowgrad = (x.copy() for x in good)
    rowgrad[2, :, :-1] *= np.float32(1 + 2.0 ** -17)                        # 64 ulp on every item-row entry
    assert fails(score, stats, rowgrad)
