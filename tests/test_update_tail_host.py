"""CPU side of the update-tail tests (``tests/test_update_tail.py`` holds the GPU side): the rounding bound the Adam kernel is held to is itself held by an
operation-by-operation float32 evaluation of the rule on the same inputs, and the recorded step's table of Adam scalars against the formula."""
import math

import numpy as np
import pytest
import torch

import update_tail_reference as R


@pytest.mark.parametrize('t', R.STEPS)
@pytest.mark.parametrize('hyper', sorted(R.HYPERS))
def test_float32_evaluation_of_the_adam_rule_stays_inside_the_counted_bounds(hyper, t):
    """The rule evaluated operation by operation in numpy float32 against the float64 rule over 120,000 elements per case: within K_v, K_m, K_p = 8, 6, 6 roundings of the
    scales that ``update_tail_reference`` derives (its docstring counts them).  This case guards the BOUND: a kernel case that fails on the GPU while this one passes is a
    wrong kernel, not a tight bar."""
    gen = torch.Generator().manual_seed(17 + t % 1000)
    p, g, m, v = R.draw_inputs(120_000, gen)
    ref = R.adam_reference(p, g, m, v, R.HYPERS[hyper], t)
    p1, m1, v1 = R.adam_float32(p.numpy(), g.numpy(), m.numpy(), v.numpy(), R.HYPERS[hyper], t)
    errors = R.adam_errors(torch.from_numpy(p1), torch.from_numpy(m1), torch.from_numpy(v1), ref)
    print(f'float32 rule, {hyper}, t = {t}: {errors}')
    R.assert_adam_within_bounds(errors, f'{hyper}, t = {t}')
    # the inputs hold what they are meant to: exact zeros in every tensor, elements whose denominator is eps alone, |g| <= 10^4
    assert int((p == 0).sum()) > 0 and int(((g == 0) & (v == 0)).sum()) > 0 and int(((m == 0) & (g == 0)).sum()) > 0
    assert float(g.abs().max()) <= 1e4


def test_the_bound_notices_a_wrong_update():
    """The three bounds are not vacuous: ``sqrt(v / bias2_sqrt)`` for ``sqrt(v) / bias2_sqrt``, a bias correction formed in float32, and beta1 where beta2 belongs
    are each far outside them."""
    gen = torch.Generator().manual_seed(5)
    p, g, m, v = R.draw_inputs(50_000, gen)
    hyper, t = R.HYPERS['decay'], 1000
    ref = R.adam_reference(p, g, m, v, hyper, t)
    good = R.adam_float32(p.numpy(), g.numpy(), m.numpy(), v.numpy(), hyper, t)
    assert R.adam_errors(*(torch.from_numpy(x) for x in good), ref)['p'] <= R.K_P
    lr, beta1, beta2, eps, wd = (np.float32(x) for x in hyper)
    step_size, bias2_sqrt = (np.float32(x) for x in R.step_scalars(lr, beta1, beta2, t))
    v1 = good[2]
    # (a) the square root taken of the quotient
    wrong = p.numpy() - step_size * (good[1] / (np.sqrt(v1 / bias2_sqrt) + eps))
    assert R.adam_errors(torch.from_numpy(wrong), torch.from_numpy(good[1]), torch.from_numpy(v1), ref)['p'] > 100 * R.K_P
    # (b) the bias corrections in float32: at a small step count 1 - beta2^t cancels, and the rounding of beta2^t to float32 is hundreds of u of it
    hyper_b, t_b = R.HYPERS['long_memory'], 2
    ref_b = R.adam_reference(p, g, m, v, hyper_b, t_b)
    good_b = R.adam_float32(p.numpy(), g.numpy(), m.numpy(), v.numpy(), hyper_b, t_b)
    lr_b, beta1_b, beta2_b, eps_b, _ = (np.float32(x) for x in hyper_b)
    bad_step = lr_b / (np.float32(1) - np.power(beta1_b, np.float32(t_b)))
    bad_sqrt = np.sqrt(np.float32(1) - np.power(beta2_b, np.float32(t_b)))
    assert (bad_step, bad_sqrt) != tuple(np.float32(x) for x in R.step_scalars(lr_b, beta1_b, beta2_b, t_b))
    wrong = p.numpy() - bad_step * (good_b[1] / (np.sqrt(good_b[2]) / bad_sqrt + eps_b))
    assert R.adam_errors(torch.from_numpy(wrong), torch.from_numpy(good_b[1]), torch.from_numpy(good_b[2]), ref_b)['p'] > 2 * R.K_P
    # (c) beta1 in the second moment's first term
    g1 = g.numpy() + wd * p.numpy()
    wrong_v = beta1 * v.numpy() + (np.float32(1) - beta2) * g1 * g1
    assert R.adam_errors(torch.from_numpy(good[0]), torch.from_numpy(good[1]), torch.from_numpy(wrong_v), ref)['v'] > 1000 * R.K_V


@pytest.mark.parametrize('first', [1, 2048, 2049, 10 ** 6])
def test_adam_step_scalars_table_rows(first):
    """Row ``t - first`` of ``Adam.step_scalars`` is ``(float32(lr32 / (1 - beta1_32^t)), float32(sqrt(1 - beta2_32^t)))`` - the bias corrections in float64, as
    ``ihg_adam_step`` forms them - wherever the table starts."""
    from ihgnn_amd.optim import Adam
    for lr, betas in ((1e-3, (0.9, 0.999)), (3e-3 * 0.98 ** 7, (0.5, 0.9999)), (1e-2, (0.0, 0.3))):
        table = Adam.step_scalars(first, 40, lr, betas)
        assert table.dtype == torch.float32 and tuple(table.shape) == (40, 2) and table.device.type == 'cpu'
        assert bool(torch.isfinite(table).all())
        lr32, b1, b2 = R.f32(lr), R.f32(betas[0]), R.f32(betas[1])
        for k in range(40):
            t = first + k
            want = (np.float32(lr32 / (1.0 - b1 ** t)), np.float32(math.sqrt(1.0 - b2 ** t)))
            assert (np.float32(table[k, 0]), np.float32(table[k, 1])) == want, (first, k, lr, betas)
            assert want == tuple(np.float32(x) for x in R.step_scalars(lr, betas[0], betas[1], t))


def test_adam_step_scalars_at_the_first_step_with_zero_betas():
    from ihgnn_amd.optim import Adam
    table = Adam.step_scalars(1, 3, 0.25, (0.0, 0.0))
    assert table.tolist() == [[0.25, 1.0]] * 3              # 1 - 0^t = 1: no division by zero, no nan
    assert bool(torch.isfinite(Adam.step_scalars(1, 2048, 1e-3, (0.0, 0.999))).all())
