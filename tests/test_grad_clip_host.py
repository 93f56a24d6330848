"""CPU side of the gradient-clipping tests (``tests/test_grad_clip_kernels.py`` and ``tests/test_grad_clip_model.py`` hold the GPU side): the bounds the kernels are held
to are themselves held by the operation-by-operation emulation of the kernels' scheme in ``tests/clip_reference.py``, named mutations of that emulation each leave
them, and the host layers - flag, settings, optimizer keyword, argument checks of the new entry points - behave without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import clip_reference as C
import update_tail_reference as R

HYPER = R.HYPERS['decay']                                    # weight decay on: the order of coefficient and decay term matters
T = 7


def _grads(quads):
    return [g.numpy() for _, g, _, _ in quads]


def _max_norm_below(design, norm):
    """A bound that clips: 1e15 for the 1e20 entry (the scaled gradient stays in float32's normal range), else 0.37 of the norm (1 where the norm is not finite)."""
    if design == 'huge':
        return 1e15
    return float(np.float32(0.37 * norm)) if np.isfinite(norm) and norm > 0 else 1.0


def _check_step(quads, design, max_norm, what, check_update=True):
    """Emulated sum, record and update of one call against the float64 reference; -> (norm, coef, worst errors)."""
    grads = _grads(quads)
    norm64 = C.norm_reference(grads)
    coef64 = C.coef_reference(norm64, max_norm)
    norm, coef = C.emulate_record(C.emulate_sqnorm(grads), max_norm)
    assert C.norm_within_one_ulp(norm, norm64), (what, float(norm), norm64)
    if np.isnan(coef64):
        assert np.isnan(coef), (what, coef)
        return norm, coef, None
    assert abs(float(coef) - coef64) <= C.coef_bound(norm64, max_norm), (what, float(coef), coef64)
    if not check_update:
        return norm, coef, None
    worst = dict(p=0.0, m=0.0, v=0.0, tiny_share=0.0)
    for p, g, m, v in quads:
        if p.numel() == 0:
            continue
        ref = C.adam_reference_clipped(p, g, m, v, HYPER, T, coef64)
        got = C.emulate_update(p.numpy(), g.numpy(), m.numpy(), v.numpy(), HYPER, T, coef)
        finite = torch.isfinite(ref['p'])
        assert np.array_equal(np.isfinite(got[0]), finite.numpy()), what
        if not bool(finite.all()):
            continue                                         # (an inf entry: the same entries are NaN; the finite ones are held by the other designs)
        errors = R.adam_errors(*(torch.from_numpy(x) for x in got), ref)
        for k in worst:
            worst[k] = max(worst[k], errors[k])
    return norm, coef, worst


@pytest.mark.parametrize('design', C.DESIGNS)
@pytest.mark.parametrize('case', sorted(C.GEOMETRY))
def test_emulation_of_the_kernels_meets_the_bounds(case, design):
    """Every geometry of the ladder (counts around the chunk, 1 / 2 / 24 / 25 / 49 tensors, empty tensors, more partials than one trip of the finish loop) under every
    value design: the float32 norm within 1 ulp of float64, the coefficient within ``coef_bound``, every p, exp_avg, exp_avg_sq within K_v, K_m, K_p = 16, 10, 10 of
    the scales.  This guards the BOUNDS: a kernel case that fails on the GPU while this one passes is a wrong kernel."""
    quads = C.draw(C.GEOMETRY[case], design, 40 + sorted(C.GEOMETRY).index(case))
    norm64 = C.norm_reference(_grads(quads))
    for max_norm in (float('inf'), _max_norm_below(design, norm64)):
        what = f'{case}, {design}, max_norm {max_norm}'
        # (the 1e20 entry unclipped: its square overflows exp_avg_sq in float32, with or without this feature - the update is checked where the bound clips)
        norm, coef, worst = _check_step(quads, design, max_norm, what, check_update=not (design == 'huge' and np.isinf(max_norm)))
        if design == 'zero':
            assert float(norm) == 0.0 and float(coef) == 1.0
        if design == 'three_four':
            assert float(norm) == 5.0
        if design == 'huge':
            assert np.isfinite(norm) and abs(float(norm) - 1e20) <= 1e20 * 2 * C.U
        if design == 'nan':
            assert np.isnan(norm) and np.isnan(coef)
        if design == 'inf':
            assert np.isinf(norm) and (np.isnan(coef) if np.isinf(max_norm) else float(coef) == 0.0)
        if max_norm == float('inf') and design in ('zero', 'three_four', 'randn'):
            assert float(coef) == 1.0
        if worst is not None:
            C.assert_clipped_adam_within_bounds(worst, what)


def test_emulation_beyond_one_grid_of_chunks():
    """4,100 chunks in one tensor (what the partial kernel walks in two trips of its grid): norm and coefficient of a randn gradient within their bounds."""
    g = torch.randn(C.GRID_TRIPS, generator=torch.Generator().manual_seed(3)).numpy()
    norm64 = C.norm_reference([g])
    norm, coef = C.emulate_record(C.emulate_sqnorm([g]), 10.0)
    assert C.norm_within_one_ulp(norm, norm64) and abs(float(coef) - C.coef_reference(norm64, 10.0)) <= C.coef_bound(norm64, 10.0)


def test_the_sum_does_not_depend_on_how_the_list_is_cut():
    """A chunk's partial is a function of the chunk alone: one tensor of three chunks and the same values as three one-chunk tensors give the same double, bit for bit
    (alignment is no input of the scheme either: on the GPU it selects a load path, not an order - the ``unaligned`` case of the kernel ladder)."""
    g = torch.randn(3 * C.CHUNK, generator=torch.Generator().manual_seed(4)).numpy()
    assert C.emulate_sqnorm([g]) == C.emulate_sqnorm([g[:C.CHUNK], g[C.CHUNK:2 * C.CHUNK], g[2 * C.CHUNK:]])


# ---------------------------------------------------------------------------------------------
# named mutations, each outside a named case
# ---------------------------------------------------------------------------------------------
def test_mutation_a_dropped_partial_leaves_the_norm_bound():
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=gen).numpy() for n in C.GEOMETRY['tensors25']]        # unit scale everywhere: every chunk, the 5-element one too, is far above an ulp
    norm64 = C.norm_reference(grads)
    assert C.norm_within_one_ulp(C.emulate_record(C.emulate_sqnorm(grads), 1.0)[0], norm64)
    for chunk in (0, 24, 27):                                # the first, the first of the second launch, the last
        assert not C.norm_within_one_ulp(C.emulate_record(C.emulate_sqnorm(grads, drop_chunk=chunk), 1.0)[0], norm64), chunk


def test_mutation_a_skipped_tail_leaves_the_norm_bound():
    quads = C.draw(C.GEOMETRY['unaligned'], 'randn', 6)
    grads = _grads(quads)
    norm64 = C.norm_reference(grads)
    assert C.norm_within_one_ulp(C.emulate_record(C.emulate_sqnorm(grads), 1.0)[0], norm64)
    assert not C.norm_within_one_ulp(C.emulate_record(C.emulate_sqnorm(grads, skip_tail=True), 1.0)[0], norm64)


def test_mutation_float32_squares_overflow_at_1e20():
    quads = C.draw(C.GEOMETRY['n4097'], 'huge', 7)
    grads = _grads(quads)
    norm64 = C.norm_reference(grads)
    good = C.emulate_record(C.emulate_sqnorm(grads), 1e15)
    bad = C.emulate_record(C.emulate_sqnorm(grads, fp32_squares=True), 1e15)
    assert np.isfinite(good[0]) and C.norm_within_one_ulp(good[0], norm64)
    assert np.isinf(bad[0]) and float(bad[1]) == 0.0 and not C.norm_within_one_ulp(bad[0], norm64)


def test_mutation_fminf_clamp_hides_a_nan_norm():
    quads = C.draw(C.GEOMETRY['two'], 'nan', 8)
    total = C.emulate_sqnorm(_grads(quads))
    assert np.isnan(C.coef_reference(C.norm_reference(_grads(quads)), 1.0))
    assert np.isnan(C.emulate_record(total, 1.0)[1])
    assert float(C.emulate_record(total, 1.0, fmin_clamp=True)[1]) == 1.0


def test_mutation_coefficient_after_weight_decay_leaves_the_adam_bounds():
    quads = C.draw(C.GEOMETRY['n8193'], 'randn', 9)
    p, g, m, v = quads[0]
    norm64 = C.norm_reference([g.numpy()])
    max_norm = 0.01 * norm64
    coef64 = C.coef_reference(norm64, max_norm)
    coef = C.emulate_record(C.emulate_sqnorm([g.numpy()]), max_norm)[1]
    ref = C.adam_reference_clipped(p, g, m, v, HYPER, T, coef64)
    arrays = (p.numpy(), g.numpy(), m.numpy(), v.numpy())
    good = R.adam_errors(*(torch.from_numpy(x) for x in C.emulate_update(*arrays, HYPER, T, coef)), ref)
    bad = R.adam_errors(*(torch.from_numpy(x) for x in C.emulate_update(*arrays, HYPER, T, coef, clip_after_decay=True)), ref)
    C.assert_clipped_adam_within_bounds(good)
    assert bad['m'] > 100 * C.K_M and bad['p'] > C.K_P


def test_mutation_no_epsilon_at_norm_zero():
    quads = C.draw(C.GEOMETRY['n3'], 'zero', 10)
    total = C.emulate_sqnorm(_grads(quads))
    assert total == 0.0 and C.coef_reference(0.0, 0.0) == 0.0 and C.coef_reference(0.0, 1.0) == 1.0
    assert float(C.emulate_record(total, 0.0)[1]) == 0.0 and float(C.emulate_record(total, 1.0)[1]) == 1.0
    assert np.isnan(C.emulate_record(total, 0.0, no_eps=True)[1])              # 0 / 0


def test_statistics_emulation():
    f = np.float32
    assert C.emulate_statistics([(f(2), f(0.5)), (f(7), f(0.1)), (f(1), f(1))]) == [7.0, 2.0, 3.0]
    assert C.emulate_statistics([(f(np.nan), f(np.nan)), (f(3), f(1))]) == [3.0, 0.0, 2.0]


# ---------------------------------------------------------------------------------------------
# host layers
# ---------------------------------------------------------------------------------------------
def test_flag_and_settings():
    from ihgnn_amd import Main as driver
    from ihgnn_amd.Helpers.ArgsParser import parse_args
    from ihgnn_amd.Helpers.GlobalSettings import Gs
    assert Gs.Training.clip_grad_norm == 0.0 and parse_args([]).clip_grad_norm == 0.0
    assert parse_args(['--clip_grad_norm', '0.5']).clip_grad_norm == 0.5 and parse_args(['--clip_grad_norm', '0']).clip_grad_norm == 0.0
    for bad in ('-1', 'inf', '-inf', 'nan', 'much'):
        with pytest.raises(SystemExit):
            parse_args(['--clip_grad_norm', bad])
    try:
        driver.apply_training_settings(parse_args(['--clip_grad_norm', '2.5']))
        assert Gs.Training.clip_grad_norm == 2.5
        driver.apply_training_settings(parse_args([]))       # a run without the flag clips nothing, whatever ran before it in this process
        assert Gs.Training.clip_grad_norm == 0.0
    finally:
        Gs.Training.clip_grad_norm, Gs.Training.loss, Gs.Training.negative_pool = 0.0, 'bce', 0


def test_optimizer_keyword_and_state_dict():
    """``max_grad_norm`` is an attribute, not a ``param_groups`` key: ``state_dict()`` has the keys it has without the keyword - those of ``torch.optim.Adam``'s groups
    that this optimizer carries - and a checkpoint written with clipping on loads into an optimizer without it."""
    from ihgnn_amd.optim import Adam
    params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    plain, clipped = Adam(params, 1e-3), Adam(params, 1e-3, max_grad_norm=0.5)
    assert plain.max_grad_norm is None and clipped.max_grad_norm == 0.5 and Adam(params, max_grad_norm=float('inf')).max_grad_norm == float('inf')
    assert plain.state_dict() == clipped.state_dict()
    assert set(clipped.state_dict()['param_groups'][0]) == {'lr', 'betas', 'eps', 'weight_decay', 'params'} <= set(torch.optim.Adam(params).state_dict()['param_groups'][0])
    assert all('max_grad_norm' not in g for g in clipped.param_groups)
    plain.load_state_dict(clipped.state_dict())
    assert clipped.clip_statistics() == (0.0, 0, 0) and clipped.grad_norm is None
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            Adam(params, max_grad_norm=bad)


def test_sharded_optimizer_takes_the_keyword_on_the_host():
    """``ShardedGradientSync.optimizer(lr, weight_decay, max_grad_norm)`` in one process on the CPU (its ``torch.optim.Adam`` form): the step equals
    ``clip_grad_norm_`` + ``torch.optim.Adam`` on copies, and the statistics count it."""
    from ihgnn_amd.distributed import ShardedGradientSync
    torch.manual_seed(0)
    ours = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    sync = ShardedGradientSync(ours)
    opt = sync.optimizer(1e-2, 1e-2, max_grad_norm=0.25)
    ref = torch.optim.Adam(theirs, 1e-2, weight_decay=1e-2)
    for step in range(3):
        for p, q in zip(ours, theirs):
            g = torch.randn(p.shape)
            p.grad.copy_(g)
            q.grad = g.clone()
        sync.average_gradients()
        kept = sync.grad_shard.clone()
        opt.step()
        assert torch.equal(sync.grad_shard, kept) and opt.shard.grad is sync.grad_shard        # the gradient is not rewritten here either
        assert float(opt.grad_norm[0]) > 0.25 and float(opt.grad_norm[1]) < 1
        torch.nn.utils.clip_grad_norm_(theirs, 0.25)
        ref.step()
        for p, q in zip(ours, theirs):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-7), step
    largest, clipped, steps = opt.clip_statistics()
    assert clipped == 3 and steps == 3 and largest > 0.25 and opt.clip_statistics() == (0.0, 0, 0)
    assert sync.optimizer(1e-2).max_grad_norm is None
    fresh = sync.optimizer(1e-2, 1e-2, max_grad_norm=0.25)   # loading before the first step creates the buffers with a step that is not the run's: nothing counted
    fresh.load_state_dict(opt.state_dict())
    assert fresh.clip_statistics() == (0.0, 0, 0) and fresh.grad_norm is None


def test_new_symbols_are_declared_and_the_abi_version_stays():
    from ihgnn_amd import _lib
    lib = _lib.load()
    for name in ('ihg_grad_sqnorm_workspace_bytes', 'ihg_grad_sqnorm', 'ihg_clip_record', 'ihg_adam_step_clipped', 'ihg_adam_step_clipped_device_scalars'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 37 == lib.ihg_abi_version()   # entry points were added, none changed


def test_grad_clip_bad_arguments_return_invalid_and_launch_nothing():
    """Every argument check of the five new entries answers before any launch (this runs where there is no GPU: a launch would answer something else), also for a
    bad tensor behind the first 24; the workspace query counts one double per 4,096 elements of every tensor."""
    from ihgnn_amd import _lib
    from ihgnn_amd.optim import _AdamTensor
    lib = _lib.load()
    some = 4096                                              # a non-null, aligned address that is never dereferenced
    INV, WS = _lib.ERR_INVALID, _lib.ERR_WORKSPACE

    def table(entries):
        t = (_AdamTensor * len(entries))()
        for slot, (p, g, m, v, count) in zip(t, entries):
            slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq, slot.count = p, g, m, v, count
        return ctypes.cast(t, ctypes.c_void_p), t

    good = (some, some, some, some, 8)
    one, keep_one = table([good])
    ptr = ctypes.c_void_p(some)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    # the workspace query: grad and count only
    sizes, keep_sizes = table([(None, some, None, None, n) for n in (1, 4096, 4097, 0, 3 * 4096)])
    assert lib.ihg_grad_sqnorm_workspace_bytes(sizes, 5) == 8 * (1 + 1 + 2 + 0 + 3) and lib.ihg_grad_sqnorm_workspace_bytes(None, 0) == 0
    assert lib.ihg_grad_sqnorm_workspace_bytes(None, 1) == -1 and lib.ihg_grad_sqnorm_workspace_bytes(sizes, -1) == -1
    for bad in ((some, some, some, some, -1), (some, None, some, some, 8)):
        for entries in ([bad], [good] * 30 + [bad]):
            tab, keep = table(entries)
            assert lib.ihg_grad_sqnorm_workspace_bytes(tab, len(entries)) == -1
            assert lib.ihg_grad_sqnorm(tab, len(entries), ptr, 1 << 20, ptr, None) == INV and f'tensor {len(entries) - 1}' in _lib.last_error()
    # the norm
    assert lib.ihg_grad_sqnorm(None, 1, ptr, 64, ptr, None) == INV and lib.ihg_grad_sqnorm(one, -1, ptr, 64, ptr, None) == INV
    assert lib.ihg_grad_sqnorm(one, 1, ptr, 64, None, None) == INV and lib.ihg_grad_sqnorm(one, 1, ptr, 64, ctypes.c_void_p(some + 4), None) == INV
    assert lib.ihg_grad_sqnorm(one, 1, None, 64, ptr, None) == INV and lib.ihg_grad_sqnorm(one, 1, ctypes.c_void_p(some + 4), 64, ptr, None) == INV
    assert lib.ihg_grad_sqnorm(one, 1, ptr, 7, ptr, None) == WS and 'workspace too small' in _lib.last_error()
    assert lib.ihg_grad_sqnorm(sizes, 5, ptr, 8 * 7 - 1, ptr, None) == WS
    # the record
    assert lib.ihg_clip_record(None, 1.0, ptr, ptr, None) == INV and lib.ihg_clip_record(ptr, 1.0, None, ptr, None) == INV
    assert lib.ihg_clip_record(ptr, -1.0, ptr, ptr, None) == INV and 'max_norm' in _lib.last_error()
    assert lib.ihg_clip_record(ptr, float('nan'), ptr, None, None) == INV
    # the clipped updates: the unclipped entries' checks and a null record
    assert lib.ihg_adam_step_clipped(one, 1, *hyper, 1, None, None) == INV and lib.ihg_adam_step_clipped(one, 1, *hyper, 0, ptr, None) == INV
    assert lib.ihg_adam_step_clipped(None, 1, *hyper, 1, ptr, None) == INV and lib.ihg_adam_step_clipped(one, -1, *hyper, 1, ptr, None) == INV
    assert lib.ihg_adam_step_clipped_device_scalars(one, 1, *hyper[1:], None, ptr, None) == INV
    assert lib.ihg_adam_step_clipped_device_scalars(one, 1, *hyper[1:], ptr, None, None) == INV
    assert lib.ihg_adam_step_clipped_device_scalars(None, 1, *hyper[1:], ptr, ptr, None) == INV
    for bad in ((some, some, some, some, -1), (None, some, some, some, 8), (some, None, some, some, 8), (some, some, None, some, 8), (some, some, some, None, 8)):
        for entries in ([bad], [good] * 30 + [bad], [(None, None, None, None, 0)] * 3 + [bad]):
            tab, keep = table(entries)
            assert lib.ihg_adam_step_clipped(tab, len(entries), *hyper, 1, ptr, None) == INV, (bad, len(entries))
            assert f'tensor {len(entries) - 1}' in _lib.last_error()
            assert lib.ihg_adam_step_clipped_device_scalars(tab, len(entries), *hyper[1:], ptr, ptr, None) == INV, (bad, len(entries))
    # only empty tensors: the update has nothing to launch
    empty, keep_empty = table([(None, None, None, None, 0)] * 26)
    assert lib.ihg_adam_step_clipped(empty, 26, *hyper, 1, ptr, None) == _lib.OK and lib.ihg_adam_step_clipped_device_scalars(empty, 26, *hyper[1:], ptr, ptr, None) == _lib.OK
