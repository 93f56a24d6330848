"""The clipped optimizer step on the GPU, launch by launch through the C ABI: ``ihg_grad_sqnorm`` -> ``ihg_clip_record`` -> ``ihg_adam_step_clipped`` (and its
device-scalar form) into sentinel-guarded, NaN-prefilled buffers with workspaces of exactly the queried size, against the float64 reference and the bounds of
``tests/clip_reference.py`` (``tests/test_grad_clip_host.py`` holds the kernels' scheme, emulated operation by operation, to the same bounds on the CPU)."""
import ctypes

import numpy as np
import pytest
import torch

import clip_reference as C
import update_tail_reference as R
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

PAD = 8                                  # elements of sentinel in front of and behind every tensor (32 bytes: offset 0 of the payload is 16-byte aligned)
SENTINEL = 12345.678
HYPER = R.HYPERS['decay']                # weight decay on: the coefficient must reach the gradient before the decay term
T = 7


class _Guarded:
    """``p, g, m, v`` of one tensor as views into sentinel-filled device buffers; the gradient ``offset`` floats behind a 16-byte boundary."""

    def __init__(self, quad, offset=0):
        self.count = quad[0].numel()
        self.before, self.buffers, self.views, self.start = {}, {}, {}, {}
        for name, x in zip('pgmv', quad):
            off = offset if name == 'g' else 0
            buf = torch.full((PAD + off + self.count + PAD,), SENTINEL, dtype=torch.float32, device=dev())
            assert buf.data_ptr() % 16 == 0
            buf[PAD + off: PAD + off + self.count] = x.to(dev())
            self.before[name] = x.clone()
            self.buffers[name], self.views[name], self.start[name] = buf, buf[PAD + off: PAD + off + self.count], PAD + off

    def assert_surroundings_untouched(self, what):
        for name in 'pgmv':
            buf, s = self.buffers[name], self.start[name]
            assert bool((buf[:s] == SENTINEL).all()) and bool((buf[s + self.count:] == SENTINEL).all()), f'{what}: memory around {name} was written'
        g = self.views['g'].cpu()
        assert g.view(torch.int32).equal(self.before['g'].view(torch.int32)), f'{what}: the gradient was written'


def _table(tensors):
    from ihgnn_amd.optim import _AdamTensor
    table = (_AdamTensor * len(tensors))()
    for slot, x in zip(table, tensors):
        if x.count:
            slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = (x.views[n].data_ptr() for n in 'pgmv')
        slot.count = x.count                                 # (an empty tensor: null pointers)
    return table


def _guarded_output(n, dtype, fill=float('nan')):
    buf = torch.full((n + 2,), SENTINEL, dtype=dtype, device=dev())
    buf[1:-1] = fill
    return buf


def _norm_and_record(lib, tensors, max_norm, stats=None):
    """The two launches in front of the update: -> (sum buffer, clip buffer, partials buffer), each with one guard element on either side."""
    from ihgnn_amd import _lib, ops
    table = _table(tensors)
    bytes_needed = int(lib.ihg_grad_sqnorm_workspace_bytes(ctypes.cast(table, ctypes.c_void_p), len(tensors)))
    assert bytes_needed == 8 * sum(-(-x.count // C.CHUNK) for x in tensors)
    partials, total, clip = _guarded_output(bytes_needed // 8, torch.float64), _guarded_output(1, torch.float64), _guarded_output(2, torch.float32)
    _lib.check(lib.ihg_grad_sqnorm(ctypes.cast(table, ctypes.c_void_p), len(tensors), ctypes.c_void_p(partials[1:].data_ptr()), bytes_needed,
                                   ctypes.c_void_p(total[1:].data_ptr()), ops._stream()), 'ihg_grad_sqnorm')
    _lib.check(lib.ihg_clip_record(ctypes.c_void_p(total[1:].data_ptr()), max_norm, ctypes.c_void_p(clip[1:].data_ptr()),
                                   None if stats is None else ctypes.c_void_p(stats[1:].data_ptr()), ops._stream()), 'ihg_clip_record')
    return total, clip, partials


def _step(specs, quads, max_norm, hyper=HYPER, t=T, device_scalars=False):
    """One call of the step on fresh guarded copies of ``quads``; ``max_norm=None``: the unclipped entry.  -> dict(tensors, sum, norm, coef)."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    tensors = [_Guarded(quad, C.offset_of(spec)) for spec, quad in zip(specs, quads)]
    table = _table(tensors)
    lr, beta1, beta2, eps, wd = hyper
    out = dict(tensors=tensors)
    scalars = torch.tensor(R.step_scalars(lr, beta1, beta2, t), dtype=torch.float32).to(dev())
    if max_norm is None:
        _lib.check(lib.ihg_adam_step(ctypes.cast(table, ctypes.c_void_p), len(tensors), lr, beta1, beta2, eps, wd, t, ops._stream()), 'ihg_adam_step')
    else:
        total, clip, partials = _norm_and_record(lib, tensors, max_norm)
        if device_scalars:
            _lib.check(lib.ihg_adam_step_clipped_device_scalars(ctypes.cast(table, ctypes.c_void_p), len(tensors), beta1, beta2, eps, wd, ctypes.c_void_p(scalars.data_ptr()),
                                                                ctypes.c_void_p(clip[1:].data_ptr()), ops._stream()), 'ihg_adam_step_clipped_device_scalars')
        else:
            _lib.check(lib.ihg_adam_step_clipped(ctypes.cast(table, ctypes.c_void_p), len(tensors), lr, beta1, beta2, eps, wd, t, ctypes.c_void_p(clip[1:].data_ptr()),
                                                 ops._stream()), 'ihg_adam_step_clipped')
        torch.cuda.synchronize()
        for buf in (total, clip, partials):
            assert float(buf[0]) == float(buf[-1]) == float(torch.tensor(SENTINEL, dtype=buf.dtype)), 'a guard element of an output was written'
        out.update(sum=float(total[1]), norm=np.float32(clip[1].item()), coef=np.float32(clip[2].item()), partials=partials[1:-1].cpu().numpy())
    torch.cuda.synchronize()
    for k, x in enumerate(tensors):
        x.assert_surroundings_untouched(f'tensor {k}')
    return out


def _bits_equal(a, b):
    for x, y in zip(a['tensors'], b['tensors']):
        for name in 'pgmv':
            if not torch.equal(x.buffers[name].view(torch.int32), y.buffers[name].view(torch.int32)):
                return False
    return True


def _check_update(run, quads, coef64, what):
    """p, exp_avg, exp_avg_sq of every tensor against the float64 rule on ``coef64 g``: the same entries finite, those within K_v, K_m, K_p of their scales."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for x, (p, g, m, v) in zip(run['tensors'], quads):
        if x.count == 0:
            continue
        got = [x.views[n].detach().cpu() for n in 'pmv']
        if np.isnan(coef64):
            assert all(bool(torch.isnan(y).all()) for y in got), f'{what}: a NaN coefficient must reach every entry'
            continue
        ref = C.adam_reference_clipped(p, g, m, v, HYPER, T, coef64)
        keep = torch.isfinite(ref['p']) & torch.isfinite(ref['m']) & torch.isfinite(ref['v'])
        for y in got:
            assert torch.equal(torch.isfinite(y), keep), f'{what}: finite entries differ from the reference\'s'
        if not bool(keep.any()):
            continue
        errors = R.adam_errors(*(y[keep] for y in got), {k: r[keep] for k, r in ref.items()})
        assert errors['tiny_share'] <= R.MAX_TINY_SHARE, what
        for k in worst:
            worst[k] = max(worst[k], errors[k])
    print(f'clipped adam {what}: worst error / (u x scale) {worst}  (bounds K_p, K_m, K_v = {C.K_P}, {C.K_M}, {C.K_V})')
    assert worst['v'] <= C.K_V and worst['m'] <= C.K_M and worst['p'] <= C.K_P, (what, worst)
    return worst


def _max_norm_below(design, norm):
    if design == 'huge':
        return 1e15                                          # (the scaled gradient stays in float32's normal range, the scaled 1e20 entry squares without overflow)
    return float(np.float32(0.37 * norm)) if np.isfinite(norm) and norm > 0 else 1.0


LADDER = [(case, design) for case in sorted(C.GEOMETRY) for design in ('randn', 'three_four')] + \
         [(case, design) for case in ('two', 'tensors25', 'unaligned') for design in ('zero', 'huge', 'nan', 'inf')]


@pytest.mark.parametrize('case,design', LADDER)
def test_clipped_step_over_the_ladder(case, design):
    """Counts 1, 3, 4,095, 4,096, 4,097, 8,193; 1, 2, 24, 25, 49 tensors; empty tensors among others; gradients one and three floats off alignment; 258 partials (a
    second trip of the finish loop) - under the value designs (all zero; 3 and 4 among zeros; randn; one 1e20; one NaN; one inf):

    * the double sum equals the operation-by-operation emulation of the kernels' scheme bit for bit (finite sums), the partials buffer is written exactly;
    * norm within 1 float32 ulp of float64 - exactly 0, 5 and finite at 1e20 for those designs - and the coefficient within its bound, NaN where torch's rule gives NaN;
    * ``max_norm`` = inf and above the norm: coef exactly 1 and p, exp_avg, exp_avg_sq, guards included, bit-equal to ``ihg_adam_step``;
    * ``max_norm`` below the norm: every entry within K_v, K_m, K_p = 16, 10, 10 of its scale (weight decay on), the same entries non-finite as in the reference (a
      NaN reaches everything, an inf entry alone turns NaN under a finite bound); a second run gives the same bits;
    * the gradient and the memory around every tensor are as they were."""
    specs = C.GEOMETRY[case]
    quads = C.draw(specs, design, 40 + sorted(C.GEOMETRY).index(case))
    grads = [g.numpy() for _, g, _, _ in quads]
    norm64 = C.norm_reference(grads)
    emulated = C.emulate_sqnorm(grads)
    below = _max_norm_below(design, norm64)
    above = float('inf') if not np.isfinite(norm64) else float(np.float32(2 * norm64 + 1))
    plain = _step(specs, quads, None) if design != 'huge' else None
    for max_norm in (float('inf'), above, below):
        what = f'{case}, {design}, max_norm {max_norm:g}'
        run = _step(specs, quads, max_norm)
        coef64 = C.coef_reference(norm64, max_norm)
        print(f'{what}: sum {run["sum"]!r} (emulated {emulated!r}) norm {run["norm"]!r} (float64 {norm64!r}) coef {run["coef"]!r} (float64 {coef64!r})')
        if np.isfinite(emulated):
            assert run['sum'] == emulated, what
            assert np.array_equal(run['partials'], np.concatenate([C.emulate_partials(g) for g in grads] + [np.zeros(0)])), what
        else:
            assert np.isnan(run['sum']) == np.isnan(emulated) and np.isinf(run['sum']) == np.isinf(emulated), what
        assert C.norm_within_one_ulp(run['norm'], norm64), what
        if design == 'zero':
            assert float(run['norm']) == 0.0 and float(run['coef']) == 1.0
        if design == 'three_four':
            assert float(run['norm']) == 5.0
        if design == 'huge':
            assert np.isfinite(run['norm'])
        if np.isnan(coef64):
            assert np.isnan(run['coef']), what
        else:
            assert abs(float(run['coef']) - coef64) <= C.coef_bound(norm64, max_norm), what
        if max_norm != below or design == 'zero':
            if design in ('zero', 'three_four', 'randn'):
                assert float(run['coef']) == 1.0 and _bits_equal(run, plain), what
            continue
        _check_update(run, quads, coef64, what)
        assert _bits_equal(run, _step(specs, quads, max_norm)), f'{what}: two runs differ'
        if plain is not None and design in ('three_four', 'randn'):
            assert not _bits_equal(run, plain)               # (the coefficient did reach the update)


def test_norm_beyond_one_grid_of_chunks():
    """One gradient of 4,100 chunks (16.8 M elements: a second trip of the partial kernel's grid, the last chunk partial), drawn on the device: the double sum equals
    the emulation bit for bit, the norm is within 1 ulp of float64, a second call gives the same bits."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    g = torch.randn(C.GRID_TRIPS, generator=torch.Generator(device=dev()).manual_seed(3), device=dev())

    class _Only:
        count = C.GRID_TRIPS
        views = dict(p=g, g=g, m=g, v=g)                     # (the norm reads grad and count only)
    runs = []
    for _ in range(2):
        total, clip, partials = _norm_and_record(lib, [_Only], 10.0)
        torch.cuda.synchronize()
        assert float(partials[0]) == float(partials[-1]) == SENTINEL and not bool(torch.isnan(partials[1:-1]).any())
        runs.append((float(total[1]), clip[1:3].tolist()))
    host = g.cpu().numpy()
    norm64 = C.norm_reference([host])
    print(f'16.8 M elements: sum {runs[0][0]!r}, norm {runs[0][1][0]!r} against float64 {norm64!r}')
    assert runs[0] == runs[1] and runs[0][0] == C.emulate_sqnorm([host])
    assert C.norm_within_one_ulp(runs[0][1][0], norm64)
    assert abs(runs[0][1][1] - C.coef_reference(norm64, 10.0)) <= C.coef_bound(norm64, 10.0)


def test_statistics_after_three_steps_of_known_norms():
    """Norms 5, 10 and 2.5 under ``max_norm`` 6: the record holds (10, 1, 3); a NaN norm afterwards counts a step and leaves the maximum."""
    from ihgnn_amd import _lib
    lib = _lib.load()
    stats = _guarded_output(3, torch.float32, fill=0.0)
    records = []
    for scale in (1.0, 2.0, 0.5, float('nan')):
        quad = [torch.zeros(C.CHUNK + 3) for _ in range(4)]
        quad[1][0], quad[1][-1] = 3.0 * scale, 4.0 * scale
        _, clip, _ = _norm_and_record(lib, [_Guarded(quad)], 6.0, stats)
        torch.cuda.synchronize()
        records.append((np.float32(clip[1].item()), np.float32(clip[2].item())))
        if scale == 0.5:
            assert stats[1:-1].tolist() == [10.0, 1.0, 3.0] == C.emulate_statistics(records)
    assert [float(n) for n, _ in records[:3]] == [5.0, 10.0, 2.5] and [float(c) for _, c in records[:3]] == [1.0, float(np.float32(6.0) / (np.float32(10.0) + np.float32(1e-6))), 1.0]
    assert stats[1:-1].tolist() == [10.0, 1.0, 4.0] == C.emulate_statistics(records)
    assert float(stats[0]) == float(stats[-1]) == np.float32(SENTINEL)


@pytest.mark.parametrize('case', ['n4097', 'tensors25', 'unaligned', 'empties'])
def test_clipped_device_scalars_entry_is_bitwise_the_host_scalars_entry(case):
    specs = C.GEOMETRY[case]
    quads = C.draw(specs, 'randn', 77)
    max_norm = _max_norm_below('randn', C.norm_reference([g.numpy() for _, g, _, _ in quads]))
    a, b = _step(specs, quads, max_norm), _step(specs, quads, max_norm, device_scalars=True)
    assert _bits_equal(a, b) and a['sum'] == b['sum'] and a['coef'] == b['coef'] < 1
    assert any(not torch.equal(x.views['p'].cpu(), x.before['p']) for x in b['tensors'] if x.count)


def test_clipped_step_without_weight_decay():
    """The 'plain' hyper-parameters (no decay term: ``g coef`` feeds ``g - m`` and ``g g`` directly) at t = 1 and t = 1000: clipped, the same bounds; with
    ``max_norm`` = inf, coef exactly 1 and p, exp_avg, exp_avg_sq, guards included, bit-equal to ``ihg_adam_step`` - over aligned and unaligned gradients."""
    specs = C.GEOMETRY['tensors25'] + C.GEOMETRY['unaligned']
    quads = C.draw(specs, 'randn', 78)
    norm64 = C.norm_reference([g.numpy() for _, g, _, _ in quads])
    max_norm = _max_norm_below('randn', norm64)
    for t in (1, 1000):
        unclipped, open_bound = _step(specs, quads, None, hyper=R.HYPERS['plain'], t=t), _step(specs, quads, float('inf'), hyper=R.HYPERS['plain'], t=t)
        assert float(open_bound['coef']) == 1.0 and _bits_equal(open_bound, unclipped), t
        assert any(not torch.equal(x.views['p'].cpu(), x.before['p']) for x in unclipped['tensors'])
        run = _step(specs, quads, max_norm, hyper=R.HYPERS['plain'], t=t)
        worst = dict(p=0.0, m=0.0, v=0.0)
        for x, (p, g, m, v) in zip(run['tensors'], quads):
            ref = R.adam_reference(p, g.double() * C.coef_reference(norm64, max_norm), m, v, R.HYPERS['plain'], t)
            errors = R.adam_errors(*(x.views[n].detach().cpu() for n in 'pmv'), ref)
            worst = {k: max(worst[k], errors[k]) for k in worst}
        assert worst['v'] <= C.K_V and worst['m'] <= C.K_M and worst['p'] <= C.K_P, (t, worst)
