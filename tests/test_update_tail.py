"""The loss-and-update end of a training step on the GPU, each launch on its own against float64: ``ihg_adam_step`` / ``ihg_adam_step_device_scalars`` element by
element, 3,000-step Adam trajectories, the recorded step's table of Adam scalars, ``ihg_bce_with_logits`` and ``ihg_hem_score_fwd / bwd`` (+ ``_typed0``).

The references and the rounding counts behind every bound are in ``tests/update_tail_reference.py``; ``tests/test_update_tail_host.py`` holds a plain float32
evaluation of the Adam rule to the same bounds on a machine without a GPU.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import update_tail_reference as R
from test_gpu_parity import dev, rel

pytestmark = pytest.mark.gpu

U = R.U
PAD = 8                                  # elements of sentinel in front of and behind every tensor (32 bytes: offset 0 of the payload is 16-byte aligned)
SENTINEL = 12345.678
CHUNK = 4096                             # kAdamChunk (csrc/tail.hip): elements per workgroup trip; 24 = kAdamMaxTensors per launch, 256 * 16 workgroups per grid
BIG = CHUNK * CHUNK + CHUNK * 3 + 17     # beyond one grid of chunks: the kernel's grid-stride loop takes a second trip, the last chunk is partial


# =============================================================================================
# 1. one Adam launch
# =============================================================================================
class _Padded:
    """``p, g, m, v`` of one tensor as views into sentinel-filled buffers: the parameter at element offset ``off_p`` past a 16-byte boundary, the gradient at ``off_g``, both
    moments at ``off_mv``.  ``before``: the four inputs as they were drawn (same device)."""

    def __init__(self, count, generator, off_p=0, off_g=0, off_mv=0, device=None):
        device = device or dev()
        drawn = R.draw_inputs(count, generator, device=generator.device)
        self.count, self.before, self.buffers, self.views, self.start = count, {}, {}, {}, {}
        for name, x, off in zip('pgmv', drawn, (off_p, off_g, off_mv, off_mv)):
            buf = torch.full((PAD + off + count + PAD,), SENTINEL, dtype=torch.float32, device=device)
            assert buf.data_ptr() % 16 == 0
            buf[PAD + off: PAD + off + count] = x.to(device)
            self.before[name] = x.to(device)
            self.buffers[name], self.views[name], self.start[name] = buf, buf[PAD + off: PAD + off + count], PAD + off
            assert self.views[name].data_ptr() % 16 == (4 * off) % 16 or count == 0

    def assert_surroundings_untouched(self, what):
        for name in 'pmv':
            buf, s = self.buffers[name], self.start[name]
            assert bool((buf[:s] == SENTINEL).all()) and bool((buf[s + self.count:] == SENTINEL).all()), f'{what}: memory around {name} was written'
        assert torch.equal(self.views['g'], self.before['g']), f'{what}: the gradient was written'


def _draw(specs, seed, device='cpu'):
    """One ``_Padded`` per spec - a count, or ``(count, off_p, off_g, off_mv)`` - drawn from one generator."""
    gen = torch.Generator(device=device).manual_seed(seed)
    return [_Padded(spec, gen) if isinstance(spec, int) else _Padded(spec[0], gen, *spec[1:]) for spec in specs]


def _launch(tensors, hyper, t, device_scalars=False):
    """One update of every tensor at step count ``t`` in ONE ``step()`` (or ``launch_with_device_scalars``) call: the state is written into the optimizer directly."""
    from ihgnn_amd.optim import Adam
    lr, beta1, beta2, eps, wd = hyper
    params = []
    for x in tensors:
        p = x.views['p'].requires_grad_()
        p.grad = x.views['g']
        params.append(p)
    opt = Adam(params, lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd)
    for p, x in zip(params, tensors):
        opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=x.views['m'], exp_avg_sq=x.views['v'])
    if device_scalars:
        scalars = torch.tensor(R.step_scalars(lr, beta1, beta2, t), dtype=torch.float32).to(dev())
        opt.launch_with_device_scalars(scalars)
        opt.advance()
    else:
        opt.step()
    torch.cuda.synchronize()
    assert all(int(opt.state[p]['step']) == t for p in params)
    return opt


def _check(tensors, hyper, t, what, slice_elements=1 << 21):
    """Every element of every tensor against the float64 rule (on the device, a slice at a time), the memory around every tensor."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    tiny, total = 0.0, 0
    for k, x in enumerate(tensors):
        x.assert_surroundings_untouched(f'{what}, tensor {k}')
        for lo in range(0, x.count, slice_elements):
            sl = slice(lo, min(lo + slice_elements, x.count))
            ref = R.adam_reference(*(x.before[n][sl] for n in 'pgmv'), hyper, t)
            errors = R.adam_errors(x.views['p'].detach()[sl], x.views['m'][sl], x.views['v'][sl], ref)
            for n in 'pmv':
                worst[n] = max(worst[n], errors[n])
            tiny += errors['tiny_share'] * 3 * (sl.stop - sl.start)
            total += 3 * (sl.stop - sl.start)
    worst['tiny_share'] = tiny / max(total, 1)
    print(f'adam {what}: worst error / (u x scale) {worst}  (bounds K_p, K_m, K_v = {R.K_P}, {R.K_M}, {R.K_V})')
    R.assert_adam_within_bounds(worst, what)


MIXED = [4097, (3 * CHUNK + 5, 1, 0, 0), 20000, (1000, 0, 3, 0), 3]


@pytest.mark.parametrize('t', R.STEPS)
@pytest.mark.parametrize('hyper', sorted(R.HYPERS))
def test_adam_launch_matches_the_float64_rule(hyper, t):
    """One ``ihg_adam_step`` launch at step count t (1 ... 10^6, where beta1^t has long underflowed) for five hyper-parameter sets, every element of p, exp_avg, exp_avg_sq
    against the float64 rule with the hyper-parameters as the ABI receives them: within K_p, K_m, K_v = 6, 6, 8 roundings of scales that carry the rule's two
    cancellations (counted in ``update_tail_reference``; a float32 evaluation on the CPU is held to the same numbers by ``test_update_tail_host``).  An element whose
    scale is 0 is exact; at most 1 % of the elements may have a scale in float32's subnormal range and be left out (asserted; the inputs hold none)."""
    tensors = _draw(MIXED, 100 + t % 997)
    _launch(tensors, R.HYPERS[hyper], t)
    _check(tensors, R.HYPERS[hyper], t, f'{hyper}, t = {t}')


def _cycle(n):
    counts = (5, CHUNK, 1, CHUNK + 1, 100, CHUNK - 1, 33, 2 * CHUNK)
    offsets = ((0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 2, 0), (3, 3, 3), (0, 0, 0), (2, 0, 1), (0, 0, 0))
    return [(counts[k % 8],) + offsets[k % 8] for k in range(n)]


def _with_empties():
    specs = _cycle(30)
    for k in (0, 5, 6, 24, 29):                           # first, two in a row between others, at position 24 (the first slot of a second launch), last
        specs[k] = (0,) + specs[k][1:]
    return specs


GEOMETRY = {
    # counts around the chunk: one element, below / at / above the vector width, one below / exactly / one above a chunk, two chunks, three chunks and a tail
    'counts': [1, 3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 5],
    # >= 3 chunks each; parameter unaligned and moments aligned (the whole tensor takes the scalar path over FULL chunks - what a shard of a flat buffer is), a count that
    # is a multiple of the chunk, gradient alone unaligned, moments alone unaligned, everything unaligned alike
    'views': [(3 * CHUNK + 5, 1, 0, 0), (4 * CHUNK, 2, 0, 0), (3 * CHUNK, 3, 0, 0), (3 * CHUNK + 7, 0, 1, 0), (3 * CHUNK, 0, 0, 2), (5 * CHUNK + 1, 1, 1, 1)],
    'tensors25': _cycle(25),                              # one more than a launch's table holds: the second launch of one call
    'tensors48': _cycle(48),                              # two full tables
    'tensors49': _cycle(49),                              # a third launch for one tensor
    'empties': _with_empties(),
    'big': [BIG],
}


def _geometry_tensors(case):
    if case == 'big':                                       # drawn on the device: 16.8 M elements, 270 MB with state and the kept inputs
        return _draw(GEOMETRY[case], 7, device=dev())
    return _draw(GEOMETRY[case], 7)


@pytest.mark.parametrize('case', sorted(GEOMETRY))
def test_adam_launch_geometry(case):
    """The launch geometry of ``ihg_adam_step``, each case ONE ``step()`` call with weight decay at t = 7: counts around the 4,096-element chunk, views that put the
    parameter / the gradient / the moments off 16-byte alignment (the scalar path over full chunks), 25 / 48 / 49 tensors (a second and a third launch behind
    kAdamMaxTensors = 24), zero-element tensors first / last / at position 24 / between others, and one tensor beyond a whole grid of chunks (256 x 16 x 4,096 elements;
    compared on the device in float64 slices).  Every element against the float64 rule; the memory in front of and behind p, exp_avg, exp_avg_sq keeps its sentinel."""
    tensors = _geometry_tensors(case)
    _launch(tensors, R.HYPERS['decay'], 7)
    _check(tensors, R.HYPERS['decay'], 7, case)


@pytest.mark.parametrize('case', sorted(GEOMETRY))
def test_adam_device_scalars_launch_is_bitwise_the_host_scalars_launch(case):
    """``ihg_adam_step_device_scalars`` fed ``(float32(lr / (1 - beta1^t)), float32(sqrt(1 - beta2^t)))`` leaves bit for bit what ``ihg_adam_step`` leaves at the same t,
    sentinels included, over every geometry case."""
    outs = []
    for device_scalars in (False, True):
        tensors = _geometry_tensors(case)
        _launch(tensors, R.HYPERS['decay'], 7, device_scalars)
        outs.append(tensors)
    for k, (a, b) in enumerate(zip(*outs)):
        for name in 'pgmv':
            assert torch.equal(a.buffers[name], b.buffers[name]), (case, k, name)
    assert any(not torch.equal(x.views['p'], x.before['p']) for x in outs[1])       # (the update did happen)


def test_adam_refused_call_updates_nothing():
    """A call whose 31st tensor is bad is refused as a whole: the 24 tensors of what would have been its first launch keep their values."""
    from ihgnn_amd import _lib
    from ihgnn_amd.optim import _AdamTensor
    lib = _lib.load()
    tensors = _draw(_cycle(31), 11)
    table = (_AdamTensor * 31)()
    for slot, x in zip(table, tensors):
        slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = (x.views[n].data_ptr() for n in 'pgmv')
        slot.count = x.count
    table[30].exp_avg = None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ihg_adam_step(ctypes.cast(table, ctypes.c_void_p), 31, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, stream) == _lib.ERR_INVALID
    scalars = torch.ones(2, device=dev())
    assert lib.ihg_adam_step_device_scalars(ctypes.cast(table, ctypes.c_void_p), 31, 0.9, 0.999, 1e-8, 0.0, ctypes.c_void_p(scalars.data_ptr()), stream) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    for x in tensors:
        for n in 'pgmv':
            assert torch.equal(x.views[n], x.before[n])


# =============================================================================================
# 2. long horizons
# =============================================================================================
CHECKPOINTS = (1, 10, 100, 1000, 2049, 3000)


@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
def test_adam_trajectory_over_3000_steps(weight_decay):
    """3,000 steps of ``ihgnn_amd.optim.Adam`` on three tensors (an unaligned view of a flat buffer, 4,099 elements, [333, 5] - the last one skips every third step, so
    its count lags and a step is two launches) against the float64 rule with float32-rounded hyper-parameters, on gradients drawn independently of the parameters with
    a per-step scale 10^((t mod 7) - 4).  At t = 1, 10, 100, 1,000, 2,049, 3,000 the ``rel`` of p, exp_avg, exp_avg_sq (worst tensor) may be 4 x what
    ``torch.optim.Adam`` in float32 ON THE CPU shows against the same float64 trajectory on the same gradients - both are random walks of float32 roundings, so either
    can be the larger at a given step; an update that is off by 10^-4 relative every step has drifted tens of times further - and never needs to be below 2u = 1.2e-7,
    one rounding of the largest element.  (6,000 optimizer steps on three implementations: about ten seconds, most of it the two CPU optimizers.)"""
    from ihgnn_amd.optim import Adam
    lr, betas, eps = 3e-3, (0.9, 0.999), 1e-8
    lr32, b1, b2, eps32, wd32 = (R.f32(x) for x in (lr, betas[0], betas[1], eps, weight_decay))
    gen = torch.Generator().manual_seed(31)
    flat = torch.randn(5003, generator=gen)
    start = [flat[1:5001].clone(), torch.randn(4099, generator=gen), torch.randn(333, 5, generator=gen)]
    flat_gpu = flat.to(dev())
    assert flat_gpu[1:5001].data_ptr() % 16 == 4
    ours = [flat_gpu[1:5001].requires_grad_()] + [x.clone().to(dev()).requires_grad_() for x in start[1:]]
    theirs = [x.clone().requires_grad_() for x in start]
    hip = Adam(ours, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    cpu32 = torch.optim.Adam(theirs, lr=lr32, betas=(b1, b2), eps=eps32, weight_decay=wd32)
    exact = [dict(p=x.double(), m=torch.zeros_like(x, dtype=torch.float64), v=torch.zeros_like(x, dtype=torch.float64), t=0) for x in start]
    figures = []
    for step in range(1, CHECKPOINTS[-1] + 1):
        scale = 10.0 ** (step % 7 - 4)
        for k in range(3):
            g = torch.randn(start[k].shape, generator=gen) * scale
            if k == 2 and step % 3 == 0:
                ours[k].grad = theirs[k].grad = None
                continue
            ours[k].grad, theirs[k].grad = g.to(dev()), g.clone()
            e = exact[k]
            e['t'] += 1
            g64 = g.double() + wd32 * e['p']
            e['m'] = e['m'] + (g64 - e['m']) * (1.0 - b1)
            e['v'] = b2 * e['v'] + (1.0 - b2) * g64 * g64
            e['p'] = e['p'] - lr32 / (1.0 - b1 ** e['t']) * e['m'] / (e['v'].sqrt() / (1.0 - b2 ** e['t']) ** 0.5 + eps32)
        hip.step()
        cpu32.step()
        if step in CHECKPOINTS:
            for name, key in (('p', None), ('exp_avg', 'm'), ('exp_avg_sq', 'v')):
                got = max(rel(ours[k] if key is None else hip.state[ours[k]][name], exact[k][key or 'p']) for k in range(3))
                ref = max(rel(theirs[k] if key is None else cpu32.state[theirs[k]][name], exact[k][key or 'p']) for k in range(3))
                figures.append((step, name, got, ref))
                print(f'adam trajectory wd = {weight_decay}: t = {step:5d} {name:10s} HIP {got:.2e}   torch float32 on the CPU {ref:.2e}')
    assert int(hip.state[ours[2]]['step']) == 2000 and int(hip.state[ours[0]]['step']) == 3000
    assert flat_gpu[0].item() == flat[0].item()            # the floats around the view
    assert torch.equal(flat_gpu[5001:].cpu(), flat[5001:])
    for step, name, got, ref in figures:
        assert got <= max(4.0 * ref, 2.0 * U), (step, name, got, ref)


# =============================================================================================
# 3. the recorded step's table of Adam scalars, at the optimizer
# =============================================================================================
def test_adam_stepped_through_the_scalar_table_is_bitwise_the_eager_optimizer(monkeypatch):
    """Two ``Adam`` instances over equal parameters and equal gradient streams: one stepped by ``step()``, the other by ``launch_with_device_scalars`` + ``advance()``
    with the scalars that ``CapturedTrainingStep._refresh_scalars`` copies out of its table, the table cut to 3 steps: 11 steps roll it over three times, the learning
    rate changes before step 4 (a table edge) and before step 8 (mid-table).  p, exp_avg, exp_avg_sq are equal bit for bit after every step.  (The table logic runs on a
    ``CapturedTrainingStep`` without a recording: ``_refresh_scalars`` reads the optimizer, the table and the two-float device buffer only.)"""
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.optim import Adam
    monkeypatch.setattr(CapturedTrainingStep, 'TABLE_STEPS', 3)
    gen = torch.Generator().manual_seed(8)
    shapes = [(4099,), (64, 65), (7,)]
    start = [torch.randn(*s, generator=gen) for s in shapes]
    eager = [x.clone().to(dev()).requires_grad_() for x in start]
    tabled = [x.clone().to(dev()).requires_grad_() for x in start]
    a = Adam(eager, lr=1e-3, weight_decay=1e-2)
    b = Adam(tabled, lr=1e-3, weight_decay=1e-2)
    b.ensure_state()
    rec = object.__new__(CapturedTrainingStep)
    rec.optimizer, rec.scalars = b, torch.zeros(2, dtype=torch.float32, device=dev())
    rec._table, rec._table_first, rec._table_lr = None, 0, None
    firsts = []
    for step in range(1, 12):
        if step in (4, 8):
            for opt in (a, b):
                opt.param_groups[0]['lr'] *= 0.98 ** (step // 4) * 0.5
        for p, q in zip(eager, tabled):
            g = (torch.randn(p.shape, generator=gen) * 10.0 ** (step % 3 - 2)).to(dev())
            p.grad, q.grad = g, g.clone()
        a.step()
        assert b.next_step() == step
        rec._refresh_scalars()
        firsts.append(rec._table_first)
        assert tuple(rec._table.shape) == (3, 2)
        want = R.step_scalars(b.param_groups[0]['lr'], 0.9, 0.999, step)
        assert rec.scalars.tolist() == list(want), step
        b.launch_with_device_scalars(rec.scalars)
        b.advance()
        for p, q in zip(eager, tabled):
            assert torch.equal(p, q), step
            assert torch.equal(a.state[p]['exp_avg'], b.state[q]['exp_avg']) and torch.equal(a.state[p]['exp_avg_sq'], b.state[q]['exp_avg_sq']), step
    assert firsts == [1, 1, 1, 4, 4, 4, 7, 8, 8, 8, 11]     # rebuilt when it ran out (4, 7, 11) and on the learning-rate change (4, 8)
    assert a.next_step() == b.next_step() == 12


# =============================================================================================
# 4. ihg_bce_with_logits
# =============================================================================================
def _bce_launch(scores, labels):
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    s, y = scores.to(dev()), labels.to(dev())
    loss = torch.full((), float('nan'), dtype=torch.float32, device=dev())
    dscores = torch.full((s.shape[0] + 2,), SENTINEL, dtype=torch.float32, device=dev())
    _lib.check(lib.ihg_bce_with_logits(ops._ptr(s), ops._ptr(y), s.shape[0], ops._ptr(loss), ops._ptr(dscores[1:]), ops._stream()), 'ihg_bce_with_logits')
    torch.cuda.synchronize()
    assert float(dscores[0]) == float(dscores[-1]) == np.float32(SENTINEL)
    return loss.cpu(), dscores[1:-1].cpu()


@functools.lru_cache(maxsize=None)
def _bce_float32_cpu_figures():
    """What ``torch.nn.BCEWithLogitsLoss`` in float32 on the CPU shows against the float64 values over all the sizes: (worst relative loss error, worst |dscores n| error)."""
    worst_loss, worst_grad = 0.0, 0.0
    for n in R.BCE_SIZES:
        scores, labels = R.bce_inputs(n)
        want_loss, want_grad = R.bce_reference(scores, labels)
        s = scores.clone().requires_grad_()
        loss = torch.nn.BCEWithLogitsLoss()(s, labels)
        loss.backward()
        worst_loss = max(worst_loss, abs(float(loss.detach()) - want_loss) / abs(want_loss))
        worst_grad = max(worst_grad, float(np.abs(s.grad.double().numpy() * n - want_grad).max()))
    return worst_loss, worst_grad


@pytest.mark.parametrize('n', R.BCE_SIZES)
def test_bce_with_logits_matches_float64(n):
    """``ihg_bce_with_logits`` on its own at the lengths around its 1,024-thread tree and at the logits where a BCE goes wrong (+-0, +-1e-8, |s| = 16.7 where 1 + e
    rounds to 1, 88.8 and 104 where expf underflows, 3e4; soft labels), against float64 ``max(s, 0) - s y + log1p(exp(-|s|))`` and ``(sigmoid(s) - y) / n``.  The loss
    (relative) and ``dscores n`` (absolute) may be 4 x as far from float64 as torch's float32 BCEWithLogitsLoss on the CPU is over these sizes (the kernel sums in another
    tree and calls another libm's expf / log1pf; a missing branch of the stable forms is off by 10^-1 beyond |s| = 17).  Exactly: the gradient is finite everywhere,
    it is -y / n at s = -3e4 and (1 - y) / n at s = +3e4 to two roundings (1 / n and the product), and a second launch gives the same bits."""
    ref_loss, ref_grad = _bce_float32_cpu_figures()
    scores, labels = R.bce_inputs(n)
    want_loss, want_grad = R.bce_reference(scores, labels)
    loss, dscores = _bce_launch(scores, labels)
    loss2, dscores2 = _bce_launch(scores, labels)
    got_loss = abs(float(loss.detach()) - want_loss) / abs(want_loss)
    got_grad = float(np.abs(dscores.double().numpy() * n - want_grad).max())
    print(f'bce n = {n}: loss rel {got_loss:.2e} (torch float32 on the CPU, worst over the sizes: {ref_loss:.2e}), dscores n abs {got_grad:.2e} ({ref_grad:.2e})')
    assert bool(torch.isfinite(dscores).all()) and bool(torch.isfinite(loss))
    assert torch.equal(loss, loss2) and torch.equal(dscores, dscores2)
    for k in range(min(n, len(R.BCE_EDGES))):
        if abs(float(scores[k])) == 3e4:
            exact = ((1.0 if scores[k] > 0 else 0.0) - float(labels[k])) / n
            assert abs(float(dscores[k]) - exact) <= 2 * U * abs(exact), (k, float(dscores[k]), exact)
    assert ref_loss > 0 and ref_grad > 0
    assert got_loss <= 4 * ref_loss and got_grad <= 4 * ref_grad


# =============================================================================================
# 5. ihg_hem_score_fwd / bwd and the _typed0 pair
# =============================================================================================
N_USERS, N_QUERIES, N_ITEMS, N_UPPER = 40, 15, 50, 70
N_NODES = N_USERS + N_QUERIES + N_ITEMS
HEM_BATCHES = (1, 63, 65, 3300)
HEM_LAMBDAS = (0.0, 0.3, 1.0)


def _slices(buffer, n_layers, dim):
    """Layer matrices as column slices of one wider buffer: same row stride > dim, starts off 16-byte alignment."""
    return [buffer[:, 1 + l * (dim + 1): 1 + l * (dim + 1) + dim] for l in range(n_layers)]


def _hem_check_forward(got, want, abs_terms, n_layers, dim, what):
    """Per row: the kernel rounds each product five times (1 - lam, two weighted rows, their sum, the product with the item row), a lane adds n_layers x ceil(dim / 64) of
    them in sequence, six shuffle steps and the bias follow: |error| <= u (n_layers ceil(dim / 64) + 12) (sum of |products| + |bias|) - a rounding count, tighter than
    ``rel <= RTOL_SUM`` for every row that does not cancel and meaningful for the rows that do (a batch of one row has no other row to be relative to)."""
    bound = U * (n_layers * -(-dim // 64) + 12) * abs_terms
    err = np.abs(got.double().cpu().numpy() - want)
    assert (err <= bound).all(), f'{what}: score error / bound {float((err / np.maximum(bound, 1e-300)).max()):.2f}'


def _hem_check_backward(rowgrad, width, batch, grads, scales, ds, what):
    """Per entry: user and query rows ``ds w X[i]`` round four times at most (ds = dscores x grad_scale, 1 - lam, two products): <= 4u |ds w X[i]|; the item row
    ``ds (lam X[q] + (1 - lam) X[u])`` six times (1 - lam, two products, the sum, ds, the product): <= 6u |ds| (lam |X[q]| + (1 - lam) |X[u]|).  An entry whose scale is 0
    (lam = 0 or 1, a zero row standing for an isolated node) is exactly 0.  Column L d: d bias = ds for the item row, 0 for the other two; the columns behind it keep
    their sentinel."""
    got = rowgrad.double().cpu().numpy().reshape(3, batch, -1)
    for k, factor in ((0, 4), (1, 4), (2, 6)):
        err = np.abs(got[k][:, :width] - grads[k])
        assert (err <= factor * U * scales[k]).all(), f'{what}: row block {k}: error / (u scale) {float((err / np.maximum(U * scales[k], 1e-300)).max()):.2f}'
    assert (got[0][:, width] == 0).all() and (got[1][:, width] == 0).all()
    assert (np.abs(got[2][:, width] - ds) <= U * np.abs(ds)).all()
    if got.shape[2] > width + 1:
        assert (got[:, :, width + 1:] == np.float32(SENTINEL)).all(), f'{what}: columns behind the bias column were written'


@pytest.mark.parametrize('dim', [1, 7, 33, 64, 100, 256, 320])
@pytest.mark.parametrize('n_layers', [1, 2, 5, 8])
def test_hem_score_kernels_match_float64(n_layers, dim):
    """``ihg_hem_score_fwd / bwd`` and the ``_typed0`` pair on their own, for 1 - 8 layer outputs of any width that are column slices of a wider buffer, batches of 1, 63,
    65 and 3,300 rows and lam = 0, 0.3, 1 (rotating over the batches so that every pair occurs over the cases), against float64
    ``sum_l X_l[i] (lam X_l[q] + (1 - lam) X_l[u]) + bias[i]`` and its three row gradients.  Three call forms per batch:

    * ``ops.hem_score`` and ``ihg_hem_score_bwd`` (host ``grad_scale`` = float32(1 / 3)) with every layer in one numbering;
    * ``ihg_hem_score_fwd_typed0`` / ``ops._hem_row_gradients`` with the layers above layer 0 in a numbering of their own (``rows_upper``) that holds -1 for some users,
      some queries, some items and both user and query of a row: the forward still adds the bias there, the backward writes the gradient of zero rows (zeros where
      the formula has a zero factor - never stale memory), ``grad_scale`` x a device scalar (0.75 x 3 / 128: exact in float32, so the count of four roundings holds);
    * the same with layer 0 read from three typed tables (``layer0_rows``, ``type_begin``; rows 1.. of a user and an item table, the query rows) against the same values
      assembled by ``torch.cat``, into a sentinel-filled ``rowgrad`` of width L d + 4."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    case = [1, 2, 5, 8].index(n_layers) * 7 + [1, 7, 33, 64, 100, 256, 320].index(dim)
    gen = torch.Generator().manual_seed(500 + case)
    width = n_layers * dim
    wide = torch.randn(N_NODES, n_layers * (dim + 1) + 3, generator=gen).to(dev())
    wide_up = torch.randn(N_UPPER, n_layers * (dim + 1) + 3, generator=gen).to(dev())
    layers, upper = _slices(wide, n_layers, dim), _slices(wide_up, n_layers, dim)
    user_table, query_rows, item_table = (torch.randn(n, dim + 2, generator=gen).to(dev()) for n in (N_USERS + 1, N_QUERIES, N_ITEMS + 1))
    layer0 = torch.cat([user_table[1:, :dim], query_rows[:, :dim], item_table[1:, :dim]])
    layer0_rows = (ctypes.c_void_p * 3)(user_table[1:, :dim].data_ptr(), query_rows.data_ptr(), item_table[1:, :dim].data_ptr())
    type_begin = (ctypes.c_int64 * 4)(0, N_USERS, N_USERS + N_QUERIES, N_NODES)
    bias = torch.randn(N_ITEMS, generator=gen).to(dev())
    host = lambda xs: [x.double().cpu().numpy() for x in xs]
    for b_index, batch in enumerate(HEM_BATCHES):
        lam = HEM_LAMBDAS[(case + b_index) % 3]
        what = f'L = {n_layers}, d = {dim}, B = {batch}, lam = {lam}'
        items = torch.randint(0, N_ITEMS, (batch,), generator=gen)
        rows = torch.cat([torch.randint(0, N_USERS, (batch,), generator=gen), N_USERS + torch.randint(0, N_QUERIES, (batch,), generator=gen), N_USERS + N_QUERIES + items])
        rows_upper = torch.randint(0, N_UPPER, (3 * batch,), generator=gen)
        rows_upper[torch.rand(3 * batch, generator=gen) < 0.2] = -1
        for r, blocks in enumerate(((0,), (1,), (2,), (0, 1))):     # the first rows: user / query / item / user and query isolated
            if r < batch:
                keep = rows_upper[r::batch].clone()
                rows_upper[r::batch] = torch.where(keep < 0, torch.zeros_like(keep), keep)
                for k in blocks:
                    rows_upper[k * batch + r] = -1
        dscores = (torch.randn(batch, generator=gen) / batch)
        rows_d, upper_d, items_d, dscores_d = rows.to(dev()), rows_upper.to(dev()), items.to(dev()), dscores.to(dev())
        rows_np, upper_np, items_np, bias_np = rows.numpy(), rows_upper.numpy(), items.numpy(), bias.double().cpu().numpy()

        # (a) one numbering, the plain entry points
        scale = R.f32(1.0 / 3.0)
        ds = dscores.double().numpy() * scale
        want, abs_terms, grads, scales = R.hem_reference(host(layers), rows_np, None, items_np, bias_np, lam, ds)
        got = ops.hem_score(layers, rows_d, items_d, bias, lam, N_USERS + N_QUERIES)
        _hem_check_forward(got, want, abs_terms, n_layers, dim, what + ' (plain)')
        ptrs = (ctypes.c_void_p * n_layers)(*[x.data_ptr() for x in layers])
        rowgrad = torch.full((3 * batch, width + 4), SENTINEL, dtype=torch.float32, device=dev())
        _lib.check(lib.ihg_hem_score_bwd(ptrs, n_layers, wide.stride(0), dim, ops._ptr(rows_d), ops._ptr(dscores_d), scale, lam, ops._ptr(rowgrad), width + 4, batch,
                                         ops._stream()), 'ihg_hem_score_bwd')
        _hem_check_backward(rowgrad, width, batch, grads, scales, ds, what + ' (plain)')

        # (b) the layers above layer 0 in their own numbering with isolated nodes; the upstream gradient a device scalar
        mixed = [layers[0]] + upper[1:]
        device_scale = torch.tensor(3.0 / 128.0, dtype=torch.float32, device=dev())
        ds = dscores.double().numpy() * (0.75 * 3.0 / 128.0)
        want, abs_terms, grads, scales = R.hem_reference(host(mixed), rows_np, upper_np, items_np, bias_np, lam, ds)
        ptrs = (ctypes.c_void_p * n_layers)(*[x.data_ptr() for x in mixed])
        got = torch.full((batch,), SENTINEL, dtype=torch.float32, device=dev())
        _lib.check(lib.ihg_hem_score_fwd_typed0(ptrs, n_layers, wide.stride(0), dim, None, 0, None, ops._ptr(rows_d), ops._ptr(upper_d), ops._ptr(items_d), ops._ptr(bias),
                                                lam, ops._ptr(got), batch, ops._stream()), 'ihg_hem_score_fwd_typed0')
        _hem_check_forward(got, want, abs_terms, n_layers, dim, what + ' (rows_upper)')
        rowgrad = ops._hem_row_gradients(mixed, rows_d, items_d, bias, lam, dscores_d, 0.75, None, device_scale, upper_d)
        assert tuple(rowgrad.shape) == (3 * batch, width + 4)
        _hem_check_backward(rowgrad[:, :width + 1], width, batch, grads, scales, ds, what + ' (rows_upper)')

        # (c) layer 0 from the typed tables
        typed = [layer0] + upper[1:]
        want, abs_terms, grads, scales = R.hem_reference(host(typed), rows_np, upper_np, items_np, bias_np, lam, ds)
        ptrs = (ctypes.c_void_p * n_layers)(query_rows.data_ptr(), *[x.data_ptr() for x in upper[1:]])
        got = torch.full((batch,), SENTINEL, dtype=torch.float32, device=dev())
        _lib.check(lib.ihg_hem_score_fwd_typed0(ptrs, n_layers, wide_up.stride(0), dim, layer0_rows, dim + 2, type_begin, ops._ptr(rows_d), ops._ptr(upper_d), ops._ptr(items_d),
                                                ops._ptr(bias), lam, ops._ptr(got), batch, ops._stream()), 'ihg_hem_score_fwd_typed0')
        _hem_check_forward(got, want, abs_terms, n_layers, dim, what + ' (typed layer 0)')
        rowgrad = torch.full((3 * batch, width + 4), SENTINEL, dtype=torch.float32, device=dev())
        _lib.check(lib.ihg_hem_score_bwd_typed0(ptrs, n_layers, wide_up.stride(0), dim, layer0_rows, dim + 2, type_begin, ops._ptr(rows_d), ops._ptr(upper_d), ops._ptr(dscores_d),
                                                ops._ptr(device_scale), 0.75, lam, ops._ptr(rowgrad), width + 4, batch, ops._stream()), 'ihg_hem_score_bwd_typed0')
        _hem_check_backward(rowgrad, width, batch, grads, scales, ds, what + ' (typed layer 0)')
    torch.cuda.synchronize()


def test_hem_score_plain_entry_points_are_the_typed0_ones_bitwise():
    """``ihg_hem_score_fwd / _bwd`` forward into the body of the ``_typed0`` pair with no typed layer 0, no ``rows_upper`` and no device scalar: the same kernel with the
    same arguments, so scores and row gradients are ``torch.equal`` - 2 layers of 100 columns (two passes over the lanes, the second partial), 5 rows (a partly filled
    second workgroup), 12 nodes; the row gradients in sentinel-filled buffers of width 2 x 100 + 4, where a write behind the bias column shows."""
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    n_layers, dim, batch, n_nodes = 2, 100, 5, 12
    width = n_layers * dim
    gen = torch.Generator().manual_seed(577)
    layers = [torch.randn(n_nodes, dim, generator=gen).to(dev()) for _ in range(n_layers)]
    bias = torch.randn(4, generator=gen).to(dev())
    items = torch.randint(0, 4, (batch,), generator=gen)
    rows = torch.cat([torch.randint(0, 4, (batch,), generator=gen), 4 + torch.randint(0, 4, (batch,), generator=gen), 8 + items]).to(dev())
    items, dscores = items.to(dev()), torch.randn(batch, generator=gen).to(dev())
    ptrs = (ctypes.c_void_p * n_layers)(*[x.data_ptr() for x in layers])
    scores = [torch.full((batch,), SENTINEL, dtype=torch.float32, device=dev()) for _ in range(2)]
    rowgrad = [torch.full((3 * batch, width + 4), SENTINEL, dtype=torch.float32, device=dev()) for _ in range(2)]
    _lib.check(lib.ihg_hem_score_fwd(ptrs, n_layers, dim, dim, ops._ptr(rows), ops._ptr(items), ops._ptr(bias), 0.3, ops._ptr(scores[0]), batch, ops._stream()), 'ihg_hem_score_fwd')
    _lib.check(lib.ihg_hem_score_fwd_typed0(ptrs, n_layers, dim, dim, None, 0, None, ops._ptr(rows), None, ops._ptr(items), ops._ptr(bias), 0.3, ops._ptr(scores[1]), batch,
                                            ops._stream()), 'ihg_hem_score_fwd_typed0')
    _lib.check(lib.ihg_hem_score_bwd(ptrs, n_layers, dim, dim, ops._ptr(rows), ops._ptr(dscores), 0.75, 0.3, ops._ptr(rowgrad[0]), width + 4, batch, ops._stream()),
               'ihg_hem_score_bwd')
    _lib.check(lib.ihg_hem_score_bwd_typed0(ptrs, n_layers, dim, dim, None, 0, None, ops._ptr(rows), None, ops._ptr(dscores), None, 0.75, 0.3, ops._ptr(rowgrad[1]), width + 4,
                                            batch, ops._stream()), 'ihg_hem_score_bwd_typed0')
    assert bool((scores[0] != SENTINEL).all()) and torch.equal(scores[0], scores[1])
    assert bool((rowgrad[0][:, :width + 1] != SENTINEL).all()) and bool((rowgrad[0][:, width + 1:] == SENTINEL).all()) and torch.equal(rowgrad[0], rowgrad[1])


def test_hem_score_refuses_nine_layers():
    from ihgnn_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(4, 4, device=dev())
    rows, items = torch.zeros(3, dtype=torch.int64, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev())
    out = torch.zeros(3, 40, device=dev())
    ptrs = (ctypes.c_void_p * 9)(*[x.data_ptr()] * 9)
    assert lib.ihg_hem_score_fwd(ptrs, 9, 4, 4, ops._ptr(rows), ops._ptr(items), ops._ptr(out), 0.5, ops._ptr(out), 1, ops._stream()) == _lib.ERR_INVALID
    assert '1..8' in _lib.last_error()
    assert lib.ihg_hem_score_bwd(ptrs, 9, 4, 4, ops._ptr(rows), ops._ptr(out), 1.0, 0.5, ops._ptr(out), 40, 1, ops._stream()) == _lib.ERR_INVALID
    with pytest.raises(_lib.IhgnnHipError):
        ops.hem_score([x] * 9, rows, items, torch.zeros(4, device=dev()), 0.5, 0)
