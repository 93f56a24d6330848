"""GPU: gradient clipping through the optimizer, the recorded step, the sharded and the cotangent exchange (a one-rank process group with the collectives forced on)
and the driver, on the small fixture graph the loss model tests use.  References and bounds: ``tests/clip_reference.py``.

Run as a script (``python tests/test_grad_clip_model.py --child sharded | cotangent``) this file is the one-rank child process of the two exchange tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import clip_reference as C
import update_tail_reference as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD = 1e-2, 1e-2
HYPER = (LR, 0.9, 0.999, 1e-8, WD)
CLIP = 1e-3                                                  # far below the fixture's gradient norms (1e-2 .. 1): every step clips


def dev():
    return torch.device('cuda:0')


def fixture_dataset():
    from ihgnn_amd import synth
    from ihgnn_amd.Dataset import GraphDataset
    w = synth.draw(60, 20, 80, 25, 500)
    return GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())


def build_model(ds, d=32, seed=11):
    from ihgnn_amd.Models import HemPredictionLayer, IHGNNLayer, RawGnn
    torch.manual_seed(seed)
    return RawGnn(dev(), ds, d, IHGNNLayer, 2, 3, False, HemPredictionLayer, 0.5).to(dev())


def snapshot(model, opt):
    """name -> (p, g, m, v) clones on the CPU of every parameter that has a gradient (zero moments before the first step)."""
    out = {}
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        state = opt.state.get(p, {})
        zeros = torch.zeros_like(p)
        out[name] = tuple(x.detach().cpu().clone().reshape(-1) for x in (p, p.grad, state.get('exp_avg', zeros), state.get('exp_avg_sq', zeros)))
    return out


def assert_step_within_bounds(before, model, opt, t, max_norm, what):
    """The step just taken from ``before`` against the float64 reference driven with the same gradients: norm within 1 ulp, coefficient within its bound, every
    entry of p, exp_avg, exp_avg_sq within K_v, K_m, K_p of its scale.  -> (norm64, coef64)."""
    norm64 = C.norm_reference([g.numpy() for _, g, _, _ in before.values()])
    coef64 = C.coef_reference(norm64, max_norm)
    norm, coef = opt.grad_norm.tolist()
    assert C.norm_within_one_ulp(norm, norm64) and abs(coef - coef64) <= C.coef_bound(norm64, max_norm), (what, norm, norm64, coef, coef64)
    worst = dict(p=0.0, m=0.0, v=0.0, tiny_share=0.0)
    params = dict(model.named_parameters())
    for name, (p, g, m, v) in before.items():
        ref = C.adam_reference_clipped(p, g, m, v, HYPER, t, coef64)
        state = opt.state[params[name]]
        errors = R.adam_errors(params[name].detach().cpu().reshape(-1), state['exp_avg'].cpu().reshape(-1), state['exp_avg_sq'].cpu().reshape(-1), ref)
        worst = {k: max(worst[k], errors[k]) for k in worst}
    print(f'{what}: norm {norm!r} (float64 {norm64!r}) coef {coef!r}; worst error / (u x scale) {worst}')
    C.assert_clipped_adam_within_bounds(worst, what)
    return norm64, coef64


def assert_reference_is_torchs_rule(before, t, max_norm, coef64):
    """``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` in float64 on copies of the same p, g, exp_avg, exp_avg_sq (hyper-parameters as the ABI receives
    them, float32 values) against the reference restatement: exp_avg and exp_avg_sq to 1e-9 relative - float64 roundings and the 3e-14 between torch's 1e-6 and the
    float32 1e-6 the kernel adds.  The parameters besides by ``2u x 3.2 lr``: the reference takes ``lr / (1 - beta1^t)`` and ``sqrt(1 - beta2^t)`` rounded to float32, as
    the ABI passes them (u relative each), torch forms them in float64, and an Adam update is at most ``lr max(1, (1 - beta1) / sqrt(1 - beta2))`` = 3.2 lr in size."""
    lr, b1, b2, eps, wd = (R.f32(x) for x in HYPER)
    copies = {name: torch.nn.Parameter(p.double()) for name, (p, _, _, _) in before.items()}
    opt = torch.optim.Adam(copies.values(), lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for name, (_, g, m, v) in before.items():
        copies[name].grad = g.double()
        opt.state[copies[name]] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    torch.nn.utils.clip_grad_norm_(list(copies.values()), R.f32(max_norm), norm_type=2, error_if_nonfinite=False)
    opt.step()
    for name, (p, g, m, v) in before.items():
        ref = C.adam_reference_clipped(p, g, m, v, HYPER, t, coef64)
        for got, want, slack in ((copies[name].detach(), ref['p'], 2 * C.U * 3.2 * lr), (opt.state[copies[name]]['exp_avg'], ref['m'], 0.0),
                                 (opt.state[copies[name]]['exp_avg_sq'], ref['v'], 0.0)):
            assert float((got - want).abs().max()) <= 1e-9 * max(float(want.abs().max()), 1e-300) + slack, name


def test_eager_clipped_steps_match_the_float64_reference_and_torch():
    """Three eager steps with ``max_grad_norm`` = 1e-3 (every step clips; weight decay on), each held to the bounds against the float64 reference driven with the step's own
    gradients and moments; the reference itself is ``clip_grad_norm_`` + ``torch.optim.Adam`` in float64 on copies.  ``.grad`` is not rewritten; the statistics say 3 of 3."""
    from ihgnn_amd.optim import Adam
    ds = fixture_dataset()
    m = build_model(ds)
    opt = Adam(m.parameters(), LR, weight_decay=WD, max_grad_norm=CLIP)
    norms = []
    for t, (u, q, i, y) in enumerate(ds.sample_batches(40, 3, seed=9), start=1):
        m.bce_loss(u, q, i, y).backward()
        before = snapshot(m, opt)
        opt.step()
        norm64, coef64 = assert_step_within_bounds(before, m, opt, t, CLIP, f'step {t}')
        assert coef64 < 1
        assert_reference_is_torchs_rule(before, t, CLIP, coef64)
        for name, p in m.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad.cpu().reshape(-1), before[name][1]), f'{name}: .grad was rewritten'
        norms.append(norm64)
        opt.zero_grad()
    largest, clipped, steps = opt.clip_statistics()
    assert (clipped, steps) == (3, 3) and C.norm_within_one_ulp(largest, max(norms))
    assert opt.clip_statistics() == (0.0, 0, 0)


def test_off_and_infinite_bounds_are_todays_step_bit_for_bit():
    """``max_grad_norm=None`` (no launch added: the record stays ``None``) and ``max_grad_norm=inf`` (three launches, coefficient exactly 1) leave the same parameters and
    moments, bit for bit, over three steps with weight decay."""
    from ihgnn_amd.optim import Adam
    ds = fixture_dataset()
    batches = list(ds.sample_batches(40, 3, seed=9))
    results = []
    for bound in (None, float('inf')):
        m = build_model(ds)
        opt = Adam(m.parameters(), LR, weight_decay=WD, max_grad_norm=bound)
        for u, q, i, y in batches:
            m.bce_loss(u, q, i, y).backward()
            opt.step()
            opt.zero_grad()
            assert (opt.grad_norm is None) if bound is None else (float(opt.grad_norm[1]) == 1.0 and float(opt.grad_norm[0]) > 0)
        results.append(({k: v.clone() for k, v in m.state_dict().items()}, [(opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for p in m.parameters()]))
    (p0, s0), (p1, s1) = results
    for name in p0:
        assert torch.equal(p0[name], p1[name]), name
    for (m0, v0), (m1, v1) in zip(s0, s1):
        assert torch.equal(m0, m1) and torch.equal(v0, v1)


def test_recorded_clipped_step_equals_the_eager_one_and_a_changed_bound_is_stale():
    """Four replays of a step recorded with clipping on equal four eager steps bit for bit - loss, parameters, the last record, the statistics (which advance per
    replay); the bound is baked into the recording: after ``optimizer.max_grad_norm`` changes ``stale()`` says so, ``step()`` refuses, and a new recording takes it."""
    from ihgnn_amd import synth
    from ihgnn_amd.captured_step import CapturedTrainingStep
    from ihgnn_amd.Dataset import GraphDataset
    from ihgnn_amd.optim import Adam
    w = synth.draw(300, 40, 200, 50, 4000, seed=21, distribution='powerlaw')
    ds = GraphDataset.from_arrays(w.user_count, w.query_count, w.item_count, w.vocab_size, w.bag_words, w.bag_offsets, w.triples, device=dev())
    batches = list(ds.sample_batches(100, 4, seed=5))
    kept = []

    def run(recorded):
        m = build_model(ds, d=64, seed=7)
        opt = Adam(m.parameters(), 1e-3, weight_decay=WD, max_grad_norm=CLIP)
        step = CapturedTrainingStep(m, opt, batches[0][0].shape[0], warmup_batch=batches[0]) if recorded else None
        losses = []
        for u, q, i, y in batches:
            if recorded:
                losses.append(step.step(u, q, i, y).clone())
            else:
                loss = m.bce_loss(u, q, i, y)
                loss.backward(); opt.step(); opt.zero_grad()
                losses.append(loss.detach().clone())
        kept.append((step, opt))
        return losses, {k: v.clone() for k, v in m.state_dict().items()}, opt.grad_norm.clone(), opt.clip_statistics(reset=False)

    l0, p0, r0, s0 = run(False)
    l1, p1, r1, s1 = run(True)
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    for name in p0:
        assert torch.equal(p0[name], p1[name]), name
    assert torch.equal(r0, r1) and s0 == s1 and s0[1:] == (4, 4) and float(r0[1]) < 1
    step, opt = kept[-1]
    assert not step.stale() and not step.stale(full=True)
    opt.max_grad_norm = 0.5
    assert step.stale() and step.stale(full=True)
    with pytest.raises(RuntimeError, match='baked into the recording'):
        step.step(*batches[0])
    again = CapturedTrainingStep(step.model, opt, batches[0][0].shape[0], warmup_batch=batches[0])
    assert not again.stale()
    again.step(*batches[0])
    torch.cuda.synchronize()
    assert float(opt.grad_norm[1]) == float(np.float32(0.5) / (np.float32(opt.grad_norm[0].item()) + np.float32(1e-6))) or float(opt.grad_norm[1]) == 1.0
    opt.max_grad_norm = None                                 # off: the recording with the three launches is stale as well
    assert again.stale()


# ---------------------------------------------------------------------------------------------
# a one-rank process group with the collectives forced on (child process: this file run as a script)
# ---------------------------------------------------------------------------------------------
def _child(mode):
    """One step of the fixture model under ``mode`` in a one-rank group (``IHG_FORCE_COLLECTIVES=1``: every collective runs, as an identity) beside the same step of the
    plain optimizer: both records and both sets of parameters are held to the float64 reference of the plain step's gradients - the sharded optimizer cuts its flat
    shard into other chunks than the parameter list, so its double sum may differ in the last bits, its float32 norm by one ulp, and its parameters by what
    ``clip_reference``'s bounds allow around one reference; under ``cotangent`` the norm is local and ``check_replicas()`` stays 0."""
    import torch.distributed as dist
    from ihgnn_amd import distributed as ihg_dist
    from ihgnn_amd.optim import Adam
    ihg_dist.init_from_env('nccl')
    torch.cuda.set_device(dev())
    ds = fixture_dataset()
    u, q, i, y = next(iter(ds.sample_batches(40, 1, seed=9)))
    plain = build_model(ds)
    opt0 = Adam(plain.parameters(), LR, weight_decay=WD, max_grad_norm=CLIP)
    plain.bce_loss(u, q, i, y).backward()
    before = snapshot(plain, opt0)
    opt0.step()
    norm64, coef64 = assert_step_within_bounds(before, plain, opt0, 1, CLIP, 'plain')
    model = build_model(ds)
    sync = ihg_dist.make_gradient_sync(model, mode)
    assert sync.distributed
    sync.broadcast_parameters(0)
    opt = sync.optimizer(LR, WD, max_grad_norm=CLIP) if sync.owns_optimizer else Adam(model.parameters(), LR, weight_decay=WD, max_grad_norm=CLIP)
    if mode == 'cotangent':
        model.bce_loss(u, q, i, y, cotangent_sync=sync).backward()
    else:
        model.bce_loss(u, q, i, y).backward()
    sync.average_gradients()
    opt.step()
    torch.cuda.synchronize()
    norm, coef = opt.grad_norm.tolist()
    norm0, coef0 = opt0.grad_norm.tolist()
    print(f'{mode}: norm {norm!r} coef {coef!r}; plain optimizer {norm0!r} {coef0!r}; float64 {norm64!r} {coef64!r}', flush=True)
    assert C.norm_within_one_ulp(norm, norm64) and abs(norm - norm0) <= float(np.spacing(np.float32(norm0)))
    assert abs(coef - coef64) <= C.coef_bound(norm64, CLIP)
    worst = dict(p=0.0)
    params = dict(model.named_parameters())
    for name, (p, g, m, v) in before.items():
        ref = C.adam_reference_clipped(p, g, m, v, HYPER, 1, coef64)
        err = (params[name].detach().cpu().reshape(-1).double() - ref['p']).abs()
        assert bool((err[ref['S_p'] == 0] == 0).all())
        keep = ref['S_p'] >= R.TINY_SCALE
        worst['p'] = max(worst['p'], float((err[keep] / (C.U * ref['S_p'][keep])).max()))
    print(f'{mode}: worst parameter error / (u x scale) {worst["p"]} (bound {C.K_P})', flush=True)
    assert worst['p'] <= C.K_P
    assert opt.clip_statistics()[1:] == (1, 1)
    if mode == 'cotangent':
        assert sync.check_replicas() == 0.0
    dist.barrier()
    dist.destroy_process_group()
    print('OK', flush=True)


@pytest.mark.parametrize('mode', ['sharded', 'cotangent'])
def test_one_rank_group_clips_to_the_same_record(mode):
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0', IHG_FORCE_COLLECTIVES='1',
               PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', mode], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith('OK'), r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [True, False])
def test_driver_logs_the_gradient_norm_when_clipping_is_on(clip, tmp_path):
    """``python -m ihgnn_amd.Main ... --clip_grad_norm 0.5 --query_transform gru --loss bpr`` in a child process, two epochs on the fixture corpus: exit 0, the settings
    line names the bound, every epoch logs ``grad norm max ... | clipped n of m steps``; without the flag neither appears."""
    from ihgnn_amd import synth
    w = synth.draw(60, 20, 80, 25, 500, seed=4, eval_logs=30)
    synth.write_files(w, str(tmp_path / 'Data' / 'Synth' / 'Tiny'))
    command = [sys.executable, '-m', 'ihgnn_amd.Main', '--ds', 'Synth/Tiny/', '--gnn', 'IHGNN', '--gnns', '2', '--fo', '3', '--emb', '32', '--seed', '3', '--loss', 'bpr',
               '--query_transform', 'gru', '--ec', '2', '--est', '2', '--etf', '2'] + (['--clip_grad_norm', '0.5'] if clip else [])
    r = subprocess.run(command, cwd=str(tmp_path), capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', '')))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / 'Results' / 'Synth-Tiny-RawGnn-2IHGNNLayer-O3-emb32'
    log = open(out / 'train_log.txt', encoding='utf-8').read()
    lines = re.findall(r'grad norm max (\S+) +\| clipped (\d+) of (\d+) steps', log)
    if not clip:
        assert lines == [] and 'clip grad norm' not in log
        return
    assert '| clip grad norm 0.5' in log and len(lines) == 2, log[-2000:]
    for largest, clipped, steps in lines:
        assert np.isfinite(float(largest)) and float(largest) > 0 and 0 <= int(clipped) <= int(steps) and int(steps) == int(lines[0][2]) >= 1


if __name__ == '__main__':
    _child(sys.argv[sys.argv.index('--child') + 1])
