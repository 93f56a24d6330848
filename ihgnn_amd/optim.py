"""``Adam``: ``torch.optim.Adam`` for the parameters of this package's models, stepped by one HIP launch.

Same constructor keywords, update rule, ``state_dict`` layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter) and
checkpoint compatibility as ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (reference ``Main.py:192``; amsgrad,
maximize and tensor learning rates are not carried).  The elementwise update is a pure HBM stream; torch's multi-tensor kernel
reaches ~3.2 TB/s on the 16 M embedding parameters of the C2 workload, ``ihg_adam_step`` is a single vectorised pass.

``max_grad_norm`` (not in the reference; default ``None`` = off, and then every launch is what it is without the keyword): the step of
``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` followed by ``Adam.step()`` - one more read of the gradients for their global L2 norm
(``ihg_grad_sqnorm``), a one-thread launch that turns it into the coefficient (``ihg_clip_record``), and the update on ``grad * coef``
(``ihg_adam_step_clipped``).  The one difference from torch: ``.grad`` is not rewritten; the scaled gradient is ``p.grad * optimizer.grad_norm[1]``.
"""
import ctypes
from typing import Iterable, Optional

import torch
from torch.optim import Optimizer

from . import _lib

CHUNK = 4096                                                 # kAdamChunk (csrc/tail.hip): elements per partial of the gradient norm


class _AdamTensor(ctypes.Structure):
    _fields_ = [('param', ctypes.c_void_p), ('grad', ctypes.c_void_p), ('exp_avg', ctypes.c_void_p), ('exp_avg_sq', ctypes.c_void_p),
                ('count', ctypes.c_int64)]


def _table(items):
    table = (_AdamTensor * len(items))()
    for slot, (p, grad, state) in zip(table, items):
        slot.param, slot.grad = p.data_ptr(), grad.data_ptr()
        slot.exp_avg, slot.exp_avg_sq = state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr()
        slot.count = p.numel()
    return table


class Adam(Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm: Optional[float] = None):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f'invalid Adam hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0:
            raise ValueError(f'invalid Adam hyper-parameters: max_grad_norm={max_grad_norm} (None = off, else >= 0; inf allowed)')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        # an attribute, not a param_groups key: the norm is global over every group, and state_dict() stays torch.optim.Adam's
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None                                # float32 [2] on the device: (norm, coef) of the last clipped step
        self._clip_stats = None                              # float32 [3] on the device: largest norm, steps with coef < 1, steps (since the last reset)
        self._clip_sum = None                                # float64 [1]: the sum of squares the record is formed from
        self._clip_partials = None                           # float64 [chunks]: ihg_grad_sqnorm's workspace
        self._sum_reduce = None                              # callable(sum) between the norm and the record: a sharded optimizer adds the ranks' sums there

    # ------------------------------------------------------------------ clipping by the global gradient norm
    def _ensure_clip_buffers(self, device, chunks: int) -> None:
        if self.grad_norm is None or self.grad_norm.device != device:
            self.grad_norm = torch.zeros(2, dtype=torch.float32, device=device)
            self._clip_stats = torch.zeros(3, dtype=torch.float32, device=device)
            self._clip_sum = torch.zeros(1, dtype=torch.float64, device=device)
            self._clip_partials = None
        if self._clip_partials is None or self._clip_partials.numel() < chunks:
            self._clip_partials = torch.empty(max(chunks, 1), dtype=torch.float64, device=device)

    def _launch_clip_record(self, lib, items, stream) -> ctypes.c_void_p:
        """Norm of the gradients of ``items`` (every parameter group's) and the clip record from it; -> the record's address for the clipped update."""
        device = items[0][0].device
        self._ensure_clip_buffers(device, sum(-(-p.numel() // CHUNK) for p, _, _ in items))
        table = _table(items)
        partials = self._clip_partials
        _lib.check(lib.ihg_grad_sqnorm(ctypes.cast(table, ctypes.c_void_p), len(items), ctypes.c_void_p(partials.data_ptr()), partials.numel() * 8,
                                       ctypes.c_void_p(self._clip_sum.data_ptr()), stream), 'ihg_grad_sqnorm')
        if self._sum_reduce is not None:
            self._sum_reduce(self._clip_sum)
        _lib.check(lib.ihg_clip_record(ctypes.c_void_p(self._clip_sum.data_ptr()), self.max_grad_norm, ctypes.c_void_p(self.grad_norm.data_ptr()),
                                       ctypes.c_void_p(self._clip_stats.data_ptr()), stream), 'ihg_clip_record')
        return ctypes.c_void_p(self.grad_norm.data_ptr())

    def clip_statistics(self, reset: bool = True):
        """``(largest gradient norm, steps whose gradient was scaled down, steps)`` since the last reset: ONE host read of the three-float record the clip launch
        keeps on the device (the training loop asks once per epoch; no step synchronises).  ``(0.0, 0, 0)`` before the first clipped step."""
        if self._clip_stats is None:
            return 0.0, 0, 0
        largest, clipped, steps = self._clip_stats.tolist()
        if reset:
            self._clip_stats.zero_()
        return largest, int(clipped), int(steps)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        launches = []                                        # (group, step count, items) in launch order
        for group in self.param_groups:
            by_step = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse:
                    raise _lib.IhgnnHipError('ihgnn_amd.optim.Adam steps dense float32 GPU parameters (no CPU path)')
                if not p.is_contiguous():
                    raise _lib.IhgnnHipError('ihgnn_amd.optim.Adam needs contiguous parameters')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = torch.tensor(0.0)                      # host-side counter, as torch keeps it for non-capturable Adam
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if torch.is_tensor(state['step']) and state['step'].is_cuda:   # a checkpoint loaded with map_location=device: keep the
                    state['step'] = state['step'].cpu()                        # counter on the host (int() below would sync every step)
                state['step'] += 1
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(int(state['step']), []).append((p, grad, state))
            launches.extend((group, step, items) for step, items in by_step.items())
        if not launches:
            return loss
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        clip = None
        if self.max_grad_norm is not None:
            clip = self._launch_clip_record(lib, [item for _, _, items in launches for item in items], stream)
        for group, step, items in launches:
            beta1, beta2 = group['betas']
            table = _table(items)
            if clip is None:
                _lib.check(lib.ihg_adam_step(ctypes.cast(table, ctypes.c_void_p), len(items), float(group['lr']), float(beta1), float(beta2),
                                             float(group['eps']), float(group['weight_decay']), step, stream), 'ihg_adam_step')
            else:
                _lib.check(lib.ihg_adam_step_clipped(ctypes.cast(table, ctypes.c_void_p), len(items), float(group['lr']), float(beta1), float(beta2),
                                                     float(group['eps']), float(group['weight_decay']), step, clip, stream), 'ihg_adam_step_clipped')
        return loss

    # ------------------------------------------------------------------ recorded steps (ihgnn_amd/captured_step.py)
    @staticmethod
    def step_scalars(first_step: int, count: int, lr: float, betas) -> torch.Tensor:
        """``(lr / (1 - beta1^t), sqrt(1 - beta2^t))`` for the steps ``t = first_step .. first_step + count - 1``: float32 ``[count, 2]`` on the host, what
        ``ihg_adam_step_device_scalars`` reads.  Exactly ``ihg_adam_step``'s arithmetic: lr and the betas arrive there as fp32, the bias corrections are formed in double."""
        import numpy as np
        lr, beta1, beta2 = (float(np.float32(x)) for x in (lr, betas[0], betas[1]))
        steps = np.arange(first_step, first_step + count, dtype=np.float64)
        return torch.from_numpy(np.stack([lr / (1.0 - np.power(beta1, steps)), np.sqrt(1.0 - np.power(beta2, steps))], 1).astype(np.float32))

    def next_step(self, group_index: int = 0) -> int:
        """The step number the next update of a parameter group will carry (all its parameters share one count)."""
        group = self.param_groups[group_index]
        steps = {int(self.state[p]['step']) if len(self.state.get(p, {})) else 0 for p in group['params'] if p.requires_grad}
        if len(steps) > 1:
            raise _lib.IhgnnHipError('a recorded Adam step needs one step count per parameter group')
        return (steps.pop() if steps else 0) + 1

    @torch.no_grad()
    def ensure_state(self) -> None:
        """Create the moment buffers of every trainable parameter now (a recording must not allocate them) - and, with ``max_grad_norm`` set, the clip record, its
        statistics and the norm's workspace, sized for all of them."""
        trainable = []
        for group in self.param_groups:
            for p in group['params']:
                if p.requires_grad and len(self.state[p]) == 0:
                    self.state[p]['step'] = torch.tensor(0.0)
                    self.state[p]['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self.state[p]['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if p.requires_grad:
                    trainable.append(p)
        if self.max_grad_norm is not None and trainable:
            self._ensure_clip_buffers(trainable[0].device, sum(-(-p.numel() // CHUNK) for p in trainable))

    @torch.no_grad()
    def launch_with_device_scalars(self, scalars: torch.Tensor) -> None:
        """The update of parameter group 0 with the two step-dependent scalars taken from ``scalars`` (float32 ``[2]`` on the device) when the
        kernel runs; the host-side step counters are NOT advanced (``advance()`` does that once per replay).  With ``max_grad_norm`` set the norm and the clip record
        are launched in front of it, as ``step()`` does."""
        lib = _lib.load()
        if len(self.param_groups) != 1:
            raise _lib.IhgnnHipError('a recorded Adam step handles one parameter group')
        group = self.param_groups[0]
        items = []
        for p in group['params']:
            if p.grad is None:
                continue
            state = self.state[p]
            if len(state) == 0:
                state['step'] = torch.tensor(0.0)
                state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not p.grad.is_contiguous() or not p.is_contiguous():
                raise _lib.IhgnnHipError('a recorded Adam step needs contiguous parameters and gradients')
            items.append((p, p.grad, state))
        table = _table(items)
        beta1, beta2 = group['betas']
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.max_grad_norm is not None and items:
            clip = self._launch_clip_record(lib, items, stream)
            _lib.check(lib.ihg_adam_step_clipped_device_scalars(ctypes.cast(table, ctypes.c_void_p), len(items), float(beta1), float(beta2), float(group['eps']),
                                                                float(group['weight_decay']), ctypes.c_void_p(scalars.data_ptr()), clip, stream),
                       'ihg_adam_step_clipped_device_scalars')
            return
        _lib.check(lib.ihg_adam_step_device_scalars(ctypes.cast(table, ctypes.c_void_p), len(items), float(beta1), float(beta2), float(group['eps']),
                                                    float(group['weight_decay']), ctypes.c_void_p(scalars.data_ptr()), stream), 'ihg_adam_step_device_scalars')

    def advance(self) -> None:
        """Count one step on every parameter (after a replay of a recorded step)."""
        for group in self.param_groups:
            for p in group['params']:
                state = self.state.get(p)
                if state:
                    if torch.is_tensor(state['step']) and state['step'].is_cuda:
                        state['step'] = state['step'].cpu()
                    state['step'] += 1
