"""Adam and SGD on gfx950 — the optimizers configs name (``torch.optim.Adam`` in the reference's
configs/sge_sg_*.yaml, ``torch.optim.SGD`` for the DeepWalk / node2vec / word2vec.c update;
instantiated at config_parser/core.py:43-53).

``Adam``: same hyper-parameters, state names (``step``, ``exp_avg``, ``exp_avg_sq``) and update as
torch's single-tensor Adam (torch/optim/adam.py, amsgrad=False); the scalars are computed on
the host in float64 exactly as torch computes them, the tensor update runs in one streaming
kernel per parameter (dw_adam_dense) that can also zero the gradient in the same pass
(``zero_grad_in_step=True``: saves the separate zero_grad pass over V x d).

Fused form (``fuse_into_sgns=True``, the default): when this optimizer holds exactly a model's
two embedding tables, Word2VecTrainer's walk-batch step applies the update itself, inside the
SGNS kernels (the output table's Adam in the records gather, the input table's on a side
stream overlapping it; see Word2VecTrainer._fused_walk_step). It claims the step with
``begin_fused_step``, and the ``step()`` that follows skips those parameters once.

``SGD`` (torch.optim.SGD's hyper-parameters, state name ``momentum_buffer`` and update, bit for
bit torch's on CPU fp32: dw_sgd_dense) has the same handshake in a simpler form: plain SGD
leaves a row with zero gradient where it is, so Word2VecTrainer's walk-batch step applies the
update to the rows the batch lists and to nothing else (``SGD.step_touched`` ->
dw_sgd_rows), exactly.
"""
from typing import Dict, Iterable, List, Sequence, Tuple, Union

import torch
from torch.optim import Optimizer

from shallow_encoders import _native


class Adam(Optimizer):
    """Adam with the math of ``torch.optim.Adam`` (dense; every row moves every step)."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, amsgrad: bool = False, *,
                 zero_grad_in_step: bool = True, fuse_into_sgns: bool = True, **unsupported):
        if unsupported:
            bad = {k: v for k, v in unsupported.items() if v not in (None, False)}
            if bad:
                raise NotImplementedError(f'HIP Adam does not support {sorted(bad)}')
        if amsgrad:
            raise NotImplementedError('HIP Adam does not implement amsgrad')
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid beta parameters: {betas}')
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        amsgrad=False)
        super().__init__(params, defaults)
        self.zero_grad_in_step = zero_grad_in_step
        self.fuse_into_sgns = fuse_into_sgns
        self._fused_done = set()   # ids of parameters whose update this step already applied
        self._alt: Dict[int, torch.Tensor] = {}   # second buffer of double-buffered parameters
        # ids of parameters whose .grad is known to be all zero (a fresh buffer, or one a
        # zeroing step consumed): the fused step needs it — its interior rows never read g
        self._grads_clean = set()

    # ---- fused form ---------------------------------------------------------------------------
    def can_fuse(self, params: List[torch.Tensor]) -> bool:
        """True when this optimizer's update of exactly ``params`` (one group, HIP fp32
        contiguous tensors, gradients zeroed by the step) may run inside the SGNS step."""
        if not (self.fuse_into_sgns and self.zero_grad_in_step) or len(self.param_groups) != 1:
            return False
        mine = self.param_groups[0]['params']
        if len(mine) != len(params) or {id(p) for p in mine} != {id(p) for p in params}:
            return False
        return all(p.device.type == 'cuda' and p.dtype == torch.float32 and p.is_contiguous()
                   and p.grad is not None and p.grad.is_contiguous()
                   and id(p) in self._grads_clean for p in params)

    def mark_grads(self, params: List[torch.Tensor], clean: bool) -> None:
        """Record that the gradients of ``params`` are all zero (``clean``: a new zero buffer)
        or may not be (something accumulated into them outside a fused step)."""
        for p in params:
            (self._grads_clean.add if clean else self._grads_clean.discard)(id(p))

    def begin_fused_step(self, params: List[torch.Tensor]) -> List[Tuple[dict, tuple]]:
        """Count one step for each of ``params`` (state created on first use) and return
        ``(state, dw_adam_dense scalars)`` per parameter; the next ``step()`` skips them."""
        out = []
        group = self.param_groups[0]
        for p in params:
            state = self._state_of(p)
            state['step'] += 1
            out.append((state, self._scalars(group, float(state['step'].item()))))
            self._fused_done.add(id(p))
            self._grads_clean.add(id(p))     # the fused step leaves the gradient zero
        return out

    def alt_buffer(self, p: torch.Tensor) -> torch.Tensor:
        """The second buffer of a double-buffered parameter (allocated once)."""
        b = self._alt.get(id(p))
        if b is None or b.shape != p.shape or b.device != p.device:
            b = torch.empty_like(p)
            self._alt[id(p)] = b
        return b

    def swap_alt(self, p: torch.Tensor) -> None:
        """``p`` takes the second buffer's storage (just written by an out-of-place update);
        its old storage becomes the second buffer."""
        b = self._alt[id(p)]
        self._alt[id(p)] = p.data
        p.data = b

    def _state_of(self, p: torch.Tensor) -> dict:
        state = self.state[p]
        if len(state) == 0:
            state['step'] = torch.tensor(0.0, dtype=torch.float32)
            state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @staticmethod
    def _scalars(group: dict, step: float) -> tuple:
        """dw_adam_dense's scalars, float64 on the host as torch derives them."""
        beta1, beta2 = group['betas']
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        return (1 - beta1, beta2, 1 - beta2, bias_correction2 ** 0.5,
                -(group['lr'] / bias_correction1), group['eps'], group['weight_decay'])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done, self._fused_done = self._fused_done, set()
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None or id(p) in done:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('HIP Adam does not support sparse gradients')
                if p.dtype != torch.float32 or p.device.type != 'cuda':
                    raise TypeError('HIP Adam needs float32 parameters on a HIP device')
                state = self._state_of(p)
                state['step'] += 1
                scalars = self._scalars(group, float(state['step'].item()))
                g = p.grad
                if not g.is_contiguous():
                    g = g.contiguous()
                    p.grad = g
                with torch.cuda.device(p.device):
                    _native.call('dw_adam_dense', _native.ptr(p), _native.ptr(g),
                                 _native.ptr(state['exp_avg']), _native.ptr(state['exp_avg_sq']),
                                 p.numel(), *scalars, 1 if self.zero_grad_in_step else 0,
                                 _native.stream(p.device))
                self.mark_grads([p], self.zero_grad_in_step)
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """With ``zero_grad_in_step`` the step already left every gradient zero: keep the
        buffers (no extra pass, no reallocation). Otherwise behave like torch."""
        if self.zero_grad_in_step:
            return
        super().zero_grad(set_to_none=set_to_none)


# Rows or dense, per table, from counts alone: with every listed id distinct the rows form
# (dw_sgd_rows) reads and writes p and g of one row per id, at most 16 d bytes an id, against
# 16 d V bytes for the dense pass (dw_sgd_dense with zero_grad) over a V-row table. So below
# ROWS_MAX_IDS_PER_ROW * V ids it can never move more than the dense pass does, apart from the
# id reads (4 or 8 bytes against 16 d); duplicates and rows without a gradient only lower its
# side (a claim, at most one read).
ROWS_MAX_IDS_PER_ROW = 1


def rows_apply(n_ids: int, n_rows: int) -> bool:
    """True when a table of ``n_rows`` rows whose step lists ``n_ids`` ids goes by rows."""
    return n_ids < ROWS_MAX_IDS_PER_ROW * n_rows


class SGD(Optimizer):
    """SGD with the math of ``torch.optim.SGD`` (momentum, dampening, nesterov, L2 weight decay)."""

    def __init__(self, params: Iterable, lr: float = 1e-3, momentum: float = 0,
                 dampening: float = 0, weight_decay: float = 0, nesterov: bool = False, *,
                 zero_grad_in_step: bool = True, **unsupported):
        bad = {k: v for k, v in unsupported.items() if v not in (None, False)}
        if bad:
            raise NotImplementedError(f'HIP SGD does not support {sorted(bad)}')
        if lr < 0.0:
            raise ValueError(f'Invalid learning rate: {lr}')
        if momentum < 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if weight_decay < 0.0:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        # (torch's keys, so a state_dict of this optimizer loads into torch.optim.SGD and back)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, maximize=False, foreach=None, differentiable=False,
                        fused=None)
        super().__init__(params, defaults)
        self.zero_grad_in_step = zero_grad_in_step
        self.force_dense = False   # step_touched always takes the dense pass (timing studies)
        self.last_apply: Dict[torch.Tensor, str] = {}   # parameter -> 'rows' | 'dense'
        self._fused_done = set()   # ids of parameters whose update this step already applied
        self._status: Dict[torch.device, torch.Tensor] = {}

    # ---- touched-rows form --------------------------------------------------------------------
    def can_step_touched(self, params: List[torch.Tensor]) -> bool:
        """True when this optimizer is plain SGD (momentum = weight_decay = 0) over exactly
        ``params`` (one group, HIP fp32 contiguous tensors, gradients zeroed by the step): a row
        without a gradient then stays where it is, and ``step_touched`` is the whole update."""
        if not self.zero_grad_in_step or len(self.param_groups) != 1:
            return False
        group = self.param_groups[0]
        mine = group['params']
        if group['momentum'] != 0 or group['weight_decay'] != 0 or group['maximize']:
            return False
        if len(mine) != len(params) or {id(p) for p in mine} != {id(p) for p in params}:
            return False
        return all(p.device.type == 'cuda' and p.dtype == torch.float32 and p.is_contiguous()
                   and p.dim() == 2 and p.grad is not None and p.grad.is_contiguous()
                   for p in params)

    def status(self, device: torch.device) -> torch.Tensor:
        """The device status word of the rows steps on ``device`` (``check_status``)."""
        st = self._status.get(device)
        if st is None:
            st = self._status[device] = torch.zeros(1, dtype=torch.int32, device=device)
        return st

    def check_status(self) -> None:
        """Synchronising: raise if a rows step met an id outside its table."""
        for st in self._status.values():
            _native.check_status(st, 'SGD touched-rows step')

    @torch.no_grad()
    def step_rows(self, p: torch.Tensor, ids: Union[torch.Tensor, Sequence[torch.Tensor]],
                  claim: torch.Tensor) -> None:
        """Plain SGD on the rows of ``p`` listed in ``ids`` (one int32 / int64 device tensor or
        several; duplicates apply once), gradients of those rows left zero; the ``step()`` that
        follows skips ``p`` once. ``claim``: int32 [ceil(V / 32)] zeros, left zero."""
        group = self._group_of(p)
        if group['momentum'] != 0 or group['weight_decay'] != 0:
            raise ValueError('step_rows is exact only for momentum == weight_decay == 0')
        V, d = p.shape
        if claim.dtype != torch.int32 or claim.numel() < (V + 31) // 32:
            raise ValueError('claim must be int32 [ceil(V / 32)]')
        nlr = -float(group['lr'])
        with torch.cuda.device(p.device):
            s = _native.stream(p.device)
            for t in ([ids] if isinstance(ids, torch.Tensor) else ids):
                if t.dtype not in (torch.int32, torch.int64):
                    raise TypeError('row ids must be int32 or int64')
                # (a second list sees the first one's rows with g = 0: nothing moves twice)
                _native.call('dw_sgd_rows', _native.ptr(p), _native.ptr(p.grad), V, d,
                             _native.ptr(t), t.element_size(), t.numel(), _native.ptr(claim), nlr,
                             _native.ptr(self.status(p.device)), s)
        self.last_apply[p] = 'rows'
        self._fused_done.add(id(p))

    @torch.no_grad()
    def step_touched(self, p: torch.Tensor, ids: Sequence[torch.Tensor],
                     claim: torch.Tensor) -> None:
        """This step's update of ``p``, whose gradient is zero outside the rows in ``ids``: by
        rows or by the dense pass, whichever ``rows_apply`` says moves fewer bytes."""
        if not self.force_dense and rows_apply(sum(t.numel() for t in ids), p.shape[0]):
            self.step_rows(p, ids, claim)
            return
        self._dense(p, self._group_of(p))
        self._fused_done.add(id(p))

    def _group_of(self, p: torch.Tensor) -> dict:
        for group in self.param_groups:
            if any(q is p for q in group['params']):
                return group
        raise ValueError('not a parameter of this optimizer')

    def _dense(self, p: torch.Tensor, group: dict) -> None:
        if p.grad.is_sparse:
            raise RuntimeError('HIP SGD does not support sparse gradients')
        if p.dtype != torch.float32 or p.device.type != 'cuda':
            raise TypeError('HIP SGD needs float32 parameters on a HIP device')
        if not p.is_contiguous():
            raise ValueError('HIP SGD needs contiguous parameters')
        g = p.grad
        if not g.is_contiguous():
            g = g.contiguous()
            p.grad = g
        mu = float(group['momentum'])
        buf, first = None, False
        if mu != 0:
            state = self.state[p]
            buf = state.get('momentum_buffer')
            if buf is None:   # torch: the first step's buffer is the gradient (no dampening)
                first = True
                buf = state['momentum_buffer'] = torch.empty_like(
                    p, memory_format=torch.contiguous_format)
        with torch.cuda.device(p.device):
            _native.call('dw_sgd_dense', _native.ptr(p), _native.ptr(g), _native.ptr(buf),
                         p.numel(), -float(group['lr']), float(group['weight_decay']), mu,
                         1.0 - float(group['dampening']), 1 if group['nesterov'] else 0,
                         1 if first else 0, 1 if self.zero_grad_in_step else 0,
                         _native.stream(p.device))
        self.last_apply[p] = 'dense'

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done, self._fused_done = self._fused_done, set()
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None or id(p) in done:
                    continue
                self._dense(p, group)
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """With ``zero_grad_in_step`` the step already left every gradient zero: keep the
        buffers (no extra pass, no reallocation). Otherwise behave like torch."""
        if self.zero_grad_in_step:
            return
        super().zero_grad(set_to_none=set_to_none)
