"""Word2VecTrainer (reference: word2vec/trainer.py:18-165) on the fused gfx950 SGNS kernel.

Keeps the reference surface — ``Word2VecTrainer(model, optimizer, scheduler, neg_samples,
vocab_size)``, ``.model/.optimizer/.scheduler``, ``training_step(batch) -> loss dict``,
``on_train_epoch_end``, ``configure_optimizers() -> ([opt], [sched])`` and the logged metric
names (``train/loss``, ``train/positive-loss``, ``train/negative-loss``, ``epoch/lr``,
``train-epoch/*``, ``train-metrics/recall``, ``train-metrics/precision``).

``training_step`` accepts either batch format:
  * ``(inputs, targets)`` from W2VCollateFunctional (the reference's format), or
  * a device int32 walk tensor [n_walks, L] (GraphDataset.walk_batches): windows are formed
    inside the kernel, nothing is materialised on the host.

Gradient delivery:
  * ``manual_grads = True`` (the in-repo loop, tools/train.py, bench.py): the kernel adds the
    gradient of the batch-mean loss straight into ``param.grad``; the HIP Adam step consumes
    and zeroes it. No autograd graph, no host synchronisation per step.
  * ``manual_grads = False`` (default; a Lightning-style loop calling ``loss.backward()``):
    the returned ``loss`` carries a grad_fn whose backward hands over the same gradients.

Fused step (``manual_grads`` + walk batches + the HIP Adam holding exactly the two tables, one
device, records path): ``training_step`` also applies the optimizer update, the way bench.py's
step does. The three pieces run as follows:
  * SGNS pass 1 runs first, after which the input-table gradient is final.
  * The input table's Adam then runs on a side stream, out of place into the table's second
    buffer, overlapping the output-table phase, which still reads the current input table.
  * The output table's Adam is fused into that phase's records gather
    (dw_sgns_walks_phase2_adam).
The optimizer's ``step()`` that follows is then a no-op for the two tables (Adam.begin_fused_step).
Same update as SGNS + ``optimizer.step()`` up to float-atomic summation order
(test_gpu_trainer.py::test_fused_trainer_step_equals_unfused).

SGD touched-rows step (``manual_grads`` + walk batches + the HIP SGD holding exactly the two
tables with momentum = weight_decay = 0): the SGNS kernels accumulate the gradient as in the
unfused step, then ``training_step`` steps the rows the batch lists and nothing else
(_sgd_walk_step; exact, since plain SGD leaves a row without a gradient where it is), or the
whole table where the batch lists at least as many ids as the table has rows. The optimizer's
``step()`` that follows skips the two tables. Refuses the deterministic mode.

Noise: ``noise='torch'`` draws the reference's uniform negatives with torch's global CPU
generator (generate_noise_batch, exact under ``torch.manual_seed``); ``noise='device'`` draws
the same law on the device (Philox keyed by ``seed`` and the running centre counter).
``noise='unigram'`` (a documented departure from the reference's uniform law: what word2vec.c,
gensim and the node2vec reference code draw) draws negatives in proportion to
``noise_weights ** noise_power`` (0.75) on the device, from an alias table over the vocabulary
built once (sgns.unigram_table), with the same Philox keys; an id of weight 0 is never drawn.

Shared negatives (``shared_negatives=S`` > 0; off by default, a documented departure from the
reference): the L - 2R centres of a walk share S negatives drawn once per
walk under the chosen law ('device' or 'unigram'), each weighted 2R K / S so the loss keeps its
expectation and scale. A device walk batch then runs one MFMA kernel (dw_sgns_walks_shared: no
per-pair gathers, no records, no sort) into ``param.grad`` and the optimizer's ordinary dense
``step()`` applies the update. Needs ``manual_grads``; refuses ``noise='torch'`` and
``max_norm`` (constructor), the deterministic mode, pairs / CBOW batches and shapes outside the
kernel's limits (first step). Graph replay does not cover it (GraphedTrainerStep.eligible).

Deviation (documented): per-step loss values stay on the device; the reference's per-step
``.detach().cpu()`` NaN assert (trainer.py:116,121) runs once per epoch instead.
"""
from typing import Dict, List, Union

import torch
from torch.optim import Optimizer

from shallow_encoders import _native
from shallow_encoders.word2vec import exact
from shallow_encoders.word2vec.model import W2VBase
from shallow_encoders.word2vec.sgns import (SGNSLoss, _use_records, device_noise, loss_terms,
                                            renorm_, sgns_accumulate, sgns_phase_bytes,
                                            sgns_shared_accumulate, shared_shape_error,
                                            unigram_noise, unigram_table_host)
from shallow_encoders.word2vec.utils import torch_helper
from shallow_encoders.word2vec.utils.meter import MetricMeter
from shallow_encoders.word2vec.utils.sampling import generate_noise_batch

try:  # keep Lightning compatibility when it is installed (it is not in this image)
    import pytorch_lightning as _pl
    _Base = _pl.LightningModule
    _HAS_PL = True
except ImportError:  # pragma: no cover - depends on the environment
    _Base = torch.nn.Module
    _HAS_PL = False


class Word2VecTrainer(_Base):
    """Trains a W2V model with the fused SGNS kernel."""

    def __init__(self, model: W2VBase, optimizer: Optimizer, scheduler, neg_samples: int,
                 vocab_size: int, noise: str = 'torch', seed: int = 0, context_radius: int = None,
                 noise_weights: torch.Tensor = None, noise_power: float = 0.75,
                 shared_negatives: int = 0):
        super().__init__()
        if noise not in ('torch', 'device', 'unigram'):
            raise ValueError('noise must be "torch", "device" or "unigram"')
        self._shared = int(shared_negatives)
        if self._shared < 0:
            raise ValueError('shared_negatives must be >= 0 (0: off)')
        if self._shared > 0:
            if noise == 'torch':
                raise ValueError('shared_negatives draws one block of ids per walk: the '
                                 'reference\'s noise="torch" stream (one draw per pair) has no '
                                 'meaning there; use noise="device" or "unigram"')
            if getattr(model, 'max_norm', None) is not None:
                raise ValueError('shared_negatives does not support max_norm')
        # noise='unigram': the alias table over the vocabulary, built here on the host (native
        # code, no device needed) and moved to the tables' device by the first step
        self._noise_table_host = self._noise_table = None
        self._noise_bufs: Dict[tuple, torch.Tensor] = {}
        if noise == 'unigram':
            if noise_weights is None:
                raise ValueError('noise="unigram" needs noise_weights: one non-negative weight '
                                 'per vocabulary id (counts or degrees; id 0 is <unk>)')
            noise_weights = torch.as_tensor(noise_weights)
            if noise_weights.dim() != 1 or noise_weights.numel() != vocab_size:
                raise ValueError(f'noise_weights must have vocab_size = {vocab_size} entries, got '
                                 f'shape {tuple(noise_weights.shape)}')
            self._noise_table_host = unigram_table_host(noise_weights, noise_power)
        elif noise_weights is not None:
            raise ValueError('noise_weights is only used by noise="unigram"')
        self._optimizer = optimizer
        self._scheduler = scheduler
        self._neg_samples = neg_samples
        self._vocab_size = vocab_size
        self._model = model
        self._meter = MetricMeter()
        self._noise_mode = noise
        self._seed = int(seed)
        self._noise_offset = 0
        self._context_radius = context_radius
        self.manual_grads = False
        self.logged: Dict[str, object] = {}
        self._side = None          # side stream of the fused step (input-table Adam)
        self._row_flags = None     # fused output-table Adam scratch
        self._sgd_claim = None     # claim bitmap of the SGD touched-rows step (both tables)
        # set while word2vec/graphed.py GraphedTrainerStep captures the step: the steps add
        # their loss sums here and skip the per-step metrics (read once per replay), and
        # _capture_scatter = 'atomic' takes the atomic output-table scatter (tiny batches)
        self._capture_acc = None
        self._capture_scatter = None
        # set by GraphedTrainerStep for noise='torch': the step's negatives, already drawn on the
        # device from torch's generator stream (graph/rng.py DeviceMT.randint)
        self._noise_override = None
        # the deterministic mode's accumulators (word2vec/exact.py; DW_DETERMINISTIC=1)
        self._exact = None

    # ---- reference properties -------------------------------------------------------------
    @property
    def model(self) -> W2VBase:
        return self._model

    @property
    def optimizer(self) -> Optimizer:
        return self._optimizer

    @optimizer.setter
    def optimizer(self, optimizer: Optimizer) -> None:
        self._optimizer = optimizer

    @property
    def scheduler(self):
        return self._scheduler

    @scheduler.setter
    def scheduler(self, scheduler) -> None:
        self._scheduler = scheduler

    @property
    def meter(self) -> MetricMeter:
        return self._meter

    # ---- logging ------------------------------------------------------------------------------
    def log(self, name: str, value, prog_bar: bool = False, **kwargs) -> None:  # noqa: D401
        if _HAS_PL and getattr(self, '_trainer', None) is not None:
            return super().log(name, value, prog_bar=prog_bar, **kwargs)
        self.logged[name] = value
        return None

    def _log_loss(self, loss: Dict[str, torch.Tensor], prefix: str, log_step: bool = True) -> None:
        assert prefix in ['train', 'val'], f'Invalid prefix value "{prefix}"!'
        assert 'loss' in loss, \
            f'When returning loss as dictionary it has to have key "loss". Found: {list(loss.keys())}'
        for name, value in loss.items():
            value = value.detach()
            self._meter.push(f'{prefix}-epoch/{name}', value)
            if log_step:
                self.log(f'{prefix}/{name}', value, prog_bar=False)

    def forward(self, inputs: torch.Tensor, outputs: torch.Tensor, proba: bool = True) -> torch.Tensor:
        return self._model(inputs, outputs, proba=proba)

    # ---- training -----------------------------------------------------------------------------
    def _status(self, device) -> torch.Tensor:
        st = getattr(self, '_renorm_status', None)
        if st is None or st.device != device:
            st = torch.zeros(1, dtype=torch.int32, device=device)
            self._renorm_status = st
        return st

    def _noise(self, n_centres: int, n_ctx: int, device) -> Union[torch.Tensor, None]:
        if self._noise_mode == 'device':
            return None
        if self._noise_override is not None:
            return self._noise_override
        if self._noise_mode == 'unigram':
            return self._unigram_noise(n_centres, n_ctx, torch.device(device))
        noise = generate_noise_batch(n_centres, n_ctx, self._neg_samples, self._vocab_size)
        return noise.to(device, non_blocking=True)

    # at most this many step shapes keep their negatives' buffer (text batches vary in size)
    NOISE_BUFFERS = 8

    def _unigram_noise(self, n_centres: int, n_ctx: int, dev: torch.device) -> torch.Tensor:
        """This step's negatives (the centre counter is not yet advanced) in the persistent
        buffer of its shape: a captured step allocates nothing, and its replays fill the buffer
        they were captured with (GraphedTrainerStep holds on to it)."""
        if self._noise_table is None or self._noise_table.device != dev:
            self._noise_table = self._noise_table_host.to(dev)
            self._noise_bufs.clear()
        key = (n_centres, n_ctx)
        buf = self._noise_bufs.pop(key, None)
        if buf is None:
            buf = torch.empty((n_centres, n_ctx, self._neg_samples), dtype=torch.int64, device=dev)
            while len(self._noise_bufs) >= self.NOISE_BUFFERS:   # the least recently used
                self._noise_bufs.pop(next(iter(self._noise_bufs)))
        self._noise_bufs[key] = buf
        return unigram_noise(n_centres, n_ctx, self._neg_samples, self._noise_table, self._seed,
                             self._noise_offset, dev, out=buf)

    def _shared_ids(self, n_walks: int, offset: int, dev: torch.device) -> torch.Tensor:
        """int64 [n_walks, 1, S]: the step's shared negatives, walk w's from the Philox centre
        counter ``offset + w`` under the trainer's noise law, in the persistent buffer of the
        shape (as _unigram_noise keeps its buffers)."""
        S = self._shared
        if self._noise_mode == 'unigram' and (self._noise_table is None
                                              or self._noise_table.device != dev):
            self._noise_table = self._noise_table_host.to(dev)
            self._noise_bufs.clear()
        key = ('shared', n_walks, S)
        buf = self._noise_bufs.pop(key, None)
        if buf is None or buf.device != dev:
            buf = torch.empty((n_walks, 1, S), dtype=torch.int64, device=dev)
            while len(self._noise_bufs) >= self.NOISE_BUFFERS:   # the least recently used
                self._noise_bufs.pop(next(iter(self._noise_bufs)))
        self._noise_bufs[key] = buf
        if self._noise_mode == 'unigram':
            return unigram_noise(n_walks, 1, S, self._noise_table, self._seed, offset, dev,
                                 out=buf)
        return device_noise(n_walks, 1, S, self._vocab_size, self._seed, offset, dev, out=buf)

    def _shared_step(self, batch, w_in, w_out) -> Dict[str, torch.Tensor]:
        """The shared-negatives step (module docstring): ids for the batch's walks, then
        dw_sgns_walks_shared into the two gradient buffers; the update is the optimizer's."""
        from shallow_encoders.word2vec.optim import Adam
        if not isinstance(batch, torch.Tensor):
            raise ValueError('shared_negatives takes device walk batches [n_walks, L], not '
                             '(inputs, targets) pairs / CBOW batches')
        if exact.enabled():
            raise ValueError('shared_negatives has no deterministic mode (float atomics)')
        if not self.manual_grads:
            raise ValueError('shared_negatives needs manual_grads = True (the kernel adds into '
                             'param.grad; there is no autograd form)')
        R = self._context_radius
        if R is None:
            raise ValueError('walk batches need context_radius (set it on the trainer)')
        dev = w_in.device
        walks = batch if batch.dtype == torch.int32 else batch.to(torch.int32)
        walks = walks.to(dev).contiguous()
        n, L = walks.shape
        bad = shared_shape_error(L, R, self._shared, w_in.shape[1], w_in.shape[0])
        if bad is not None:
            raise ValueError(f'shared_negatives: {bad}')
        n_centres, C = n * (L - 2 * R), 2 * R
        offset = self._noise_offset
        ids = self._shared_ids(n, offset, dev)
        self._noise_offset += n_centres
        fresh = [p for p in (w_in, w_out) if p.grad is None]
        for p in fresh:
            p.grad = torch.zeros_like(p)
        acc = sgns_shared_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad,
                                     self._neg_samples, walks=walks, context_radius=R,
                                     shared_ids=ids)
        if isinstance(self._optimizer, Adam):
            self._optimizer.mark_grads([w_in, w_out], False)   # accumulated, not consumed
        t = loss_terms(acc, n_centres * C, self._neg_samples)
        loss = {k: t[k] for k in ('loss', 'positive-loss', 'negative-loss')}
        self._log_loss(loss, prefix='train', log_step=True)
        self.log('epoch/lr', torch_helper.get_optim_lr(self.optimizer))
        self._meter.push('train-metrics/recall', t['recall'])
        self._meter.push('train-metrics/precision', t['precision'])
        return loss

    def training_step(self, batch, *args, **kwargs) -> Dict[str, torch.Tensor]:
        w_in = self._model.input_weight
        w_out = self._model.output_weight
        dev = w_in.device
        if self._shared:
            return self._shared_step(batch, w_in, w_out)
        if isinstance(batch, torch.Tensor):           # device walks [n, L]
            R = self._context_radius
            if R is None:
                raise ValueError('walk batches need context_radius (set it on the trainer)')
            walks = batch if batch.dtype == torch.int32 else batch.to(torch.int32)
            walks = walks.to(dev).contiguous()
            n, L = walks.shape
            n_centres, C = n * (L - 2 * R), 2 * R
            src, targets = walks, None
        else:                                         # (inputs, targets) from the collate fn
            inputs, targets = batch                   # sg: (B, 1), (B, 2R); cbow: (B, 2R), (B, 1)
            targets = targets.to(dev, torch.long).contiguous()
            n_centres, C = targets.shape
            src = inputs.to(dev, torch.long).reshape(n_centres, -1).contiguous()
            if src.shape[1] == 1:
                src = src.reshape(-1)
            R = C // 2
        noise = self._noise(n_centres, C, dev)
        offset = self._noise_offset
        self._noise_offset += n_centres
        max_norm = self._model.max_norm
        if max_norm is not None:
            # nn.Embedding(max_norm) renormalises every row the reference's two forwards look
            # up (inputs in the in table; targets and negatives in the out table) before the
            # loss: materialise the device negatives, renormalise, then run the fused step
            if targets is None:
                raise NotImplementedError('max_norm with device walk batches: use the collate '
                                          '(pairs) dataloader')
            if noise is None:
                noise = device_noise(n_centres, C, self._neg_samples, self._vocab_size,
                                     self._seed, offset, dev)
            st = self._status(dev)
            renorm_(w_in, src, max_norm, st)
            renorm_(w_out, targets, max_norm, st)
            renorm_(w_out, noise, max_norm, st)
        if self.manual_grads:
            from shallow_encoders.word2vec.optim import Adam
            fresh = [p for p in (w_in, w_out) if p.grad is None]
            for p in fresh:
                p.grad = torch.zeros_like(p)
            if isinstance(self._optimizer, Adam):
                self._optimizer.mark_grads(fresh, True)
            sgd_touched = targets is None and self._capture_acc is None and \
                self._can_sgd_touched(w_in, w_out)
            if sgd_touched and exact.enabled():
                raise NotImplementedError(
                    'the SGD touched-rows step has no deterministic mode (DW_DETERMINISTIC=1): '
                    'it steps the float gradient buffers, which the fixed-point accumulators '
                    'replace; use the HIP Adam, or SGD with momentum or weight decay')
            if exact.enabled():   # int64 fixed-point accumulators for the two gradient buffers
                if self._exact is None:
                    self._exact = exact.Registry()
                scale = 1.0 / max(n_centres * C, 1)
                self._exact.ensure(0, w_in.grad, scale)
                self._exact.ensure(1, w_out.grad, scale)
            elif self._exact is not None:
                self._exact.release()
                self._exact = None
            if targets is None and self._capture_scatter != 'atomic' and \
                    self._can_fuse_step(w_in, w_out, C):
                acc = self._fused_walk_step(w_in, w_out, src, R, noise, offset)
            elif sgd_touched:
                acc = self._sgd_walk_step(w_in, w_out, src, R, noise, offset)
            elif targets is None:
                acc = sgns_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad,
                                      self._neg_samples, walks=src, context_radius=R, noise=noise,
                                      seed=self._seed, noise_offset=offset,
                                      loss_acc=self._capture_acc,
                                      scatter=self._capture_scatter or 'sorted')
            else:
                acc = sgns_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad,
                                      self._neg_samples, inputs=src, targets=targets, noise=noise,
                                      seed=self._seed, noise_offset=offset)
            if isinstance(self._optimizer, Adam) and not self._optimizer._fused_done:
                self._optimizer.mark_grads([w_in, w_out], False)   # accumulated, not consumed
            if self._capture_acc is not None:   # a captured step: metrics once per replay
                return None
            t = loss_terms(acc, n_centres * C, self._neg_samples)
            loss = {k: t[k] for k in ('loss', 'positive-loss', 'negative-loss')}
            recall, precision = t['recall'], t['precision']
        else:
            outs = SGNSLoss.apply(w_in, w_out, src, targets, noise, R, self._neg_samples,
                                  self._seed, offset)
            loss = {'loss': outs[0], 'positive-loss': outs[1], 'negative-loss': outs[2]}
            recall, precision = outs[3], outs[4]
        self._log_loss(loss, prefix='train', log_step=True)
        self.log('epoch/lr', torch_helper.get_optim_lr(self.optimizer))
        self._meter.push('train-metrics/recall', recall)
        self._meter.push('train-metrics/precision', precision)
        return loss

    # ---- fused step -----------------------------------------------------------------------------
    def _can_fuse_step(self, w_in, w_out, n_ctx: int) -> bool:
        from shallow_encoders.word2vec.optim import Adam
        opt = self._optimizer
        return (isinstance(opt, Adam) and w_in.device.type == 'cuda'
                and _use_records('sorted', n_ctx, self._neg_samples, w_in.shape[0])
                and opt.can_fuse([w_in, w_out]))

    def _fused_walk_step(self, w_in, w_out, walks, R: int, noise, offset: int) -> torch.Tensor:
        """Pass 1 -> input-table Adam on the side stream (into the second buffer) || output-table
        phase with its Adam fused -> join -> swap the input table's buffers."""
        from shallow_encoders.word2vec.sharding import adam_to_scalars, overlap_adam_blocks
        opt = self._optimizer
        (st_in, sc_in), (st_out, sc_out) = opt.begin_fused_step([w_in, w_out])
        dev = w_in.device
        K = self._neg_samples
        V, d = w_in.shape
        n, L = walks.shape
        kw = dict(walks=walks, context_radius=R, noise=noise, seed=self._seed,
                  noise_offset=offset)
        acc = sgns_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad, K,
                              phase=1, loss_acc=self._capture_acc, **kw)
        if self._side is None or self._side.device != dev:
            self._side = torch.cuda.Stream(dev)
        if self._row_flags is None or self._row_flags.numel() != V or \
                self._row_flags.device != dev:
            self._row_flags = torch.zeros(V, dtype=torch.uint8, device=dev)
        alt = opt.alt_buffer(w_in)
        main = torch.cuda.current_stream(dev)
        ready = torch.cuda.Event()
        ready.record(main)
        pb = sgns_phase_bytes(n, L, R, K, d, V, 'sorted', True)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            adam_to_scalars(w_in.detach(), alt, w_in.grad, st_in['exp_avg'],
                            st_in['exp_avg_sq'], sc_in, True,
                            overlap_adam_blocks(V * d * 4 * 7, pb['sort'] + pb['pass2']))
            done = torch.cuda.Event()
            done.record(self._side)
        sgns_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad, K, phase=2,
                        loss_acc=acc,
                        out_adam={'m': st_out['exp_avg'], 'v': st_out['exp_avg_sq'],
                                  'flags': self._row_flags, 'scalars': sc_out}, **kw)
        main.wait_event(done)
        opt.swap_alt(w_in)
        return acc

    # ---- SGD touched-rows step ------------------------------------------------------------------
    def _can_sgd_touched(self, w_in, w_out) -> bool:
        from shallow_encoders.word2vec.optim import SGD
        opt = self._optimizer
        return (isinstance(opt, SGD) and w_in.device.type == 'cuda'
                and w_in.shape[0] < 2 ** 31 and opt.can_step_touched([w_in, w_out]))

    def _sgd_buffer(self, key: tuple, shape: tuple, dtype, dev: torch.device) -> torch.Tensor:
        """A persistent id buffer of the SGD step, as _unigram_noise keeps its negatives:
        allocated on the first step of a shape."""
        buf = self._noise_bufs.pop(key, None)
        if buf is None or buf.device != dev:
            buf = torch.empty(shape, dtype=dtype, device=dev)
            while len(self._noise_bufs) >= self.NOISE_BUFFERS:   # the least recently used
                self._noise_bufs.pop(next(iter(self._noise_bufs)))
        self._noise_bufs[key] = buf
        return buf

    def _sgd_walk_step(self, w_in, w_out, walks, R: int, noise, offset: int) -> torch.Tensor:
        """Plain SGD (module docstring of word2vec/optim.py): the gradient by the unchanged SGNS
        kernels, then the update of the rows the batch lists — the centre columns for the input
        table, every walk node and every negative for the output table (a superset of the rows
        with a gradient: a window's targets are walk nodes). The optimizer picks rows or dense
        per table from the id counts (optim.rows_apply); its ``step()`` then skips both tables.
        Both updates run on the step's stream, one after the other: at C3's 64-walk shape the two
        take 0.18 ms together, and no side-stream form was measured."""
        opt = self._optimizer
        dev = w_in.device
        K = self._neg_samples
        V = w_in.shape[0]
        n, L = walks.shape
        n_centres, C = n * (L - 2 * R), 2 * R
        if noise is None:   # noise='device': the ids the kernels would draw, materialised once
            noise = device_noise(n_centres, C, K, self._vocab_size, self._seed, offset, dev,
                                 out=self._sgd_buffer(('sgd-noise', n_centres, C),
                                                      (n_centres, C, K), torch.int64, dev))
        acc = sgns_accumulate(w_in.detach(), w_out.detach(), w_in.grad, w_out.grad, K,
                              walks=walks, context_radius=R, noise=noise, seed=self._seed,
                              noise_offset=offset)
        centres = self._sgd_buffer(('sgd-centres', n, L - 2 * R), (n, L - 2 * R), torch.int32,
                                   dev)
        centres.copy_(walks[:, R:L - R])
        words = (V + 31) // 32
        if self._sgd_claim is None or self._sgd_claim.numel() != words or \
                self._sgd_claim.device != dev:   # the claim bitmap: zero between rows steps
            self._sgd_claim = torch.zeros(words, dtype=torch.int32, device=dev)
        opt.step_touched(w_in, [centres], self._sgd_claim)
        opt.step_touched(w_out, [walks, noise.contiguous()], self._sgd_claim)
        return acc

    def push_replayed(self, terms: Dict[str, torch.Tensor], n_steps: int) -> Dict[str, torch.Tensor]:
        """The metrics of ``n_steps`` graph-replayed steps (word2vec/graphed.py
        GraphedTrainerStep): their mean loss terms stand for each of the steps in the epoch
        means, as training_step's per-step pushes would; returns the loss dict."""
        loss = {k: terms[k] for k in ('loss', 'positive-loss', 'negative-loss')}
        for _ in range(n_steps):
            self._log_loss(loss, prefix='train', log_step=False)
            self._meter.push('train-metrics/recall', terms['recall'])
            self._meter.push('train-metrics/precision', terms['precision'])
        for name, value in loss.items():
            self.log(f'train/{name}', value)
        self.log('epoch/lr', torch_helper.get_optim_lr(self.optimizer))
        return loss

    def on_train_epoch_end(self) -> Dict[str, float]:
        """Log the epoch means; one host synchronisation per epoch (NaN check included)."""
        st = getattr(self, '_renorm_status', None)
        if st is not None:
            _native.check_status(st, 'max_norm renormalisation')
        if hasattr(self._optimizer, 'check_status'):   # the HIP SGD's rows steps
            self._optimizer.check_status()
        if self._meter.is_empty:
            return {}
        out = {}
        for name, value in self._meter.get_all():
            v = float(value)
            assert v == v, f'Got nan value for key "{name}"!'
            out[name] = v
            self.log(name, v, prog_bar=name.endswith('/loss'))
        return out

    def configure_optimizers(self):
        return [self._optimizer], [self._scheduler]
