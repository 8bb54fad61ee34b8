"""WaveNet model: host-side mirror of src/model.py::WaveNet over the gfx950 HIP library.

Same constructor keywords, method names, argument meaning, tensor layouts
(channels-last ``(B, T, C)`` fp32) and exception types as the reference class; everything
underneath is ``libwn_hip.so`` (no TensorFlow, no CPU fallback).  PyTorch is used only for
device memory, streams and ``torch.distributed`` (RCCL).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import math
from typing import List, Optional

import numpy as np
import torch

from . import _guard, _lib, dp, generation
from . import spec as _spec
from .autograd import _NetFn
from .generation import GenerationSession, _RowControls      # (these two and MeanSquaredError: for those who import them
from .layers import WaveNetLayer                             # from this module)
from .metrics import MeanSquaredError, _Mean
from .optim import Adam


class _ConvHandle:
  """Read-only handle on one conv / dense of the flat parameter buffer (``.kernel``/``.bias``)."""

  def __init__(self, model, name):
    self._model, self._name = model, name

  @property
  def kernel(self):
    return self._model._tensor(self._name + '/kernel')

  @property
  def bias(self):
    return self._model._tensor(self._name + '/bias')

  @property
  def weights(self):
    return [self.kernel, self.bias]


def _disarms_frames(fn):
  """Local conditioning: ``_split_inputs`` arms the condition's frames for the call; whatever happens, the call ends with
  the plan disarmed, so that a pass without frames (generation, a globally conditioned model) never sees them."""
  @functools.wraps(fn)
  def wrapper(self, *args, **kwargs):
    try:
      return fn(self, *args, **kwargs)
    finally:
      self._arm_frames(0)
  return wrapper


class WaveNet(generation._Generation, torch.nn.Module):
  """WaveNet model class (src/model.py:11-556)."""
  _TAIL_METRICS = 5      # device-reduced metric slots behind {loss, reg_loss, range_flag} in the gradient bucket

  def __init__(self,
               kernel_size: int = 2,
               channels: int = 32,
               blocks: int = 10,
               layers_per_block: int = 1,
               activation=None,
               conditioning=None,
               mapping_layers=None,
               mapping_activation=None,
               dropout: float = 0,
               dilation_bound: int = 512,
               num_mixtures=None,
               sampling_function: str = 'categorical',
               bits=8,
               skip_channels=None,
               dilation_channels=None,
               use_residual=True,
               use_skip=True,
               final_layers_channels=None,
               l2_reg_factor: float = 0,
               device=None,
               seed: int = 0):
    super().__init__()
    s = _spec.validate(kernel_size, channels, blocks, layers_per_block, activation, conditioning,
                       mapping_layers, mapping_activation, dropout, dilation_bound, num_mixtures,
                       sampling_function, bits, skip_channels, dilation_channels, use_residual,
                       use_skip, final_layers_channels, l2_reg_factor)
    self.spec = s
    self.regularization = s.l2_reg_factor > 0
    self.num_mixtures = num_mixtures
    self.use_skip = use_skip
    self.sampling_function = sampling_function
    self.bits = bits
    self.conditioning = conditioning
    self.dropout = s.dropout
    self.receptive_field = s.receptive_field            # src/model.py:122
    self._device = torch.device(device) if device is not None else torch.device('cuda', 0)
    self._seed = seed
    self._plan = None
    self._cond_inputs = None
    self._names: List[str] = []
    self._ws = {}
    self.built = False
    self.optimizer = None
    self._averaged = None                 # inside averaged_weights(): the raw weights' storage, swapped out of flat_params
    self._metrics_from_compilation = []
    self.loss_tracker = _Mean('loss')
    self.reg_loss = _Mean('reg_loss') if self.regularization else None
    self._sample_calls = 0
    # steps / evaluation passes / generate calls that left the range of the split-precision kernels and were repeated
    # in exact fp32 (each costs a second, slower pass; train.py logs them per epoch)
    self.train_guard_trips = 0
    self.test_guard_trips = 0
    self.score_guard_trips = 0
    self.generation_guard_trips = 0
    # None = automatic: a single replica reads its step scalars back between forward and backward; data-parallel replicas
    # take them from the gradient bucket's tail after the ONE all-reduce of the step (no second collective per step)
    self.early_logs = None
    # call() / logits() read the forward range guard back after every pass (one blocking device-to-host copy) and repeat
    # the pass in exact fp32 when it tripped.  False skips the read -- for latency-critical inference on weights known to
    # stay in range; range_tripped_last_forward() checks the same slot later.
    self.range_check = True
    self._last_fwd = None
    self._log_mirror, self._log_event = None, None
    self._drop_step = 0                   # training calls made so far (dropout mask counter; saved by io.save_weights)
    self._fused_step_sample = True        # train_step draws its metric sample inside the library
    self._drop_armed_step = 0             # the mask counter last handed to the library
    # generation stamp of the 'train' workspace: every pass that writes it bumps the stamp, and the backward of a
    # differentiable() graph refuses to run on activations that are no longer its own
    self._train_gen = 0
    self._vjp_anchor = None
    # structure handles (attribute names of the reference)
    dil = s.dilations
    lpb = s.layers_per_block
    self.causal = _ConvHandle(self, 'causal')
    self.wavenet_blocks = [
        WaveNetLayer(kernel=s.kernel_size, channels=s.channels,
                     dilation_rate=dil[b * lpb:(b + 1) * lpb], activation=s.activation,
                     dilation_channels=s.dilation_channels, residual=s.use_residual,
                     skip_channels=s.skip_channels, l2_reg_factor=s.l2_reg_factor, dropout=s.dropout,
                     condition=conditioning is not None, _owner=(self, b))
        for b in range(s.blocks)]
    self.final = [_ConvHandle(self, f'final{i}') for i in range(len(s.final_layers_channels) + 1)]
    self.mapping = [_ConvHandle(self, f'mapping{j}') for j in range(len(s.mapping_layers))] \
        if conditioning is not None else None
    self._frames_armed = 0                # condition frames armed in the plan (local conditioning, per call)
    self._last_frames = None              # F of the last training-form call (kernel_report)
    self._last_train_frames = 0           # F of the last pass that wrote the training workspace (training_intermediate)
    if conditioning is None:
      self.build(None)

  # ------------------------------------------------------------------ build
  def build(self, input_shape):
    """Create the plan and the parameters (src/model.py:171-211).  With conditioning the
    condition width is only known from the first input, as in Keras."""
    if self.built:
      return
    s = self.spec
    cond_inputs = 0
    if self.conditioning is not None:
      cond_inputs = int(input_shape[1][-1])
    self._cond_inputs = cond_inputs
    cfg = _lib.WnConfig()
    cfg.kernel_size, cfg.channels, cfg.blocks = s.kernel_size, s.channels, s.blocks
    cfg.layers_per_block = s.layers_per_block
    cfg.activation = _lib.ACTIVATIONS[s.activation]
    cfg.dilation_bound = s.dilation_bound
    cfg.num_mixtures = s.num_mixtures or 0
    cfg.head = _lib.HEADS[s.sampling_function]
    cfg.bits = s.bits
    cfg.skip_channels = s.skip_channels or 0
    cfg.dilation_channels = s.dilation_channels or 0
    cfg.use_residual, cfg.use_skip = int(s.use_residual), int(s.use_skip)
    if len(s.final_layers_channels) > _lib.WN_MAX_FINAL or len(s.mapping_layers) > _lib.WN_MAX_MAPPING:
      raise NotImplementedError('too many final / mapping layers')
    cfg.n_final = len(s.final_layers_channels)
    for i, c in enumerate(s.final_layers_channels):
      cfg.final_channels[i] = c
    cfg.cond_inputs = cond_inputs
    cfg.n_mapping = len(s.mapping_layers)
    for i, c in enumerate(s.mapping_layers):
      cfg.mapping_channels[i] = c
    cfg.mapping_activation = _lib.ACTIVATIONS[s.mapping_activation]
    cfg.l2_reg_factor = s.l2_reg_factor
    L = _lib.lib()
    plan = L.wn_plan_create(C.byref(cfg))
    if not plan:
      raise ValueError(L.wn_last_error_string().decode())
    self._plan = C.c_void_p(plan)
    if s.dropout > 0:
      if s.dropout >= 1:
        raise ValueError('Dropout must be between 0 and 1.')
      _lib.check(L.wn_plan_set_dropout(self._plan, s.dropout, self._seed, 0))
    shapes = s.param_shapes(cond_inputs)
    n = L.wn_plan_num_tensors(self._plan)
    assert n == len(shapes), (n, len(shapes))
    self._names = [nm for nm, _ in shapes]
    self._offsets, self._shapes = [], []
    off, ln = C.c_int64(), C.c_int64()
    nd, isk = C.c_int32(), C.c_int32()
    sh = (C.c_int64 * 3)()
    for i, (nm, shp) in enumerate(shapes):
      _lib.check(L.wn_plan_tensor_info(self._plan, i, C.byref(off), C.byref(ln), C.byref(nd), sh, C.byref(isk)))
      # (local conditioning: the library's mapping stack is the Dense stack over the B * F condition rows; the variable is the
      # reference's 1x1 Conv1D kernel (1, cin, w) with the same flat element order)
      lib_shp = shp[1:] if (self.conditioning == 'local' and nm.startswith('mapping') and len(shp) == 3) else shp
      assert tuple(sh[:nd.value]) == tuple(lib_shp), (nm, tuple(sh[:nd.value]), shp)
      self._offsets.append(off.value)
      self._shapes.append(tuple(shp))
    total = L.wn_plan_param_count(self._plan)
    # Keras defaults: glorot-uniform kernels, zero biases (no initializer passed anywhere)
    g = torch.Generator().manual_seed(self._seed)
    flat = torch.zeros(total, dtype=torch.float32)
    for nm, shp, o in zip(self._names, self._shapes, self._offsets):
      if nm.endswith('kernel'):
        if len(shp) == 3:
          fan_in, fan_out = shp[0] * shp[1], shp[0] * shp[2]
        else:
          fan_in, fan_out = shp
        lim = math.sqrt(6.0 / (fan_in + fan_out))
        cnt = int(np.prod(shp))
        flat[o:o + cnt] = (torch.rand(cnt, generator=g) * 2 - 1) * lim
    self.flat_params = torch.nn.Parameter(flat.to(self._device), requires_grad=False)
    # gradient bucket = [flat gradient | loss, reg_loss, range_flag, device-reduced metrics]: the data-parallel exchange
    # is ONE all-reduce
    self._grad_bucket = torch.zeros(self.flat_params.numel() + 3 + self._TAIL_METRICS, dtype=torch.float32,
                                    device=self._device)
    self.flat_grads = self._grad_bucket[:self.flat_params.numel()]
    self.built = True
    if self.optimizer is not None:
      self.optimizer.build(self)

  def __del__(self):
    try:
      if self._plan is not None:
        _lib.lib().wn_plan_destroy(self._plan)
        self._plan = None
    except Exception:  # interpreter shutdown
      pass

  def kernel_report(self) -> str:
    """Which kernel family each phase selects for this network (the fast paths are shape-specialised)."""
    buf = C.create_string_buffer(2048)
    _lib.check(_lib.lib().wn_plan_describe(self._plan, buf, 2048))
    text = buf.value.decode()
    if self.conditioning == 'local':
      # the frames of the last training-form call (F > 1: the bias table has a row per frame and its gradient comes from
      # wn_cond_frame_sum_kernel; F = 1 runs the global model's kernels)
      frames = 'F=none yet' if self._last_frames is None else f'F={self._last_frames}' + \
          (' (per-frame bias rows, wn_cond_frame_sum_kernel)' if self._last_frames > 1 else ' (the global kernels)')
      text += f' | conditioning=local {frames}'
    return text

  def _log_kernels_once(self):
    import os
    import sys
    if not getattr(self, '_kernels_logged', False) and os.environ.get('WN_LOG_KERNELS'):
      self._kernels_logged = True
      print('[wavenets_amd] ' + self.kernel_report(), file=sys.stderr)

  # ------------------------------------------------------------------ weights
  def _tensor(self, name):
    i = self._names.index(name)
    o, shp = self._offsets[i], self._shapes[i]
    return self.flat_params.data[o:o + int(np.prod(shp))].view(*shp)

  @property
  def trainable_variables(self):
    """Views on the flat buffer in Keras creation order."""
    return [self._tensor(n) for n in self._names]

  @property
  def variable_names(self):
    return list(self._names)

  def get_weights(self):
    return [t.detach().cpu().numpy().copy() for t in self.trainable_variables]

  def set_weights(self, weights):
    self._not_averaged('set_weights')
    self._train_gen += 1                  # a differentiable() graph of the old weights is void
    if len(weights) != len(self._names):
      raise ValueError(f'expected {len(self._names)} arrays, got {len(weights)}')
    for t, w in zip(self.trainable_variables, weights):
      w = torch.as_tensor(np.asarray(w), dtype=torch.float32)
      if tuple(w.shape) != tuple(t.shape):
        raise ValueError(f'shape mismatch {tuple(w.shape)} vs {tuple(t.shape)}')
      t.copy_(w)

  def _not_averaged(self, what):
    if self._averaged is not None:
      raise RuntimeError(f'{what} inside averaged_weights(): the scope runs on the averaged weights and is read-only')

  @contextlib.contextmanager
  def averaged_weights(self):
    """Context manager (Adam(use_ema=True)): inside it every pass -- call, logits, test_step, generate, get_weights,
    io.save_weights(model, '*.weights.h5') -- runs on the optimizer's exponential moving average of the weights.  The
    storage behind ``flat_params`` is swapped for the average (every pass takes the parameters as a pointer and rebuilds
    its weight images from it on each call): no copy, no second plan.  On exit, also through an exception, the raw
    weights are back bit for bit.  Training, set_weights and training checkpoints raise RuntimeError inside it."""
    opt = self.optimizer
    if opt is None or not getattr(opt, 'use_ema', False):
      raise RuntimeError('averaged_weights() needs compile(optimizer=Adam(use_ema=True))')
    self._not_averaged('averaged_weights()')
    if not self.built:
      raise RuntimeError('averaged_weights(): the model is not built yet')
    opt.build(self)
    raw = self.flat_params.data
    self._averaged = raw
    self.flat_params.data = opt.ema
    try:
      yield self
    finally:
      self.flat_params.data = raw
      self._averaged = None

  def gradients(self):
    """Gradient views matching trainable_variables (after train_step / loss_and_grads)."""
    return [self.flat_grads[o:o + int(np.prod(s))].view(*s) for o, s in zip(self._offsets, self._shapes)]

  # ------------------------------------------------------------------ compile
  def compile(self, **kwargs):
    """src/model.py:157-169."""
    if 'loss' in kwargs:
      raise ValueError('Loss must be set in the model init function.')
    self._metrics_from_compilation = []
    if 'metrics' in kwargs and kwargs['metrics'] is not None:
      for metric in kwargs['metrics']:
        self._metrics_from_compilation.append(metric)
    self.loss_tracker = _Mean('loss')
    if self.regularization:
      self.reg_loss = _Mean('reg_loss')
    self.optimizer = kwargs.get('optimizer')
    if self.optimizer is not None and self.built:
      self.optimizer.build(self)

  @property
  def metrics(self):
    # the reference appends to the same list on every access (src/model.py:350-360); not reproduced
    m = list(self._metrics_from_compilation) + [self.loss_tracker]
    if self.regularization:
      m.append(self.reg_loss)
    return m

  # ------------------------------------------------------------------ helpers
  def _workspace(self, key, floats):
    ws = self._ws.get(key)
    if ws is None or ws.numel() < floats:
      ws = torch.empty(int(floats), dtype=torch.float32, device=self._device)
      self._ws[key] = ws
    return ws

  def _split_inputs(self, inputs):
    if self.conditioning is not None:
      x, cond = inputs
      cond = torch.as_tensor(cond, dtype=torch.float32, device=self._device).contiguous()
    else:
      x, cond = inputs, None
    x = torch.as_tensor(x, dtype=torch.float32, device=self._device).contiguous()
    if x.dim() != 3 or x.shape[-1] != 1:
      raise ValueError('input must have shape (batch, samples, 1)')
    if self.conditioning == 'local':
      return self._split_local(x, cond)
    if not self.built:
      self.build([tuple(x.shape), tuple(cond.shape)] if cond is not None else tuple(x.shape))
    if cond is not None and (cond.dim() != 2 or cond.shape[0] != x.shape[0] or cond.shape[1] != self._cond_inputs):
      raise ValueError('condition must have shape (batch, n_cond)')
    return x, cond

  def _split_local(self, x, cond):
    """Local conditioning: the condition is (B, F), the reference's form (one channel,
    src/model.py:133), or (B, F, Cin).  Returns it as the library takes it -- (B, F, Cin) with the plan armed for F frames,
    or (B, Cin) for F == 1, which is the global model's call -- the view keeps the caller's autograd graph.  The callers
    are wrapped in ``_disarms_frames``."""
    if cond.dim() == 2:
      cond = cond[:, :, None]
    if cond.dim() != 3 or cond.shape[0] != x.shape[0] or cond.shape[1] < 1:
      raise ValueError('condition must have shape (batch, frames) or (batch, frames, n_cond)')
    if not self.built:
      self.build([tuple(x.shape), tuple(cond.shape)])
    if cond.shape[2] != self._cond_inputs:
      raise ValueError(f'condition must have {self._cond_inputs} channels (got {cond.shape[2]})')
    F = int(cond.shape[1])
    self._last_frames = F
    if F == 1:
      return x, cond[:, 0, :].contiguous()
    self._arm_frames(F)          # T % F and hop % 32 are checked by the library against the T of the call, before any launch
    return x, cond.contiguous()

  def _arm_frames(self, frames):
    frames = int(frames) if frames and frames > 1 else 0
    # (an argument check may raise before the object has a plan)
    if frames != getattr(self, '_frames_armed', 0) and getattr(self, '_plan', None) is not None:
      _lib.check(_lib.lib().wn_plan_set_cond_frames(self._plan, frames))
      self._frames_armed = frames

  # ------------------------------------------------------------------ call
  @_disarms_frames
  def call(self, inputs, training=False):
    """src/model.py:213-239: probabilities (categorical) or linear mixture parameters.  (Reads the pass's range-guard
    float back -- one host sync -- and repeats the pass with the exact-fp32 kernels when an activation left the range
    of the split-precision ones.)"""
    x, cond = self._split_inputs(inputs)
    return self._forward_guarded(x, cond, want_probs=True, training=bool(training and self.dropout > 0))

  def _forward_guarded(self, x, cond, want_probs, training):
    B, T = x.shape[0], x.shape[1]
    L = _lib.lib()
    ws = self._workspace('train' if training else 'fwd', L.wn_plan_workspace_floats(self._plan, B, T, int(training)))
    out = torch.empty(B, T, self.spec.out_channels, dtype=torch.float32, device=self._device)
    fn = L.wn_forward_training if training else L.wn_forward
    if training:
      self._train_gen += 1
      self._last_train_frames = self._frames_armed
      # the Dropout layers are active (src/layers.py:195-196): a fresh mask per call, as in a training step
      self._arm_dropout()

    def run():
      _lib.check(fn(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                    _lib.ptr(out) if want_probs else None, None if want_probs else _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                    _lib.stream_ptr()))

    def keep_guard():
      # the pass's guard float, copied out of the shared workspace on the stream (a later pass on the same workspace -- another
      # call, a test_step -- overwrites the slot; this one-float copy is what range_tripped_last_forward() reads)
      slot = L.wn_plan_range_slot(self._plan, B, T, int(training))
      self._last_fwd = (ws[slot:slot + 1].clone(), training)
    _guard.guarded(self, run, lambda: self._guard_over(*self._last_fwd), after_first=keep_guard,
                   skip=not self.range_check or L.wn_debug_value(1) == 1)
    return out

  def range_tripped_last_forward(self) -> bool:
    """Deferred form of the guard check of call() / logits() (range_check = False): did the last call() / logits() pass
    leave the range of the split-precision kernels?  (Repeat it inside `with model.exact_fp32():` if so.  With
    range_check = False nothing else checks: an unchecked pass may hold inf / NaN.)"""
    if self._last_fwd is None:
      return False
    return bool(self._guard_over(*self._last_fwd))

  def forward(self, inputs, training=False):
    return self.call(inputs, training=training)

  @_disarms_frames
  def logits(self, inputs):
    """Pre-softmax head output (parity checks)."""
    x, cond = self._split_inputs(inputs)
    return self._forward_guarded(x, cond, want_probs=False, training=False)

  # ------------------------------------------------------------------ training
  @staticmethod
  def _world():
    return dp.world_size()

  @staticmethod
  def _rank():
    return dp.rank()

  def training_intermediate(self, what: int, idx: int, B: int, T: int):
    """View on an intermediate the last loss_and_grads call (B utterances, T predicted samples) left in the
    training workspace (wn_debug_ws_region; parity tests compare these with the oracle's autograd values).
    what 0..12 as listed in include/wn_hip.h; 13: GP[b][i], the gradient at the pre-activation output of inner conv i of
    block b (idx = b * (layers_per_block - 1) + i, as for 11); 14: XD[idx], the dropped copy of block input idx, which
    exists only with dropout > 0 (ValueError otherwise, as for every absent region)."""
    off, ln = C.c_int64(), C.c_int64()
    # (local conditioning: the regions behind the conditioning's lie where the pass with its F frames carved them)
    with _guard.kept_pass(self, self._last_train_frames):
      _lib.check(_lib.lib().wn_debug_ws_region(self._plan, B, T, what, idx, C.byref(off), C.byref(ln)))
    return self._ws['train'][off.value:off.value + ln.value]

  @contextlib.contextmanager
  def exact_fp32(self):
    """Context manager: the calling thread's launches use the exact-fp32 MFMA kernels (no fp16 hi|lo operand split)."""
    L = _lib.lib()
    prev = L.wn_debug_value(1)
    L.wn_debug_set(1, 1)
    try:
      yield
    finally:
      L.wn_debug_set(1, prev)

  def _guard_over(self, guard, training):
    """Reads a pass's copied range-guard float (one host sync) against the limit of the split-precision kernels."""
    m = float(guard)
    # with dropout the split kernels read H * mask / (1 - rate) while H is what the slot records
    limit = _lib.lib().wn_range_limit() * ((1.0 - self.dropout) if (training and self.dropout > 0) else 1.0)
    return not (m < limit)

  def set_drop_step(self, n: int):
    """Training calls already made (resume): the next dropout mask is that of call n + 1."""
    self._drop_step = int(n)

  def _arm_dropout(self):
    # every replica draws its own mask each step (MirroredStrategy runs an independent Dropout per replica):
    # mask counter = call_index * world + rank + 1; single process: 1, 2, 3, ...
    if self.dropout > 0:
      step = self._drop_step * self._world() + self._rank() + 1
      _lib.check(_lib.lib().wn_plan_set_dropout(self._plan, self.dropout, self._seed, step))
      self._drop_armed_step = step
      self._drop_step += 1

  @staticmethod
  def _check_sample_weight(data, sample_weight):
    """The shape check of ``sample_weight`` against the batch, on shapes alone: before the model is built and before
    anything is queued.  Returns the weight as given (None: no weights)."""
    if sample_weight is None:
      return None
    x = data[0] if isinstance(data, (tuple, list)) else data
    xs, ws = tuple(getattr(x, 'shape', ())), tuple(getattr(sample_weight, 'shape', np.shape(sample_weight)))
    if len(xs) >= 2:
      B, T = int(xs[0]), int(xs[1]) - 1
      if ws not in ((B, T), (B, T, 1), (B,)):
        raise ValueError(f'sample_weight must have shape ({B}, {T}), ({B}, {T}, 1) or ({B},): one weight per target '
                         f'x[b, t + 1], or one per utterance (got {ws})')
    return sample_weight

  def _row_weights(self, sample_weight, B, T):
    """(B, T) fp32 on the device; a per-utterance (B,) weight is expanded there."""
    if sample_weight is None:
      return None
    w = torch.as_tensor(sample_weight, dtype=torch.float32, device=self._device)
    if w.dim() == 1:
      w = w[:, None].expand(B, T)
    return w.reshape(B, T).contiguous()

  @_disarms_frames
  def loss_and_grads(self, data, global_batch=None, n_replicas=None, want_pred=False, want_sample=False,
                     _loss_in_bucket=False, _between=None, sample_weight=None):
    """Forward + loss + backward of this replica's rows (src/model.py:319-335).

    Fills ``self.flat_grads`` with d(sum_local l / B_global)/d(theta); returns
    (loss tensor[3] = {loss, reg_loss, range_flag}, pred or None, y_true).  range_flag = 1: a forward activation left
    the range of the split-precision kernels and the results are not valid (train_step then repeats the step with the
    exact-fp32 kernels; a direct caller checks loss[2] and does the same through ``exact_fp32()``).  ``want_sample``: the step also draws
    ``sample_waveform(pred)`` (src/model.py:338) from the logits inside the library -- same draw, no (B,T,C)
    probability tensor -- and returns it in place of pred; when the library cannot (deterministic / more than
    1024 classes) pred is returned and the caller samples from it.

    ``sample_weight``: fp32 ``(B, T)``, ``(B, T, 1)`` or per utterance ``(B,)``; ``w[b, t]`` weighs the
    target ``x[b, t + 1]``.  loss = sum w l / global_batch: the normaliser stays the global batch as in
    ``tf.nn.compute_average_loss``, there is no division by sum w -- scale ``w`` yourself for a mean over the valid samples.
    A weight of 0 removes the row whatever it holds (inf and NaN included); all ones give the bits of the call without
    weights.  Negative and non-finite weights are not checked (a plain product).  The draw of ``want_sample`` is made for
    every row and does not see the weights."""
    sample_weight = self._check_sample_weight(data, sample_weight)
    self._not_averaged('loss_and_grads')
    x, cond = self._split_inputs(data)
    B, T = x.shape[0], x.shape[1] - 1
    if T < 1:
      raise ValueError('training data must hold at least 2 samples per utterance')
    world = self._world()
    if global_batch is None:
      global_batch = B * world                         # compute_average_loss, src/model.py:328-329
    if n_replicas is None:
      n_replicas = world
    L = _lib.lib()
    self._log_kernels_once()
    ws = self._workspace('train', L.wn_plan_workspace_floats(self._plan, B, T, 1))
    self._train_gen += 1
    self._last_train_frames = self._frames_armed
    # train_step keeps {loss, reg_loss} in the gradient bucket's tail (one all-reduce); other callers get their own tensor
    loss = self._grad_bucket[self.flat_params.numel():] if _loss_in_bucket else \
        torch.empty(3, dtype=torch.float32, device=self._device)
    sample = None
    if want_sample and self._fused_step_sample:
      sample = torch.empty(B, T, 1, dtype=torch.float32, device=self._device)
      if L.wn_plan_arm_step_sample(self._plan, _lib.ptr(sample), 0, 0x0402, self._sample_calls + 1) == 0:
        self._sample_calls += 1
      else:
        sample = None
    want_pred = want_pred or (want_sample and sample is None)
    pred = torch.empty(B, T, self.spec.out_channels, dtype=torch.float32, device=self._device) if want_pred else None
    self._arm_dropout()
    weights = self._row_weights(sample_weight, B, T)

    def run():
      _lib.check(L.wn_train_fwd_bwd(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                                    int(global_batch), int(n_replicas), _lib.ptr(self.flat_grads),
                                    _lib.ptr(loss), _lib.ptr(pred), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    with _guard.row_weights(self._plan, weights, B * T):      # (disarmed behind the step sample)
      try:
        if _between is None:
          run()
          out = (sample if sample is not None else self.sample_waveform(pred)) if want_sample else pred
        else:
          # the step as two calls: forward + loss, the caller's own work (its read-back of loss / metrics), backward
          try:
            L.wn_plan_set_train_phases(self._plan, 1)
            run()
            out = (sample if sample is not None else self.sample_waveform(pred)) if want_sample else pred
            _between(loss, out, x[:, 1:, :])
            L.wn_plan_set_train_phases(self._plan, 2)
            run()
          finally:
            L.wn_plan_set_train_phases(self._plan, 3)
      finally:
        if sample is not None:
          L.wn_plan_arm_step_sample(self._plan, None, 0, 0, 0)      # never leave a stale pointer armed
    return loss, out, x[:, 1:, :]

  def train_step(self, data, sample_weight=None):
    """src/model.py:309-348.  Data-parallel: the flat gradient (and the step's scalars) are
    SUM-all-reduced over RCCL before the (replicated, deterministic) optimizer step.

    Range guard: the split-precision kernels need |activation| < 65504.  The step's range flag rides in the bucket's
    tail through the all-reduce, the optimizer kernel skips the update on every replica when it is set, and the step is
    then repeated here with the exact-fp32 kernels (same dropout mask, same optimizer iteration); ``train_guard_trips``
    counts those repeats (a tripped step costs a second, ~2.7x slower one).

    ``sample_weight``: Keras's third element of the step's data, semantics as in ``loss_and_grads``.  The step keeps its
    launches (the loss kernels take the factor per row).  A compiled ``MeanSquaredError`` becomes Keras's weighted mean
    sum w (y - sample)^2 / sum w (0 when sum w == 0); under data parallelism the replicas' ratios are averaged."""
    sample_weight = self._check_sample_weight(data, sample_weight)
    if self.optimizer is None:
      raise RuntimeError('compile(optimizer=...) first')
    self._not_averaged('train_step')
    wkw = {} if sample_weight is None else {'sample_weight': sample_weight}
    kept = []                                        # the pass that stands: (lv, dev_metrics, y_true, sample)

    def run():
      kept[:] = self._train_step_once(data, sample_weight)

    def undo():
      self.optimizer.undo_last_apply()               # (iterations, accumulated) as before the skipped launch
      self._drop_step -= 1 if self.dropout > 0 else 0
    # lv[2] > 0: tripped on some replica -> on all of them after the SUM (the step has read its scalars back already)
    _guard.guarded(self, run, lambda: kept[0][2] > 0, before_rerun=undo, counter='train_guard_trips', count_first=True)
    lv, pending, y_true, sample = kept
    return self._commit_step(lv, pending, y_true, sample, wkw, reg_loss=True)

  def _tail_metrics(self):
    """The compiled metrics whose reduction runs on the device, into the tail slots behind {loss, reg_loss, range_flag}."""
    return [m for m in self._metrics_from_compilation if hasattr(m, 'update_state_device')][:self._TAIL_METRICS]

  def _commit_step(self, lv, dev_metrics, y_true, sample, wkw, reg_loss):
    """The host end of train_step / test_step: lv[3:] into the device-reduced metrics, lv[0] (and lv[1], where ``reg_loss``
    says the step reports it) into the trackers, the host metrics updated from the sample; returns the logs."""
    for m, v in zip(dev_metrics, lv[3:]):
      m.commit(v)
    for metric in self.metrics:
      if metric.name == 'loss':
        metric.update_state(lv[0])
      elif metric.name == 'reg_loss':
        if reg_loss:
          metric.update_state(lv[1])
      elif not hasattr(metric, 'update_state_device'):
        metric.update_state(y_true, sample, **wkw)
    return {m.name: m.result() for m in self.metrics if reg_loss or m.name != 'reg_loss'}

  def _mirror(self, vec):
    """Queues the device-to-host copy of the step's scalars into pinned memory and records the event the host waits on."""
    if self._log_mirror is None or self._log_mirror.numel() != vec.numel():
      self._log_mirror = torch.empty(vec.numel(), dtype=torch.float32, pin_memory=True)
      self._log_event = torch.cuda.Event()
    self._log_mirror.copy_(vec, non_blocking=True)
    self._log_event.record()

  def _train_step_once(self, data, sample_weight=None):
    """One pass of the step.  The scalars a step reports -- {loss, reg_loss, range flag, device-reduced metrics} -- live in
    the gradient bucket's tail, each already scaled so that the SUM over the replicas is the reported value.

    * single replica (no process group; ``early_logs`` True): they are final right after the loss kernels, so their
      pinned copy is queued THERE, between the forward and the backward half, and the host waits for that copy only: it
      returns with ~4 ms of the step still queued and has the next step's launches out before the GPU runs dry.
    * data parallel (a process group exists; ``early_logs`` False): ONE collective per step -- the bucket's SUM
      all-reduce carries gradients and tail together (train.py:203, src/model.py:328-336); the pinned copy of the reduced
      tail is queued right behind it, the optimizer behind that, and the host waits for the copy's event (no blocking
      ``tolist()`` at the end of the step).  ``early_logs = True`` under a process group instead all-reduces a copy of
      the few scalars between forward and backward (a second, tiny collective) and reads them early."""
    if not self.built:
      try:
        self._split_inputs(data)                        # Keras builds on the first call (the condition width fixes the shapes)
      finally:
        self._arm_frames(0)                             # (a local condition arms its frames: loss_and_grads does so itself)
    want_metric = len(self._metrics_from_compilation) > 0
    dev_metrics = self._tail_metrics()
    early = self.early_logs if self.early_logs is not None else not dp.initialized()
    world = self._world()
    n = self.flat_params.numel()
    tail = self._grad_bucket[n:]
    nt = 3 + len(dev_metrics)
    wkw = {} if sample_weight is None else {'sample_weight': sample_weight}      # a metric gets the keyword only with weights

    def queue_metrics(sample, y_true):
      for i, m in enumerate(dev_metrics):
        m.update_state_device(y_true, sample, out=tail[3 + i:4 + i], scale=1.0 / world, **wkw)

    # Adam(gradient_accumulation_steps=k): micro-steps 1 .. k-1 only store the gradient and do not reduce it; what is
    # reduced is a clone of the few scalars, whose flag then guards the store on every replica alike.  On micro-step k each
    # replica forms its own mean ahead of the bucket's all-reduce (it writes flat_grads only, which a repeated step
    # recomputes).  Without the keyword ``updates`` is always True and form_mean does nothing.
    updates = self.optimizer.updates_next()
    reduced = []                                        # the early branch's reduced scalars, for a storing micro-step

    def scalars_alone():
      vec = tail[:nt]
      if dp.initialized():
        vec = vec.clone()
        dp.allreduce_bucket(vec)
      return vec

    if early:
      def between(loss, sample, y_true):
        queue_metrics(sample, y_true)
        vec = scalars_alone()
        reduced.append(vec)
        self._mirror(vec)
      loss, sample, y_true = self.loss_and_grads(data, want_sample=want_metric, _loss_in_bucket=True, _between=between, **wkw)
      if updates:
        self.optimizer.clip_local_gradients(self)       # clip_before_reduce only; in place, see the note below
        self.optimizer.form_mean(self, skip_flag=tail[2:3])
        dp.allreduce_bucket(self._grad_bucket)          # gradients + tail; no-op without a process group
        self.optimizer.apply_gradients(self, skip_flag=tail[2:3])
      else:
        self.optimizer.apply_gradients(self, skip_flag=reduced[0][2:3])
    elif not updates:
      loss, sample, y_true = self.loss_and_grads(data, want_sample=want_metric, _loss_in_bucket=True, **wkw)
      queue_metrics(sample, y_true)
      vec = scalars_alone()                             # the micro-step's only collective: a few floats
      self._mirror(vec)
      self.optimizer.apply_gradients(self, skip_flag=vec[2:3])
    else:
      loss, sample, y_true = self.loss_and_grads(data, want_sample=want_metric, _loss_in_bucket=True, **wkw)
      queue_metrics(sample, y_true)
      # Adam(clip_before_reduce=True) clips THIS replica's gradient in place ahead of the SUM (one path, with or without a
      # process group; the tail behind the gradient is not touched).  In place is safe under the range guard: a tripped
      # step is skipped by the flag and repeated from scratch, gradients recomputed, so nothing is clipped twice.
      self.optimizer.clip_local_gradients(self)
      self.optimizer.form_mean(self, skip_flag=tail[2:3])
      dp.allreduce_bucket(self._grad_bucket)            # the step's ONE collective: gradients + {loss, reg_loss, flag, metrics}
      self._mirror(tail[:nt])
      self.optimizer.apply_gradients(self, skip_flag=tail[2:3])
    self._log_event.synchronize()
    return self._log_mirror.tolist(), dev_metrics, y_true, sample

  @_disarms_frames
  def test_step(self, data, sample_weight=None):
    """src/model.py:362-391 (range guard as in train_step: a tripped pass is repeated with the exact-fp32 kernels and
    counted in ``test_guard_trips``).  ``sample_weight``: as in ``train_step`` -- loss = sum w l / global_batch, a compiled
    ``MeanSquaredError`` the weighted mean."""
    sample_weight = self._check_sample_weight(data, sample_weight)
    x, cond = self._split_inputs(data)
    B, T = x.shape[0], x.shape[1] - 1
    weights = self._row_weights(sample_weight, B, T)
    wkw = {} if weights is None else {'sample_weight': weights}
    world = self._world()
    L = _lib.lib()
    ws = self._workspace('fwd', L.wn_plan_workspace_floats(self._plan, B, T, 0))
    want_metric = len(self._metrics_from_compilation) > 0
    dev_metrics = self._tail_metrics()
    vec = torch.zeros(3 + len(dev_metrics), dtype=torch.float32, device=self._device)
    pred = torch.empty(B, T, self.spec.out_channels, dtype=torch.float32, device=self._device) if want_metric else None
    kept = []                                        # the pass that stands: (lv, sample)

    def once():
      with _guard.row_weights(self._plan, weights, B * T):
        _lib.check(L.wn_eval_loss(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                                  B * world, _lib.ptr(vec), _lib.ptr(pred), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr()))
      sample = self.sample_waveform(pred) if want_metric else None
      # as in train_step: device-side metric reductions into the same vector, ONE collective (loss sums over the replicas;
      # reg_loss unused; flag: any replica; metrics: replica means), ONE device-to-host read
      for i, m in enumerate(dev_metrics):
        m.update_state_device(x[:, 1:, :], sample, out=vec[3 + i:4 + i], scale=1.0 / world, **wkw)
      dp.allreduce_bucket(vec)
      kept[:] = vec.tolist(), sample
    _guard.guarded(self, once, lambda: kept[0][2] > 0, counter='test_guard_trips', count_first=True)
    lv, sample = kept
    return self._commit_step(lv, dev_metrics, x[:, 1:, :], sample, wkw, reg_loss=False)

  @_disarms_frames
  def score(self, data, sample_weight=None, per_sample=False):
    """Per-utterance negative log-likelihoods of ``data`` in one evaluation pass.

    ``data`` is what ``test_step`` takes: ``x (B, T + 1, 1)`` or ``(x, cond)``; the pass is the inference forward (no
    dropout) and works inside ``averaged_weights()``.  Returns a dict of device tensors::

      'nll'             (B,)  sum_t w[b, t] l[b, t], in nats
      'weight'          (B,)  sum_t w[b, t]; exactly T without sample_weight
      'nll_per_sample'  (B,)  nll / weight
      'bits_per_sample' (B,)  nll / (weight ln 2)
      'rows'            (B, T)  w[b, t] l[b, t] as the loss kernel stored it -- only with per_sample=True

    ``l`` is the per-row loss exactly as ``loss_fn`` defines it for the head: Keras's clipped cross entropy of a categorical
    head; for a mixture head the negative log of the bin mass (logistic) or of the density (gaussian), so "bits per sample"
    of a mixture head is that NLL divided by ln 2 and nothing more (a density's is not bounded below by 0).  There is no
    1 / global_batch factor and no L2 term; no metric is updated and nothing is all-reduced: a replica scores its own rows.

    ``sample_weight``: the shapes of ``train_step`` (``(B, T)``, ``(B, T, 1)`` or ``(B,)``), the semantics of DESIGN.md
    section 25 -- a weight of 0 removes the row whatever it holds, so ``data.length_weights(lengths, T)`` scores padded
    utterances of different lengths.  Where ``weight == 0`` the two ratios are NaN (0 / 0); they are not special-cased.

    Range guard as in ``test_step``: a tripped pass is repeated under ``exact_fp32()`` and counted in
    ``score_guard_trips`` (one host read of the flag per call)."""
    sample_weight = self._check_sample_weight(data, sample_weight)
    x, cond = self._split_inputs(data)
    B, T = x.shape[0], x.shape[1] - 1
    if T < 1:
      raise ValueError('score needs at least 2 samples per utterance')
    weights = self._row_weights(sample_weight, B, T)
    L = _lib.lib()
    ws = self._workspace('fwd', L.wn_plan_workspace_floats(self._plan, B, T, 0))
    out = torch.empty(2 * B + 1, dtype=torch.float32, device=self._device)
    nll, weight, flag = out[:B], out[B:2 * B], out[2 * B:]
    rows = torch.empty(B, T, dtype=torch.float32, device=self._device) if per_sample else None

    def once():
      with _guard.row_weights(self._plan, weights, B * T):
        _lib.check(L.wn_score(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T, _lib.ptr(nll),
                              _lib.ptr(weight), _lib.ptr(rows), _lib.ptr(flag), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    _guard.guarded(self, once, lambda: float(flag) > 0, counter='score_guard_trips', count_first=True)
    nll, weight = nll.clone(), weight.clone()
    res = {'nll': nll, 'weight': weight, 'nll_per_sample': nll / weight, 'bits_per_sample': nll / (weight * math.log(2.0))}
    if per_sample:
      res['rows'] = rows
    return res

  def eval_intermediate(self, what: int, B: int, T: int):
    """View on a region of the inference workspace as the last ``test_step`` / ``score`` / ``call`` over (B, T) left it
    (wn_debug_eval_region: 5 the logits, 12 the per-row losses; tests tell from them which loss path a pass took)."""
    off, ln = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().wn_debug_eval_region(self._plan, B, T, what, C.byref(off), C.byref(ln)))
    return self._ws['fwd'][off.value:off.value + ln.value]

  # ------------------------------------------------------------------ autograd
  @_disarms_frames
  def differentiable(self, inputs, training=False, output='probs'):
    """The network as one ``torch.autograd`` node: returns ``(B, T, C_out)`` with a ``grad_fn``, for losses the training
    step does not have built in (label smoothing, distillation, a loss on the expected sample, a gradient
    at the input waveform or the condition).  DESIGN.md section 20.  Masks and per-sample weights do not need it: ``train_step``,
    ``test_step`` and ``loss_and_grads`` take ``sample_weight`` inside the fused step.

    ``output='probs'`` is what ``call()`` returns, ``'logits'`` the pre-softmax head output; for the mixture heads both
    are the same linear parameters.  A loss of the form ``-log p[target]`` on ``'probs'`` meets ``0 * inf`` where a
    probability underflows: such losses take ``output='logits'`` and ``torch.log_softmax``.  A non-finite gradient
    handed to ``backward`` gives non-finite gradients (nothing is clipped or guarded there).

    ``training=True`` on a model with ``dropout > 0`` draws a fresh mask exactly as ``call(training=True)`` does;
    otherwise the Dropout layers are off for the pass.  The forward range guard is that of ``call()``: a tripped pass is
    repeated in exact fp32, and backward runs in the math mode (and on the mask) of the pass that was kept, wherever
    it is called from.

    ``backward`` always leaves d<g, out>/d(theta) in ``model.flat_grads`` (overwritten, as ``loss_and_grads`` does; nothing
    of the built-in losses is added: no 1/global_batch, no L2 term), so ``model.optimizer.apply_gradients(model)`` takes
    the step.  It also reaches ``flat_params.grad`` only after ``flat_params.requires_grad_(True)``; the gradients at
    the waveform and the condition are formed only when those tensors require grad.  Under data parallelism the caller
    reduces ``flat_grads`` itself (``dp.allreduce_gradients``).

    One graph is alive at a time: the saved activations live in the model's training workspace.  ``backward`` raises
    RuntimeError when another pass used that workspace since (``loss_and_grads``, ``train_step``,
    ``call(training=True)``, another ``differentiable``), when the weights changed since (``optimizer.apply_gradients``,
    ``finalize_variable_values``, ``set_weights``), on a second run of the same graph (``retain_graph``) and under
    ``create_graph=True`` (no second derivatives).  Writing ``flat_params`` by hand in between is not detected."""
    if output not in ('probs', 'logits'):
      raise ValueError(f"output must be 'probs' or 'logits' (got {output!r})")
    self._not_averaged('differentiable')
    x, cond = self._split_inputs(inputs)
    if self._vjp_anchor is None:
      # the node must exist even when no input asks for a gradient (flat_grads is its product): a zero-size input that does
      self._vjp_anchor = torch.zeros(0, dtype=torch.float32, device=self._device, requires_grad=True)
    return _NetFn.apply(x, cond, self.flat_params, self._vjp_anchor, self, bool(training and self.dropout > 0),
                        output == 'probs')

  def _set_dropout_state(self, rate, step):
    if self.dropout > 0:
      _lib.check(_lib.lib().wn_plan_set_dropout(self._plan, rate, self._seed, step))

  # ------------------------------------------------------------------ sampling / loss
  def prepare_target(self, x):
    """src/model.py:151-155: Discretization (bit-exact bucket indices) or identity."""
    if self.num_mixtures is not None:
      return x
    x = torch.as_tensor(x, dtype=torch.float32, device=self._device).contiguous()
    idx = torch.empty(x.shape, dtype=torch.int32, device=self._device)
    _lib.check(_lib.lib().wn_quantize(_lib.ptr(x), _lib.ptr(idx), x.numel(), self.bits, _lib.stream_ptr()))
    return idx

  def sample_waveform(self, inputs, deterministic=False, temperature=1.0, top_k=0, seed=None, top_p=1.0):
    """src/model.py:393-503: (B,T,C_out) -> (B,T,1).  Stochastic draws use Philox keyed by the
    reference's seed (4,2) -> 0x0402 plus a per-call offset (TF's stream is not reproducible).
    temperature / top_k / seed (additions): categorical rows are drawn from p^(1/T) over the
    top_k most probable classes (ties: lower class index first; 0 or >= classes = all), mixture rows from
    [w / T | mu | s + ln T]; seed replaces the key 0x0402.  top_p in (0, 1] (categorical only; 1.0 = off): of the classes
    top_k kept, the shortest prefix of the same ranking whose tempered mass reaches top_p of the total.  The defaults
    are the draw without them, bit for bit."""
    pred = torch.as_tensor(inputs, dtype=torch.float32, device=self._device).contiguous()
    if pred.dim() != 3:
      raise ValueError('prediction must have shape (batch, samples, channels)')
    B, T, Cc = pred.shape
    sampling = self._sampling(temperature, top_k, seed, Cc, top_p)
    out = torch.empty(B, T, 1, dtype=torch.float32, device=self._device)
    self._sample_calls += 1
    _lib.check(_lib.lib().wn_sample_waveform_sampled(_lib.HEADS[self.sampling_function], _lib.ptr(pred), B * T, Cc,
                                                      self.num_mixtures or 0, self.bits, int(bool(deterministic)),
                                                      C.byref(sampling), self._sample_calls, _lib.ptr(out),
                                                      _lib.stream_ptr()))
    return out

  def loss_fn(self, target, pred):
    """src/model.py:505-551: per-(b,t) loss, shape (B,T)."""
    pred = torch.as_tensor(pred, dtype=torch.float32, device=self._device).contiguous()
    B, T, Cc = pred.shape
    if self.sampling_function == 'categorical':
      tgt = torch.as_tensor(target, device=self._device).to(torch.int32).contiguous()
    else:
      tgt = torch.as_tensor(target, dtype=torch.float32, device=self._device).contiguous()
    if tgt.numel() != B * T:
      raise ValueError('target must have shape (batch, samples, 1)')
    out = torch.empty(B, T, dtype=torch.float32, device=self._device)
    _lib.check(_lib.lib().wn_loss_fn(_lib.HEADS[self.sampling_function], _lib.ptr(tgt), _lib.ptr(pred), B * T, Cc,
                                      self.num_mixtures or 0, self.bits, _lib.ptr(out), _lib.stream_ptr()))
    return out

  # ------------------------------------------------------------------ generation
  def compute_receptive_field(self, sampling_frequency):
    """src/model.py:553-556."""
    return self.receptive_field / sampling_frequency
