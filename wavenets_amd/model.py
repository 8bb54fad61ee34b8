"""WaveNet model: host-side mirror of src/model.py::WaveNet over the gfx950 HIP library.

Same constructor keywords, method names, argument meaning, tensor layouts
(channels-last ``(B, T, C)`` fp32) and exception types as the reference class; everything
underneath is ``libwn_hip.so`` (no TensorFlow, no CPU fallback).  PyTorch is used only for
device memory, streams and ``torch.distributed`` (RCCL).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import spec as _spec
from .layers import WaveNetLayer
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


class MeanSquaredError:
  """Minimal stand-in for tf.keras.metrics.MeanSquaredError (train.py:227)."""
  name = 'mean_squared_error'

  def __init__(self):
    self._scratch = None
    self.reset_state()

  def reset_state(self):
    self.total, self.count = 0.0, 0

  def update_state(self, y_true, y_pred, sample_weight=None):
    self.total += float(self.update_state_device(y_true, y_pred, sample_weight=sample_weight))
    self.count += 1

  # two-phase form used by train_step / test_step: the reduction is queued behind the step's kernels (one library launch
  # pair, no torch arithmetic) and its value comes back in the step's single device-to-host read.  ``out``: a one-float
  # device view to write into (the gradient bucket's tail in a training step); ``scale`` = 1 / replicas makes the SUM
  # over the replicas the mean Keras reports.  ``sample_weight`` (one weight per element of y_true, or per utterance):
  # Keras's weighted mean sum(w d^2) / sum(w) of the step, 0 when sum(w) == 0, both sums in the same pass on the device;
  # the replicas' ratios are then averaged, which is the global weighted mean only when they hold equal sum(w).
  def update_state_device(self, y_true, y_pred, out=None, scale=1.0, sample_weight=None):
    n = y_true.numel()
    if out is None:
      out = torch.empty(1, dtype=torch.float32, device=y_true.device)
    if self._scratch is None or self._scratch.device != y_true.device:
      self._scratch = torch.empty(2048, dtype=torch.float32, device=y_true.device)
    if sample_weight is not None:
      w = torch.as_tensor(sample_weight, dtype=torch.float32, device=y_true.device)
      if w.numel() != n:
        if w.dim() != 1 or w.shape[0] != y_true.shape[0]:
          raise ValueError(f'sample_weight must hold one weight per element of y_true {tuple(y_true.shape)} or one per '
                           f'utterance (got {tuple(w.shape)})')
        w = w.reshape(-1, *([1] * (y_true.dim() - 1))).expand(y_true.shape)
      _lib.check(_lib.lib().wn_weighted_squared_error(_lib.ptr(y_true.contiguous()), _lib.ptr(y_pred.contiguous()),
                                                      _lib.ptr(w.contiguous()), n, float(scale), _lib.ptr(out),
                                                      _lib.ptr(self._scratch), _lib.stream_ptr()))
      return out
    _lib.check(_lib.lib().wn_sum_squared_error(_lib.ptr(y_true.contiguous()), _lib.ptr(y_pred.contiguous()), n,
                                               float(scale) / n, _lib.ptr(out), _lib.ptr(self._scratch),
                                               _lib.stream_ptr()))
    return out

  def commit(self, value):
    self.total += float(value)
    self.count += 1

  def result(self):
    return self.total / max(self.count, 1)


class _Mean:
  def __init__(self, name):
    self.name = name
    self.reset_state()

  def reset_state(self):
    self.total, self.count = 0.0, 0

  def update_state(self, v):
    self.total += float(v)
    self.count += 1

  def result(self):
    return self.total / max(self.count, 1)


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


class _NetFn(torch.autograd.Function):
  """WaveNet.differentiable: wn_forward_training on the model's training workspace, wn_vjp from the gradient autograd
  hands back.  Inputs (x, cond, flat_params) and a zero-size anchor that keeps the node alive."""

  @staticmethod
  def forward(ctx, x, cond, flat_params, anchor, model, drop, want_probs):
    L = _lib.lib()
    B, T = x.shape[0], x.shape[1]
    x, cond = x.detach(), (cond.detach() if cond is not None else None)
    # the workspace layout depends on the dropout rate in force: set it first (off unless this pass draws a mask)
    if drop:
      model._arm_dropout()
    else:
      model._set_dropout_state(0.0, 0)
    state = (model.dropout if drop else 0.0, model._drop_armed_step if drop else 0)
    frames = cond.shape[1] if (cond is not None and cond.dim() == 3) else 0     # local conditioning, F > 1
    try:
      model._arm_frames(frames)
      ws = model._workspace('train', L.wn_plan_workspace_floats(model._plan, B, T, 1))
      model._train_gen += 1
      model._last_train_frames = frames if frames > 1 else 0
      out = torch.empty(B, T, model.spec.out_channels, dtype=torch.float32, device=model._device)

      def run():
        _lib.check(L.wn_forward_training(model._plan, _lib.ptr(flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                                         _lib.ptr(out) if want_probs else None, None if want_probs else _lib.ptr(out),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
      run()
      mode = L.wn_debug_value(1)
      slot = L.wn_plan_range_slot(model._plan, B, T, 1)
      if model.range_check and mode != 1 and model._guard_over(ws[slot:slot + 1].clone(), drop):
        with model.exact_fp32():
          run()
        mode = 1
    finally:
      model._set_dropout_state(model.dropout, model._drop_armed_step)
      model._arm_frames(0)
    ctx.model, ctx.mode, ctx.drop_state, ctx.stamp, ctx.done = model, mode, state, model._train_gen, False
    ctx.want_probs, ctx.frames = want_probs, frames
    ctx.save_for_backward(x, cond)
    return out

  @staticmethod
  @torch.autograd.function.once_differentiable          # second derivatives are refused, not returned without a graph
  def backward(ctx, g):
    model = ctx.model
    if ctx.done:
      raise RuntimeError('differentiable: this graph has already been run backward (one pass of activations is kept: '
                         'retain_graph re-runs are not supported; call differentiable again)')
    if model._train_gen != ctx.stamp:
      raise RuntimeError('differentiable: another pass used the training workspace between forward and backward '
                         '(loss_and_grads / train_step, call(training=True) or another differentiable), or the '
                         'weights changed (optimizer step, set_weights): the saved activations are gone or stale; '
                         'one graph is alive at a time')
    model._not_averaged('backward of differentiable')
    ctx.done = True
    x, cond = ctx.saved_tensors
    flat_params = model.flat_params                # (read in place: the optimizer writes it through the library)
    L = _lib.lib()
    B, T = x.shape[0], x.shape[1]
    g = g.to(torch.float32).contiguous()
    need_x, need_c, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
    g_x = torch.empty_like(x) if need_x else None
    g_c = torch.empty_like(cond) if (need_c and cond is not None) else None
    ws = model._ws['train']
    # the math mode and the mask of the pass that was kept, whatever the calling thread's are now
    prev = L.wn_debug_value(1)
    L.wn_debug_set(1, ctx.mode)
    model._set_dropout_state(*ctx.drop_state)
    try:
      model._arm_frames(ctx.frames)
      _lib.check(L.wn_vjp(model._plan, _lib.ptr(flat_params), _lib.ptr(x), _lib.ptr(cond), B, T, _lib.ptr(g),
                          0 if ctx.want_probs else 1, _lib.ptr(model.flat_grads), _lib.ptr(g_x), _lib.ptr(g_c),
                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    finally:
      L.wn_debug_set(1, prev)
      model._set_dropout_state(model.dropout, model._drop_armed_step)
      model._arm_frames(0)
    return g_x, g_c, (model.flat_grads.clone() if need_p else None), None, None, None, None


_RELAY_GAVE_UP = ('wn_generate: a workgroup of the generation relay gave up waiting for its predecessor '
                  '(code {}); the samples of this {} are invalid')


class _RowControls:
  """Sampling controls per utterance: B checked struct wn_sampling entries and their Philox streams,
  packed by wn_sampling_rows_pack (host only) into the table of struct wn_sampling_row that wn_generate_rows_chunk reads
  from device memory, and the flags that say what the union of the rows asks for."""

  def __init__(self, entries, streams, head, classes):
    B = len(entries)
    self.entries, self.streams = list(entries), (list(streams) if streams is not None else None)
    arr = (_lib.WnSampling * B)(*[_lib.WnSampling(e.temperature, e.top_k, e.seed, e.top_p) for e in entries])
    st = (C.c_uint64 * B)(*streams) if streams is not None else None
    self.host = (_lib.WnSamplingRow * B)()
    flags = C.c_int32(0)
    _lib.check(_lib.lib().wn_sampling_rows_pack(arr, st, B, head, classes, self.host, C.byref(flags)))
    self.flags = int(flags.value)

  def __len__(self):
    return len(self.entries)

  def device_table(self, device):
    """The table as a float tensor on `device`: one copy, made once per call or session."""
    return torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.float32).to(device)


def _as_rows(name, v):
  """None for a scalar argument, else the entries of a list, tuple, numpy array or 1-D tensor as Python values."""
  if isinstance(v, torch.Tensor):
    v = v.detach().cpu().numpy()
  if isinstance(v, np.ndarray):
    if v.ndim == 0:
      return None
    if v.ndim != 1:
      raise ValueError(f'{name} must be a scalar or a sequence of one entry per utterance (got shape {tuple(v.shape)})')
    return v.tolist()
  if isinstance(v, (list, tuple)):
    return [e.item() if isinstance(e, (np.generic, torch.Tensor)) else e for e in v]
  return None


class GenerationSession:
  """One sequence of WaveNet.generation_session(...), continued chunk by chunk (wn_generate_chunk).

  position: samples emitted so far.  exact: the session runs under exact_fp32() from here on (a chunk left the range
  of the split-precision kernels, or the sequence was begun in exact-fp32 mode, whose priming pass does not prepare
  what a split-precision step reads).  Otherwise a chunk runs in the math mode of the calling context.

  start: the index of the sequence's first sample; position begins there, the first chunk is
  wn_generate_rows_begin.  admit() puts new requests into rows of the running batch.

  origins: per row, the index its clock counts from -- row b draws sample t from the Philox counter
  (stream[b], t - origins[b]).  All zero unless the session was created with own_clock=True or a request admitted by admit_own_clock;
  row_positions is position - origins[b], the number of samples row b's present clock has counted."""

  def __init__(self, model, sampling, condition, window, batch_size, use_queues, deterministic, start=0, own_clock=False,
               frames=None, hop=None):
    L = _lib.lib()
    self._model, self._sampling, self._cond, self._window = model, sampling, condition, window
    # local conditioning: frames (B, F, Cin) and the samples per frame.  The step that emits sample g,
    # counted from `start`, uses frame g // hop; the priming pass uses frame 0 (`condition`).  A row an admission replaced
    # has left the schedule and keeps the condition set_condition gives it.
    self._frames, self._hop, self._frame = frames, hop, 0
    self._off_schedule = set()
    # per-row controls: the device table of the session, read by every chunk (and by the exact-fp32 rerun of one)
    self._rows = sampling.device_table(model._device) if isinstance(sampling, _RowControls) else None
    self._B, self._queued, self._det = int(batch_size), int(bool(use_queues)), int(bool(deterministic))
    # its own workspace (never model._workspace('gen')): other sessions and one-shot generate calls leave it alone
    self._ws = torch.zeros(int(L.wn_generate_workspace_floats(model._plan, self._B, self._queued)), dtype=torch.float32,
                           device=model._device)
    off, n = C.c_int64(), C.c_int64()
    _lib.check(L.wn_generate_state_range(model._plan, self._B, self._queued, C.byref(off), C.byref(n)))
    # what steps write and a continuation reads, and where a chunk's range-guard trip restores it from
    self._state = self._ws[off.value:off.value + n.value]
    self._shadow = torch.empty_like(self._state)
    self._slot = int(L.wn_generate_guard_slot(model._plan, self._B, self._queued))
    self._weights = (model.flat_params.data_ptr(), model._train_gen)
    self._failed = False
    self._start = int(start)
    self._admitted = False                 # admit() has replaced rows: the window no longer begins this batch
    self._scratch = {}                     # admit(): the scratch workspace of k rows, kept per k
    self.position = self._start
    self.exact = False
    # the rows' clock origins: None (every origin 0, the entry points without the argument) or B uint64 on the device,
    # read by every chunk like the table; own_clock: every row counts from `start`
    self._origin = None
    if own_clock:
      self._origin = torch.full((self._B,), self._start, dtype=torch.int64, device=model._device)
    self._origins = [self._start if own_clock else 0] * self._B

  @property
  def origins(self):
    return list(self._origins)

  @property
  def row_positions(self):
    return [self.position - o for o in self._origins]

  def generate(self, n):
    """The next (B, n, 1) samples, n >= 1.  A chunk that raises leaves position where it was.  With a frame schedule
    (local conditioning) the chunk is split at the frame boundaries and the condition table rewritten there; a chunk that
    would run past the last frame raises ValueError before anything is made."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
      raise ValueError(f'n must be an int >= 1 (got {n!r})')
    if self._frames is None:
      return self._generate_chunk(int(n))
    n, hop, F = int(n), self._hop, self._frames.shape[1]
    done = self.position - self._start
    if done + n > F * hop:
      raise ValueError(f'generation session: {done} + {n} samples run past the {F} condition frames of hop {hop} '
                       f'({F * hop} samples)')
    pieces = []
    while n > 0:
      g = self.position - self._start
      f = g // hop
      if f != self._frame:
        self._to_frame(f)
      take = min(n, (f + 1) * hop - g)
      pieces.append(self._generate_chunk(take))
      n -= take
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces, 1)

  def _to_frame(self, f):
    cond = self._frames[:, f, :].clone()
    if self._off_schedule:
      keep = torch.tensor(sorted(self._off_schedule), device=cond.device)
      cond[keep] = self._cond[keep]
    self._write_condition(cond)
    self._frame = f

  def _write_condition(self, cond):
    """self._cond = cond, and into the bias table of the workspace when the sequence has begun (the priming pass of a
    sequence that has not takes it from self._cond)."""
    m, L = self._model, _lib.lib()
    cond = cond.contiguous()
    if self.position > self._start:
      if not self._queued:
        raise NotImplementedError('set_condition needs use_queues=True: the sliding window maps the condition in every step')

      def run():
        _lib.check(L.wn_generate_set_condition(m._plan, _lib.ptr(m.flat_params), _lib.ptr(cond), self._B, 1, _lib.ptr(self._ws),
                                               self._ws.numel(), _lib.stream_ptr()))
      if self.exact:
        with m.exact_fp32():
          run()
      else:
        run()
    self._cond = cond

  def set_condition(self, condition, slots=None):
    """A new condition for running rows, from the next step on: (B, Cin), or (k, Cin) for the k rows `slots`.  Works on a
    globally conditioned model too.  On a session with a frame schedule the rows still on the schedule are rewritten at
    the next frame boundary; rows an admission replaced are driven by this call alone."""
    m = self._model
    self._check_usable()
    if self._cond is None:
      raise ValueError('set_condition: the model has no conditioning')
    condition = torch.as_tensor(condition, dtype=torch.float32, device=m._device)
    if condition.dim() == 3 and condition.shape[1] == 1:
      condition = condition[:, 0, :]
    cond = self._cond.clone()
    if slots is None:
      if tuple(condition.shape) != tuple(cond.shape):
        raise ValueError(f'condition must have shape {tuple(cond.shape)} (got {tuple(condition.shape)})')
      cond.copy_(condition)
    else:
      slot_list = [int(slots)] if isinstance(slots, (int, np.integer)) else [int(v) for v in slots]
      if any(v < 0 or v >= self._B for v in slot_list) or len(set(slot_list)) != len(slot_list):
        raise ValueError(f'slots must be distinct ints in [0, {self._B}) (got {slot_list})')
      if tuple(condition.shape) != (len(slot_list), cond.shape[1]):
        raise ValueError(f'condition must have shape {(len(slot_list), cond.shape[1])} (got {tuple(condition.shape)})')
      cond[torch.tensor(slot_list, device=m._device)] = condition
    self._write_condition(cond)

  def _generate_chunk(self, n):
    m, L, first = self._model, _lib.lib(), self.position
    self._check_usable()
    out = torch.empty(self._B, n, 1, dtype=torch.float32, device=m._device)
    begins = first == self._start            # the chunk that begins the sequence from the window

    def run():
      window = _lib.ptr(self._window) if begins else None
      if self._rows is not None:
        # (start = 0 runs the call it always ran)
        head = (m._plan, _lib.ptr(m.flat_params), window, _lib.ptr(self._cond), self._B, first, n, self._det, self._queued,
                _lib.ptr(self._rows), self._sampling.flags)
        tail = (_lib.ptr(out), _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr())
        if self._origin is not None:          # (the range-guard rerun below repeats with the same origins)
          entry = L.wn_generate_rows_begin_origin if begins and first > 0 else L.wn_generate_rows_chunk_origin
          _lib.check(entry(*head, _lib.ptr(self._origin), *tail))
        else:
          entry = L.wn_generate_rows_begin if begins and first > 0 else L.wn_generate_rows_chunk
          _lib.check(entry(*head, *tail))
        return
      _lib.check(L.wn_generate_chunk(m._plan, _lib.ptr(m.flat_params), window,
                                     _lib.ptr(self._cond), self._B, first, n, self._det, self._queued,
                                     C.byref(self._sampling), _lib.ptr(out), _lib.ptr(self._ws), self._ws.numel(),
                                     _lib.stream_ptr()))
    if self.exact or L.wn_debug_value(1) == 1:
      # exact fp32 cannot trip: no shadow copy, no host read
      with m.exact_fp32():
        run()
      if begins:
        self.exact = True
    else:
      if not begins:
        self._shadow.copy_(self._state)              # device to device, on the call's stream
      run()
      guard, watchdog = self._ws[self._slot:self._slot + 2].cpu()
      if int(watchdog.view(torch.int32)) != 0:
        self._failed = True
        raise RuntimeError(_RELAY_GAVE_UP.format(int(watchdog.view(torch.int32)), 'chunk'))
      if not (float(guard) < L.wn_range_limit()):
        # the tripped run has overwritten the raw-sample slots and ring slots of its steps: back to the state in front
        # of the chunk, the chunk again and everything after it on the exact-fp32 kernels (same seed: same draws); the
        # samples already handed out stand
        if not begins:
          self._state.copy_(self._shadow)
        with m.exact_fp32():
          run()
        m.generation_guard_trips += 1
        self.exact = True
    self.position = first + n
    return out

  def _check_usable(self):
    m = self._model
    if self._failed:
      raise RuntimeError('generation session: an earlier chunk failed; its state is invalid')
    if (m.flat_params.data_ptr(), m._train_gen) != self._weights:
      raise RuntimeError('generation session: the weights changed since the session was created (optimizer step, '
                         'set_weights, finalize_variable_values, or an averaged_weights() boundary); start a new session')

  def admit(self, slots, sample, condition=None, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None):
    """New requests into rows of the running batch (wn_generate_admit).  slots: an int or k distinct
    ints in [0, B); sample: (k, >= receptive_field, 1), the prompts; condition: (k, cond_inputs) on a conditioned net;
    the controls as in generate, scalars or k-sequences; stream: k ints, required.  Returns (k, 1, 1): every request's
    first sample, index position - 1 of the session; from the next chunk on row slots[j] is request j.  That row, from
    the returned sample on, is bit for bit a session of B = 1 begun with start = position - 1 from the request's own
    arguments; every other row is what it is without the admission.  Queued sessions with per-row controls only, after
    their first chunk.  The admitted rows draw on the session's clock; admit_own_clock gives them their own."""
    return self._admit(slots, sample, condition, temperature, top_k, seed, top_p, stream, False)

  def admit_own_clock(self, slots, sample, condition=None, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None):
    """admit, with the admitted rows on their own clock: they count from their own first sample --
    origin position - 1, so the returned sample is drawn from counter (stream, 0).  Such a row is then bit for bit
    model.generate(n, sample=prompt, use_queues=True, stream=[id], <its controls>) of the request alone, whichever slot,
    batch and position it was admitted at.  The other rows keep their clocks.  (A method of its own: admit's parameter
    list is what section 32 fixed.)"""
    return self._admit(slots, sample, condition, temperature, top_k, seed, top_p, stream, True)

  def _admit(self, slots, sample, condition, temperature, top_k, seed, top_p, stream, own_clock):
    m, L = self._model, _lib.lib()
    if not self._queued:
      raise RuntimeError('generation session: admit needs a session with use_queues=True (the sliding window has no '
                         'state rows to move)')
    if self._rows is None:
      raise RuntimeError('generation session: admit needs per-row controls (create the session with stream=)')
    if self.position < 1 or self.position == self._start:
      raise RuntimeError(f'generation session: admit needs position >= 1 and a begun sequence (position is {self.position}); '
                         'generate the first chunk before admitting')
    self._check_usable()
    one = not isinstance(slots, (list, tuple, np.ndarray, torch.Tensor))
    slot_list = [slots] if one else _as_rows('slots', slots)
    if slot_list is None or len(slot_list) < 1:
      raise ValueError(f'slots must be an int or a sequence of distinct ints (got {slots!r})')
    for j, v in enumerate(slot_list):
      if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < self._B:
        raise ValueError(f'slots[{j}] must be an int in [0, {self._B}) (got {v!r})')
      if v in slot_list[:j]:
        raise ValueError(f'slots[{j}] = {v} is a duplicate (the slots must be distinct)')
    slot_list = [int(v) for v in slot_list]
    k, rf = len(slot_list), m.receptive_field
    sample = torch.as_tensor(sample, dtype=torch.float32, device=m._device)
    if sample.dim() != 3 or sample.shape[0] != k or sample.shape[2] != 1 or sample.shape[1] < rf:
      raise ValueError(f'sample must have shape ({k}, >= {rf}, 1) for {k} slots (got {tuple(sample.shape)})')
    sample = sample[:, -rf:, :].contiguous()
    if m.conditioning is not None and condition is None:
      raise ValueError('Conditioning must be provided.')
    if condition is not None:
      condition = torch.as_tensor(condition, dtype=torch.float32, device=m._device).contiguous()
      if m.conditioning == 'local' and condition.dim() == 3 and condition.shape[1] == 1:
        condition = condition[:, 0, :].contiguous()          # a held condition as one frame, (k, 1, Cin)
      if self._cond is None or tuple(condition.shape) != (k,) + tuple(self._cond.shape[1:]):
        want = None if self._cond is None else (k,) + tuple(self._cond.shape[1:])
        raise ValueError(f'condition must have shape {want} (got {tuple(condition.shape)})')
    if stream is None:
      raise ValueError('stream is required: one Philox stream id per admitted request')
    new = m._sampling_rows(k, temperature, top_k, seed, top_p, stream, 2 ** m.bits, True)
    # the whole table again: the error text names the session's row, the flags are the new union
    old = self._sampling
    entries = list(old.entries)
    streams = list(old.streams) if old.streams is not None else list(range(self._B))
    for j, b in enumerate(slot_list):
      entries[b], streams[b] = new.entries[j], new.streams[j]
    table = _RowControls(entries, streams, _lib.HEADS[m.sampling_function], 2 ** m.bits)
    rows_k = new.device_table(m._device)
    if k not in self._scratch:
      self._scratch[k] = torch.zeros(int(L.wn_generate_admit_scratch_floats(m._plan, k)), dtype=torch.float32, device=m._device)
    scratch = self._scratch[k]
    first_out = torch.empty(k, 1, 1, dtype=torch.float32, device=m._device)
    slots_c = (C.c_int32 * k)(*slot_list)
    # a session without an origin array gets one of zeros at its first admit_own_clock, and keeps it
    origin = self._origin
    if origin is None and own_clock:
      origin = torch.zeros(self._B, dtype=torch.int64, device=m._device)
    origin_k = None if origin is None else torch.full((k,), self.position - 1 if own_clock else 0, dtype=torch.int64,
                                                      device=m._device)

    def run():
      head = (m._plan, _lib.ptr(m.flat_params), _lib.ptr(sample), _lib.ptr(condition), k, slots_c, self._B, self.position,
              self._det, _lib.ptr(rows_k), new.flags)
      tail = (_lib.ptr(first_out), _lib.ptr(self._ws), self._ws.numel(), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr())
      if origin_k is not None:              # (the range-guard rerun below repeats with the same origins)
        _lib.check(L.wn_generate_admit_origin(*head, _lib.ptr(origin_k), *tail))
      else:
        _lib.check(L.wn_generate_admit(*head, *tail))
    if self.exact or L.wn_debug_value(1) == 1:
      with m.exact_fp32():
        run()
    else:
      run()
      slot = int(L.wn_generate_guard_slot(m._plan, k, 1))
      if not (float(scratch[slot]) < L.wn_range_limit()):
        # the admission's priming pass left the range of the split-precision kernels: again on the exact-fp32 kernels
        # (the move overwrites the same rows: nothing to restore), and the session stays there
        with m.exact_fp32():
          run()
        m.generation_guard_trips += 1
        self.exact = True
    # the session's own records: rows slots[j] of the device table (in place: the chunks read this tensor) and of the condition
    self._sampling = table
    self._rows.copy_(table.device_table(m._device))
    if origin is not None:
      origin[torch.tensor(slot_list, device=m._device)] = origin_k
      self._origin = origin
      for b in slot_list:
        self._origins[b] = self.position - 1 if own_clock else 0
    if condition is not None:
      if not self._admitted:
        self._cond = self._cond.clone()          # (the caller's tensor stays as it is)
      self._cond[torch.tensor(slot_list, device=m._device)] = condition
      self._off_schedule.update(slot_list)         # (a frame schedule per admitted request is a follow-up: section 36)
    self._admitted = True
    return first_out

  def reset(self):
    """Back to the start: the next chunk begins the sequence again from the window, on the same workspace (and with the
    same origins)."""
    if self._admitted:
      raise RuntimeError('generation session: reset after admit is not possible (the rows the window began are gone); '
                         'start a new session')
    self.position = self._start
    self._failed = False


class WaveNet(torch.nn.Module):
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

  def averaged_weights(self):
    """Context manager (Adam(use_ema=True)): inside it every pass -- call, logits, test_step, generate, get_weights,
    io.save_weights(model, '*.weights.h5') -- runs on the optimizer's exponential moving average of the weights.  The
    storage behind ``flat_params`` is swapped for the average (every pass takes the parameters as a pointer and rebuilds
    its weight images from it on each call): no copy, no second plan.  On exit, also through an exception, the raw
    weights are back bit for bit.  Training, set_weights and training checkpoints raise RuntimeError inside it."""
    import contextlib

    @contextlib.contextmanager
    def _cm():
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
    return _cm()

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
    run()
    # the pass's guard float, copied out of the shared workspace on the stream (a later pass on the same workspace -- another
    # call, a test_step -- overwrites the slot; this one-float copy is what range_tripped_last_forward() reads)
    slot = L.wn_plan_range_slot(self._plan, B, T, int(training))
    self._last_fwd = (ws[slot:slot + 1].clone(), training)
    if self.range_check and L.wn_debug_value(1) != 1 and self._guard_over(*self._last_fwd):
      with self.exact_fp32():
        run()
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
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
      return dist.get_world_size()
    return 1

  @staticmethod
  def _rank():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
      return dist.get_rank()
    return 0

  def training_intermediate(self, what: int, idx: int, B: int, T: int):
    """View on an intermediate the last loss_and_grads call (B utterances, T predicted samples) left in the
    training workspace (wn_debug_ws_region; parity tests compare these with the oracle's autograd values).
    what 0..12 as listed in include/wn_hip.h; 13: GP[b][i], the gradient at the pre-activation output of inner conv i of
    block b (idx = b * (layers_per_block - 1) + i, as for 11); 14: XD[idx], the dropped copy of block input idx, which
    exists only with dropout > 0 (ValueError otherwise, as for every absent region)."""
    off, ln = C.c_int64(), C.c_int64()
    # (local conditioning: the regions behind the conditioning's lie where the pass with its F frames carved them)
    try:
      self._arm_frames(self._last_train_frames)
      _lib.check(_lib.lib().wn_debug_ws_region(self._plan, B, T, what, idx, C.byref(off), C.byref(ln)))
    finally:
      self._arm_frames(0)
    return self._ws['train'][off.value:off.value + ln.value]

  def exact_fp32(self):
    """Context manager: the calling thread's launches use the exact-fp32 MFMA kernels (no fp16 hi|lo operand split)."""
    import contextlib

    @contextlib.contextmanager
    def _cm():
      L = _lib.lib()
      prev = L.wn_debug_value(1)
      L.wn_debug_set(1, 1)
      try:
        yield
      finally:
        L.wn_debug_set(1, prev)
    return _cm()

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
    try:
      if weights is not None:
        _lib.check(L.wn_plan_arm_row_weights(self._plan, _lib.ptr(weights), B * T))
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
      if weights is not None:
        L.wn_plan_arm_row_weights(self._plan, None, 0)
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
    lv, pending, y_true, sample = self._train_step_once(data, sample_weight)
    if lv[2] > 0:                                    # tripped on some replica -> on all of them after the SUM
      self.train_guard_trips += 1
      self.optimizer.undo_last_apply()               # (iterations, accumulated) as before the skipped launch
      self._drop_step -= 1 if self.dropout > 0 else 0
      with self.exact_fp32():
        lv, pending, y_true, sample = self._train_step_once(data, sample_weight)
    for m, v in zip(pending, lv[3:]):
      m.commit(v)
    for metric in self.metrics:
      if metric.name == 'loss':
        metric.update_state(lv[0])
      elif metric.name == 'reg_loss':
        metric.update_state(lv[1])
      elif not hasattr(metric, 'update_state_device'):
        metric.update_state(y_true, sample, **wkw)
    return {m.name: m.result() for m in self.metrics}

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
    from . import dp
    if not self.built:
      try:
        self._split_inputs(data)                        # Keras builds on the first call (the condition width fixes the shapes)
      finally:
        self._arm_frames(0)                             # (a local condition arms its frames: loss_and_grads does so itself)
    compiled = self._metrics_from_compilation
    want_metric = len(compiled) > 0
    dev_metrics = [m for m in compiled if hasattr(m, 'update_state_device')][:self._TAIL_METRICS]
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
    from . import dp
    sample_weight = self._check_sample_weight(data, sample_weight)
    x, cond = self._split_inputs(data)
    B, T = x.shape[0], x.shape[1] - 1
    weights = self._row_weights(sample_weight, B, T)
    wkw = {} if weights is None else {'sample_weight': weights}
    world = self._world()
    L = _lib.lib()
    ws = self._workspace('fwd', L.wn_plan_workspace_floats(self._plan, B, T, 0))
    compiled = self._metrics_from_compilation
    want_metric = len(compiled) > 0
    dev_metrics = [m for m in compiled if hasattr(m, 'update_state_device')][:self._TAIL_METRICS]
    vec = torch.zeros(3 + len(dev_metrics), dtype=torch.float32, device=self._device)
    pred = torch.empty(B, T, self.spec.out_channels, dtype=torch.float32, device=self._device) if want_metric else None

    def once():
      try:
        if weights is not None:
          _lib.check(L.wn_plan_arm_row_weights(self._plan, _lib.ptr(weights), B * T))
        _lib.check(L.wn_eval_loss(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                                  B * world, _lib.ptr(vec), _lib.ptr(pred), _lib.ptr(ws), ws.numel(),
                                  _lib.stream_ptr()))
      finally:
        if weights is not None:
          L.wn_plan_arm_row_weights(self._plan, None, 0)
      sample = self.sample_waveform(pred) if want_metric else None
      # as in train_step: device-side metric reductions into the same vector, ONE collective (loss sums over the replicas;
      # reg_loss unused; flag: any replica; metrics: replica means), ONE device-to-host read
      for i, m in enumerate(dev_metrics):
        m.update_state_device(x[:, 1:, :], sample, out=vec[3 + i:4 + i], scale=1.0 / world, **wkw)
      dp.allreduce_bucket(vec)
      return vec.tolist(), sample
    lv, sample = once()
    if lv[2] > 0:
      self.test_guard_trips += 1
      with self.exact_fp32():
        lv, sample = once()
    for m, v in zip(dev_metrics, lv[3:]):
      m.commit(v)
    for metric in self.metrics:
      if metric.name == 'loss':
        metric.update_state(lv[0])
      elif metric.name == 'reg_loss':
        continue
      elif not hasattr(metric, 'update_state_device'):
        metric.update_state(x[:, 1:, :], sample, **wkw)
    return {m.name: m.result() for m in self.metrics if m.name != 'reg_loss'}

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
      try:
        if weights is not None:
          _lib.check(L.wn_plan_arm_row_weights(self._plan, _lib.ptr(weights), B * T))
        _lib.check(L.wn_score(self._plan, _lib.ptr(self.flat_params), _lib.ptr(x), _lib.ptr(cond), B, T, _lib.ptr(nll),
                              _lib.ptr(weight), _lib.ptr(rows), _lib.ptr(flag), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
      finally:
        if weights is not None:
          L.wn_plan_arm_row_weights(self._plan, None, 0)
      return float(flag) > 0
    if once():
      self.score_guard_trips += 1
      with self.exact_fp32():
        once()
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

  def _sampling(self, temperature, top_k, seed, classes, top_p=1.0):
    """The sampling controls of a stochastic draw as the C struct (semantics: include/wn_hip.h, struct wn_sampling),
    checked as the library checks them, before any work is queued.  classes: row length of a categorical prediction.
    top_p: a real number in (0, 1]; 1.0 is off."""
    if isinstance(top_k, bool) or not isinstance(top_k, int):
      raise ValueError(f'top_k must be an int (got {top_k!r})')
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
      raise ValueError(f'seed must be an int or None (got {seed!r})')
    t = np.float32(temperature)
    with np.errstate(all='ignore'):
      if not (t > 0 and np.isfinite(t) and np.isfinite(np.float32(1.0) / t)):
        raise ValueError(f'temperature must be finite and > 0 with a finite reciprocal (got {temperature!r})')
    if not 0 <= top_k < 2**31:
      raise ValueError(f'top_k must be >= 0 (got {top_k})')
    if top_k > 0 and self.sampling_function != 'categorical':
      raise ValueError(f'top_k applies to the categorical head only (got top_k = {top_k} with {self.sampling_function})')
    if 0 < top_k < classes and classes > _lib.WN_TOP_K_MAX_CLASSES:
      raise ValueError(f'top_k is offered for up to {_lib.WN_TOP_K_MAX_CLASSES} classes (got {classes})')
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float, np.integer, np.floating)):
      raise ValueError(f'top_p must be a real number in (0, 1] (got {top_p!r})')
    tp = np.float32(top_p)
    if not (float(top_p) > 0 and tp > 0 and tp <= 1):        # NaN fails; so does a value that rounds to 0 in fp32
      raise ValueError(f'top_p must lie in (0, 1] (got {top_p!r})')
    if tp < 1 and self.sampling_function != 'categorical':
      raise ValueError(f'top_p applies to the categorical head only (got top_p = {top_p} with {self.sampling_function})')
    if tp < 1 and classes > _lib.WN_TOP_K_MAX_CLASSES:
      raise ValueError(f'top_p is offered for up to {_lib.WN_TOP_K_MAX_CLASSES} classes (got {classes})')
    key = 0x0402 if seed is None else seed & 0xFFFFFFFFFFFFFFFF
    return _lib.WnSampling(float(t), top_k, key, float(tp))

  def _sampling_rows(self, batch_size, temperature, top_k, seed, top_p, stream, classes, have_sample=True):
    """Sampling controls given per utterance.  Each of temperature, top_k, seed and top_p is a
    scalar or a sequence (list, tuple, numpy array, 1-D tensor) of batch_size entries, entry b for utterance b; scalars
    beside sequences are broadcast.  Every row is checked by _sampling, and the error names the row.  stream: None, or
    batch_size ints in [0, 2**63), the row word of utterance b's Philox counter (None: b).
    Returns the one struct wn_sampling of today's scalar entry points when every row is equal and stream is None --
    such a call runs exactly the code it ran before -- and a _RowControls otherwise."""
    B = int(batch_size)
    cols = {}
    for name, v in (('temperature', temperature), ('top_k', top_k), ('seed', seed), ('top_p', top_p)):
      rows = _as_rows(name, v)
      if rows is not None and len(rows) != B:
        raise ValueError(f'{name} has {len(rows)} entries for a batch of {B} utterances')
      cols[name] = rows if rows is not None else [v] * B
    entries = []
    for b in range(B):
      T = cols['temperature'][b]
      if isinstance(T, bool):
        raise ValueError(f'row {b}: temperature must be a real number (got {T!r})')
      try:
        entries.append(self._sampling(T, cols['top_k'][b], cols['seed'][b], classes, cols['top_p'][b]))
      except ValueError as e:
        raise ValueError(f'row {b}: {e}') from None
    streams = None
    if stream is not None:
      streams = _as_rows('stream', stream)
      if streams is None:
        raise ValueError(f'stream must be None or a sequence of one int per utterance (got {stream!r})')
      if len(streams) != B:
        raise ValueError(f'stream has {len(streams)} entries for a batch of {B} utterances')
      for b, v in enumerate(streams):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 63:
          raise ValueError(f'row {b}: stream must be an int in [0, 2**63) (got {v!r})')
      if not have_sample:
        raise ValueError('stream requires `sample`: a caller who names the Philox streams owns the prompt')
    # (compared as the library reads them: top_k >= classes and top_p = 1 are off)
    key = lambda e: (e.temperature, 0 if e.top_k >= classes else e.top_k, e.seed, 0.0 if e.top_p >= 1 else e.top_p)
    if streams is None and all(key(e) == key(entries[0]) for e in entries):
      return entries[0]
    return _RowControls(entries, streams, _lib.HEADS[self.sampling_function], classes)

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
  def generate(self, length, batch_size: int = 1, condition=None, sample=None,
               use_queues=False, deterministic=False, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None, hop=None):
    """src/model.py:258-307 (intended semantics; the reference's kwarg / rank bugs are not
    reproduced).  Returns (B, length, 1).
    temperature / top_k / seed / top_p (additions) as in sample_waveform; an int seed is the Philox key of
    the draws and seeds the initial noise window when `sample` is None.  seed=None is seed=0x0402.
    Per utterance: each of the four may be a sequence of B entries (list, tuple, numpy array, 1-D
    tensor), entry b for utterance b; a scalar beside sequences is broadcast.  Row b of the result is bit for bit row b
    of the call at the same B whose scalar controls are row b's.  Without `sample`, row b of the noise window is row b
    of the window the scalar call with seed[b] draws.  stream: None, or B ints in [0, 2**63) -- utterance b draws from
    the Philox counter row stream[b] instead of b, so a request keeps its draws whichever batch slot it lands in
    (requires `sample`).  deterministic stays one flag for the call."""
    condition, frames, hop = self._local_frames(condition, hop, use_queues, length)
    if frames is not None:
      # a frame schedule (local conditioning): the sequence as a session, split at the frame boundaries -- the chunks of a
      # sequence, concatenated, are the one call bit for bit
      session = self.generation_session(batch_size=batch_size, condition=frames, sample=sample, use_queues=use_queues,
                                        deterministic=deterministic, temperature=temperature, top_k=top_k, seed=seed,
                                        top_p=top_p, stream=stream, hop=hop)
      if int(length) < 1:
        return torch.empty(session._B, 0, 1, dtype=torch.float32, device=self._device)
      return session.generate(int(length))
    sampling, condition, sample, batch_size = self._generation_args(batch_size, condition, sample, deterministic,
                                                                    temperature, top_k, seed, top_p, stream)
    L = _lib.lib()
    ws = self._workspace('gen', L.wn_generate_workspace_floats(self._plan, batch_size, int(bool(use_queues))))
    out = torch.empty(batch_size, int(length), 1, dtype=torch.float32, device=self._device)
    rows = sampling.device_table(self._device) if isinstance(sampling, _RowControls) else None
    def run():
      if rows is not None:      # (the range-guard rerun below repeats with the same table)
        _lib.check(L.wn_generate_rows_chunk(self._plan, _lib.ptr(self.flat_params), _lib.ptr(sample), _lib.ptr(condition),
                                            batch_size, 0, int(length), int(bool(deterministic)), int(bool(use_queues)),
                                            _lib.ptr(rows), sampling.flags, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                            _lib.stream_ptr()))
        return
      _lib.check(L.wn_generate_sampled(self._plan, _lib.ptr(self.flat_params), _lib.ptr(sample), _lib.ptr(condition),
                                       batch_size, int(length), int(bool(deterministic)), int(bool(use_queues)),
                                       C.byref(sampling), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    run()
    # range guard (one host read; the caller reads the samples anyway): an activation beyond the fp16 range of the
    # split-precision kernels -> the whole call again on the exact-fp32 kernels (same seed: same draws)
    if length > 0 and L.wn_debug_value(1) != 1:
      slot = L.wn_generate_guard_slot(self._plan, batch_size, int(bool(use_queues)))
      guard, watchdog = ws[slot:slot + 2].cpu()
      if int(watchdog.view(torch.int32)) != 0:
        raise RuntimeError(_RELAY_GAVE_UP.format(int(watchdog.view(torch.int32)), 'call'))
      if not (float(guard) < L.wn_range_limit()):
        self.generation_guard_trips += 1
        with self.exact_fp32():
          run()
    return out

  def _local_frames(self, condition, hop, use_queues, length=None):
    """Local conditioning in generation: condition (B, F) or (B, F, Cin) and hop, the samples per
    frame.  Returns (the priming pass's condition = frame 0 as (B, Cin), frames (B, F, Cin) or None, hop): None is a held
    condition with no end (F == 1 without hop).  Other models: (condition, None, None)."""
    if self.conditioning != 'local' or condition is None:
      if hop is not None:
        raise ValueError('hop belongs to conditioning=\'local\' with a condition of frames')
      return condition, None, None
    condition = torch.as_tensor(condition, dtype=torch.float32, device=self._device)
    if condition.dim() == 2:
      condition = condition[:, :, None]
    if condition.dim() != 3 or condition.shape[1] < 1:
      raise ValueError('condition must have shape (batch, frames) or (batch, frames, n_cond)')
    F = int(condition.shape[1])
    first = condition[:, 0, :].contiguous()
    if hop is None:
      if F > 1:
        raise ValueError(f'hop is required with {F} condition frames: the samples generated per frame')
      return first, None, None
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1:
      raise ValueError(f'hop must be an int >= 1 (got {hop!r})')
    if F > 1 and not use_queues:
      raise NotImplementedError('a frame schedule needs use_queues=True: the reference\'s sliding window re-upsamples the whole '
                                'condition onto the window at every step, which defines nothing usable')
    if length is not None and int(length) > F * int(hop):
      raise ValueError(f'length {int(length)} runs past the {F} condition frames of hop {int(hop)} ({F * int(hop)} samples)')
    return first, condition.contiguous(), int(hop)

  def _generation_args(self, batch_size, condition, sample, deterministic, temperature, top_k, seed, top_p, stream=None):
    """The argument handling of generate and generation_session: the sampling controls checked, condition and sample on
    the device, the batch size they imply, the initial window (the last receptive_field samples of `sample`, or zeros /
    seeded noise), the model built.  Returns (sampling, condition, window, batch_size); sampling is the struct
    wn_sampling of the call, or a _RowControls when the controls differ between utterances or `stream` is given."""
    per_row = stream is not None or any(_as_rows(n, v) is not None for n, v in (
        ('temperature', temperature), ('top_k', top_k), ('seed', seed), ('top_p', top_p)))
    # (scalars: checked first, as ever; per utterance: once the batch size is known, below)
    sampling = None if per_row else self._sampling(temperature, top_k, seed, 2 ** self.bits, top_p)
    if self.conditioning is not None and condition is None:
      raise ValueError('Conditioning must be provided.')
    if condition is not None:
      condition = torch.as_tensor(condition, dtype=torch.float32, device=self._device).contiguous()
    if sample is not None:
      sample = torch.as_tensor(sample, dtype=torch.float32, device=self._device).contiguous()
    if condition is not None and sample is not None:
      if condition.shape[0] != sample.shape[0]:
        raise ValueError('Condition and sample must have same batch size.')
    if condition is not None:
      batch_size = condition.shape[0]
    if sample is not None:
      batch_size = sample.shape[0]
    rf = self.receptive_field
    if per_row:
      sampling = self._sampling_rows(batch_size, temperature, top_k, seed, top_p, stream, 2 ** self.bits, sample is not None)
    if sample is None:
      if deterministic:
        sample = torch.zeros(batch_size, rf, 1, device=self._device)
      elif isinstance(sampling, _RowControls):
        # row b of the (B, rf, 1) noise the scalar call with seed[b] draws: one host randn per distinct seed
        noise = {}
        for e in sampling.entries:
          if e.seed not in noise:
            noise[e.seed] = torch.randn(batch_size, rf, 1, generator=torch.Generator(device='cpu').manual_seed(int(e.seed)))
        sample = torch.stack([noise[e.seed][b] for b, e in enumerate(sampling.entries)]).to(self._device)
      else:
        g = torch.Generator(device='cpu').manual_seed(int(sampling.seed))
        sample = torch.randn(batch_size, rf, 1, generator=g).to(self._device)
    if sample.shape[1] != rf:
      if sample.shape[1] < rf:
        raise ValueError('sample must hold at least receptive_field samples')
      sample = sample[:, -rf:, :].contiguous()
    if not self.built:
      self.build([tuple(sample.shape), tuple(condition.shape)] if condition is not None else tuple(sample.shape))
    return sampling, condition, sample, batch_size

  def generation_session(self, batch_size: int = 1, condition=None, sample=None, use_queues=False, deterministic=False,
                         temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None, start=0, own_clock=False, hop=None):
    """A sequence made in pieces: the arguments of generate without `length`, with the same checks (per-utterance
    controls and `stream` included: the session keeps the device table of its rows).  The chunks of
    session.generate(n), concatenated, are bit for bit generate(total, same arguments).  The
    session owns its workspace and is bound to the weights as they are now: after an optimizer step, set_weights,
    finalize_variable_values, or entering / leaving averaged_weights() its generate raises RuntimeError.
    start: an int >= 0, the index of the sequence's first sample -- the draw of sample t uses the
    Philox counter (stream, t), so a sequence begun at `start` draws what a request admitted at that position draws
    (GenerationSession.admit).  start > 0 needs per-row controls: passing stream= is enough.
    own_clock=True: every row counts from `start` -- sample t is drawn from counter (stream, t - start),
    so the session is bit for bit the session with start=0, stochastic draws included.  Needs per-row controls too.
    hop (conditioning='local'): the samples per condition frame; session.generate splits its chunks at
    the frame boundaries and raises ValueError at the chunk that would run past the last frame."""
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
      raise ValueError(f'start must be an int >= 0 (got {start!r})')
    if not isinstance(own_clock, bool):
      raise ValueError(f'own_clock must be a bool (got {own_clock!r})')
    condition, frames, hop = self._local_frames(condition, hop, use_queues)
    sampling, condition, window, batch_size = self._generation_args(batch_size, condition, sample, deterministic,
                                                                    temperature, top_k, seed, top_p, stream)
    if start > 0 and not isinstance(sampling, _RowControls):
      raise ValueError('start > 0 needs per-row sampling controls: pass stream= (one Philox stream id per utterance)')
    if own_clock and not isinstance(sampling, _RowControls):
      raise RuntimeError('generation session: own_clock needs per-row controls (create the session with stream=)')
    return GenerationSession(self, sampling, condition, window, batch_size, use_queues, deterministic, int(start), own_clock,
                             frames, hop)

  def generate_stream(self, length, chunk, **kwargs):
    """Generator over a generation_session(**kwargs): yields (B, min(chunk, rest), 1) tensors until `length` samples are
    out; concatenated they are generate(length, **kwargs).  The arguments are checked here, not at the first next()."""
    length, chunk = int(length), int(chunk)
    if chunk < 1:
      raise ValueError(f'chunk must be >= 1 (got {chunk})')
    session = self.generation_session(**kwargs)

    def pieces():
      while session.position < length:
        yield session.generate(min(chunk, length - session.position))
    return pieces()

  def compute_receptive_field(self, sampling_frequency):
    """src/model.py:553-556."""
    return self.receptive_field / sampling_frequency
