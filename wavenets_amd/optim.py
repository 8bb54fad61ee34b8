"""Keras-semantics Adam with per-tensor clipnorm, fused on the GPU (train.py:225-226).

``Adam(learning_rate=5e-4, clipnorm=1.0)`` mirrors ``tf.keras.optimizers.Adam``: epsilon
(1e-7) is added to sqrt(v) outside the bias correction, each gradient tensor is clipped to
``clipnorm`` independently (tf.clip_by_norm) before the moment update.

Under data parallelism the order of clip and SUM matters.  ``clip_before_reduce=False`` (default) clips the reduced
gradient inside the Adam launch; ``clip_before_reduce=True`` clips every replica's own gradient ahead of the all-reduce
(``clip_local_gradients``, the Keras 3 order) and the Adam launch then clips nothing.  The flag is configuration, not
state: checkpoints do not carry it.

``use_ema=True`` (Keras's keyword, with ``ema_momentum`` and ``ema_overwrite_frequency``) keeps an exponential moving
average of the weights in ``ema``, written by the same launch as the update: after the parameter update of the 1-based
step ``t``, ``ema = p`` at ``t == 1`` and ``ema = ema + (p - ema) * (1 - ema_momentum)`` afterwards; every
``ema_overwrite_frequency``-th step then sets ``p = ema``.  The average is state: ``.weights.npz`` checkpoints carry it
(``adam_ema``).  ``WaveNet.averaged_weights()`` runs the model's passes on it.

The other Keras keywords ride in a sibling of the same launch (``wn_adam_step_ext``), picked only when one of them is on:

* ``global_clipnorm=c``: one factor ``c / max(N, c)`` for every tensor, ``N`` the norm of the whole gradient; a non-finite
  norm makes every clipped gradient NaN (Keras's poisoning).  ``clipvalue=c``: elementwise clamp to ``[-c, c]``, NaN kept.
  At most one of ``clipnorm``, ``global_clipnorm`` and ``clipvalue`` may be set.  With ``clip_before_reduce`` both are
  applied to the replica's own gradient ahead of the all-reduce (``clip_local_gradients``), as ``clipnorm`` is.
* ``weight_decay=wd`` (AdamW): ``p = p - (p * wd) * lr`` ahead of the Adam update of the same step, on every tensor not
  named to ``exclude_from_weight_decay`` (before ``build``, as in Keras).  It never enters the gradient or the moments.
* ``amsgrad=True``: ``vhat = max(vhat, v)`` is one more state stream (``adam_vhat`` in checkpoints) and the denominator.

``gradient_accumulation_steps=k`` (Keras's keyword; ``None`` or an int >= 2): ``apply_gradients`` is still called once per
micro-step.  Calls 1 .. k-1 of a cycle only store the gradient (``wn_grad_accumulate``); call k forms the mean
``g = (g_k + acc) / k``, leaves it in ``model.flat_grads``, clips THAT with whichever clip is set (Keras 3
``base_optimizer``: divide, then ``_clip_gradients``), runs the Adam step exactly as it is -- decay, amsgrad and ema
unchanged -- and starts a new cycle.  ``iterations`` stays the number of UPDATES applied: Adam's ``t``, the clock of
``ema_overwrite_frequency`` and ``adam_iterations`` in checkpoints; ``accumulated`` (0 .. k-1) is the number of micro-steps
held in the accumulator.  The accumulator ``accum`` is state (``adam_accum`` / ``adam_accumulated`` in checkpoints): one fp32
buffer of the parameters' size that ``build`` allocates only with ``k``; the first micro-step of a cycle overwrites it (no
memset, no read of what it held).  fp32 throughout, in a fixed order: ``acc = g_1``, then ``acc = acc + g_j``, then
``(g_k + acc) / (float)k``, one correctly rounded operation per element and nothing fused.  A micro-step whose range flag is
up reaches neither buffer.  Not with ``clip_before_reduce``: the clips act on the accumulated mean and there is no
per-replica, per-micro-batch clip to define.
"""
from __future__ import annotations

import ctypes as C
import math
import re

import torch

from . import _lib


class Adam:
  def __init__(self, learning_rate: float = 0.001, beta_1: float = 0.9, beta_2: float = 0.999,
               epsilon: float = 1e-7, clipnorm=None, clip_before_reduce: bool = False,
               use_ema: bool = False, ema_momentum: float = 0.99, ema_overwrite_frequency=None,
               global_clipnorm=None, clipvalue=None, weight_decay=None, amsgrad: bool = False,
               gradient_accumulation_steps=None):
    if not isinstance(clip_before_reduce, bool):
      raise ValueError(f'clip_before_reduce must be a bool, got {clip_before_reduce!r}')
    if not isinstance(use_ema, bool):
      raise ValueError(f'use_ema must be a bool, got {use_ema!r}')
    if use_ema:                                      # as in Keras, the other two are not looked at without the flag
      if isinstance(ema_momentum, bool) or not isinstance(ema_momentum, (int, float)) or \
          not math.isfinite(ema_momentum) or not 0.0 <= ema_momentum <= 1.0:
        raise ValueError(f'ema_momentum must be a finite float in [0, 1], got {ema_momentum!r}')
      f = ema_overwrite_frequency
      if f is not None and (isinstance(f, bool) or not isinstance(f, int) or f < 1):
        raise ValueError(f'ema_overwrite_frequency must be None or an int >= 1, got {f!r}')
    if sum(c is not None for c in (clipnorm, global_clipnorm, clipvalue)) > 1:
      raise ValueError('Only one of `clipnorm`, `clipvalue` and `global_clipnorm` can be set. Received: '
                       f'clipnorm={clipnorm!r}, clipvalue={clipvalue!r}, global_clipnorm={global_clipnorm!r}')
    for name, c in (('global_clipnorm', global_clipnorm), ('clipvalue', clipvalue)):
      if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or not c > 0):
        raise ValueError(f'{name} must be None or a finite number > 0, got {c!r}')
    wd = weight_decay
    if wd is not None and (isinstance(wd, bool) or not isinstance(wd, (int, float)) or not math.isfinite(wd) or wd < 0):
      raise ValueError(f'weight_decay must be None or a finite number >= 0, got {wd!r}')
    if not isinstance(amsgrad, bool):
      raise ValueError(f'amsgrad must be a bool, got {amsgrad!r}')
    k = gradient_accumulation_steps
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 2):
      raise ValueError(f'`gradient_accumulation_steps` must be an integer >= 2. Received: gradient_accumulation_steps={k!r}')
    if k is not None and clip_before_reduce:
      raise ValueError('gradient_accumulation_steps and clip_before_reduce=True cannot be combined: with accumulation the '
                       'clips act on the accumulated mean, there is no per-replica, per-micro-batch clip')
    self.learning_rate = float(learning_rate)
    self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
    self.clipnorm = clipnorm
    self.clip_before_reduce = clip_before_reduce
    self.use_ema, self.ema_momentum, self.ema_overwrite_frequency = use_ema, ema_momentum, ema_overwrite_frequency
    self.global_clipnorm = None if global_clipnorm is None else float(global_clipnorm)
    self.clipvalue = None if clipvalue is None else float(clipvalue)
    self.weight_decay = None if weight_decay is None else float(weight_decay)
    self.amsgrad = amsgrad
    self._exclude_vars, self._exclude_names = [], []
    self.gradient_accumulation_steps = k
    self.iterations = 0                              # updates applied (with accumulation: not calls)
    self.accumulated = 0                             # micro-steps held in ``accum``, 0 .. k-1
    self._before = (0, 0)                            # (iterations, accumulated) ahead of the last apply_gradients
    self._mean_formed = False                        # form_mean() ran for the micro-step that apply_gradients finishes
    self.m = self.v = self.vhat = self.ema = self.accum = self._scratch = self._decay_flags = None
    self.ext_steps = 0                               # steps that took wn_adam_step_ext (the default path never counts)

  def exclude_from_weight_decay(self, var_list=None, var_names=None):
    """Keras's method: tensors that ``weight_decay`` leaves alone.  ``var_list``: tensors of ``model.trainable_variables``
    (matched by storage and offset); ``var_names``: patterns, ``re.search``ed in ``model.variable_names``.  Before ``build``
    only; calls add up."""
    if self.m is not None:
      raise ValueError('This optimizer has already been built: `exclude_from_weight_decay()` can only be called before '
                       'the optimizer is built.')
    for t in var_list or []:
      if not isinstance(t, torch.Tensor):
        raise ValueError(f'exclude_from_weight_decay: var_list holds {type(t).__name__}, not a tensor of the model')
      self._exclude_vars.append(t)
    for pat in var_names or []:
      if not isinstance(pat, str):
        raise ValueError(f'exclude_from_weight_decay: var_names holds {pat!r}, not a string')
      re.compile(pat)
      self._exclude_names.append(pat)

  def decays(self, model):
    """Per tensor of ``model.variable_names``: does ``weight_decay`` touch it?  (All False without a weight decay.)"""
    if not self.weight_decay:
      return [False] * len(model.variable_names)
    excluded = [any(re.search(pat, name) for pat in self._exclude_names) for name in model.variable_names]
    if self._exclude_vars:
      params = model.trainable_variables
      for t in self._exclude_vars:
        hit = [i for i, q in enumerate(params) if q is t or (
            q.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() and q.storage_offset() == t.storage_offset()
            and q.numel() == t.numel())]
        if not hit:
          raise ValueError('exclude_from_weight_decay: a tensor of var_list is not a trainable variable of this model')
        excluded[hit[0]] = True
    return [not e for e in excluded]

  def build(self, model):
    """Allocate the moment buffers (src/model.py:211 optimizer.build)."""
    if self.m is None or self.m.numel() != model.flat_params.numel():
      self.m = torch.zeros_like(model.flat_params.data)
      self.v = torch.zeros_like(model.flat_params.data)
      self._scratch = torch.zeros(len(model.variable_names) + 8, dtype=torch.float32,
                                  device=model.flat_params.device)
      self.ema = self.vhat = self.accum = self._decay_flags = None
      self.accumulated = 0                           # another model's sums are gone with the buffer: a new cycle
    if self.gradient_accumulation_steps and self.accum is None:
      self.accum = torch.empty_like(model.flat_params.data)        # the first micro-step of a cycle overwrites it
    if self.amsgrad and self.vhat is None:
      self.vhat = torch.zeros_like(model.flat_params.data)
    if self.weight_decay and self._decay_flags is None and (self._exclude_vars or self._exclude_names):
      # the per-tensor on/off table of the decay, beside the scratch (no table: every tensor decays)
      self._decay_flags = torch.tensor([int(d) for d in self.decays(model)], dtype=torch.int32).to(model.flat_params.device)
    if self.use_ema and self.ema is None:
      # a copy of the current weights: an optimizer that starts averaging at t > 1 (a resume from a checkpoint without
      # an average) averages from the loaded weights
      self.ema = model.flat_params.data.clone()

  def clip_local_gradients(self, model):
    """``clip_before_reduce``: clip this replica's ``model.flat_grads`` per tensor, in place, ahead of the all-reduce.
    ``global_clipnorm`` and ``clipvalue`` likewise (the sum of squares, then one factor for all tensors; an elementwise
    clamp).  Nothing happens without the flag or without a clip."""
    if not self.clip_before_reduce:
      return
    if self.global_clipnorm or self.clipvalue:
      self.build(model)
      mode, c = (_lib.WN_CLIP_GLOBAL_NORM, self.global_clipnorm) if self.global_clipnorm else (_lib.WN_CLIP_VALUE, self.clipvalue)
      _lib.check(_lib.lib().wn_clip_gradients_ext(model._plan, _lib.ptr(model.flat_grads), mode, c, _lib.ptr(self._scratch),
                                                  _lib.stream_ptr()))
      return
    if not self.clipnorm:
      return
    self.build(model)
    _lib.check(_lib.lib().wn_clip_gradients(model._plan, _lib.ptr(model.flat_grads), float(self.clipnorm),
                                            _lib.ptr(self._scratch), _lib.stream_ptr()))

  def _extended(self):
    """Is a keyword on that only wn_adam_step_ext serves?  (weight_decay 0.0 is off.)"""
    return bool(self.global_clipnorm or self.clipvalue or self.weight_decay or self.amsgrad)

  def _clip_in_step(self, c):
    """Does the clip value ``c`` act inside the Adam launch?  (clip_local_gradients has clipped already: no second clip.)"""
    return bool(c) and not self.clip_before_reduce

  def _overwrite_now(self):
    """1 when this step (``iterations``, already counted) ends with p = ema, else 0."""
    f = self.ema_overwrite_frequency
    return 1 if f is not None and self.iterations % f == 0 else 0

  def _options(self):
    o = _lib.WnAdamOptions()
    o.lr, o.beta1, o.beta2, o.eps = self.learning_rate, self.beta_1, self.beta_2, self.epsilon
    for mode, c in ((_lib.WN_CLIP_NORM, self.clipnorm), (_lib.WN_CLIP_GLOBAL_NORM, self.global_clipnorm),
                    (_lib.WN_CLIP_VALUE, self.clipvalue)):
      if self._clip_in_step(c):
        o.clip_mode, o.clip = mode, float(c)
    o.weight_decay = self.weight_decay or 0.0
    o.amsgrad = int(self.amsgrad)
    o.decay_flags = None if self._decay_flags is None else self._decay_flags.data_ptr()
    if self.use_ema:
      o.ema_momentum, o.ema_overwrite = float(self.ema_momentum), self._overwrite_now()
    return o

  def updates_next(self):
    """Will the next ``apply_gradients`` move the weights?  (Always, without ``gradient_accumulation_steps``.)"""
    k = self.gradient_accumulation_steps
    return not k or self.accumulated == k - 1

  def _accumulate(self, model, mode, skip_flag):
    _lib.check(_lib.lib().wn_grad_accumulate(_lib.ptr(self.accum), _lib.ptr(model.flat_grads), model.flat_grads.numel(), mode,
                                             self.gradient_accumulation_steps, _lib.ptr(skip_flag), _lib.stream_ptr()))

  def form_mean(self, model, skip_flag=None):
    """On the last micro-step of a cycle: ``model.flat_grads = (flat_grads + accum) / k``, once.  ``apply_gradients`` does
    this itself; a data-parallel caller calls it ahead of the all-reduce (every replica forms its own mean, the SUM of the
    means is reduced) and ``apply_gradients`` then finds it done.  Writes ``flat_grads`` only.  Nothing happens without
    ``gradient_accumulation_steps`` or on a storing micro-step."""
    if not self.gradient_accumulation_steps or not self.updates_next() or self._mean_formed:
      return
    self.build(model)
    self._accumulate(model, _lib.WN_ACCUM_FINISH, skip_flag)
    self._mean_formed = True

  def undo_last_apply(self):
    """The ``(iterations, accumulated)`` pair from before the last ``apply_gradients``: the counters of a micro-step that the
    range guard skipped on the device and that is about to be repeated.  Without accumulation: ``iterations -= 1``."""
    self.iterations, self.accumulated = self._before

  def apply_gradients(self, model, skip_flag=None):
    """One update of model.flat_params from model.flat_grads (src/model.py:336).  ``skip_flag``: a device float;
    when it is non-zero the kernel leaves parameters and moments untouched (the range guard of the split-precision
    mode tripped and the caller repeats the step with the exact-fp32 kernels, see WaveNet.train_step)."""
    self.build(model)
    self._before = (self.iterations, self.accumulated)
    k = self.gradient_accumulation_steps
    if k:
      if not self.updates_next():                    # micro-steps 1 .. k-1: store and return; nothing else moves
        self._accumulate(model, _lib.WN_ACCUM_ADD if self.accumulated else _lib.WN_ACCUM_FIRST, skip_flag)
        self.accumulated += 1
        return
      self.form_mean(model, skip_flag)
      self._mean_formed = False
      self.accumulated = 0
    self.iterations += 1
    model._train_gen = getattr(model, '_train_gen', 0) + 1      # the weights move: a differentiable() graph of the old ones is void
    if self._extended():
      self.ext_steps += 1
      o = self._options()
      _lib.check(_lib.lib().wn_adam_step_ext(
          model._plan, _lib.ptr(model.flat_params), _lib.ptr(model.flat_grads), _lib.ptr(self.m), _lib.ptr(self.v),
          _lib.ptr(self.vhat if self.amsgrad else None), _lib.ptr(self.ema if self.use_ema else None), self.iterations,
          C.byref(o), _lib.ptr(self._scratch), _lib.ptr(skip_flag), _lib.stream_ptr()))
      return
    clipnorm = float(self.clipnorm) if self._clip_in_step(self.clipnorm) else 0.0
    if self.use_ema:
      _lib.check(_lib.lib().wn_adam_step_ema(
          model._plan, _lib.ptr(model.flat_params), _lib.ptr(model.flat_grads), _lib.ptr(self.m), _lib.ptr(self.v),
          _lib.ptr(self.ema), self.iterations, self.learning_rate, self.beta_1, self.beta_2, self.epsilon,
          clipnorm, float(self.ema_momentum), self._overwrite_now(), _lib.ptr(self._scratch), _lib.ptr(skip_flag),
          _lib.stream_ptr()))
      return
    _lib.check(_lib.lib().wn_adam_step_guarded(
        model._plan, _lib.ptr(model.flat_params), _lib.ptr(model.flat_grads), _lib.ptr(self.m),
        _lib.ptr(self.v), self.iterations, self.learning_rate, self.beta_1, self.beta_2, self.epsilon,
        clipnorm, _lib.ptr(self._scratch), _lib.ptr(skip_flag), _lib.stream_ptr()))

  def finalize_variable_values(self, model):
    """Keras's name: the weights become their average (p <- ema), e.g. at the end of training.  Nothing happens without
    ``use_ema``."""
    if not self.use_ema:
      return
    if getattr(model, '_averaged', None) is not None:
      raise RuntimeError('finalize_variable_values inside averaged_weights(): leave the scope first')
    self.build(model)
    model._train_gen = getattr(model, '_train_gen', 0) + 1
    model.flat_params.data.copy_(self.ema)
