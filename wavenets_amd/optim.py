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
"""
from __future__ import annotations

import math

import torch

from . import _lib


class Adam:
  def __init__(self, learning_rate: float = 0.001, beta_1: float = 0.9, beta_2: float = 0.999,
               epsilon: float = 1e-7, clipnorm=None, clip_before_reduce: bool = False,
               use_ema: bool = False, ema_momentum: float = 0.99, ema_overwrite_frequency=None):
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
    self.learning_rate = float(learning_rate)
    self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
    self.clipnorm = clipnorm
    self.clip_before_reduce = clip_before_reduce
    self.use_ema, self.ema_momentum, self.ema_overwrite_frequency = use_ema, ema_momentum, ema_overwrite_frequency
    self.iterations = 0
    self.m = self.v = self.ema = self._scratch = None

  def build(self, model):
    """Allocate the moment buffers (src/model.py:211 optimizer.build)."""
    if self.m is None or self.m.numel() != model.flat_params.numel():
      self.m = torch.zeros_like(model.flat_params.data)
      self.v = torch.zeros_like(model.flat_params.data)
      self._scratch = torch.zeros(len(model.variable_names) + 8, dtype=torch.float32,
                                  device=model.flat_params.device)
      self.ema = None
    if self.use_ema and self.ema is None:
      # a copy of the current weights: an optimizer that starts averaging at t > 1 (a resume from a checkpoint without
      # an average) averages from the loaded weights
      self.ema = model.flat_params.data.clone()

  def clip_local_gradients(self, model):
    """``clip_before_reduce``: clip this replica's ``model.flat_grads`` per tensor, in place, ahead of the all-reduce.
    Nothing happens without the flag or without a clipnorm."""
    if not (self.clip_before_reduce and self.clipnorm):
      return
    self.build(model)
    _lib.check(_lib.lib().wn_clip_gradients(model._plan, _lib.ptr(model.flat_grads), float(self.clipnorm),
                                            _lib.ptr(self._scratch), _lib.stream_ptr()))

  def apply_gradients(self, model, skip_flag=None):
    """One update of model.flat_params from model.flat_grads (src/model.py:336).  ``skip_flag``: a device float;
    when it is non-zero the kernel leaves parameters and moments untouched (the range guard of the split-precision
    mode tripped and the caller repeats the step with the exact-fp32 kernels, see WaveNet.train_step)."""
    self.build(model)
    self.iterations += 1
    model._train_gen = getattr(model, '_train_gen', 0) + 1      # the weights move: a differentiable() graph of the old ones is void
    if self.use_ema:
      f = self.ema_overwrite_frequency
      _lib.check(_lib.lib().wn_adam_step_ema(
          model._plan, _lib.ptr(model.flat_params), _lib.ptr(model.flat_grads), _lib.ptr(self.m), _lib.ptr(self.v),
          _lib.ptr(self.ema), self.iterations, self.learning_rate, self.beta_1, self.beta_2, self.epsilon,
          float(self.clipnorm) if self.clipnorm and not self.clip_before_reduce else 0.0, float(self.ema_momentum),
          1 if f is not None and self.iterations % f == 0 else 0,
          _lib.ptr(self._scratch), _lib.ptr(skip_flag), _lib.stream_ptr()))
      return
    _lib.check(_lib.lib().wn_adam_step_guarded(
        model._plan, _lib.ptr(model.flat_params), _lib.ptr(model.flat_grads), _lib.ptr(self.m),
        _lib.ptr(self.v), self.iterations, self.learning_rate, self.beta_1, self.beta_2, self.epsilon,
        float(self.clipnorm) if self.clipnorm and not self.clip_before_reduce else 0.0,     # no second clip
        _lib.ptr(self._scratch), _lib.ptr(skip_flag), _lib.stream_ptr()))

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
