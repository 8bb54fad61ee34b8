"""Host-side metrics of a compiled model: the stand-in for tf.keras.metrics.MeanSquaredError, whose reduction runs on the
device behind the step's kernels, and the running mean of the step's loss scalars."""
from __future__ import annotations

import torch

from . import _lib


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
