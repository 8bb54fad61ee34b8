"""The reference of the scoring tests (WaveNet.score): float64 on the CPU oracle.

  rows[b, t] = w[b, t] l[b, t],   nll[b] = sum_t rows[b, t],   weight[b] = sum_t w[b, t]

with l the oracle's per-row loss of tests/weighted_reference.py (row_losses) on O.model_forward: no 1 / global_batch, no L2
term.  Rows with w == 0 are taken out BEFORE anything of them is evaluated, as in weighted_reference: their predictions and
targets never reach the loss function and their row is +0, whatever the row holds.

Pinned without a GPU in tests/test_score_cpu.py: sum_b nll[b] / B against O.loss_and_grads for w = 1, and the causal identity
(a padded utterance under length_weights scores what the utterance cut to its length scores)."""
import torch

import weighted_reference as W
from oracle import wavenet_oracle as O


def forward(x, params, cfg, cond=None):
  """The part of a score that does not see the weights: (pred (B, T, C_out), target (B, T, 1)) in float64 of x (B, T + 1, 1)."""
  with torch.no_grad():
    ps = [p.detach().double() for p in params]
    x = x.double()
    cond = cond.double() if cond is not None else None
    target = O.prepare_target(x[:, 1:, :], cfg)
    return O.model_forward(x[:, :-1, :], ps, cfg, cond), target


def score_from(pred, target, cfg, w=None):
  """w (B, T) or None (all ones).  Returns dict(rows (B, T), nll (B,), weight (B,), target_prob (B, T) or None):
  target_prob is the softmax probability of the target class of a categorical head, for callers that must know how far
  the rows are from Keras's clip (rows of weight 0 may hold anything there)."""
  with torch.no_grad():
    B, T = pred.shape[0], pred.shape[1]
    w = torch.ones(B, T, dtype=torch.float64) if w is None else torch.as_tensor(w).double().reshape(B, T)
    keep = w != 0
    rows = torch.zeros(B, T, dtype=torch.float64)
    rows[keep] = w[keep] * W.row_losses(target[keep], pred[keep], cfg)
    target_prob = None
    if cfg.sampling_function == 'categorical':
      safe = torch.where(keep, target.reshape(B, T), torch.zeros(B, T, dtype=target.dtype))
      target_prob = torch.gather(pred, -1, safe.long().reshape(B, T, 1))[..., 0]
    return dict(rows=rows, nll=rows.sum(dim=1), weight=w.sum(dim=1), target_prob=target_prob)


def score(x, params, cfg, w=None, cond=None):
  """x (B, T + 1, 1), w (B, T) or None.  Samples behind the last weighted target may hold anything, NaN included: the
  network is causal and their rows are never evaluated."""
  pred, target = forward(x, params, cfg, cond)
  return score_from(pred, target, cfg, w)
