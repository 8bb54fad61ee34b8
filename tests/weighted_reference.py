"""The reference of the sample_weight tests: fp64 autograd on the CPU oracle.

  loss = sum_{b,t} w[b,t] l[b,t] / global_batch + the oracle's L2 term

with l the oracle's per-row loss -- O.loss_categorical, O.loss_logistic_exact (not O.loss_logistic) or
O.loss_gaussian -- on O.model_forward.  Rows with w == 0 are taken out BEFORE anything of them is evaluated: their
predictions and targets never reach the loss function, so a row whose own loss is inf leaves the sum and the gradients
finite, which is what "a zero weight is a select" asks of the kernels.

Pinned without a GPU in tests/test_sample_weight_cpu.py: against O.loss_and_grads for w = 1, and against the sum of
O.loss_and_grads over each utterance alone, cut to its length, for w = length_weights (the network is causal, so that is an
identity which does not trust the weighting)."""
import torch

from oracle import wavenet_oracle as O


def row_losses(target, pred, cfg):
  """Per-row loss of rows already selected: pred (rows, C_out), target (rows, 1) (class indices or fp values)."""
  if cfg.sampling_function == 'categorical':
    return O.loss_categorical(target[:, 0], pred)
  if cfg.sampling_function == 'logistic':
    return O.loss_logistic_exact(target, pred, cfg.num_mixtures, cfg.bits)
  if cfg.sampling_function == 'gaussian':
    return O.loss_gaussian(target, pred, cfg.num_mixtures)
  raise NotImplementedError(cfg.sampling_function)


def weighted_loss_and_grads(x, params, cfg, w, cond=None, global_batch=None, n_replicas=1):
  """x (B, T + 1, 1), w (B, T): w[b, t] weighs the target x[b, t + 1].  Everything in float64.
  Returns dict(loss, reg, grads, pred, target_prob): target_prob (B, T) is the softmax probability of the target class
  (categorical head; None otherwise), for the callers that must know how far the rows are from Keras's clip."""
  ps = [p.detach().double().clone().requires_grad_(True) for p in params]
  x = x.double()
  w = torch.as_tensor(w).double().reshape(x.shape[0], x.shape[1] - 1)
  cond = cond.double() if cond is not None else None
  inputs, y_true = x[:, :-1, :], x[:, 1:, :]
  target = O.prepare_target(y_true, cfg)
  pred = O.model_forward(inputs, ps, cfg, cond)
  keep = w != 0
  per = row_losses(target[keep], pred[keep], cfg)           # (rows kept,)
  Bg = x.shape[0] if global_batch is None else global_batch
  loss = (w[keep] * per).sum() / Bg
  reg = O.l2_penalty(ps, cfg) / n_replicas if cfg.l2_reg_factor > 0 else loss.new_zeros(())
  grads = torch.autograd.grad(loss + reg, ps, allow_unused=True)
  grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, ps)]
  target_prob = None
  if cfg.sampling_function == 'categorical':
    target_prob = torch.gather(pred.detach(), -1, target.long().reshape(x.shape[0], -1, 1))[..., 0]
  return dict(loss=loss.detach(), reg=reg.detach(), grads=grads, pred=pred.detach(), target_prob=target_prob)


def weighted_mse(y_true, sample, w):
  """Keras's weighted MeanSquaredError: sum w (y - s)^2 / sum w in float64, 0 when sum w == 0."""
  y, s, w = y_true.double().reshape(-1), sample.double().reshape(-1), torch.as_tensor(w).double().reshape(-1)
  den = float(w.sum())
  return float((w * (y - s) ** 2).sum()) / den if den != 0 else 0.0
