"""Pins of tests/weighted_reference.py, the fp64 reference of the sample_weight tests, and of the data helpers that make the
weights (wavenets_amd.data.length_weights, frame_padded).  No GPU.

(a) all weights 1: the reference is O.loss_and_grads.
(b) w = length_weights(l, T): the reference is the sum over the utterances of O.loss_and_grads of each utterance alone, cut
    to l_b + 1 samples, at global_batch = B.  The network is causal, so the predictions before the cut do not see what lies
    behind it: an identity that pins the weighting without trusting it.
For the logistic head O.loss_and_grads is taken with the row loss of DESIGN.md section 17 (O.loss_logistic_exact in
O.loss_logistic's place): the two agree to the cancellation noise of sigmoid(a) - sigmoid(b) in float64 only, and the
kernels' reference is the exact one."""
import pytest
import torch

import weighted_reference as W
from oracle import wavenet_oracle as O
from test_gpu_parity import MODEL_CASES, _inputs

CASES = ['cat_small_fused', 'mol', 'gauss', 'cond']
B, T = 3, 150
LENGTHS = (150, 113, 1)


@pytest.fixture
def exact_logistic(monkeypatch):
  monkeypatch.setattr(O, 'loss_logistic', O.loss_logistic_exact)


def _setup(name):
  kw = dict(MODEL_CASES[name])
  cond_inputs = kw.pop('cond_inputs', 0)
  cfg = O.OracleConfig(**kw, cond_inputs=cond_inputs)
  params = [p.double() for p in O.init_params(cfg, seed=4, bias_range=0.1)]
  x, cond = _inputs(dict(MODEL_CASES[name]), B, T + 1, seed=8)
  return cfg, params, x.double(), (cond.double() if cond is not None else None)


def _close(got, want, tol, what):
  scale = max(float(want.abs().max()), 1e-300)
  err = float((got - want).abs().max())
  assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize('name', CASES)
def test_all_ones_is_the_oracles_step(name, exact_logistic):
  cfg, params, x, cond = _setup(name)
  loss, reg, grads, pred = O.loss_and_grads(x, params, cfg, cond)
  ref = W.weighted_loss_and_grads(x, params, cfg, torch.ones(B, T), cond)
  _close(ref['loss'], loss, 1e-12, 'loss')
  _close(ref['pred'], pred, 1e-12, 'pred')
  assert float(ref['reg']) == float(reg)
  for i, (g, r) in enumerate(zip(ref['grads'], grads)):
    _close(g, r, 1e-12, f'grad {i}')


@pytest.mark.parametrize('name', CASES)
def test_length_weights_are_each_utterance_alone_cut_to_its_length(name, exact_logistic):
  from wavenets_amd.data import length_weights
  cfg, params, x, cond = _setup(name)
  w = length_weights(LENGTHS, T)
  # what lies behind the cut must not matter: make it loud
  xn = x.clone()
  for b, l in enumerate(LENGTHS):
    xn[b, l + 1:] = 0.9
  ref = W.weighted_loss_and_grads(xn, params, cfg, w, cond)
  loss = torch.zeros((), dtype=torch.float64)
  grads = [torch.zeros_like(p) for p in params]
  for b, l in enumerate(LENGTHS):
    lb, _, gb, _ = O.loss_and_grads(x[b:b + 1, :l + 1], params, cfg, cond[b:b + 1] if cond is not None else None, global_batch=B)
    loss = loss + lb
    grads = [a + g for a, g in zip(grads, gb)]
  _close(ref['loss'], loss, 1e-10, 'loss')
  for i, (g, r) in enumerate(zip(ref['grads'], grads)):
    _close(g, r, 1e-10, f'grad {i}')
  # and it is not the unweighted step
  full = W.weighted_loss_and_grads(xn, params, cfg, torch.ones(B, T), cond)
  assert abs(float(full['loss']) - float(ref['loss'])) > 1e-3 * abs(float(ref['loss']))


def test_a_row_of_weight_zero_never_reaches_the_loss_function():
  """A target the mixture gives no mass in float64 (loss inf, gradient NaN through autograd) under weight 0."""
  cfg, params, x, cond = _setup('mol')
  params = [torch.zeros_like(p) for p in params]
  params[-1][cfg.num_mixtures:2 * cfg.num_mixtures] = 1.0          # every mean 1
  params[-1][2 * cfg.num_mixtures:] = -7.0                        # every log-scale -7
  x = torch.full_like(x, 0.999)
  x[:, 1::3] = -1.0
  w = torch.ones(B, T)
  w[:, 0::3] = 0.0                                                 # target x[b, t + 1] = -1 <=> t % 3 == 0
  bad = W.weighted_loss_and_grads(x, params, cfg, torch.ones(B, T), cond)
  assert not bool(torch.isfinite(bad['loss']))
  ref = W.weighted_loss_and_grads(x, params, cfg, w, cond)
  assert bool(torch.isfinite(ref['loss'])) and all(bool(torch.isfinite(g).all()) for g in ref['grads'])
  assert float(ref['grads'][-1].abs().max()) > 0


def test_weighted_mse():
  y, s = torch.tensor([0.0, 1.0, 2.0, 5.0]), torch.tensor([1.0, 1.0, 0.0, 0.0])
  assert W.weighted_mse(y, s, torch.tensor([1.0, 1.0, 0.5, 0.0])) == pytest.approx((1 + 0 + 0.5 * 4) / 2.5, rel=1e-15)
  assert W.weighted_mse(y, s, torch.zeros(4)) == 0.0


def test_length_weights():
  from wavenets_amd.data import length_weights
  w = length_weights([3, 0, 5, 9], 5)
  assert w.dtype == torch.float32 and w.shape == (4, 5)
  assert w.tolist() == [[1, 1, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]
  assert torch.equal(length_weights(torch.tensor([2]), 4), torch.tensor([[1.0, 1.0, 0.0, 0.0]]))


def test_frame_padded_keeps_the_tail_as_a_masked_frame():
  from wavenets_amd.data import frame, frame_padded
  L = 40
  x = torch.arange(1, 2 * L + 1 + 17 + 1, dtype=torch.float32) / 1000.0       # no zero among the real samples
  frames, w = frame_padded(x, L)
  assert frames.shape == (3, L + 1, 1) and w.shape == (3, L) and w.dtype == torch.float32
  assert torch.equal(frames[:2], frame(x, L))
  assert bool((w[:2] == 1).all())
  # the last frame starts on the last sample of the frame before it and holds 17 real targets, then zeros
  assert torch.equal(frames[2, :18, 0], x[2 * L:]) and bool((frames[2, 18:] == 0).all())
  assert w[2].tolist() == [1.0] * 17 + [0.0] * (L - 17)
  # weight 1 on exactly the targets that are real: target t of a frame is its sample t + 1
  assert torch.equal(w[2] == 1, frames[2, 1:, 0] != 0)
  assert frame_padded(x.reshape(-1, 1), L)[0].shape == (3, L + 1, 1)


def test_frame_padded_adds_no_frame_when_nothing_is_left():
  from wavenets_amd.data import frame, frame_padded
  L = 40
  x = torch.arange(1, 2 * L + 2, dtype=torch.float32) / 1000.0                # exactly 2 L + 1 samples
  frames, w = frame_padded(x, L)
  assert torch.equal(frames, frame(x, L)) and frames.shape[0] == 2 and torch.equal(w, torch.ones(2, L))
  # one sample more is one real target more
  frames, w = frame_padded(torch.cat([x, x[:1]]), L)
  assert frames.shape[0] == 3 and w[2].tolist() == [1.0] + [0.0] * (L - 1)
  # shorter than a frame: one padded frame
  frames, w = frame_padded(x[:5], L)
  assert frames.shape == (1, L + 1, 1) and w[0].tolist() == [1.0] * 4 + [0.0] * (L - 4)
