"""Pins of tests/score_reference.py, the fp64 reference of the scoring tests.  No GPU.

(a) all weights 1: sum_b nll[b] / B is the loss of O.loss_and_grads, and weight[b] = T.
(b) the causal identity: a padded utterance under length_weights scores exactly what the utterance cut to its length scores
    alone -- whatever lies behind the cut, NaN included.
For the logistic head O.loss_and_grads is taken with the row loss of DESIGN.md section 17, as in tests/test_sample_weight_cpu.py."""
import pytest
import torch

import score_reference as S
from oracle import wavenet_oracle as O
from test_sample_weight_cpu import CASES, B, T, LENGTHS, _setup, exact_logistic  # noqa: F401  (exact_logistic: fixture)


@pytest.mark.parametrize('name', CASES)
def test_all_ones_sum_to_the_oracles_loss(name, exact_logistic):
  cfg, params, x, cond = _setup(name)
  loss, _, _, _ = O.loss_and_grads(x, params, cfg, cond)
  for w in (None, torch.ones(B, T)):
    ref = S.score(x, params, cfg, w, cond)
    assert ref['rows'].shape == (B, T) and ref['nll'].shape == (B,) and ref['weight'].tolist() == [float(T)] * B
    got = float(ref['nll'].sum()) / B
    assert abs(got - float(loss)) <= 1e-12 * abs(float(loss)), (name, got, float(loss))
    assert bool((ref['rows'] > 0).all()) or cfg.sampling_function == 'gaussian'      # (a density's NLL may be negative)
  assert (ref['target_prob'] is None) == (cfg.sampling_function != 'categorical')


@pytest.mark.parametrize('name', CASES)
def test_a_padded_utterance_scores_as_the_utterance_cut_to_its_length(name, exact_logistic):
  from wavenets_amd.data import length_weights
  cfg, params, x, cond = _setup(name)
  w = length_weights(LENGTHS, T)
  xn = x.clone()
  for b, l in enumerate(LENGTHS):
    xn[b, l + 1:] = float('nan') if b == 1 else 1e30           # what lies behind the cut must not matter: make it loud
  ref = S.score(xn, params, cfg, w, cond)
  assert bool(torch.isfinite(ref['rows']).all()) and ref['weight'].tolist() == [float(l) for l in LENGTHS]
  for b, l in enumerate(LENGTHS):
    alone = S.score(x[b:b + 1, :l + 1], params, cfg, None, cond[b:b + 1] if cond is not None else None)
    assert float(alone['weight'][0]) == float(l)
    err = (ref['rows'][b, :l] - alone['rows'][0]).abs().max().item()
    assert err <= 1e-10 * alone['rows'].abs().max().item(), (name, b, err)
    assert abs(float(ref['nll'][b]) - float(alone['nll'][0])) <= 1e-10 * abs(float(alone['nll'][0])), (name, b)
    assert bool((ref['rows'][b, l:] == 0).all())
  # and it is not the unweighted score
  full = S.score(x, params, cfg, None, cond)
  assert abs(float(full['nll'][2]) - float(ref['nll'][2])) > 1e-3 * abs(float(ref['nll'][2]))


def test_a_general_weight_is_a_product_row_by_row():
  cfg, params, x, cond = _setup('cat_small_fused')
  g = torch.Generator().manual_seed(3)
  w = torch.rand(B, T, generator=g, dtype=torch.float64) * 2
  w[:, ::7] = 0.0
  one, ref = S.score(x, params, cfg, None, cond), S.score(x, params, cfg, w, cond)
  assert torch.allclose(ref['rows'], w * one['rows'], rtol=1e-14, atol=0)
  assert torch.equal(ref['weight'], w.sum(dim=1)) and torch.equal(ref['nll'], ref['rows'].sum(dim=1))
