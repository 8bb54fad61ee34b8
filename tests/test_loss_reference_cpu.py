"""The fp64 references of the mixture losses against 50-digit arithmetic (tests/golden/mix_tails.npz, written by
tests/golden/make_mix_tails.py): rows at the -7 floor of the log-scales, at the 1e8 cap of the Gaussian argument and in
both far tails of sharp components.  The GPU loss tests (tests/test_gpu_loss_edges.py) take O.loss_logistic_exact and
O.loss_gaussian as their references there; this file is what entitles them to.  No GPU.  """
import math
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mix_tails.npz')


def groups():
  z = np.load(GOLDEN)
  out = []
  for k in sorted(z.files):
    if not k.endswith('_pred'):
      continue
    key = k[:-5]
    kind, m, b = key.split('_')
    g = dict(key=key, kind=kind, M=int(m[1:]), bits=int(b[1:]),
             **{f: z[f'{key}_{f}'] for f in ('pred', 'y', 'loss', 'grad', 'exp10')})
    g['tail'] = z[f'{key}_tail'] if kind == 'logistic' else np.zeros(len(g['y']), np.int8)
    out.append(g)
  return out


GROUPS = groups()


def reference(g, pred=None, y=None, exact=True):
  """(loss rows, dL/dpred rows) of a fixture group in fp64 from the fp32 inputs."""
  pred = torch.from_numpy(g['pred'] if pred is None else pred).double().requires_grad_(True)
  y = torch.from_numpy(g['y'] if y is None else y).double().unsqueeze(-1)
  if g['kind'] == 'gaussian':
    loss = O.loss_gaussian(y, pred, g['M'])
  else:
    loss = (O.loss_logistic_exact if exact else O.loss_logistic)(y, pred, g['M'], g['bits'])
  fin = torch.isfinite(loss)
  grad, = torch.autograd.grad(loss[fin].sum(), pred)
  return loss.detach(), grad, fin


def test_fixture_covers_the_table():
  Ms = {(g['kind'], g['M']) for g in GROUPS}
  for kind in ('logistic', 'gaussian'):
    assert {1, 2, 10, 32} <= {m for k, m in Ms if k == kind}
  assert {g['bits'] for g in GROUPS if g['kind'] == 'logistic'} == {8, 16}
  n = sum(len(g['y']) for g in GROUPS)
  assert 200 <= n <= 1000 and os.path.getsize(GOLDEN) < 100 * 1024
  for g in GROUPS:
    e = g['exp10']
    assert not np.any((e >= -320) & (e <= -280)), g['key']         # the denormal band is not generated
    assert np.array_equal(np.isinf(g['loss']), e < -320), g['key']
    assert g['pred'].dtype == np.float32 and g['y'].dtype == np.float32 and g['loss'].dtype == np.float64
  # the floor and its fp32 neighbours, below the floor, the Gaussian cap
  ls1 = np.concatenate([g['pred'][:, 2] for g in GROUPS if g['M'] == 1])
  m7 = np.float32(-7)
  for v in (np.float32(-9), m7, np.nextafter(m7, np.float32(-8)), np.nextafter(m7, np.float32(0)), np.float32(3)):
    assert np.any(ls1 == v)
  assert any(np.any(g['pred'][:, g['M']:2 * g['M']] == np.float32(-2e5)) for g in GROUPS if g['kind'] == 'gaussian')


@pytest.mark.parametrize('g', GROUPS, ids=[g['key'] for g in GROUPS])
def test_fp64_reference_reproduces_the_exact_rows(g):
  """Losses to 1e-12 relative, gradients to 1e-9 of the row's largest entry: double arithmetic with at most 5 digits of
  cancellation in sigmoid(hi) - sigmoid(lo) -- at bits = 16 and log-scale <= 0.  The table also holds log-scale 3 at
  bits = 16, where the bin is 2 h e^-3 = 7.6e-7 wide in the sigmoid's argument and the difference of two values near 0.5
  cancels 7 digits.  Each sigmoid (an exp and a division) is within 2 units of 2^-53 of its own size s <= 1/2, and
  the mass is about s (1 - s) 2 h e^-ls >= s h e^-ls: the likelihood carries a relative error of up to
  8 * 2^-53 / (h e^-ls), and the loss the same as an absolute one.  That term is added for the logistic rows (1.2e-10
  at ls = 0, 2.3e-9 at ls = 3, both at bits = 16; 1e-13 at the floor); it follows from the double format and the
  formula, not from what the function returns.
  Gradients likewise get an absolute term: an entry is a difference of terms t / lik, each rounded at 2^-53 of its own
  size, and the difference can be far smaller than the terms (a weight 40 above the rest: dL/dw = w (1 - comp / lik) is
  4e-18, below one rounding of 1; a masked log-scale under a target on the mean: every exact entry is 0).  The terms
  are bounded by w comp / lik <= 1 for the weights and by sigma'(a) e^-ls / comp <= 1 / (2 h) for a logistic mean, so
  the term is 2^-52 and 2^-52 / (2 h); next to a row's largest entry it is nothing wherever that entry is not tiny."""
  loss, grad, fin = reference(g)
  assert np.array_equal(fin.numpy(), np.isfinite(g['loss']))
  exact = torch.from_numpy(g['loss'])
  tol = 1e-12 * exact[fin].abs()
  if g['kind'] == 'logistic':
    M = g['M']
    ls = torch.from_numpy(g['pred'][:, 2 * M:]).double().clamp(min=-7.0).max(dim=-1).values
    tol = tol + (8 * 2.0 ** -53 / (0.5 / 2 ** g['bits'] * torch.exp(-ls)))[fin]
  err = (loss[fin] - exact[fin]).abs()
  print(g['key'], 'worst loss err / tol', (err / tol).max().item(), 'worst rel', (err / exact[fin].abs()).max().item())
  assert torch.all(err <= tol), (err / tol).max()
  assert torch.all(loss[~fin] == float('inf'))
  gex = torch.from_numpy(g['grad'])[fin]
  floor = 2.0 ** -52 * (2 ** g['bits'] if g['kind'] == 'logistic' else 1.0)
  gtol = 1e-9 * gex.abs().max(dim=-1, keepdim=True).values + floor
  gerr = ((grad[fin] - gex).abs() / gtol).max().item()
  print(g['key'], 'worst gradient err / tol', gerr)
  assert gerr <= 1.0


@pytest.mark.parametrize('g', [g for g in GROUPS if g['kind'] == 'logistic'],
                         ids=[g['key'] for g in GROUPS if g['kind'] == 'logistic'])
def test_loss_as_written_loses_the_upper_tail(g):
  """O.loss_logistic (the source's own sigmoid(a) - sigmoid(b), in fp64) against the same rows: right where no component
  that matters has b > 12 (2^-53 e^12 / (2 h e^7) < 1e-7 relative at the floor, less for broader components), inf or
  off by more than ln 2 / 2 where components with b > 37 hold more than half of the likelihood.  The fixture would be
  trivially easy if this test could not tell the two functions apart."""
  loss, _, _ = reference(g, exact=False)
  exact = torch.from_numpy(g['loss'])
  tail = torch.from_numpy(g['tail'])
  fin = torch.isfinite(exact)
  none = (tail == 0) & fin
  assert torch.all((loss[none] - exact[none]).abs() <= 1e-6 * exact[none].abs().clamp(min=1.0))
  upper = (tail == 1) & fin
  assert torch.all(torch.isinf(loss[upper]) | ((loss[upper] - exact[upper]).abs() > 0.34))


def test_upper_tail_rows_exist_and_the_stated_numbers_hold():
  tails = np.concatenate([g['tail'][np.isfinite(g['loss'])] for g in GROUPS if g['kind'] == 'logistic'])
  assert (tails == 1).sum() >= 16 and (tails == 0).sum() >= 100
  # one component at the floor, bits = 16, mu = 0
  pred = torch.tensor([[0.0, 0.0, -7.0]], dtype=torch.float64)
  for y, want in ((0.03, 36.989338), (0.01, 15.056709)):
    lo = O.loss_logistic(torch.tensor([[-y]], dtype=torch.float64), pred, 1, 16).item()
    up = O.loss_logistic(torch.tensor([[y]], dtype=torch.float64), pred, 1, 16).item()
    ex = [O.loss_logistic_exact(torch.tensor([[s * y]], dtype=torch.float64), pred, 1, 16).item() for s in (1, -1)]
    assert abs(lo - want) < 1e-6 and abs(ex[0] - want) < 1e-6 and ex[0] == ex[1]
    assert up == float('inf') if y == 0.03 else abs(up - want) < 1e-6


@pytest.mark.parametrize('g', GROUPS, ids=[g['key'] for g in GROUPS])
def test_mirror_law(g):
  """loss(y; mu) == loss(-y; -mu) on every row.  Negation is exact in fp32 and in double, and the exact logistic loss
  takes the same side for both rows (hi and lo swap roles, the values are the same), so the rows agree to the bit.
  The Gaussian as the source writes it caps (y - mu) / sigma from above only: beyond the cap one side is
  exp(-0.5e16) = 0 and the other exp(-x^2 / 2) = 0 as well, so the law survives there too."""
  M = g['M']
  mirrored = g['pred'].copy()
  mirrored[:, M:2 * M] = -mirrored[:, M:2 * M]
  loss, _, _ = reference(g)
  lm, _, _ = reference(g, pred=mirrored, y=-g['y'])
  assert torch.equal(loss, lm)


def test_clip_indicator_of_one_class_moves_a_gradient_by_2e_7_unless_it_is_the_targets():
  """The categorical GPU tests excuse no element near the clip thresholds.  What entitles them to: the loss is
  continuous in q across 1e-7, and the clip's indicator c_k of a class k that is NOT the target enters dL/dlogits
  (wn_catrow.h: g_j = q_j (c_j / S - [j = t] c_t / p_t - dot), dot = A / S - c_t q_t / p_t, A = sum_j c_j q_j) through
  A and through g_k's own first term: taking q_k across the threshold moves every g_j by at most q_k / S + q_j q_k / S
  <= 2e-7 (times gscale).  The target's own indicator is another matter: c_t multiplies q_t / p_t = 1, so g_t jumps
  by (1 - q_t) q_t / p_t, by 1 where q_t crosses 1e-7 (the kink of -log(clip(q_t))).  The GPU cases therefore keep every target's
  probability 30 % away from both thresholds (asserted there), and only there is nothing excused."""
  Cn, cs, eps = 256, 161, 1e-7
  b = (torch.rand(Cn, generator=torch.Generator().manual_seed(8), dtype=torch.float64) * 2 - 1) * 0.4
  b[0], b[Cn - 1], b[cs] = 0.4, -0.4, math.log(1e7)

  def grad(q, c, t):
    p = q.clamp(eps, 1 - eps)
    S, A = p.sum(), (q * c).sum()
    dot = A / S - c[t] * q[t] / p[t]
    g = c / S - dot
    g[t] -= c[t] / p[t]
    return q * g

  q = torch.softmax(b, -1)
  inside = ((q >= eps) & (q <= 1 - eps)).double()
  assert 64 <= inside.sum() <= 192                            # the row straddles the threshold
  for t in (cs, 0, Cn - 1):
    lg = b.clone().requires_grad_(True)
    auto, = torch.autograd.grad(O.loss_categorical(torch.tensor([[t]]), torch.softmax(lg, -1).reshape(1, 1, Cn)).sum(), lg)
    base = grad(q, inside, t)
    assert (base - auto).abs().max() <= 1e-12
    worst = 0.0
    for k in range(Cn):
      if k == t or abs(q[k].item() / eps - 1) > 0.5:
        continue
      c = inside.clone()
      c[k] = 1 - c[k]
      worst = max(worst, (grad(q, c, t) - base).abs().max().item())
    print(f'target {t}: flipping one other class moves a gradient by at most {worst:.3e}')
    assert 0 < worst <= 2e-7
  for t in (0, Cn - 1):                                         # q_t = 1.49e-7 and 0.67e-7
    c = inside.clone()
    c[t] = 1 - c[t]
    jump = (grad(q, c, t) - grad(q, inside, t)).abs().max().item()
    print(f'target {t}: flipping its own indicator moves its gradient by {jump:.6f}')
    assert jump > 0.5
