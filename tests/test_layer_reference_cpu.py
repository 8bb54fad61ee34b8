"""tests/layer_reference.py pinned against fp64 autograd of the oracle's block (O.layer_forward); no GPU, no libwn_hip.

Every output of the restatement -- x_out, skip, the intermediates u, gate, z, the gradient at u, g_x, g_cond and every
parameter gradient -- must equal autograd's to 1e-10 of the tensor's max, for an objective <g_xout, x_out> + <g_skip, skip>
with both gradients, with g_xout alone and with g_skip alone (a gradient that is None does not enter the objective; a
parameter the objective does not reach has a zero gradient).

This also pins the oracle's time-varying condition (B, T, Cc), which the model tests only use as a (B, 1, Cc) broadcast."""
import pytest
import torch

import layer_reference as LR
from oracle import wavenet_oracle as O

# name: R, D, S, KS, dilations, activation, residual, Cin, Cc, B, T
LAYERS = {
    'k2_d1_skip':          (8, 8, 12, 2, [1], None, True, 8, 0, 2, 23),
    'k3_d1_noskip':        (6, 6, None, 3, [3], None, True, 6, 0, 3, 29),
    'k2_d1_tanh':          (8, 8, 10, 2, [2], 'tanh', True, 8, 0, 2, 21),
    'k2_d1_leaky_noskip':  (8, 8, None, 2, [4], 'leaky_relu', True, 8, 0, 2, 21),
    'k2_d3_tanh':          (8, 8, 10, 2, [1, 2, 4], 'tanh', True, 8, 0, 2, 31),
    'k3_d3_leaky_noskip':  (8, 8, None, 3, [1, 3, 2], 'leaky_relu', True, 8, 0, 2, 37),
    'nores_cin1':          (8, 8, 6, 2, [2], None, False, 1, 0, 3, 19),
    'nores_cin16_d2_tanh': (8, 8, None, 2, [2, 1], 'tanh', False, 16, 0, 2, 27),
    'cond3_skip':          (8, 8, 12, 2, [2], None, True, 8, 3, 2, 25),
    'cond8_k3_d3_leaky':   (8, 12, None, 3, [1, 2, 4], 'leaky_relu', True, 8, 8, 2, 33),
    'D_ne_R_skip':         (8, 12, 20, 2, [2], None, True, 8, 0, 2, 22),
    'long_dilation_k3':    (8, 8, 12, 3, [32], None, True, 8, 0, 3, 40),        # shifts 64 >= T and 32 > T / 2
    'long_dilation_cond':  (6, 10, 9, 2, [3, 17], 'leaky_relu', True, 6, 3, 2, 30),
}
MODES = ['both', 'xout_only', 'skip_only']


def make(name, seed=0):
  """(x, cond or None, params, g_xout, g_skip, keywords of layer_reference without the gradients), all float64."""
  R, D, S, KS, dil, act, res, cin, Cc, B, T = LAYERS[name]
  g = torch.Generator().manual_seed(1000 + seed)
  rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  uni = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * 0.4
  params, c = [], cin
  for i in range(len(dil)):
    cout = 2 * D if i == len(dil) - 1 else D
    params += [uni(KS, c, cout), uni(cout)]
    c = cout
  params += [uni(1, D, R), uni(R)]
  if S is not None:
    params += [uni(1, D, S), uni(S)]
  if Cc:
    params += [uni(1, Cc, 2 * D), uni(2 * D)]
  x = rnd(B, T, cin) * 0.7
  cond = rnd(B, T, Cc) if Cc else None
  kw = dict(dilations=dil, kernel_size=KS, activation=act, residual=res, has_skip=S is not None)
  return x, cond, params, rnd(B, T, R), rnd(B, T, S or R), kw


def autograd(x, cond, params, g_xout, g_skip, kw, inner_branch=None):
  xr = x.clone().requires_grad_(True)
  cr = cond.clone().requires_grad_(True) if cond is not None else None
  pr = [p.clone().requires_grad_(True) for p in params]
  taps = {}
  xo, sk = O.layer_forward(xr, pr, dilations=kw['dilations'], activation_name=kw['activation'], residual=kw['residual'],
                           has_skip=kw['has_skip'], cond=cr, taps=taps, inner_branch=inner_branch)
  obj = 0
  if g_xout is not None:
    obj = obj + (xo * g_xout).sum()
  if g_skip is not None:
    obj = obj + (sk * g_skip).sum()
  wrt = [xr, taps['u']] + ([cr] if cr is not None else []) + pr
  gr = torch.autograd.grad(obj, wrt, allow_unused=True)
  gr = [torch.zeros_like(w) if g is None else g for g, w in zip(gr, wrt)]
  out = dict(x_out=xo.detach(), skip=sk.detach(), u=taps['u'].detach(), gate=taps['gate'].detach(), z=taps['z'].detach(),
             pre=[q.detach() for q in taps['pre']], p=[q.detach() for q in taps['p']], g_x=gr[0], g_u=gr[1])
  k = 2
  out['g_cond'] = None
  if cr is not None:
    out['g_cond'] = gr[2]
    k = 3
  out['param_grads'] = list(gr[k:])
  return out


def close(name, got, ref):
  assert got.shape == ref.shape, (name, got.shape, ref.shape)
  scale = ref.abs().max().item()
  err = (got - ref).abs().max().item()
  assert err <= 1e-10 * scale, (name, err, scale)


def compare(got, ref, kw, has_cond):
  for key in ('x_out', 'skip', 'u', 'gate', 'z', 'g_u', 'g_x'):
    close(key, got[key], ref[key])
    assert ref[key].abs().max() > 0 or key in ('g_u', 'g_x')
  for i, (a, b) in enumerate(zip(got['pre'], ref['pre'])):
    close(f'pre[{i}]', a, b)
  for i, (a, b) in enumerate(zip(got['p'], ref['p'])):
    close(f'p[{i}]', a, b)
  assert len(got['pre']) == len(ref['pre']) == len(kw['dilations']) - 1
  if has_cond:
    close('g_cond', got['g_cond'], ref['g_cond'])
  else:
    assert got['g_cond'] is None and got['dW_c'] is None and got['db_c'] is None
  names = LR.param_grad_names(len(kw['dilations']), kw['has_skip'], has_cond)
  assert len(names) == len(got['param_grads']) == len(ref['param_grads'])
  for n, a, b in zip(names, got['param_grads'], ref['param_grads']):
    close(n, a, b)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(LAYERS))
def test_restatement_equals_fp64_autograd(name, mode):
  x, cond, params, g_xout, g_skip, kw = make(name)
  if mode == 'xout_only':
    g_skip = None
  if mode == 'skip_only':
    g_xout = None
  got = LR.layer_reference(x, cond, params, g_xout=g_xout, g_skip=g_skip, **kw)
  ref = autograd(x, cond, params, g_xout, g_skip, kw)
  compare(got, ref, kw, cond is not None)
  # an absent gradient leaves its 1x1 conv's parameters exactly zero (with skip_channels), and the data gradients non-zero
  if kw['has_skip'] and mode == 'xout_only':
    assert not got['dW_s'].any() and not got['db_s'].any() and got['dW_r'].any()
  if kw['has_skip'] and mode == 'skip_only':
    assert not got['dW_r'].any() and not got['db_r'].any() and got['dW_s'].any()
  assert got['g_u'].abs().max() > 0 and got['g_x'].abs().max() > 0
  # no pre-activation within rounding of a kink: the comparison above did not depend on a side
  if kw['activation'] == 'leaky_relu':
    for q in got['pre']:
      assert q.abs().min() >= 1e-5


def test_neither_gradient_gives_zeros():
  x, cond, params, _, _, kw = make('cond3_skip')
  got = LR.layer_reference(x, cond, params, g_xout=None, g_skip=None, **kw)
  for t in [got['g_x'], got['g_cond'], got['g_u']] + got['param_grads']:
    assert not t.any()


def test_residual_term_only_through_x_out():
  """Without skip_channels the skip output is the PRE-residual 1x1 output: g_skip alone adds no residual term to g_x."""
  x, cond, params, g_xout, g_skip, kw = make('k3_d1_noskip')
  a = LR.layer_reference(x, cond, params, g_xout=None, g_skip=g_skip, **kw)
  b = LR.layer_reference(x, cond, params, g_xout=g_skip, g_skip=None, **kw)
  assert kw['residual'] and not kw['has_skip']
  assert torch.equal(b['g_x'], a['g_x'] + g_skip)
  assert torch.equal(a['dW_r'], b['dW_r'])


def test_kink_side_taken_from_the_implementation_only_inside_the_tolerance():
  """leaky_relu stack with pre-activations of exactly 0 (zero first-conv bias, zero input rows): there the side comes from
  inner_branch, as in O.activation_with_branch; everywhere else from the element's own sign."""
  name = 'k3_d3_leaky_noskip'
  x, cond, params, g_xout, g_skip, kw = make(name)
  params[1] = torch.zeros_like(params[1])
  x[:, 5:9] = 0
  plain = LR.layer_reference(x, cond, params, g_xout=g_xout, g_skip=g_skip, **kw)
  at_kink = plain['pre'][0].abs() < O.KINK_TOL
  assert at_kink.sum() >= 8
  branch = [~(q >= 0) for q in plain['pre']]         # the other side everywhere: only the kink elements may follow it
  got = LR.layer_reference(x, cond, params, g_xout=g_xout, g_skip=g_skip, inner_branch=branch, **kw)
  ref = autograd(x, cond, params, g_xout, g_skip, kw, inner_branch=branch)
  compare(got, ref, kw, False)
  assert (got['g_x'] - plain['g_x']).abs().max() > 1e-6
