"""tests/bwd_restatement.py pinned against fp64 autograd of the oracle (no GPU, no libwn_hip).

For each small network every intermediate, the gradient with respect to every intermediate and every parameter gradient
come from ONE fp64 autograd pass over oracle/wavenet_oracle.py.  The exact intermediates and upstream gradients are fed to
the restatement in the role of the workspace tensors; each restated product must then equal autograd's to 1e-10 of the
tensor's max.  Networks whose head can fold (skip_channels and a hidden head layer) are checked in both forms: the folded
form gets neither the skip sum nor its gradient.

T is 40..67 with dilations up to 32 / 27 / 64 (larger than T / 2): taps before the utterance's start, reversed taps past its
end, and nothing may leak from one utterance into the next.

DEEP holds stacks of 2, 3 and 5 convs per block: the inner activated outputs P, the gradients GP at
their pre-activation outputs and, under dropout, the dropped block inputs XD join the workspace tensors.  Every deep
network and two depth-1 networks also run with dropout 0.1, and for every case the forward restatement (H, XD, P, AG, Z,
skip sum) is pinned against the same pass: XD exactly, everything else to 1e-10 of its max."""
import functools

import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O

NETS = {
    # name: (config, B, T)
    'r16_k2_skip_head': (dict(blocks=6, channels=16, kernel_size=2, dilation_bound=64, skip_channels=24,
                              final_layers_channels=[20, 12], activation='leaky_relu', bits=5), 2, 53),
    'r8_k3_skip_head': (dict(blocks=4, channels=8, kernel_size=3, dilation_bound=81, skip_channels=16,
                             final_layers_channels=[16], activation='tanh', bits=4), 3, 41),
    'r32_k2_noskipch_nohead': (dict(blocks=7, channels=32, kernel_size=2, dilation_bound=128, bits=5), 2, 67),
    'r8_k2_noskipch_head': (dict(blocks=6, channels=8, kernel_size=2, dilation_bound=64, final_layers_channels=[8],
                                 activation='relu', bits=4), 2, 40),
    'r16_k2_skip_nohead': (dict(blocks=6, channels=16, kernel_size=2, dilation_bound=64, skip_channels=8, bits=4), 3, 47),
    'r16_k2_global_mapped': (dict(blocks=6, channels=16, kernel_size=2, dilation_bound=64, skip_channels=24,
                                  final_layers_channels=[16], conditioning='global', mapping_layers=[6, 8],
                                  mapping_activation='leaky_relu', cond_inputs=3, bits=5), 3, 53),
    'r8_k3_global_unmapped': (dict(blocks=4, channels=8, kernel_size=3, dilation_bound=81, skip_channels=8,
                                   final_layers_channels=[8], conditioning='global', cond_inputs=4, bits=4), 2, 41),
    'r16_k2_no_residual': (dict(blocks=6, channels=16, kernel_size=2, dilation_bound=64, skip_channels=16,
                                final_layers_channels=[12], use_residual=False, bits=4), 2, 59),
    'r16_k2_dilation_channels': (dict(blocks=6, channels=16, dilation_channels=8, kernel_size=2, dilation_bound=64,
                                      skip_channels=24, final_layers_channels=[16], bits=4), 2, 45),
    'r8_k2_mol': (dict(blocks=6, channels=8, kernel_size=2, dilation_bound=64, skip_channels=16,
                       final_layers_channels=[8], num_mixtures=3, sampling_function='logistic', bits=16), 2, 50),
    'r8_k2_no_skip_head': (dict(blocks=6, channels=8, kernel_size=2, dilation_bound=64, skip_channels=8, use_skip=False,
                                final_layers_channels=[8], bits=4), 2, 43),
}
# stacks deeper than one conv: name: (config, B, T)
DEEP = {
    'd2_r16_k2_skip_head_leaky': (dict(blocks=3, layers_per_block=2, channels=16, kernel_size=2, dilation_bound=64,
                                       skip_channels=24, final_layers_channels=[20], activation='leaky_relu', bits=5), 2, 53),
    'd3_r8_k3_skip_head_relu': (dict(blocks=2, layers_per_block=3, channels=8, kernel_size=3, dilation_bound=81,
                                     skip_channels=16, final_layers_channels=[16], activation='relu', bits=4), 3, 41),
    # the shape of the reference's default network: 5 convs a block, no skip convs, mapped global condition, gaussian mixture
    'd5_r32_k2_noskipch_global_gauss': (dict(blocks=2, layers_per_block=5, channels=32, kernel_size=2, dilation_bound=64,
                                             final_layers_channels=[16], activation='leaky_relu', conditioning='global',
                                             mapping_layers=[6, 8], mapping_activation='leaky_relu', cond_inputs=3,
                                             num_mixtures=4, sampling_function='gaussian', bits=16), 2, 47),
    'd2_r8_k3_noskipch_nohead_relu': (dict(blocks=2, layers_per_block=2, channels=8, kernel_size=3, dilation_bound=81,
                                           activation='relu', bits=4), 2, 40),
    'd3_r16_k2_global_unmapped_skip': (dict(blocks=2, layers_per_block=3, channels=16, kernel_size=2, dilation_bound=64,
                                            skip_channels=8, final_layers_channels=[12], activation='relu',
                                            conditioning='global', cond_inputs=4, bits=4), 3, 61),
    'd2_r8_k2_mol': (dict(blocks=3, layers_per_block=2, channels=8, kernel_size=2, dilation_bound=64, skip_channels=16,
                          final_layers_channels=[8], activation='leaky_relu', num_mixtures=3, sampling_function='logistic',
                          bits=16), 2, 50),
}
DROPOUT = (0.1, 123, 7)                            # (rate, seed, step)
# (network, dropout rate): every deep network with and without dropout, two depth-1 networks with it
DEEP_CASES = [(n, r) for n in DEEP for r in (0.0, 0.1)] + [('r16_k2_skip_head', 0.1), ('r8_k3_global_unmapped', 0.1)]


@functools.lru_cache(maxsize=None)
def _autograd(name, rate=0.0):
  kw, B, T = (NETS.get(name) or DEEP[name])
  cfg = O.OracleConfig(**kw)
  L = cfg.layers_per_block
  dropout = (rate,) + DROPOUT[1:] if rate > 0 else None
  assert max(O.dilation_schedule(cfg)) > T / 2
  names = [n for n, _ in O.param_shapes(cfg)]
  ps = [p.double().requires_grad_(True) for p in O.init_params(cfg, seed=3, bias_range=0.3, dtype=torch.float64)]
  x = O.synthetic_waveform(B, T + 1, seed=7).double()
  cond = None
  if cfg.cond_inputs:
    cond = torch.rand(B, cfg.cond_inputs, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
  pred, inter = O.model_forward(x[:, :-1], ps, cfg, cond, return_intermediates=True, dropout=dropout)
  loss = O.loss_fn(O.prepare_target(x[:, 1:], cfg), pred, cfg).sum() / B
  nf, N = len(cfg.final_layers_channels), cfg.blocks
  pre = inter['head_pre'] + [inter['logits']]
  want = {('GF', i): pre[i] for i in range(nf + 1)}
  want.update({('GU', b): inter['u'][b] for b in range(N)})
  want.update({('GH', b): inter['h'][b] for b in range(N + 1)})
  want.update({('GP', b, i): inter['pre'][b][i] for b in range(N) for i in range(L - 1)})
  want['g_skipsum'] = inter['skip_sum']
  keys = list(want)
  gr = torch.autograd.grad(loss, [want[k] for k in keys] + ps, allow_unused=True)
  grads = {k: (g if g is not None else torch.zeros_like(want[k])) for k, g in zip(keys, gr)}
  pgrads = {n: (g if g is not None else torch.zeros_like(p)) for n, g, p in zip(names, gr[len(keys):], ps)}
  ws = dict(grads)
  for b in range(N + 1):
    ws['H', b] = inter['h'][b].detach()
  for b in range(N):
    # (Z with a padded leading dimension, as the workspace keeps it: the restatement must ignore the padding)
    z = inter['z'][b].detach()
    ws['Z', b] = torch.cat([z, torch.full_like(z[..., :3], 7.0)], dim=-1)
    ws['AG', b] = inter['gate'][b].detach()
    for i in range(L - 1):
      ws['P', b, i] = inter['p'][b][i].detach()
    if dropout:
      ws['XD', b] = inter['xd'][b].detach()
  for i in range(nf):
    ws['HA', i] = O.activation(inter['head_pre'][i].detach(), cfg.activation)
  ws['skipsum'] = inter['skip_sum'].detach()
  params = {n: p.detach() for n, p in zip(names, ps)}
  fwd = {('H', b): inter['h'][b].detach() for b in range(N + 1)}
  fwd.update({('Z', b): inter['z'][b].detach() for b in range(N)})
  fwd.update({k: v for k, v in ws.items() if k[0] in ('AG', 'P', 'XD')})
  fwd['skipsum'] = ws['skipsum']
  return cfg, names, params, x[:, :-1], cond, ws, grads, pgrads, dropout, fwd


def _check(tag, restated, grads, pgrads, names, cfg):
  assert sorted(R.param_names(restated)) == sorted(names), tag          # nothing silently uncovered
  nf, N = len(cfg.final_layers_channels), cfg.blocks
  data = [('GF', i) for i in range(nf)] + [('GU', b) for b in range(N)] + [('GH', b) for b in range(N + 1)]
  data += [('GP', b, i) for b in range(N) for i in range(cfg.layers_per_block - 1)]
  for k in data:
    assert k in restated, (tag, k)
  zero_by_design = set()
  if cfg.use_skip:                                 # nothing flows into the last block's output ...
    zero_by_design.add(('GH', N))
    if cfg.skip_channels is not None:              # ... so its 1x1 conv towards it is unused
      zero_by_design |= {('param', f'block{N - 1}/conv1/kernel'), ('param', f'block{N - 1}/conv1/bias')}
  elif cfg.skip_channels is not None:              # use_skip False: the skip convs are unused
    zero_by_design |= {('param', f'block{b}/conv_skip/{w}') for b in range(N) for w in ('kernel', 'bias')}
  for k, got in restated.items():
    ref = pgrads[k[1]] if k[0] == 'param' else grads[k]
    assert got.shape == ref.shape, (tag, k, got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= 1e-10 * scale, (tag, k, err, scale)
    if k not in zero_by_design:
      assert scale > 0, (tag, k)                                         # a comparison of zeros with zeros proves nothing


@pytest.mark.parametrize('name', list(NETS))
def test_restatement_equals_fp64_autograd(name):
  cfg, names, params, x_in, cond, ws, grads, pgrads, _, _ = _autograd(name)
  restated = R.restate(cfg, params, x_in, cond, ws, folded=False)
  assert ('g_skipsum' in restated) == cfg.use_skip
  _check(name, restated, grads, pgrads, names, cfg)


@pytest.mark.parametrize('name', [n for n, (kw, _, _) in NETS.items()
                                  if kw.get('skip_channels') and kw.get('final_layers_channels') and kw.get('use_skip', True)])
def test_folded_form_equals_fp64_autograd(name):
  cfg, names, params, x_in, cond, ws, grads, pgrads, _, _ = _autograd(name)
  ws = {k: v for k, v in ws.items() if k not in ('skipsum', 'g_skipsum')}        # a folded pass never forms them
  restated = R.restate(cfg, params, x_in, cond, ws, folded=True)
  assert 'g_skipsum' not in restated
  _check(name + ' folded', restated, grads, pgrads, names, cfg)


def _id(case):
  return f'{case[0]}-drop{case[1]}'


@pytest.mark.parametrize('case', DEEP_CASES, ids=_id)
def test_deep_and_dropout_restatement_equals_fp64_autograd(case):
  name, rate = case
  cfg, names, params, x_in, cond, ws, grads, pgrads, dropout, _ = _autograd(name, rate)
  assert (dropout is not None) == (rate > 0)
  restated = R.restate(cfg, params, x_in, cond, ws, folded=False, dropout=dropout)
  assert ('g_skipsum' in restated) == cfg.use_skip
  _check(_id(case), restated, grads, pgrads, names, cfg)
  if cfg.layers_per_block == 1 and cfg.skip_channels and cfg.final_layers_channels:      # the folded form under dropout
    ws = {k: v for k, v in ws.items() if k not in ('skipsum', 'g_skipsum')}
    restated = R.restate(cfg, params, x_in, cond, ws, folded=True, dropout=dropout)
    _check(_id(case) + ' folded', restated, grads, pgrads, names, cfg)


@pytest.mark.parametrize('case', [(n, 0.0) for n in NETS] + DEEP_CASES, ids=_id)
def test_forward_restatement_equals_the_oracle_pass(case):
  name, rate = case
  cfg, names, params, x_in, cond, ws, _, _, dropout, fwd = _autograd(name, rate)
  N, L = cfg.blocks, cfg.layers_per_block
  for folded in (False, True):
    if folded and not (cfg.use_skip and cfg.skip_channels and cfg.final_layers_channels):
      continue
    given = {k: v for k, v in ws.items() if k[0] in ('H', 'Z', 'P', 'XD')}           # what the forward kernels read
    restated = R.restate_forward(cfg, params, x_in, cond, given, folded, dropout=dropout)
    want = [('H', b) for b in range(N + 1)] + [(k, b) for k in ('AG', 'Z') for b in range(N)]
    want += [('P', b, i) for b in range(N) for i in range(L - 1)]
    want += [('XD', b) for b in range(N)] if rate > 0 else []
    want += ['skipsum'] if cfg.use_skip and not folded else []
    assert sorted(restated, key=str) == sorted(want, key=str), (case, folded)
    for k, got in restated.items():
      ref = fwd[k]
      assert got.shape == ref.shape, (case, k)
      scale = ref.abs().max().item()
      assert scale > 0, (case, k)
      if k[0] == 'XD':
        assert torch.equal(got, ref), (case, k)
        dropped = (got == 0) & (ws['H', k[1]] != 0)
        assert 0 < int(dropped.sum()) < got.numel() // 4, (case, k)                 # a mask, and of about the rate
      else:
        err = (got - ref).abs().max().item()
        assert err <= 1e-10 * scale, (case, k, err, scale)


def test_depth_and_dilations_of_the_deep_cases():
  """Stacks of 2, 3 and 5 convs, both kernel sizes, 8 to 32 channels, and in each a dilation above T / 2."""
  assert {kw['layers_per_block'] for kw, _, _ in DEEP.values()} == {2, 3, 5}
  assert {kw['kernel_size'] for kw, _, _ in DEEP.values()} == {2, 3}
  assert {kw['channels'] for kw, _, _ in DEEP.values()} == {8, 16, 32}
  assert {kw['activation'] for kw, _, _ in DEEP.values()} == {'relu', 'leaky_relu'}
  for kw, B, T in DEEP.values():
    assert 2 <= B <= 3 and 40 <= T <= 67 and max(O.dilation_schedule(O.OracleConfig(**kw))) > T / 2


def test_oracle_intermediates_are_the_graph_tensors():
  """u, gate and z per block (additions to model_forward(return_intermediates=True)): z = tanh(u_f) * sigmoid(u_g) and
  gate = sigmoid(u_g) exactly, and the next block input follows from z."""
  kw, B, T = NETS['r16_k2_skip_head']
  cfg = O.OracleConfig(**kw)
  ps = O.init_params(cfg, seed=3, dtype=torch.float64)
  names = [n for n, _ in O.param_shapes(cfg)]
  x = O.synthetic_waveform(B, T, seed=7).double()
  _, inter = O.model_forward(x, ps, cfg, return_intermediates=True)
  assert inter['p'] == inter['pre'] == [[]] * cfg.blocks and all(a is b for a, b in zip(inter['xd'], inter['h']))
  assert len(inter['u']) == len(inter['gate']) == len(inter['z']) == cfg.blocks
  for b in range(cfg.blocks):
    u, g, z = inter['u'][b], inter['gate'][b], inter['z'][b]
    assert u.shape == (B, T, 2 * cfg.D) and g.shape == z.shape == (B, T, cfg.D)
    assert torch.equal(g, torch.sigmoid(u[..., cfg.D:])) and torch.equal(z, torch.tanh(u[..., :cfg.D]) * g)
    w_r, b_r = ps[names.index(f'block{b}/conv1/kernel')], ps[names.index(f'block{b}/conv1/bias')]
    assert torch.equal(inter['h'][b + 1], z @ w_r[0] + b_r + inter['h'][b])
