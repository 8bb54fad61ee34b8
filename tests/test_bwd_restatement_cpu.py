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
skip sum) is pinned against the same pass: XD exactly, everything else to 1e-10 of its max.

The head's restatement is pinned on all of these networks, folded and unfolded: HA, the logits of
O.model_forward, the loss of O.loss_and_grads and the autograd dL/dlogits, to 1e-12 of each tensor's max."""
import functools
import math

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
  fwd['logits'], fwd['x_full'] = inter['logits'].detach(), x               # (for the head's pin below)
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


def _can_fold(kw):
  return bool(kw.get('skip_channels') and kw.get('final_layers_channels') and kw.get('use_skip', True))


# (network, folded): every network in the unfolded form, and in the folded form where a head can fold
HEAD_CASES = [(n, f) for n, (kw, _, _) in list(NETS.items()) + list(DEEP.items())
              for f in ((False, True) if _can_fold(kw) and kw.get('layers_per_block', 1) == 1 else (False,))]


def test_the_head_cases_hold_every_head_form():
  kws = {n: (NETS.get(n) or DEEP[n])[0] for n, _ in HEAD_CASES}
  cat = lambda kw: kw.get('sampling_function', 'categorical') == 'categorical'
  assert any(f and cat(kws[n]) for n, f in HEAD_CASES) and any(not f and cat(kws[n]) and _can_fold(kws[n]) for n, f in HEAD_CASES)
  assert any(kw.get('skip_channels') is None and kw.get('final_layers_channels') for kw in kws.values())
  assert any(kw.get('use_skip') is False for kw in kws.values())
  assert any(not kw.get('final_layers_channels') and kw.get('skip_channels') for kw in kws.values())
  assert any(not kw.get('final_layers_channels') and kw.get('skip_channels') is None for kw in kws.values())
  assert {kw.get('sampling_function', 'categorical') for kw in kws.values()} == {'categorical', 'logistic', 'gaussian'}


@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: f'{c[0]}-{"folded" if c[1] else "unfolded"}')
def test_head_restatement_equals_the_oracle_and_fp64_autograd(case):
  """restate_head fed with the oracle's own fp64 intermediates: HA[i], the logits of O.model_forward, the loss of
  O.loss_and_grads and the dL/dlogits of the one fp64 autograd pass of _autograd, each to 1e-12 of the tensor's max.  Twice:
  without a stored logits tensor (the fused loss epilogue: the loss from HA[nf-1] through the last conv) and with one (the
  standalone loss kernels), the second with the stored logits scaled and shifted so that a restatement that ignored them
  would show.  global_batch is 2 B: the loss and the gradient halve exactly.

  One quantity does not fit 1e-12: dL/dpred of a LOGISTIC head at bits = 16.  A bin mass is the difference of two sigmoids,
  each off by up to 2^-53, so the likelihood (weights sum to 1) is off by up to 2^-52 ABSOLUTE against a value of e^-row
  (1e-5 and less), i.e. 2^-52 e^row relative, and the row's gradient with it; the numerators sigmoid'(a) - sigmoid'(b)
  cancel alike, times e^-ls.  Any two fp64 evaluations that round one sigmoid differently are that far apart:
  O.loss_logistic (autograd's) against O.loss_logistic_exact (restate_head's) by 1.0e-10 of the tensor's max, and
  O.loss_logistic_exact against ITSELF over 37-row chunks instead of the whole tensor (another vector lane, another last
  bit) by 1.5e-11.  That gradient is therefore held to 4 * 2^-52 e^(max row) max(1, e^-min ls) of the tensor's max (1e-9 to
  1e-8 here) and a single loss row, where the likelihood's relative error is the absolute one, to 4 * 2^-52 e^(max row); the
  loss, the sum in which those errors average out, stays at 1e-12 like everything else."""
  name, folded = case
  cfg, names, params, x_in, cond, ws, grads, _, _, fwd = _autograd(name)
  nf, N, M = len(cfg.final_layers_channels), cfg.blocks, cfg.num_mixtures
  Bn = x_in.shape[0]
  x = fwd['x_full']
  y_true = x[:, 1:]
  given = {k: v for k, v in ws.items() if k[0] in ('Z', 'HA')}
  if not folded:
    given.update({'skipsum': ws['skipsum']} if cfg.use_skip else {('H', N): ws['H', N]})
  loss_ref = O.loss_and_grads(x, [params[n] for n in names], cfg, cond, global_batch=2 * Bn)[0]
  want = {('HA', i): ws['HA', i] for i in range(nf)}
  want.update({'logits': fwd['logits'], ('GF', nf): grads['GF', nf] * 0.5, 'loss': loss_ref})

  def check(tag, got, ref, rows, stored):
    for k, r in ref.items():
      assert got[k].shape == r.shape, (case, tag, k)
      scale = r.abs().max().item()
      assert scale > 0, (case, tag, k)
      tol = 1e-12 * scale
      if cfg.sampling_function == 'logistic' and k in (('GF', nf), 'loss_rows'):
        ls = stored[..., 2 * M:].clamp(min=-7.0)
        bar = 4 * 2.0 ** -52 * math.exp(rows.max().item())
        assert 1e-12 < bar < 1e-8, (case, tag, bar)
        # (a row's loss: the likelihood's relative error, absolute; the gradient: relative, with the e^-ls of its numerators)
        tol = bar if k == 'loss_rows' else bar * max(1.0, math.exp(-ls.min().item())) * scale
      err = (got[k] - r).abs().max().item()
      assert err <= tol, (case, tag, k, err, scale, tol)

  got = R.restate_head(cfg, params, given, folded, y_true, 2 * Bn, row_chunk=37)      # chunks that do not divide B T
  assert sorted((k for k in got if k not in ('loss_rows', 'target_prob')), key=str) == sorted(want, key=str)
  assert ('target_prob' in got) == (M is None) and got['loss_rows'].shape == x_in.shape[:2]
  check('from HA', got, want, got['loss_rows'], fwd['logits'])
  assert abs(got['loss_rows'].sum().item() / (2 * Bn) - loss_ref.item()) <= 1e-12 * abs(loss_ref.item())

  # with a stored logits tensor the loss follows IT, the restated logits still follow HA[nf-1]
  shifted = fwd['logits'] * 1.25 + 0.01
  lg = shifted.clone().requires_grad_(True)
  pred = torch.softmax(lg, -1) if M is None else lg
  rows = O.loss_fn(O.prepare_target(y_true, cfg), pred, cfg)
  g_ref, = torch.autograd.grad(rows.sum() / (2 * Bn), lg)
  rows = rows.detach()
  got2 = R.restate_head(cfg, params, dict(given, logits=shifted), folded, y_true, 2 * Bn)
  check('from stored logits', got2, {'logits': fwd['logits'], ('GF', nf): g_ref, 'loss': rows.sum() / (2 * Bn),
                                     'loss_rows': rows}, rows, shifted)


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
