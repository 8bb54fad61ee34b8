"""Stacked dilated convs (layers_per_block > 1) and dropout at the size where a persistent wave takes several tiles and
the shifted-plane kernel a second pass -- what tests/test_gpu_fwd_tile_walk.py and tests/test_gpu_bwd_tile_walk.py leave
out.  Same B = 5, T = 27001, data and weights as those two files.

Code that runs only for these networks: wn_gemm_planes16s_kernel<2, 2, ACT, SHIFT = true> for every inner conv of a 32- or
64-channel stack (forward with positive shifts, backward as ACT = -2 with negative shifts, a power-of-two operand scale,
act'(aux) in the epilogue and a published max-abs; at most 512 workgroups of 4 waves of 64 rows, so 5 x 422 = 2110 tiles
are two passes, the second with 62 live tiles and 1986 dead waves that still take part in the barriers and the weight
ring); the rows contractions on 32-wide images padded to two row tiles; the gated last conv of the fused forward kernels
with a residual source that is not its conv input (a.res); wn_dropout_kernel forward and backward, and with it the per-block
backward of depth-1 networks off the pair chain; wn_wgrad_layer_kernel's INNER form and the batched job table over every
conv of every stack.

Test A compares every tensor the block stack and the backward phase leave in the workspace and every parameter gradient
with tests/bwd_restatement.py (each product restated in float64 from the tensors its own kernel read, pinned against fp64
autograd in tests/test_bwd_restatement_cpu.py), in both math modes, at the project's bars: activations
1e-4 absolute, data gradients 1e-4 of the tensor's max, parameter gradients 1e-4 of the tensor's max + 1e-7, XD bitwise.

Test B is bitwise, in split mode, for the cases without dropout: forward tensors of five different utterances against each
utterance alone, data gradients of five copies of one utterance against it alone (the backward operands are scaled by
running max-abs over the whole tensor: distinct utterances are not bit-comparable across batch sizes), and the logits of
an inference pass (the exact-fp32 composed kernels) against each utterance alone.  Dropout cases are left out of test B:
the mask is a hash of the element's index in the whole batch, so a copy in another batch position gets another mask.

Measured worst ratios, the mutants these tests catch and run times: DESIGN.md section 19."""
import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O
from test_gpu_baseline_nets import REFERENCE_DEFAULT
from test_gpu_bwd_tile_walk import CASES as BWD_CASES, EXACT as FLAT_EXACT, FOLDED, UNFOLDED

pytestmark = pytest.mark.gpu

B, T = 5, 27001
SEED = 123

DEEP_FWD = 'per conv of the stack, split precision in training passes'
DEEP_BWD = 'per-block composed backward, one rows contraction per conv of the stack (layers_per_block > 1)'
INNER = "inner convs through the kernel's INNER form (wn_wgrad_layer_kernel)"
BATCH_SPLIT = 'generic batched job table, split precision, every conv of every stack in one launch (wn_wgrad_batched_kernel)'
DEEP_EXACT = ('exact fp32 MFMA', 'composed per conv (rows GEMM fp32', DEEP_BWD,
              'generic batched job table in exact fp32, every conv of every stack in one launch (wn_wgrad_batched_kernel)',
              UNFOLDED)
# case: (constructor keywords, dropout rate, texts wn_plan_describe must hold in split mode, in exact-fp32 mode)
CASES = {
    # the network the benchmark times: padded 32-wide images, S == 0 / GO path, conditioning, mixture head, dropout,
    # wn_wgrad_layer_kernel INNER
    'deep32_default': (REFERENCE_DEFAULT, 0.1, (DEEP_FWD, DEEP_BWD, INNER, UNFOLDED), DEEP_EXACT),
    # the same without dropout: separates the mask from the stack, and allows the bitwise test
    'deep32_default_nodrop': (REFERENCE_DEFAULT, 0.0, (DEEP_FWD, DEEP_BWD, INNER, UNFOLDED), DEEP_EXACT),
    # 64-wide (unpadded) images, the [W_r | W_s] image, unfolded skip path
    'deep64_skip': (dict(blocks=3, layers_per_block=3, channels=64, dilation_bound=128, skip_channels=128,
                         final_layers_channels=[64], activation='leaky_relu'), 0.0,
                    (DEEP_FWD, DEEP_BWD, INNER, UNFOLDED), DEEP_EXACT),
    # three shifted planes; the split-precision batched weight-gradient table (wn_wgrad_layer_kernel is a KS = 2 kernel)
    'deep32_k3': (dict(blocks=3, layers_per_block=2, kernel_size=3, dilation_bound=81, channels=32, skip_channels=64,
                       final_layers_channels=[32], activation='relu'), 0.0,
                  (DEEP_FWD, DEEP_BWD, BATCH_SPLIT, UNFOLDED), DEEP_EXACT),
    # depth 1 with dropout.  wn_plan_describe does not show the per-call decision (TrainPaths::bwd_pairs() is false under
    # dropout): the chain runs per block through block_backward, not wn_bwd_pair_kernel / wn_bwd_s128_kernel; the fused
    # forward gets XD[b] as its conv input and H[b] as a separate residual; the weight-gradient family stays the plan's
    'drop_r64': (BWD_CASES['r64_pair'][0], 0.1, BWD_CASES['r64_pair'][1], FLAT_EXACT),
    'drop_r128': (BWD_CASES['r128'][0], 0.1, BWD_CASES['r128'][1], FLAT_EXACT),
}
NODROP = [c for c, v in CASES.items() if v[1] == 0.0]


def test_the_shape_gives_the_shifted_plane_kernel_a_second_pass():
  per32, per64 = -(-T // 32), -(-T // 64)
  assert per32 == 844 and B * per32 == 4220 > 4096     # fused and rows kernels: 2 or 3 tiles of 32 rows a wave
  assert per64 == 422 and B * per64 == 2110 > 2048     # shifted-plane kernel: gx capped at 512 workgroups x 4 waves
  assert B * per64 - 2048 == 62 and 2 * 2048 - B * per64 == 1986       # second pass: 62 live tiles, 1986 dead waves
  assert T % 32 == 25 and T % 64 == 57                 # ragged last tiles
  assert per64 <= 2048 and -(-per64 // 4) == 106       # one utterance alone: a single pass on 106 workgroups
  for case in ('deep32_default', 'deep32_default_nodrop', 'deep64_skip', 'deep32_k3'):
    kw = CASES[case][0]
    C, KS = kw['channels'], kw.get('kernel_size', 2)
    assert kw['layers_per_block'] > 1
    # the launcher's conditions for the shifted-plane form: output width, at least three k-steps of weights, 32-bit offsets
    assert C in (32, 64) and KS * (C // 16) >= 3 and B * T * C * 4 < 2 ** 32, case


def _dev():
  return torch.device('cuda', 0)


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


def _model(case, exact):
  from wavenets_amd import WaveNet
  kw, rate, split_texts, exact_texts = CASES[case]
  kw = dict(kw)
  kw.setdefault('sampling_function', 'categorical')
  kw.setdefault('bits', 8)
  model = WaveNet(**kw, dropout=rate, seed=SEED, device=_dev())
  if kw.get('conditioning'):
    model.build([(1, 8, 1), (1, B)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  report = model.kernel_report()
  for text in (exact_texts if exact else split_texts):
    assert text in report, (case, text, report)        # the family the case is there for: no drift to another path
  ocfg = O.OracleConfig(**kw, cond_inputs=B if kw.get('conditioning') else 0)
  return model, ocfg


def _region(model, what, idx, b):
  return model.training_intermediate(what, idx, b, T).reshape(b, T, -1)


def _folded(model):
  return FOLDED in model.kernel_report()


def _forward_tensors(model, ocfg, b):
  """Clones of everything the block stack's forward left in the workspace, as (b, T, channels)."""
  N, L = ocfg.blocks, ocfg.layers_per_block
  out = {('H', i): _region(model, 0, i, b).clone() for i in range(N + 1)}
  for i in range(N):
    out['Z', i] = _region(model, 1, i, b)[..., :ocfg.D].clone()
    out['AG', i] = _region(model, 2, i, b).clone()
    for j in range(L - 1):
      out['P', i, j] = _region(model, 11, i * (L - 1) + j, b).clone()
    if model.dropout > 0:
      out['XD', i] = _region(model, 14, i, b).clone()
  if not _folded(model):
    out['skipsum'] = _region(model, 3, 0, b).clone()
  return out


def _data_gradients(model, ocfg, b):
  """Clones of every data gradient the backward phase left in the workspace, as (b, T, channels)."""
  N, L, nf = ocfg.blocks, ocfg.layers_per_block, len(ocfg.final_layers_channels)
  out = {('GF', i): _region(model, 6, i, b).clone() for i in range(nf + 1)}     # (GF[nf] = dL/dlogits first)
  out.update({('GU', i): _region(model, 8, i, b).clone() for i in range(N)})
  out.update({('GP', i, j): _region(model, 13, i * (L - 1) + j, b).clone() for i in range(N) for j in range(L - 1)})
  out.update({('GH', i): _region(model, 9, i, b).clone() for i in range(N + 1)})
  if not _folded(model):
    out['g_skipsum'] = _region(model, 7, 0, b).clone()
  return out


ACTIVATIONS = ('H', 'Z', 'AG', 'P', 'skipsum')


def _family(key, L):
  if key == 'skipsum':
    return 'skip sum'
  if key == 'g_skipsum' or key[0] == 'GF':
    return 'head data gradients'
  fams = {'XD': 'XD (wn_dropout_kernel)', 'P': 'P (inner convs, forward)', 'AG': 'AG, Z (gated last conv)',
          'Z': 'AG, Z (gated last conv)', 'H': 'H (input conv; 1x1 + residual)', 'GU': 'GU (1x1 / skip + gate derivative)',
          'GP': 'GP (inner convs, backward)', 'GH': 'GH (first conv backward, mask, residual)'}
  if key[0] in fams:
    return fams[key[0]]
  n = key[1]
  for i in range(L - 1):
    if f'/dil{i}/' in n:
      return 'inner dW_d, db_d'
  for part, fam in (('/dil', 'dW_d, db_d'), ('conv1', 'dW_r, db_r'), ('conv_skip', 'dW_s, db_s'), ('conv_cond', 'dW_c, db_c'),
                    ('final', 'head dW_f, db_f'), ('causal', 'input conv dW, db'), ('mapping', 'mapping net')):
    if part in n:
      return fam
  raise KeyError(key)


@pytest.mark.parametrize('case', list(CASES))
def test_every_product_of_the_pass_against_its_fp64_restatement(case, math_mode):
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, math_mode == 'fp32')
  N, L, nf = ocfg.blocks, ocfg.layers_per_block, len(ocfg.final_layers_channels)
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None      # a different one-hot condition per utterance
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())              # five different utterances
  assert model._world() == 1
  loss, _, _ = model.loss_and_grads((x, cond) if cond is not None else x)       # (arms the dropout mask of this call)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  # the mask the pass used, as the model armed it (_arm_dropout: one process, the call counter after the call)
  dropout = (model.dropout, model._seed, model._drop_step) if model.dropout > 0 else None
  assert (dropout is not None) == (CASES[case][1] > 0) and (dropout is None or dropout[1:] == (SEED, 1))

  raw = _forward_tensors(model, ocfg, B)
  raw.update(_data_gradients(model, ocfg, B))
  folded = _folded(model)
  assert not (folded and L > 1)
  got = {k: v.double() for k, v in raw.items()}
  ws = dict(got)
  for i in range(nf):
    ws['HA', i] = _region(model, 4, i, B).double()
  names = model.variable_names
  for n, g in zip(names, model.gradients()):
    got['param', n] = g.double()
  for k in [('GU', b) for b in range(N)] + [('GH', b) for b in range(N)] + \
           [('GP', b, i) for b in range(N) for i in range(L - 1)]:
    assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0.0, (case, k)

  params = {n: t.double() for n, t in zip(names, model.trainable_variables)}
  x_in, c64 = x[:, :-1].double(), cond.double() if cond is not None else None
  ref = R.restate_forward(ocfg, params, x_in, c64, ws, folded, dropout=dropout)
  ref.update(R.restate(ocfg, params, x_in, c64, ws, folded, dropout=dropout))
  assert sorted(R.param_names(ref)) == sorted(names)                    # nothing silently uncovered
  missing = [k for k in got if k != ('GF', nf) and k not in ref]
  assert not missing, sorted(missing, key=str)
  assert (('XD', 0) in ref) == (dropout is not None) and (('P', 0, 0) in ref) == (('GP', 0, 0) in ref) == (L > 1)

  worst, failures = {}, []
  for k, r in ref.items():
    fam = _family(k, L)
    if k[0] == 'XD':                                                    # one fp32 multiply: bitwise
      g32, r32 = raw[k], r.float()
      assert bool((r32 == 0).any()) and bool((r32 != 0).any()), (case, k)
      same = torch.equal(g32, r32)
      worst[fam] = (max(worst.get(fam, (0.0, None))[0], 0.0 if same else 1.0), k)
      if not same:
        rows = (g32 != r32).any(dim=-1)
        u, t = divmod(int(rows.flatten().nonzero()[0]), T)
        failures.append(f'{k}: not bitwise equal; first row: utterance {u}, t {t}; rows that differ: {int(rows.sum())}')
      continue
    g = got[k].reshape(r.shape)
    scale = float(r.abs().max())
    diff = (g - r).abs()
    err = float(diff.max())
    if k == 'skipsum' or k[0] in ACTIVATIONS:
      bar = 1e-4
    else:
      bar = 1e-4 * scale + (1e-7 if k[0] == 'param' else 0.0)
    ratio = err / bar if bar > 0 else 0.0
    if ratio >= worst.get(fam, (0.0, None))[0]:
      worst[fam] = (ratio, k)
    if not err <= bar:
      where = ''
      if k[0] != 'param':
        rows = diff.amax(dim=-1)
        u, t = divmod(int(rows.argmax()), T)
        where = (f' worst row: utterance {u}, t {t} (32-row tile {t // 32}, 64-row tile {t // 64});'
                 f' rows over the bar: {int((rows > bar).sum())}')
      failures.append(f'{k}: max|got - ref| {err:.3e} > {bar:.3e} (max|ref| {scale:.3e}){where}')
  for fam, (ratio, k) in sorted(worst.items()):
    print(f'{case} [{math_mode}] {fam}: worst max|err| / bar {ratio:.2e} at {k}')
  assert not failures, (case, math_mode, failures)


def _rows(a, b):
  return (a != b).any(dim=-1).nonzero()[:8].flatten().tolist()


@pytest.mark.parametrize('case', NODROP)
def test_forward_rows_do_not_depend_on_the_wave_the_tile_or_the_pass(case):
  """Five different utterances in one pass (2110 tiles of 64 rows: two passes of the shifted-plane kernel; 4220 tiles of
  32 rows) against each utterance alone (422 tiles, one pass; 844 tiles, at most one a wave)."""
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, False)
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())
  loss, _, _ = model.loss_and_grads((x, cond) if cond is not None else x)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  batch = _forward_tensors(model, ocfg, B)
  assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0.0 for v in batch.values())
  assert any(k[0] == 'P' for k in batch)
  for u in range(B):
    xu = x[u:u + 1].contiguous()
    loss_u, _, _ = model.loss_and_grads((xu, cond[u:u + 1]) if cond is not None else xu)
    torch.cuda.synchronize()
    assert float(loss_u[2]) == 0.0, 'range guard tripped'
    alone = _forward_tensors(model, ocfg, 1)
    assert set(alone) == set(batch)
    for k, v in alone.items():
      assert torch.equal(batch[k][u], v[0]), \
          (case, k, u, (batch[k][u] - v[0]).abs().max().item(), _rows(batch[k][u], v[0]))


@pytest.mark.parametrize('case', NODROP)
def test_data_gradients_of_copies_of_one_utterance_equal_it_alone_bit_for_bit(case):
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, False)
  nf = len(ocfg.final_layers_channels)
  x1 = synthetic_waveforms(1, T + 1, seed=5, device=_dev())
  cond1 = torch.eye(B, device=_dev())[2:3] if ocfg.cond_inputs else None
  xb = x1.expand(B, -1, -1).contiguous()
  condb = cond1.expand(B, -1).contiguous() if cond1 is not None else None

  loss, _, _ = model.loss_and_grads((xb, condb) if condb is not None else xb, global_batch=B)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  batch = _data_gradients(model, ocfg, B)
  assert any(k[0] == 'GP' for k in batch)
  for k, v in batch.items():
    assert bool(torch.isfinite(v).all()), (case, k)
    if k[0] in ('GU', 'GF', 'GP') or (k[0] == 'GH' and k[1] < ocfg.blocks):
      assert float(v.abs().max()) > 0.0, (case, k)
  # the same 1 / global_batch keeps the rows of dL/dlogits what they were in the batch
  loss1, _, _ = model.loss_and_grads((x1, cond1) if cond1 is not None else x1, global_batch=B)
  torch.cuda.synchronize()
  assert float(loss1[2]) == 0.0, 'range guard tripped'
  alone = _data_gradients(model, ocfg, 1)
  assert set(alone) == set(batch)
  for k in [('GF', nf)] + [k for k in batch if k != ('GF', nf)]:        # dL/dlogits first: everything else follows from it
    for u in range(1, B):
      assert torch.equal(batch[k][u], batch[k][0]), \
          (case, k, f'utterance {u} of the batch != utterance 0', (batch[k][u] - batch[k][0]).abs().max().item(),
           _rows(batch[k][u], batch[k][0]))
    assert torch.equal(batch[k][0], alone[k][0]), \
        (case, k, 'utterance 0 of the batch != the utterance alone', (batch[k][0] - alone[k][0]).abs().max().item(),
         _rows(batch[k][0], alone[k][0]))


@pytest.mark.parametrize('case', NODROP)
def test_inference_logits_of_the_batch_equal_each_utterance_alone(case):
  """Inference of deep stacks runs the exact-fp32 composed kernels, which no other multi-tile test touches."""
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, False)
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())[:, :-1].contiguous()
  batch = model.logits((x, cond) if cond is not None else x).clone()
  assert not model.range_tripped_last_forward()
  assert bool(torch.isfinite(batch).all()) and float(batch.abs().max()) > 0.0
  for u in range(B):
    xu = x[u:u + 1].contiguous()
    alone = model.logits((xu, cond[u:u + 1]) if cond is not None else xu)
    assert torch.equal(batch[u], alone[0]), (case, u, (batch[u] - alone[0]).abs().max().item(), _rows(batch[u], alone[0]))
