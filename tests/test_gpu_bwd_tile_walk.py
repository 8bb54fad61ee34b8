"""The backward-data chain and the weight-gradient kernels at the size where a persistent wave takes a second and a third
32-row tile -- the backward counterpart of test_gpu_fwd_tile_walk.py, which runs the same training pass and compares only
H, Z and AG.

wn_bwd_pair_kernel, wn_bwd_s128_kernel and the rows contractions of wn_gemm16.hip / wn_gemm.hip walk the tiles with
wn_tile_walk (wn_common.h) and carry more state across a tile boundary than the forward kernel: a four-deep register ring
whose last refills already belong to the wave's next tile, an `ok` mask per ring slot, a per-tile power-of-two scale and
running max-abs slots.  One pass over 5 utterances of T = 27001 predicted samples is 5 x 844 = 4220 tiles: 2 or 3 tiles a
wave on 256 workgroups of 8 waves, ragged last tiles (27001 = 32 * 843 + 25), ragged last weight-gradient chunks
(27001 = 16 * 1687 + 9) and waves whose next tile belongs to the next utterance.

Test A compares every GH[b], GU[b], GF[i] and every parameter gradient with tests/bwd_restatement.py: each product restated
in float64 from the tensors its own kernel read (pinned against fp64 autograd in tests/test_bwd_restatement_cpu.py), in both
math modes, at the project's bar.  A wrong row or tile in a data gradient is an O(1) elementwise
error; a weight gradient that loses one row per utterance (5 of 135 005) moves by 1e-4 to 2e-4 of its max (measured with
a mutant, DESIGN.md section 18: the sums are largely same-sign), which this bar sees only just; a lost tile is clear.

Test B is bitwise: five copies of one utterance against that utterance alone (one utterance is 844 tiles on 106 workgroups:
the other branch of the walk, at most one tile a wave).  Copies, because the backward operands are scaled by running
max-abs over the whole tensor: distinct utterances are not bit-comparable across batch sizes.

Measured worst ratios, the mutants these tests catch and run times: DESIGN.md section 18."""
import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu

B, T = 5, 27001

PAIR = 'wn_bwd_pair_kernel'
S128 = 'wn_bwd_s128_kernel'
ROWS = 'two split-precision rows contractions per block'
LAYER = 'wn_wgrad_layer_kernel'
FOLDED = 'skip path: folded'
UNFOLDED = 'skip path: one contraction over all blocks'
# case: (constructor keywords, texts wn_plan_describe must hold in split mode)
CASES = {
    # dilations 1 .. 64: the reversed tap lies in the same tile, in a neighbour tile or past the utterance's end
    'r64_pair': (dict(blocks=7, dilation_bound=128, channels=64, skip_channels=256, final_layers_channels=[128, 64]),
                 (PAIR, LAYER, FOLDED)),
    'r64_pair_global': (dict(blocks=7, dilation_bound=128, channels=64, skip_channels=256, final_layers_channels=[128, 64],
                             conditioning='global', mapping_layers=[6, 8]), (PAIR, LAYER, FOLDED)),
    'r128': (dict(blocks=4, channels=128, skip_channels=256, final_layers_channels=[128]),
             (S128, 'wn_wgrad_tr_kernel', 'dW_r together with the folded skip path', FOLDED)),
    # folded, but F0 = 64 is neither the pair kernel's nor the transposed-read jobs' width (both want 128): the chain is two
    # rows contractions per block with the folded term GF[0] V(b)^T, and M = Z^T dL/da goes through wn_wgrad_skip_kernel
    # (wn_plan_describe does not name M's kernel; train_paths: mtr == 0 unless F0 == 128)
    'r64_fold_f64': (dict(blocks=4, channels=64, skip_channels=256, final_layers_channels=[64]), (ROWS, LAYER, FOLDED)),
    # 32 channels never fold (the fold needs D % 64 == 0): the skip path stays one contraction, dW_s goes through
    # wn_wgrad_skip_kernel on the gradient of the skip sum
    'r32_k2': (dict(blocks=4, channels=32, skip_channels=64, final_layers_channels=[32]), (ROWS, LAYER, UNFOLDED)),
    # (wn_wgrad_layer_kernel is a KS = 2 kernel: KS = 3 takes the batched job table)
    'r32_k3': (dict(blocks=4, channels=32, skip_channels=64, final_layers_channels=[32], kernel_size=3, dilation_bound=81),
               (ROWS, 'wn_wgrad_batched_kernel', UNFOLDED)),
    # skip_channels=None: the skip output is the pre-residual 1x1 output, g_o = GH[b+1] + g_skipsum (the GO path)
    'r32_noskipch': (dict(blocks=4, channels=32, final_layers_channels=[]), (ROWS, LAYER, UNFOLDED)),
}
EXACT = ('exact fp32 MFMA', 'two exact-fp32 rows contractions per block', UNFOLDED)


def test_the_shape_gives_waves_several_tiles_and_one_utterance_the_other_branch():
  per = -(-T // 32)
  assert per == 844 and B * per == 4220 > 4096       # 256 workgroups x 8 waves = 2048 waves: 2 or 3 tiles a wave
  assert min(256, -(-B * per // 8)) % 8 == 0         # the batch: the XCD-aware branch of wn_tile_walk
  assert per <= 2048 and -(-per // 8) == 106 and 106 % 8 != 0      # one utterance: the other branch, <= 1 tile a wave
  assert T % 32 == 25 and T % 16 == 9                # ragged last tiles and last weight-gradient chunks


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
  kw, family = CASES[case]
  model = WaveNet(**kw, sampling_function='categorical', bits=8, device=_dev())
  if kw.get('conditioning'):
    model.build([(1, 8, 1), (1, B)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  report = model.kernel_report()
  for text in (EXACT if exact else family):
    assert text in report, (case, text, report)        # the family the case is there for: no drift to another path
  ocfg = O.OracleConfig(**kw, cond_inputs=B if kw.get('conditioning') else 0)
  return model, ocfg


def _region(model, what, idx, b):
  return model.training_intermediate(what, idx, b, T).reshape(b, T, -1)


def _folded(model):
  """Whether this plan's training pass folds the skip path under the current math mode (no skip sum, no gradient of it)."""
  return FOLDED in model.kernel_report()


def _data_gradients(model, ocfg, b):
  """Clones of every data gradient the backward phase left in the workspace, as (b, T, channels)."""
  N, nf = ocfg.blocks, len(ocfg.final_layers_channels)
  out = {('GF', i): _region(model, 6, i, b).clone() for i in range(nf + 1)}     # (GF[nf] = dL/dlogits first)
  out.update({('GU', i): _region(model, 8, i, b).clone() for i in range(N)})
  out.update({('GH', i): _region(model, 9, i, b).clone() for i in range(N + 1)})
  if not _folded(model):
    out['g_skipsum'] = _region(model, 7, 0, b).clone()
  return out


def _family(key):
  if key == 'g_skipsum' or key[0] == 'GF':
    return 'head data gradients'
  if key[0] in ('GH', 'GU'):
    return {'GH': 'GH (reversed dilated conv)', 'GU': 'GU (1x1 / skip + gate derivative)'}[key[0]]
  n = key[1]
  for part, fam in (('dil0', 'dW_d, db_d'), ('conv1', 'dW_r, db_r'), ('conv_skip', 'dW_s, db_s'), ('conv_cond', 'dW_c, db_c'),
                    ('final', 'head dW_f, db_f'), ('causal', 'input conv'), ('mapping', 'mapping net')):
    if part in n:
      return fam
  raise KeyError(key)


@pytest.mark.parametrize('case', list(CASES))
def test_every_backward_product_against_its_fp64_restatement(case, math_mode):
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, math_mode == 'fp32')
  N, nf = ocfg.blocks, len(ocfg.final_layers_channels)
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None      # a different one-hot condition per utterance
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())              # five different utterances
  loss, _, _ = model.loss_and_grads((x, cond) if cond is not None else x)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'

  ws = {k: v.double() for k, v in _data_gradients(model, ocfg, B).items()}
  folded = _folded(model)
  got = dict(ws)
  for b in range(N + 1):
    ws['H', b] = _region(model, 0, b, B).double()
  for b in range(N):
    ws['Z', b] = _region(model, 1, b, B).double()
    ws['AG', b] = _region(model, 2, b, B).double()
  for i in range(nf):
    ws['HA', i] = _region(model, 4, i, B).double()
  if not folded:
    ws['skipsum'] = _region(model, 3, 0, B).double()
  names = model.variable_names
  for n, g in zip(names, model.gradients()):
    got['param', n] = g.double()
  for b in range(N):
    for k in (('GU', b), ('GH', b)):
      assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0.0, (case, k)

  params = {n: t.double() for n, t in zip(names, model.trainable_variables)}
  ref = R.restate(ocfg, params, x[:, :-1].double(), cond.double() if cond is not None else None, ws, folded)
  assert sorted(R.param_names(ref)) == sorted(names)                    # nothing silently uncovered
  assert all(k in ref for k in got if k != ('GF', nf)), sorted(set(got) - set(ref), key=str)

  worst, failures = {}, []
  for k, r in ref.items():
    g = got[k].reshape(r.shape)
    scale = float(r.abs().max())
    diff = (g - r).abs()
    err = float(diff.max())
    bar = 1e-4 * scale + (1e-7 if k[0] == 'param' else 0.0)
    fam = _family(k)
    ratio = err / scale if scale > 0 else 0.0
    if ratio >= worst.get(fam, (0.0, None))[0]:
      worst[fam] = (ratio, k)
    if not err <= bar:
      where = ''
      if k[0] != 'param':
        rows = diff.amax(dim=-1)
        u, t = divmod(int(rows.argmax()), T)
        where = f' worst row: utterance {u}, t {t} (tile {t // 32}); rows over the bar: {int((rows > bar).sum())}'
      failures.append(f'{k}: max|got - ref| {err:.3e} > {bar:.3e} (max|ref| {scale:.3e}){where}')
  for fam, (ratio, k) in sorted(worst.items()):
    print(f'{case} [{math_mode}] {fam}: worst max|err| / max|ref| {ratio:.2e} at {k}')
  assert not failures, (case, math_mode, failures)


@pytest.mark.parametrize('case', list(CASES))
def test_copies_of_one_utterance_equal_it_alone_bit_for_bit(case):
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
  for k, v in batch.items():
    assert bool(torch.isfinite(v).all()), (case, k)
    if k[0] in ('GU', 'GF') or (k[0] == 'GH' and k[1] < ocfg.blocks):
      assert float(v.abs().max()) > 0.0, (case, k)
  # the same 1 / global_batch keeps the rows of dL/dlogits what they were in the batch
  loss1, _, _ = model.loss_and_grads((x1, cond1) if cond1 is not None else x1, global_batch=B)
  torch.cuda.synchronize()
  assert float(loss1[2]) == 0.0, 'range guard tripped'
  alone = _data_gradients(model, ocfg, 1)
  assert set(alone) == set(batch)

  def rows(a, b):
    return (a != b).any(dim=-1).nonzero()[:8].flatten().tolist()

  for k in [('GF', nf)] + [k for k in batch if k != ('GF', nf)]:        # dL/dlogits first: everything else follows from it
    for u in range(1, B):
      assert torch.equal(batch[k][u], batch[k][0]), \
          (case, k, f'utterance {u} of the batch != utterance 0', (batch[k][u] - batch[k][0]).abs().max().item(),
           rows(batch[k][u], batch[k][0]))
    assert torch.equal(batch[k][0], alone[k][0]), \
        (case, k, 'utterance 0 of the batch != the utterance alone', (batch[k][0] - alone[k][0]).abs().max().item(),
         rows(batch[k][0], alone[k][0]))
