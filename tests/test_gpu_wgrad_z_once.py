"""The weight-gradient phase of 64-channel blocks with the folded skip path, where the gated activations z are read once:
wn_wgrad_tr_kernel kind 7 forms [dW_r(b) | M(b)] = z(b)^T [g_o(b) | dL/da] for two blocks a job (g_o(b) = GH[b+1], scaled by
the power of two of its own running max-abs), and wn_wgrad_layer_kernel runs without its 1x1 part (dW_d, db_d only).

Every parameter gradient, and the GH / GU they are formed from, against tests/bwd_restatement.py (each product restated in
float64 from the tensors its own kernel read), at the bar of tests/test_gpu_bwd_tile_walk.py, in both math modes: exact fp32
takes the generic job table, which pins the restatement itself.

Shapes (B = 2): 4 and 7 blocks with dilations 1 .. 64 -- a full and a short last job for jobs of two (and of four), a last
block whose g_o = GH[N] is zero with max-abs 0, dilations on both sides of a 32-row chunk.  T = 601: three time ranges of
224, 224 and 153 rows (the job rounds a range to 32 rows, the per-block kernel to 16: 208, 208, 185), a ragged range and a
ragged last chunk (153 = 4 * 32 + 25).  T = 95: one range of fewer than three chunks, so the two-chunks-ahead prologue
requests rows past the range.  'scaled': the blocks' 1x1 kernels times 4^e(b), so that the two max-abs slots one job scales
its two g_o operands by differ by more than 16 x (asserted on the GH the step left): a job that takes one segment's scale
for the other is then wrong by that factor, not in the last bits.  'global': one-hot global condition through a mapping net.
"""
import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu

B = 2
NET = dict(dilation_bound=128, channels=64, skip_channels=256, final_layers_channels=[128, 64])
SPLIT = ('wn_bwd_pair_kernel', 'wn_wgrad_layer_kernel', 'skip path: folded')
EXACT = ('exact fp32 MFMA', 'two exact-fp32 rows contractions per block', 'skip path: one contraction over all blocks')
SCALE_EXP = (0, 4, 0, 5, 0, 5, 0)        # block b's 1x1 kernel times 4^e(b)
# case: (blocks, T, extra constructor keywords, scaled 1x1 kernels)
CASES = {
    'b4_t601': (4, 601, {}, False),
    'b7_t601': (7, 601, {}, False),
    'b4_t95': (4, 95, {}, False),
    'b7_t95': (7, 95, {}, False),
    'b7_t601_scaled': (7, 601, {}, True),
    'b7_t601_global': (7, 601, dict(conditioning='global', mapping_layers=[6, 8]), False),
}


def test_the_shapes_are_the_ones_the_docstring_describes():
  assert 601 % 32 == 25 and -(-601 // 3) == 201 and -(-201 // 32) * 32 == 224 and 601 - 2 * 224 == 153 == 4 * 32 + 25
  assert -(-201 // 16) * 16 == 208 != 224                   # the per-block kernel's ranges are not the job's
  assert 95 < 3 * 32 and 95 % 32 == 31
  assert 4 % 2 == 0 and 7 % 2 == 1 and 7 % 4 == 3           # full and short last jobs, of two or of four blocks


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
  blocks, _, extra, scaled = CASES[case]
  kw = dict(NET, blocks=blocks, **extra)
  model = WaveNet(**kw, sampling_function='categorical', bits=8, device=_dev())
  if kw.get('conditioning'):
    model.build([(1, 8, 1), (1, B)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  if scaled:
    for n, t in zip(model.variable_names, model.trainable_variables):
      if n.endswith('conv1/kernel'):
        t.mul_(4.0 ** SCALE_EXP[int(n.split('/')[0][len('block'):])])
  report = model.kernel_report()
  for text in (EXACT if exact else SPLIT):
    assert text in report, (case, text, report)            # the family the case is there for: no drift to another path
  ocfg = O.OracleConfig(**kw, cond_inputs=B if kw.get('conditioning') else 0)
  return model, ocfg


def _family(key):
  if key == 'g_skipsum' or key[0] in ('GF', 'GH', 'GU'):
    return 'head data gradients' if key == 'g_skipsum' or key[0] == 'GF' else key[0]
  for part, fam in (('dil0', 'dW_d, db_d'), ('conv1', 'dW_r, db_r'), ('conv_skip', 'dW_s, db_s'), ('conv_cond', 'dW_c, db_c'),
                    ('final', 'head dW_f, db_f'), ('causal', 'input conv'), ('mapping', 'mapping net')):
    if part in key[1]:
      return fam
  raise KeyError(key)


@pytest.mark.parametrize('case', list(CASES))
def test_every_gradient_against_its_fp64_restatement(case, math_mode):
  from wavenets_amd.data import synthetic_waveforms
  model, ocfg = _model(case, math_mode == 'fp32')
  T = CASES[case][1]
  N, nf = ocfg.blocks, len(ocfg.final_layers_channels)
  folded = 'skip path: folded' in model.kernel_report()
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None      # a different one-hot condition per utterance
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())
  loss, _, _ = model.loss_and_grads((x, cond) if cond is not None else x)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'

  def region(what, idx):
    return model.training_intermediate(what, idx, B, T).reshape(B, T, -1).double()

  ws = {('GF', i): region(6, i) for i in range(nf + 1)}                 # (GF[nf] = dL/dlogits)
  ws.update({('GU', b): region(8, b) for b in range(N)})
  ws.update({('GH', b): region(9, b) for b in range(N + 1)})
  if not folded:
    ws['g_skipsum'] = region(7, 0)
  got = dict(ws)
  for b in range(N + 1):
    ws['H', b] = region(0, b)
  for b in range(N):
    ws['Z', b] = region(1, b)
    ws['AG', b] = region(2, b)
  for i in range(nf):
    ws['HA', i] = region(4, i)
  if not folded:
    ws['skipsum'] = region(3, 0)
  names = model.variable_names
  for n, g in zip(names, model.gradients()):
    got['param', n] = g.double()
  for b in range(N):
    for k in (('GU', b), ('GH', b)):
      assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0.0, (case, k)
  if CASES[case][3]:
    # blocks b0, b0 + 1 share a job: their operands g_o = GH[b0 + 1], GH[b0 + 2] carry scales at least 16 x apart
    for b0 in range(0, N - 1, 2):
      hi, lo = float(got['GH', b0 + 1].abs().max()), float(got['GH', b0 + 2].abs().max())
      print(f'{case} [{math_mode}] max|GH[{b0 + 1}]| / max|GH[{b0 + 2}]| = {hi:.3e} / {lo:.3e}')
      assert hi >= 16.0 * lo, (case, b0, hi, lo)

  params = {n: t.double() for n, t in zip(names, model.trainable_variables)}
  ref = R.restate(ocfg, params, x[:, :-1].double(), cond.double() if cond is not None else None, ws, folded)
  assert sorted(R.param_names(ref)) == sorted(names)                    # nothing silently uncovered
  assert all(k in ref for k in got if k != ('GF', nf)), sorted(set(got) - set(ref), key=str)

  worst, failures = {}, []
  for k, r in ref.items():
    g = got[k].reshape(r.shape)
    scale = float(r.abs().max())
    err = float((g - r).abs().max())
    bar = 1e-4 * scale + (1e-7 if k[0] == 'param' else 0.0)
    fam = _family(k)
    ratio = err / scale if scale > 0 else 0.0
    if ratio >= worst.get(fam, (0.0, None))[0]:
      worst[fam] = (ratio, k)
    if not err <= bar:
      failures.append(f'{k}: max|got - ref| {err:.3e} > {bar:.3e} (max|ref| {scale:.3e})')
  for fam, (ratio, k) in sorted(worst.items()):
    print(f'{case} [{math_mode}] {fam}: worst max|err| / max|ref| {ratio:.2e} at {k}')
  assert not failures, (case, math_mode, failures)
