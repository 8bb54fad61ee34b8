"""The head's forward and the loss of a training pass at the size where a persistent wave takes several tiles -- what
tests/test_gpu_fwd_tile_walk.py, tests/test_gpu_bwd_tile_walk.py and tests/test_gpu_deep_tile_walk.py leave out (DESIGN.md
section 24).  Same B = 5, T = 27001, data and weights as those three files.

At that size the three files launch the head's kernels and compare nothing they write: HA[i] and GF[nf] = dL/dlogits go
into the backward restatement as inputs.  What runs there:

  wn_gemm_planes16s_kernel<2, 4, act>   the folded skip contraction a = act(sum_b V(b)^T z_b + b'): at most 512 workgroups of
                                        4 waves, 64-row tiles, so 5 x 422 = 2110 tiles are two passes, the second with 62
                                        live tiles and 1986 dead waves that still take part in the barriers and the weight ring
  wn_gemm_planes16s_kernel<1, 8, act>   256-column head convs, 32-row tiles: 4220 tiles are three passes, the third with 124
  wn_gemm_planes16s_kernel<1, 8, -3>    the last conv with the loss as its epilogue: soft-max, clip, loss row, softmax - onehot,
                                        the published max-abs and the metric's inverse-CDF draw
  wn_gemm_rows16_kernel<4>, wn_gemm_rows16_resident_kernel<2, .>, wn_gemm_rows16_wide_kernel, wn_gemm_rows_kernel<JT>
  wn_cat_loss256_kernel (persistent: 135 005 rows are 17 passes), wn_cat_loss_kernel (512 classes), wn_mix_loss_kernel,
  wn_launch_sum

Test A compares HA[i], the logits, the loss rows, dL/dlogits, the loss and the published max-abs with
bwd_restatement.restate_head: each product in float64 from the tensors its own kernel read (pinned on the CPU in
tests/test_bwd_restatement_cpu.py), in both math modes, at the project's bars (DESIGN.md sections 5 and 17).  Test B is
bitwise: five different utterances in one pass against each utterance alone (the head's forward has no running max-abs
scale, so distinct utterances are bit-comparable).  Test C covers what leaves the pass: the metric's draw inside the step
against the draw from the step's probabilities, the evaluation loss, and inference logits and probabilities against the fp64
CPU oracle and against each utterance alone.

Which loss path ran is checked with the sentinel of tests/test_gpu_loss_edges.py: the logits region is filled before the
call, and must be untouched after a pass that fused the loss and fully overwritten after any other.

Measured worst ratios, draw counts, the mutants these tests catch and run times: DESIGN.md section 24."""
import ctypes as C

import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O
from test_gpu_bwd_tile_walk import CASES as BWD_CASES, FOLDED, UNFOLDED

gpu = pytest.mark.gpu          # per test, not per module: the shape test below needs no device and runs without one

B, T = 5, 27001
DATA_SEED = 5                # synthetic_waveforms(B, T + 1, seed=5), as in the three other tile-walk files
EPS = 1e-7                   # keras.backend.epsilon()
SENTINEL = 12345.0
NO_SKIP = 'skip path: none (use_skip False)'
KINK_CAP = 16                # rows of r64_head256 whose target probability may sit within 1e-3 of a clip threshold

_R32 = BWD_CASES['r32_k2'][0]
# case: constructor keywords beyond the 8-bit categorical head
CASES = {
    # the configs[1] head: folded <2, 4> in two passes, <1, 8, act> in three, the loss epilogue on a 256-wide operand in three;
    # the only case where the clip is active
    'r64_head256': dict(blocks=7, dilation_bound=128, channels=64, skip_channels=256, final_layers_channels=[128, 256]),
    # a 64-wide hidden layer on the resident rows kernel, the epilogue on a 64-wide operand (4 k-steps)
    'r64_pair': BWD_CASES['r64_pair'][0],
    # the head must not see the condition
    'r64_pair_global': BWD_CASES['r64_pair_global'][0],
    # the epilogue directly under the folded contraction
    'r128': BWD_CASES['r128'][0],
    # F0 == S does not fold: the skip sum on wn_gemm_rows16_wide_kernel (jt 8, nks 36 >= 32, tiles >= 2048), 2 or 3 tiles a wave
    'r64_wide_unfolded': dict(blocks=9, channels=64, skip_channels=256, dilation_bound=16, final_layers_channels=[256, 64]),
    # the last conv from a 32-wide operand: planes16s declines it (2 k-steps), wn_gemm_rows16_kernel<4> with two column blocks,
    # then the standalone wn_cat_loss256_kernel over 17 passes
    'r32_k2': _R32,
    # four column blocks, wn_cat_loss_kernel
    'r32_c512': dict(_R32, bits=9),
    # widths off the 32 grid stay on the fp32 rows kernel in split mode too
    'r32_odd_widths': dict(blocks=4, channels=32, skip_channels=64, final_layers_channels=[48, 40]),
    # no hidden layer: the head input is the skip sum of pre-residual outputs
    'r32_noskipch': BWD_CASES['r32_noskipch'][0],
    # the head reads H[N]
    'r32_noskip': dict(blocks=4, channels=32, skip_channels=64, final_layers_channels=[64], use_skip=False),
    # the configs[3] head: a 30-column output conv on the fp32 rows kernel, wn_mix_loss_kernel
    'mol_r128': dict(blocks=4, channels=128, skip_channels=256, final_layers_channels=[128, 256],
                     sampling_function='logistic', num_mixtures=10, bits=16),
    'gauss_r32': dict(blocks=4, channels=32, skip_channels=64, final_layers_channels=[32],
                      sampling_function='gaussian', num_mixtures=8, bits=16),
}
# case: what each launch of the head runs on in split mode, first to last; 'epilogue' = the loss fused into the last conv
ROUTES = {
    'r64_head256': ['fold planes16s<2,4>', 'planes16s<1,8>', 'epilogue planes16s<1,8,-3>'],
    'r64_pair': ['fold planes16s<2,4>', 'rows16_resident<2>', 'epilogue planes16s<1,8,-3>'],
    'r64_pair_global': ['fold planes16s<2,4>', 'rows16_resident<2>', 'epilogue planes16s<1,8,-3>'],
    'r128': ['fold planes16s<2,4>', 'epilogue planes16s<1,8,-3>'],
    'r64_wide_unfolded': ['skip rows16_wide', 'planes16s<1,8>', 'rows16_resident<2>', 'epilogue planes16s<1,8,-3>'],
    'r32_k2': ['skip rows16<2>', 'rows_fp32<1>', 'rows16<4> x 2 column blocks', 'wn_cat_loss256_kernel'],
    'r32_c512': ['skip rows16<2>', 'rows_fp32<1>', 'rows16<4> x 4 column blocks', 'wn_cat_loss_kernel'],
    'r32_odd_widths': ['skip rows16<2>', 'rows_fp32<2>', 'rows_fp32<2>', 'rows_fp32<8>', 'wn_cat_loss256_kernel'],
    'r32_noskipch': ['skip rows_fp32<1>', 'rows16<4> x 2 column blocks', 'wn_cat_loss256_kernel'],
    'r32_noskip': ['rows16<2>', 'epilogue planes16s<1,8,-3>'],
    'mol_r128': ['fold planes16s<2,4>', 'planes16s<1,8>', 'rows_fp32<1>', 'wn_mix_loss_kernel'],
    'gauss_r32': ['skip rows16<2>', 'rows_fp32<1>', 'rows_fp32<1>', 'wn_mix_loss_kernel'],
}


def _full(kw):
  kw = dict(kw)
  kw.setdefault('sampling_function', 'categorical')
  kw.setdefault('bits', 8)
  return kw


# ------------------------------------------------------------------------------------------
# the launcher's predicates, restated (wn_plan.hip, wn_forward.hip, wn_gemm16s.hip, wn_gemm16.hip, wn_gemm.hip)
# ------------------------------------------------------------------------------------------
def m16(v):
  return v > 0 and v % 16 == 0


def m32(v):
  return v >= 64 and v % 32 == 0


def planes16s_supported(N, plane_k, nplanes, ld, ldy):
  """wn_gemm_planes16s_supported."""
  return (N in (128, 256) and plane_k >= 16 and plane_k % 16 == 0 and nplanes * (plane_k // 16) >= 3 and ld % 4 == 0
          and ld >= plane_k and ldy % 4 == 0 and ldy >= N)


def _geometry(kw):
  kw = _full(kw)
  R_ = kw['channels']
  D = kw.get('dilation_channels') or R_
  S = kw.get('skip_channels') or 0
  cout = (1 << kw['bits']) if kw['sampling_function'] == 'categorical' else 3 * kw['num_mixtures']
  finals = list(kw.get('final_layers_channels') or []) + [cout]      # (the plan counts the output conv among its finals)
  return kw, kw['blocks'], R_, D, S, (S or R_), finals, cout


def folds(kw):
  """The fold condition of wn_plan_create (fold_F0 > 0); fold_ok adds `not exact-fp32 mode`."""
  kw, N, R_, D, S, Sh, finals, _ = _geometry(kw)
  F0 = finals[0]
  skip16 = kw.get('use_skip', True) and m16(D) and D % 8 == 0 and m32(Sh)                   # frag16_skipF
  wgrad_skip = F0 % 32 == 0 and 32 <= F0 <= 256 and D % 32 == 0 and (N * D) % 32 == 0       # wn_wgrad_skip_supported(D, F0, N D)
  return (kw.get('layers_per_block', 1) == 1 and kw.get('use_skip', True) and S > 0 and len(finals) >= 2 and F0 < S and m32(F0)
          and m32(D) and D % 64 == 0 and m16(R_) and m16(S) and D % 8 == 0 and skip16 and wgrad_skip
          and m16(F0) and m32(S))                                                           # finals[0].frag16B


def loss_fusable(kw, hc):
  """loss_fusable (wn_forward.hip) in split mode: a 256-class categorical head whose last conv has a split-precision image."""
  kw, _, _, _, _, _, finals, cout = _geometry(kw)
  return kw['sampling_function'] == 'categorical' and cout == 256 and m16(hc) and m32(finals[-1])


def _rows_route(N, K, w16, planes):
  """Gemm::run: wn_gemm_rows16_ok (N % 32, K % 16, the padded-32 rule) picks the split-precision family, whose launcher
  (wn_launch_gemm_rows16) picks the kernel; everything else is the fp32 wn_gemm_rows_kernel<JT>."""
  jt_need, jtt = -(-N // 32), -(-N // 32)
  tiles = B * -(-T // 32)
  rows16_ok = N % 32 == 0 and not (N < 64 and jtt < 2) and K % 16 == 0
  if w16 and rows16_ok:
    nks = K // 16
    if jt_need == 8 and jtt == 8 and nks >= 32 and tiles >= 2048:
      return 'rows16_wide'
    if jt_need <= 2 and jtt == 2 and nks * 2 * 2048 <= 81920 and nks % 4 == 0 and not planes:
      return 'rows16_resident<2>'
    if jt_need <= 2:
      return 'rows16<2>'
    return f'rows16<4> x {-(-jtt // 4)} column blocks'
  return f'rows_fp32<{1 if jt_need <= 1 else 2 if jt_need <= 2 else 4 if jt_need <= 4 else 8}>'


def route(kw):
  """forward_core's head in a split-precision training pass without want_pred, then loss_stage."""
  kw, N, R_, D, S, Sh, finals, cout = _geometry(kw)
  out, first = [], 0
  if folds(kw):
    F0 = finals[0]
    if planes16s_supported(F0, D, N, D, F0):
      out.append('fold planes16s<2,4>' if F0 == 128 else 'fold planes16s<1,8>')
    else:
      out.append('fold ' + _rows_route(F0, N * D, True, True))
    hc, first = F0, 1
  elif kw.get('use_skip', True):
    out.append('skip ' + _rows_route(Sh, N * D, m16(D) and m32(Sh), True))
    hc = Sh
  else:
    hc = R_
  for i in range(first, len(finals)):
    co, last = finals[i], i + 1 == len(finals)
    frag16 = m16(hc) and m32(co)
    if last and loss_fusable(kw, hc) and planes16s_supported(co, hc, 1, hc, co):
      return out + ['epilogue planes16s<1,8,-3>']
    if frag16 and planes16s_supported(co, hc, 1, hc, co):
      out.append('planes16s<2,4>' if co == 128 else 'planes16s<1,8>')
    else:
      out.append(_rows_route(co, hc, frag16, False))
    hc = co
  if kw['sampling_function'] != 'categorical':
    return out + ['wn_mix_loss_kernel']
  return out + ['wn_cat_loss256_kernel' if cout <= 256 else 'wn_cat_loss_kernel']


def fuses(case, math_mode):
  return math_mode == 'split' and ROUTES[case][-1].startswith('epilogue')


def test_the_shape_gives_the_head_kernels_several_passes_and_each_case_its_family():
  per32, per64 = -(-T // 32), -(-T // 64)
  # folded contraction <2, 4>: 64-row tiles on at most 512 workgroups x 4 waves
  assert per64 == 422 and B * per64 == 2110 > 2048 and B * per64 - 2048 == 62 and 2 * 2048 - B * per64 == 1986
  # <1, 8, act> and <1, 8, -3>: 32-row tiles on the same grid: three passes, the third with 124 live tiles
  assert per32 == 844 and B * per32 == 4220 and -(-B * per32 // 2048) == 3 and B * per32 - 2 * 2048 == 124
  # rows kernels: 256 workgroups x 8 waves: 2 or 3 tiles a wave
  assert 2 * 2048 < B * per32 <= 3 * 2048
  # wn_cat_loss256_kernel: min(ceil(rows / 4), 2048) workgroups of 4 waves, a row a wave
  assert B * T == 135005 and -(-B * T // (2048 * 4)) == 17
  assert T % 32 == 25 and T % 64 == 57                 # ragged last tiles
  # one utterance alone is a single pass of every tiled kernel (and 4 passes of the row-a-wave loss kernel against 17)
  assert per64 <= 2048 and per32 <= 2048 and -(-T // (2048 * 4)) == 4
  assert list(CASES) == list(ROUTES)
  for case, kw in CASES.items():
    assert route(kw) == ROUTES[case], (case, route(kw))
    assert B * T * max(_geometry(kw)[6] + [_geometry(kw)[5]]) * 4 < 2 ** 32, case      # 32-bit byte offsets of planes16s
  # the predicates one by one, at the widths the cases are there for
  assert planes16s_supported(128, 64, 7, 64, 128) and planes16s_supported(256, 64, 1, 64, 256)       # 4 k-steps
  assert not planes16s_supported(256, 32, 1, 32, 256)                                                # 2 k-steps: declined
  assert not planes16s_supported(64, 128, 1, 128, 64) and not planes16s_supported(512, 64, 1, 64, 512)
  assert folds(CASES['r64_head256']) and folds(CASES['r128']) and folds(CASES['mol_r128'])
  assert not folds(CASES['r64_wide_unfolded'])         # F0 == S
  assert not folds(CASES['r32_k2'])                    # D % 64
  assert not folds(CASES['r32_noskip']) and not folds(CASES['r32_noskipch'])
  assert loss_fusable(CASES['r32_k2'], 32) and not planes16s_supported(256, 32, 1, 32, 256)          # fusable, but declined
  assert not loss_fusable(CASES['r32_c512'], 32) and not loss_fusable(CASES['r32_odd_widths'], 40)
  assert not loss_fusable(CASES['mol_r128'], 256)
  assert _rows_route(256, 9 * 64, True, True) == 'rows16_wide' and 9 * 64 // 16 == 36
  assert _rows_route(256, 7 * 64, True, True) != 'rows16_wide'                                       # nks 28 < 32
  for n in (30, 24, 48, 40):
    assert n % 32 != 0 and _rows_route(n, 64, True, False).startswith('rows_fp32')                   # wn_gemm_rows16_ok: N % 32


def _dev():
  return torch.device('cuda', 0)


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


def _model(case):
  from wavenets_amd import WaveNet
  kw = _full(CASES[case])
  model = WaveNet(**kw, device=_dev())
  if kw.get('conditioning'):
    model.build([(1, 8, 1), (1, B)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  from wavenets_amd import _lib
  exact = _lib.lib().wn_debug_value(1) == 1
  report = model.kernel_report()
  text = FOLDED if (folds(kw) and not exact) else UNFOLDED if kw.get('use_skip', True) else NO_SKIP
  assert text in report, (case, text, report)          # the family the case is there for: no drift to another path
  ocfg = O.OracleConfig(**kw, cond_inputs=B if kw.get('conditioning') else 0)
  return model, ocfg


def _inputs(ocfg):
  from wavenets_amd.data import synthetic_waveforms
  x = synthetic_waveforms(B, T + 1, seed=DATA_SEED, device=_dev())      # five different utterances
  cond = torch.eye(B, device=_dev()) if ocfg.cond_inputs else None      # a different one-hot condition per utterance
  return x, cond


def _pack(x, cond, u=None):
  if u is not None:
    x, cond = x[u:u + 1].contiguous(), (cond[u:u + 1].contiguous() if cond is not None else None)
  return (x, cond) if cond is not None else x


def _region(model, what, idx, b):
  return model.training_intermediate(what, idx, b, T).reshape(b, T, -1)


def _span(model, b, what, idx):
  from wavenets_amd import _lib
  off, ln = C.c_int64(), C.c_int64()
  _lib.check(_lib.lib().wn_debug_ws_region(model._plan, b, T, what, idx, C.byref(off), C.byref(ln)))
  return off.value, ln.value


def _step(model, ocfg, data, b, fused, **kwargs):
  """One loss_and_grads call over b utterances with the logits region holding a sentinel beforehand.  Returns (loss[3],
  what loss_and_grads returned second, {key: clone of a head tensor the pass left}, max-abs slot published for GF[nf])."""
  from wavenets_amd import _lib
  nf = len(ocfg.final_layers_channels)
  model._workspace('train', _lib.lib().wn_plan_workspace_floats(model._plan, b, T, 1))      # as loss_and_grads allocates it
  (o5, n5), (o6, n6) = _span(model, b, 5, 0), _span(model, b, 6, nf)
  assert n5 == n6 and (o5 + n5 <= o6 or o6 + n6 <= o5)         # two regions, not one under two names
  model.training_intermediate(5, 0, b, T).fill_(SENTINEL)
  loss, second, _ = model.loss_and_grads(data, global_batch=B, **kwargs)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  logits = _region(model, 5, 0, b)
  if fused:
    assert bool((logits == SENTINEL).all()), 'the fused loss epilogue was expected and a logits tensor was written'
  else:
    assert not bool((logits == SENTINEL).any()), 'a standalone loss kernel was expected and the logits were not (all) written'
  got = {('HA', i): _region(model, 4, i, b).clone() for i in range(nf)}
  if not fused:
    got['logits'] = logits.clone()
  got['loss_rows'] = _region(model, 12, 0, b).reshape(b, T).clone()
  got['GF', nf] = _region(model, 6, nf, b).clone()
  amax = float(model.training_intermediate(10, 0, b, T)[nf])
  return loss, second, got, amax


def _head_inputs(model, ocfg, got, folded, b=B):
  """What the head's kernels read, in float64: Z (folded), the skip sum or H[N], every HA[i], the logits where written."""
  N = ocfg.blocks
  ws = {k: v.double() for k, v in got.items() if k == 'logits' or k[0] == 'HA'}
  if folded:
    for i in range(N):
      ws['Z', i] = _region(model, 1, i, b).double()
  elif ocfg.use_skip:
    ws['skipsum'] = _region(model, 3, 0, b).double()
  else:
    ws['H', N] = _region(model, 0, N, b).double()
  return ws


def _where(diff_rows, bar_rows):
  """Worst row of a (B, T) error map: utterance, t, its 32- and 64-row tiles with the pass each falls in on a grid of 2048
  waves, the pass of a one-row-a-wave loss kernel, and the number of rows over the bar."""
  over = diff_rows > bar_rows
  u, t = divmod(int((diff_rows / bar_rows.clamp_min(1e-300)).argmax()), T)
  i32, i64, row = u * -(-T // 32) + t // 32, u * -(-T // 64) + t // 64, u * T + t
  return (f' worst row: utterance {u}, t {t}; 32-row tile {t // 32} (pass {i32 // 2048}), 64-row tile {t // 64} (pass {i64 // 2048}),'
          f' row-kernel pass {row // 8192}; rows over the bar: {int(over.sum())}')


FAMILY = {'HA': 'HA (head convs)', 'logits': 'logits', 'loss_rows': 'loss rows', 'GF': 'dL/dlogits'}


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_every_head_product_against_its_fp64_restatement(case, math_mode):
  model, ocfg = _model(case)
  nf = len(ocfg.final_layers_channels)
  mixture = ocfg.num_mixtures is not None
  x, cond = _inputs(ocfg)
  fused = fuses(case, math_mode)
  loss, _, got, amax = _step(model, ocfg, _pack(x, cond), B, fused)
  folded = FOLDED in model.kernel_report()
  assert folded == (folds(CASES[case]) and math_mode == 'split')
  params = {n: t.double() for n, t in zip(model.variable_names, model.trainable_variables)}
  ref = R.restate_head(ocfg, params, _head_inputs(model, ocfg, got, folded), folded, x[:, 1:], B)
  assert set(got) <= set(ref) and all(bool(torch.isfinite(v).all()) for v in got.values())

  worst, failures = {}, []

  def compare(k, g, r, bar):
    """bar: a float, or a (B, T) tensor of per-row bars."""
    diff = (g - r).abs()
    rows = diff if diff.dim() == 2 else diff.amax(dim=-1)
    bar_rows = bar if torch.is_tensor(bar) else torch.full_like(rows, bar)
    ratio = float((rows / bar_rows).max())
    fam = FAMILY[k if isinstance(k, str) else k[0]]
    if ratio >= worst.get(fam, (0.0, None))[0]:
      worst[fam] = (ratio, k)
    if not ratio <= 1.0:
      failures.append(f'{k}: max|got - ref| {float(diff.max()):.3e}, err / bar {ratio:.3e} (max|ref| {float(r.abs().max()):.3e})'
                      + _where(rows, bar_rows))

  # HA[i] and the logits: 1e-4 absolute; 1e-4 of the tensor's max where that exceeds 1
  for k in [('HA', i) for i in range(nf)] + (['logits'] if 'logits' in got else []):
    assert float(ref[k].abs().max()) > 0.0, (case, k)
    compare(k, got[k].double(), ref[k], 1e-4 * max(1.0, float(ref[k].abs().max())))
  r_rows, r_g = ref['loss_rows'], ref['GF', nf]
  g_rows, g_g = got['loss_rows'].double(), got['GF', nf].double()
  assert bool(torch.isfinite(r_rows).all()) and float(r_g.abs().max()) > 0.0
  excused = 0
  if mixture:
    # section 17's bars: one fp32 rounding of a double evaluation
    compare('loss_rows', g_rows, r_rows, 1e-6 * r_rows.abs().clamp(min=1.0))
    compare(('GF', nf), g_g, r_g, 1e-6 * r_g.abs().amax(dim=-1) + 1e-30)
  else:
    compare('loss_rows', g_rows, r_rows, 1e-5)
    # the clip kink: where the target's probability crosses 1e-7 (or 1 - 1e-7) that row's own
    # gradient entry moves by a whole 1 / global_batch and both sides are right.  Rows whose restated target probability
    # lies within a relative 1e-3 of a threshold are excused, in dL/dlogits only and at the target's entry only
    qt = ref['target_prob']
    near = ((qt / EPS - 1).abs() <= 1e-3) | (((1 - qt) / EPS - 1).abs() <= 1e-3)
    excused = int(near.sum())
    assert excused <= (KINK_CAP if case == 'r64_head256' else 0), (case, math_mode, excused)
    if excused:
      target = O.quantize(x[:, 1:, 0].cpu(), ocfg.bits).to(_dev())
      keep = torch.ones_like(r_g, dtype=torch.bool)
      keep.scatter_(-1, target.unsqueeze(-1), ~near.unsqueeze(-1))
      g_g = torch.where(keep, g_g, r_g)
    compare(('GF', nf), g_g, r_g, 1e-4 * float(r_g.abs().max()) + 1e-7)
    clipped = int(((qt < EPS) | (qt > 1 - EPS)).sum())
    print(f'{case} [{math_mode}] targets clipped: {clipped} of {B * T}; rows excused at the kink: {excused}')
    assert clipped > 0 or case != 'r64_head256', case             # the case that is there for the active clip
  # the step's loss: against the restatement, and against the fp64 sum of the device's own rows
  rel = abs(float(loss[0]) - float(ref['loss'])) / abs(float(ref['loss']))
  worst['loss against the restated loss (bar 2e-5)'] = (rel / 2e-5, 'loss')
  if not rel <= 2e-5:
    failures.append(f'loss {float(loss[0])!r} against the restated {float(ref["loss"])!r}: relative {rel:.3e} > 2e-5')
  # wn_sum_stage1 adds the n = 135 005 fp32 rows in fp64 (each add within 2^-53 relative of the running sum of magnitudes: at
  # most n 2^-53 sum|v| whatever the order of the partial sums), wn_sum_stage2 adds the at most 1024 partials alike
  # (counted in the n above, generously), multiplies by (double)(float)(1 / global_batch) -- the SAME fp32 scale is used
  # here, so it contributes one fp64 rounding, 2^-53 -- and stores as fp32: 2^-24 relative of the result, the only term that
  # matters.  Bar: 2^-24 |result| + (n + 2) 2^-53 scale sum|v|; 6.0e-8 relative for rows of one sign (under the 1e-6 cap).
  scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(B), dtype=torch.float32))
  own = float(g_rows.sum()) * scale
  bar_sum = 2.0 ** -24 * abs(own) + (B * T + 2) * 2.0 ** -53 * scale * float(g_rows.abs().sum())
  assert bar_sum <= 1e-6 * abs(own)
  err_sum = abs(float(loss[0]) - own)
  worst['loss against the sum of its own rows'] = (err_sum / bar_sum, 'loss')
  if not err_sum <= bar_sum:
    failures.append(f'loss {float(loss[0])!r} against the fp64 sum of region 12 times fp32(1 / {B}) {own!r}: {err_sum:.3e} > {bar_sum:.3e}')
  # the published max-abs covers what is read back (what the range guard of the backward pass and its scales read)
  if not amax >= float(got['GF', nf].abs().max()):
    failures.append(f'max-abs slot of GF[{nf}] {amax!r} < max|GF[{nf}]| {float(got["GF", nf].abs().max())!r}')
  for fam, (ratio, k) in sorted(worst.items()):
    print(f'{case} [{math_mode}] {fam}: worst err / bar {ratio:.2e} at {k}')
  assert not failures, f'{case} [{math_mode}]:\n' + '\n'.join(failures)


def _diff_rows(a, b):
  a, b = a.reshape(T, -1), b.reshape(T, -1)
  return (a != b).any(dim=-1).nonzero()[:8].flatten().tolist()


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_head_rows_do_not_depend_on_the_wave_the_tile_or_the_pass(case):
  """Five different utterances in one pass (two passes of the folded contraction, three of the 256-column convs and the loss
  epilogue, 17 of the loss kernel) against each utterance alone (a single pass of every tiled kernel, 4 of the loss kernel), both with
  global_batch = B."""
  model, ocfg = _model(case)
  nf = len(ocfg.final_layers_channels)
  x, cond = _inputs(ocfg)
  fused = fuses(case, 'split')
  _, _, batch, _ = _step(model, ocfg, _pack(x, cond), B, fused)
  assert ('logits' in batch) == (not fused)
  assert all(float(v.abs().max()) > 0.0 for v in batch.values())
  order = [('HA', i) for i in range(nf)] + (['logits'] if not fused else []) + ['loss_rows', ('GF', nf)]
  assert sorted(order, key=str) == sorted(batch, key=str)
  for u in range(B):
    _, _, alone, _ = _step(model, ocfg, _pack(x, cond, u), 1, fused)
    for k in order:
      assert torch.equal(batch[k][u], alone[k][0]), \
          (case, k, f'utterance {u} of the batch != the utterance alone', (batch[k][u] - alone[k][0]).abs().max().item(),
           'first rows that differ:', _diff_rows(batch[k][u], alone[k][0]))


@gpu
@pytest.mark.parametrize('case', ['r64_head256', 'r64_pair', 'mol_r128', 'r32_c512'])
def test_the_draw_inside_the_step_is_the_draw_from_the_steps_probabilities(case):
  """loss_and_grads(want_sample=True) with the draw inside the library (256 classes: in the loss epilogue, three passes) and
  through pred + sample_waveform, both with the same Philox key.  The condition of
  test_train_step_metric_sample_drawn_inside_the_step (tests/test_gpu_parity.py): 256 classes, at most numel // 200 draws
  differ and each by an adjacent class at most (the two routes sum the same probabilities in different orders); mixture and
  512-class heads draw from the same logits tensor in both routes and must be equal.  A wrong row counter in a later pass
  would differ on nearly every row of that pass.  Measured at 135 005 rows: 1 draw differs on r64_head256 (in pass 0, by one
  class), none on r64_pair; with the row counter one off in passes 1 and 2 (a mutant), 51 701 and 67 469."""
  model, ocfg = _model(case)
  x, cond = _inputs(ocfg)
  draws = []
  for inside in (True, False):
    model._fused_step_sample = inside
    model._sample_calls = 7                            # the same counter before both calls: the same key
    # the fused draw rides in the epilogue; the other route asks for pred, which keeps the loss out of the epilogue
    _, samp, _, _ = _step(model, ocfg, _pack(x, cond), B, fuses(case, 'split') and inside, want_sample=True)
    assert model._sample_calls == 8 and samp.shape == (B, T, 1) and float(samp.abs().max()) <= 1.0
    draws.append(samp.clone())
  a, b = draws
  diff = (a != b).reshape(B, T)
  n = int(diff.sum())
  print(f'{case}: draws that differ between the two routes: {n} of {a.numel()}')
  if case in ('mol_r128', 'r32_c512'):
    assert torch.equal(a, b), (case, n)
    return
  where = ''
  if n:
    per_pass = torch.bincount((diff.flatten().nonzero().flatten() // T * -(-T // 32) +
                               diff.flatten().nonzero().flatten() % T // 32) // 2048, minlength=3).tolist()
    where = f'differing rows per pass of the 32-row tiles: {per_pass}'
    print(f'{case}: {where}')
  assert n <= a.numel() // 200, (case, n, where)
  assert float((a - b).abs().max()) <= 2.0 / 256 + 1e-7, case                  # an adjacent class at most


_ORACLE = {}


def _oracle_logits(case, model, ocfg, x, cond):
  """fp64 logits of all five utterances on the CPU (0.3 to 2.6 s a case), computed once a case: weights and data are fixed
  by their seeds."""
  if case not in _ORACLE:
    params = [v.detach().cpu().double() for v in model.trainable_variables]
    _ORACLE[case] = O.model_forward(x[:, :-1].cpu().double(), params, ocfg, cond.cpu().double() if cond is not None else None,
                                    return_logits=True)
  return _ORACLE[case]


@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_evaluation_and_inference_at_this_size(case):
  """test_step's loss against the restated loss of a training pass over the same batch (2e-5 relative); model.logits(x) and
  model(x) against the fp64 CPU oracle on all five utterances (1e-4 absolute, 1e-4 of the tensor's max where that exceeds
  1) and bitwise against each utterance alone."""
  from wavenets_amd import _lib
  prev = _lib.lib().wn_debug_value(1)
  _lib.lib().wn_debug_set(1, 0)
  try:
    model, ocfg = _model(case)
    x, cond = _inputs(ocfg)
    lg64 = _oracle_logits(case, model, ocfg, x, cond)
    fused = fuses(case, 'split')
    _, _, got, _ = _step(model, ocfg, _pack(x, cond), B, fused)
    folded = FOLDED in model.kernel_report()
    p64 = {n: t.double() for n, t in zip(model.variable_names, model.trainable_variables)}
    ref = R.restate_head(ocfg, p64, _head_inputs(model, ocfg, got, folded), folded, x[:, 1:], B)
    ev = model.test_step(_pack(x, cond))['loss']
    rel = abs(ev - float(ref['loss'])) / abs(float(ref['loss']))
    print(f'{case}: evaluation loss {ev!r}, restated training loss {float(ref["loss"])!r}, relative {rel:.2e}')
    assert model.test_guard_trips == 0 and rel <= 2e-5, (case, ev, float(ref['loss']))

    xin = x[:, :-1].contiguous()
    lg64 = lg64.to(_dev())
    want = {'logits': lg64, 'call': torch.softmax(lg64, -1) if ocfg.num_mixtures is None else lg64}
    batch = {}
    for name, fn in (('logits', model.logits), ('call', model)):
      out = fn(_pack(xin, cond)).clone()
      assert not model.range_tripped_last_forward() and out.shape == want[name].shape
      scale = float(want[name].abs().max())
      diff = (out.double() - want[name]).abs().amax(dim=-1)
      bar = 1e-4 * max(1.0, scale)
      print(f'{case}: model.{name} against the fp64 oracle: max|err| {float(diff.max()):.3e} (bar {bar:.1e}, max|ref| {scale:.3e})')
      assert float(diff.max()) <= bar, (case, name, _where(diff, torch.full_like(diff, bar)))
      batch[name] = out
    for u in range(B):
      for name, fn in (('logits', model.logits), ('call', model)):
        alone = fn(_pack(xin, cond, u))
        assert torch.equal(batch[name][u], alone[0]), \
            (case, name, u, (batch[name][u] - alone[0]).abs().max().item(), _diff_rows(batch[name][u], alone[0]))
  finally:
    _lib.lib().wn_debug_set(1, prev)
