"""WaveNet.score / wn_score on the device: per-utterance negative log-likelihoods in one evaluation
pass, against the fp64 reference of tests/score_reference.py (pinned on the CPU in tests/test_score_cpu.py) and, where the
statement is about bits, against the device's own passes.

Standard batch of the sample_weight tests: B = 3, T = 150 (T mod 32 = 22), std_weights(), the nets of its NETS table, both
math modes.  Which path ran is asserted first in every scoring pass, with the sentinel of tests/test_gpu_loss_edges.py in the
logits region of the INFERENCE workspace (wn_debug_eval_region 5): untouched after a pass that formed the loss rows in the
last conv's epilogue (the evaluation form, wn_gemm_planes16s_kernel<1, 8, -5 / -6>), fully overwritten after any other.

Bars.  nll[b]: the project's loss bar, 2e-5 relative.  weight[b]: exact.  A row: four times the worst error, per head, of the
rows a training pass of the parent commit left in training region 12 on this same batch with these same weights (both math
modes, all nets of the head; DESIGN.md section 26 holds the measured figures):

  head          worst |row - fp64 reference| at the parent      bar
  categorical   2.022e-6 (cat_small_fused, split)                 8.09e-6
  logistic      1.405e-6 (mol, both modes)                        5.62e-6
  gaussian      2.555e-7 (gauss, split)                           1.02e-6

Four times, because the inference and the training forward are the same arithmetic in differently scheduled kernels, and one
sample of a worst case is not its maximum.  No row is excused: the reference's target probabilities are asserted to lie far
inside Keras's clip."""
import math

import pytest
import torch

import score_reference as S
from test_gpu_parity import make_pair, _inputs, math_mode  # noqa: F401  (math_mode: fixture)
from test_gpu_sample_weight import NETS, B, T, SENTINEL, std_weights, _pair, _data, _pack, _fusable, _kw, _dev
import test_gpu_head_tile_walk as HW

pytestmark = pytest.mark.gpu

# worst |row - reference| of the parent's training rows (region 12) on the standard batch under std_weights(), per head
ROW_WORST = {'categorical': 2.021683e-06, 'logistic': 1.405361e-06, 'gaussian': 2.554538e-07}
ROW_BAR = {h: 4.0 * v for h, v in ROW_WORST.items()}


def _head(case):
  return _kw(case).get('sampling_function', 'categorical')


def score_pass(model, data, fused, b=B, t=T, **kwargs):
  """One model.score(per_sample=True) with the logits region of the inference workspace holding the sentinel beforehand;
  asserts which family of loss kernel ran.  (A pass the range guard repeated was left behind by the exact-fp32 kernels,
  which never fuse.)"""
  from wavenets_amd import _lib
  model._workspace('fwd', _lib.lib().wn_plan_workspace_floats(model._plan, b, t, 0))       # as score allocates it
  model.eval_intermediate(5, b, t).fill_(SENTINEL)
  trips = model.score_guard_trips
  s = model.score(data, per_sample=True, **kwargs)
  torch.cuda.synchronize()
  fused = fused and model.score_guard_trips == trips
  logits = model.eval_intermediate(5, b, t)
  if fused:
    assert bool((logits == SENTINEL).all()), 'the evaluation epilogue was expected and a logits tensor was written'
  else:
    assert not bool((logits == SENTINEL).any()), 'a standalone loss kernel was expected and the logits were not (all) written'
  assert all(v.is_cuda for v in s.values()) and s['rows'].shape == (b, t) and s['nll'].shape == (b,)
  return s


def _fused(case, mode):
  fused = mode == 'split' and _fusable(case)
  if case in ('cat_r64', 'cat_lpb2_r64'):
    assert fused == (mode == 'split')
  return fused


_REF = {}


def _reference(case, params, ocfg, x, cond, weighted):
  """fp64 reference of the standard batch, once a case (both math modes share it; one forward for both weightings)."""
  if case not in _REF:
    pred, target = S.forward(x, params, ocfg, cond)
    _REF[case] = {False: S.score_from(pred, target, ocfg, None), True: S.score_from(pred, target, ocfg, std_weights())}
  return _REF[case][weighted]


def _check_against(s, ref, w, head, what):
  """The bars of the module docstring: nll 2e-5 relative, weight exact, rows ROW_BAR[head]; every figure printed first."""
  b, t = ref['rows'].shape
  rows, nll, weight = s['rows'].cpu().double(), s['nll'].cpu().double(), s['weight'].cpu()
  assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(nll).all())
  rel = ((nll - ref['nll']).abs() / ref['nll'].abs()).max().item()
  err = (rows - ref['rows']).abs().max().item()
  print(f'{what}: nll worst relative {rel:.2e} (bar 2e-5); rows worst |err| {err:.3e} (bar {ROW_BAR[head]:.3e})')
  assert rel <= 2e-5, (what, nll.tolist(), ref['nll'].tolist())
  want_weight = torch.full((b,), float(t)) if w is None else w.double().sum(dim=1).float()
  assert torch.equal(weight, want_weight), (what, weight.tolist(), want_weight.tolist())
  assert err <= ROW_BAR[head], (what, err, ROW_BAR[head], divmod(int((rows - ref['rows']).abs().argmax()), t))
  if w is not None:
    assert bool((rows[w == 0] == 0).all())
  lg2 = math.log(2.0)
  assert torch.equal(s['nll_per_sample'], s['nll'] / s['weight']) and torch.equal(s['bits_per_sample'], s['nll'] / (s['weight'] * lg2))


# ------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('case', list(NETS))
def test_score_against_the_fp64_reference(case, weighted, math_mode):
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  w = std_weights() if weighted else None
  ref = _reference(case, params, ocfg, x, cond, weighted)
  if ref['target_prob'] is not None:                       # far from Keras's clip: no row sits at the kink
    keep = torch.ones(B, T, dtype=torch.bool) if w is None else w != 0
    assert bool(((ref['target_prob'][keep] > 1e-5) & (ref['target_prob'][keep] < 1 - 1e-5)).all()), case
  kw = {} if w is None else {'sample_weight': w.to(_dev())}
  s = score_pass(model, _pack(x, cond), _fused(case, math_mode), **kw)
  assert model.score_guard_trips == 0
  _check_against(s, ref, w, _head(case), f'{case} [{math_mode}] {"weighted" if weighted else "plain"}')


# ------------------------------------------------------------------------------------------ 3
def kernel_order_sum(rows):
  """wn_score_reduce_kernel restated on the device, in float64: thread i adds rows i, i + 256, ... in that order, then the
  tree over the 256 partial sums (o = 128, 64, ..., 1: v[i] += v[i + o] for i < o), one rounding to float at the end."""
  t = rows.numel()
  pad = torch.zeros(-(-t // 256) * 256, dtype=torch.float64, device=rows.device)
  pad[:t] = rows.double()
  acc = torch.zeros(256, dtype=torch.float64, device=rows.device)
  for chunk in pad.reshape(-1, 256):                       # (adding the +0 of the padding changes no bit of a sum)
    acc = acc + chunk
  o = 128
  while o > 0:
    acc = acc[:o] + acc[o:2 * o]
    o >>= 1
  return acc[0].float()


def _alone_equals_batch(model, x, cond, w, s, fused, b, t, what):
  for u in range(b):
    xu = x[u:u + 1].contiguous()
    cu = cond[u:u + 1].contiguous() if cond is not None else None
    kw = {} if w is None else {'sample_weight': w[u:u + 1].contiguous().to(_dev())}
    a = score_pass(model, _pack(xu, cu), fused, 1, t, **kw)
    bad = (a['rows'][0] != s['rows'][u]).nonzero().flatten()[:8].tolist()
    assert not bad, (what, u, 'rows of the batch != the utterance alone, first t:', bad)
    assert torch.equal(a['nll'][0], s['nll'][u]) and torch.equal(a['weight'][0], s['weight'][u]), (what, u)
    own = kernel_order_sum(s['rows'][u])
    assert torch.equal(own, s['nll'][u]), (what, u, float(own), float(s['nll'][u]))


@pytest.mark.parametrize('case', list(NETS))
def test_an_utterances_score_is_a_function_of_its_own_rows_bit_for_bit(case, math_mode):
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  w = std_weights()
  fused = _fused(case, math_mode)
  s = score_pass(model, _pack(x, cond), fused, sample_weight=w.to(_dev()))
  _alone_equals_batch(model, x, cond, w, s, fused, B, T, f'{case} [{math_mode}]')
  # the sum of the weights in the kernel's order too (exact in double whatever the order: 150 floats of 24 bits)
  for u in range(B):
    assert torch.equal(kernel_order_sum(w[u].to(_dev())), s['weight'][u])


# ------------------------------------------------------------------------------------------ 4
def raw_score(model, x, cond, w):
  """wn_score itself, without the Python surface's guard repeat: (nll, weight, rows, flag) as the call left them."""
  from wavenets_amd import _lib
  L = _lib.lib()
  b, t = x.shape[0], x.shape[1] - 1
  ws = model._workspace('fwd', L.wn_plan_workspace_floats(model._plan, b, t, 0))
  nll, weight = torch.empty(b, device=_dev()), torch.empty(b, device=_dev())
  rows, flag = torch.empty(b, t, device=_dev()), torch.empty(1, device=_dev())
  try:
    _lib.check(L.wn_plan_arm_row_weights(model._plan, _lib.ptr(w), b * t))
    _lib.check(L.wn_score(model._plan, _lib.ptr(model.flat_params), _lib.ptr(x), _lib.ptr(cond), b, t, _lib.ptr(nll),
                          _lib.ptr(weight), _lib.ptr(rows), _lib.ptr(flag), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
  finally:
    L.wn_plan_arm_row_weights(model._plan, None, 0)
  torch.cuda.synchronize()
  return nll, weight, rows, float(flag)


@pytest.mark.parametrize('case', ['cat_r64', 'cat_noskipch', 'cat_r64_c512', 'mol'])
def test_a_zero_weight_is_a_select_not_a_product(case):
  """Utterance 1 (length 113 under std_weights()) carries NaN and 1e30 behind its last weighted target.  Those samples are
  inputs of rows 114.. only (the network is causal) and targets of rows 113.. only, all of weight 0.

  Such inputs are also what the forward range guard exists for: where a pass reports them (flag 1) score() repeats it with
  the exact-fp32 kernels.  (Whether it does depends on the net: the input conv's max-abs drops a NaN, and behind a NaN and a
  1e30 under one two-tap window every row is NaN.)  So the statement is made twice: of wn_score itself in split mode --
  whatever the flag says, every output is finite and has the bits of the zero-padded call -- and of score(), compared with
  the zero-padded batch in the mode its result was computed in."""
  import contextlib
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  w = std_weights()
  assert bool((w[1, 113:] == 0).all()) and bool((w[1, :113] == 1).all())
  xz, xg = x.clone(), x.clone()
  xz[1, 114:] = 0.0
  xg[1, 114::2] = float('nan')
  xg[1, 115::2] = 1e30
  assert torch.equal(xz[1, :114], xg[1, :114])
  wd = w.to(_dev())
  cd = cond.to(_dev()) if cond is not None else None
  # wn_score, split precision
  zero, garbage = raw_score(model, xz.to(_dev()), cd, wd), raw_score(model, xg.to(_dev()), cd, wd)
  assert zero[3] == 0.0 and garbage[3] in (0.0, 1.0)
  for name, a, g in zip(('nll', 'weight', 'rows'), zero, garbage):
    assert bool(torch.isfinite(g).all()), (case, name)
    assert torch.equal(a, g), (case, name, (a - g).abs().max().item())
  assert bool((garbage[2][1, 113:] == 0).all()) and float(garbage[0][1]) > 0
  # score(): behind a trip, the repeat under exact fp32
  fused = _fused(case, 'split')
  sg = score_pass(model, _pack(xg, cond), fused, sample_weight=wd)
  tripped = model.score_guard_trips == 1
  assert tripped == (garbage[3] == 1.0)
  print(f'{case}: the padding of NaN and 1e30 {"tripped" if tripped else "did not trip"} the range guard')
  with (model.exact_fp32() if tripped else contextlib.nullcontext()):
    sz = score_pass(model, _pack(xz, cond), fused and not tripped, sample_weight=wd)
  assert model.score_guard_trips == int(tripped)
  for k in ('nll', 'weight', 'rows', 'nll_per_sample', 'bits_per_sample'):
    assert bool(torch.isfinite(sg[k]).all()), (case, k)
    assert torch.equal(sg[k], sz[k]), (case, k)


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize('case', ['cat_r64', 'cat_noskipch', 'mol', 'cond'])
def test_score_agrees_with_test_step_and_leaves_nothing_armed(case, math_mode):
  ocfg, params, model = _pair(case)
  model.compile()
  x, cond = _data(case)
  data, w = _pack(x, cond), std_weights().to(_dev())

  def evaluate(**kw):
    for m in model.metrics:
      m.reset_state()
    return model.test_step(data, **kw)['loss']
  plain = evaluate()
  s = score_pass(model, data, _fused(case, math_mode), sample_weight=w)
  again = evaluate()
  assert again == plain, (case, plain, again)              # nothing stays armed behind a score
  ev = evaluate(sample_weight=w)
  mine = float(s['nll'].double().sum()) / B
  rel = abs(mine - ev) / abs(ev)
  bar = B * 2.0 ** -23 if math_mode == 'fp32' else 2e-5    # fp32 mode: the same standalone kernel wrote both passes' rows
  print(f'{case} [{math_mode}]: sum nll / B {mine!r}, test_step {ev!r}, relative {rel:.2e} (bar {bar:.2e})')
  assert model.test_guard_trips == 0 and model.score_guard_trips == 0 and rel <= bar
  assert abs(ev - plain) > 1e-3 * abs(plain)


# ------------------------------------------------------------------------------------------ 6
WALK_CASE, WALK_B, WALK_T = 'r64_pair', 3, 22001


def test_the_walk_shape_reaches_a_second_pass_of_the_epilogue():
  """wn_launch_gemm_planes16s, 256 columns: one 32-row tile per wave and pass, tiles counted per utterance (a tile never
  straddles two utterances), min(ceil(tiles / 4), 512) workgroups of 4 waves.  (Counting the 66003 rows as one flat run
  would give 2063 tiles, a second pass of 15 and a last tile of 19 rows; the kernel's own geometry is the one below.)"""
  per_b = -(-WALK_T // 32)
  tiles = WALK_B * per_b
  grid = min(-(-tiles // 4), 512)
  assert per_b == 688 and tiles == 2064 and grid * 4 == 2048
  assert -(-tiles // (grid * 4)) == 2 and tiles - grid * 4 == 16 and WALK_T % 32 == 17
  assert per_b <= 2048                                     # an utterance alone is a single pass
  # r64_pair: the epilogue on a 64-wide operand, 4 k-steps of 16 (the case's 7 blocks feed the folded contraction above it)
  kw = HW._full(HW.CASES[WALK_CASE])
  assert kw['final_layers_channels'][-1] // 16 == 4 and HW.route(kw)[-1].startswith('epilogue')
  assert WALK_B * WALK_T * max(HW._geometry(kw)[6] + [HW._geometry(kw)[5]]) * 4 < 2 ** 32


_WALK = {}


def _walk_setup():
  if not _WALK:
    from wavenets_amd.data import synthetic_waveforms, length_weights
    model, ocfg = HW._model(WALK_CASE)
    x = synthetic_waveforms(WALK_B, WALK_T + 1, seed=HW.DATA_SEED)
    g = torch.Generator().manual_seed(21)
    w = torch.rand(WALK_B, WALK_T, generator=g) * 2
    w[:, ::7] = 0.0
    w[1] = length_weights([15000], WALK_T)[0]
    assert float(w[2, 671 * 32:].abs().max()) > 0            # the tiles of the second pass carry weight
    params = [v.detach().cpu().double() for v in model.trainable_variables]
    pred, target = S.forward(x, params, ocfg)
    _WALK.update(model=model, ocfg=ocfg, x=x, w=w, refs={False: S.score_from(pred, target, ocfg, None),
                                                          True: S.score_from(pred, target, ocfg, w)})
  return _WALK


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
def test_the_evaluation_epilogue_where_a_wave_takes_a_second_tile(weighted):
  k = _walk_setup()
  model, x = k['model'], k['x']
  w = k['w'] if weighted else None
  ref = k['refs'][weighted]
  # inside Keras's clip and away from its kink by the relative 1e-3 of tests/test_gpu_head_tile_walk.py: at 66003 rows of a
  # random net the smallest target probability is far below the 1e-5 of the small batch
  keep = torch.ones(WALK_B, WALK_T, dtype=torch.bool) if w is None else w != 0
  qt = ref['target_prob'][keep]
  print(f'{WALK_CASE}: target probabilities in [{float(qt.min()):.3e}, {float(qt.max()):.6f}]')
  assert bool(((qt > HW.EPS * (1 + 1e-3)) & (qt < 1 - HW.EPS * (1 + 1e-3))).all())
  kw = {} if w is None else {'sample_weight': w.to(_dev())}
  s = score_pass(model, x.to(_dev()), True, WALK_B, WALK_T, **kw)
  assert model.score_guard_trips == 0
  _check_against(s, ref, w, 'categorical', f'{WALK_CASE} 3 x 22001 {"weighted" if weighted else "plain"}')
  _alone_equals_batch(model, x, None, w, s, True, WALK_B, WALK_T, WALK_CASE)


# ------------------------------------------------------------------------------------------ 7
def test_python_surface():
  ocfg, params, model = _pair('cat_r64')
  x, cond = _data('cat_r64')
  data = _pack(x, cond)
  for bad in (torch.ones(B, T + 1), torch.ones(B + 1), torch.ones(B, T, 1, 1), torch.ones(T)):
    with pytest.raises(ValueError, match='sample_weight must have shape'):
      model.score(data, sample_weight=bad)
  with pytest.raises(ValueError):
    model.score(torch.zeros(B, T + 1))                     # not (B, T + 1, 1)
  with pytest.raises(ValueError):
    model.score(torch.zeros(B, 1, 1))                      # no target
  # per_sample off: no rows, the same scores
  full = model.score(data, per_sample=True)
  short = model.score(data)
  assert set(short) == {'nll', 'weight', 'nll_per_sample', 'bits_per_sample'} and set(full) == set(short) | {'rows'}
  assert all(v.is_cuda and v.shape == (B,) for v in short.values()) and full['rows'].shape == (B, T)
  assert all(torch.equal(short[k], full[k]) for k in short)
  assert short['weight'].tolist() == [float(T)] * B
  assert torch.allclose(short['bits_per_sample'], short['nll'] / (T * math.log(2.0)), rtol=1e-6, atol=0)
  # a per-utterance weight is expanded over its utterance; (B, T, 1) is (B, T)
  v = torch.tensor([0.5, 2.0, 1.25], device=_dev())
  per_u = model.score(data, sample_weight=v, per_sample=True)
  spread = model.score(data, sample_weight=v[:, None].expand(B, T).contiguous(), per_sample=True)
  col = model.score(data, sample_weight=v[:, None, None].expand(B, T, 1).contiguous(), per_sample=True)
  for k in per_u:
    assert torch.equal(per_u[k], spread[k]) and torch.equal(per_u[k], col[k]), k
  assert torch.equal(per_u['rows'], v[:, None] * full['rows']) and per_u['weight'].tolist() == [0.5 * T, 2.0 * T, 1.25 * T]
  # an utterance of weight 0: nll 0, weight 0, both ratios 0 / 0 = NaN; the others are untouched by it
  wz = torch.ones(B, T, device=_dev())
  wz[1] = 0.0
  z = model.score(data, sample_weight=wz)
  assert float(z['nll'][1]) == 0.0 and float(z['weight'][1]) == 0.0
  assert bool(torch.isnan(z['nll_per_sample'][1])) and bool(torch.isnan(z['bits_per_sample'][1]))
  for u in (0, 2):
    assert all(torch.equal(z[k][u], short[k][u]) for k in short)
  assert model.score_guard_trips == 0


def test_score_runs_on_the_averaged_weights():
  from wavenets_amd import Adam
  ocfg, params, model = _pair('cat_r64', seed=40)
  model.compile(optimizer=Adam(learning_rate=1e-2, use_ema=True, ema_momentum=0.5))
  x, cond = _data('cat_r64', seed=41)
  data = _pack(x, cond)
  for _ in range(2):
    model.train_step(data)
  raw = model.score(data)
  with model.averaged_weights():
    avg = model.score(data)
  assert not torch.equal(raw['nll'], avg['nll'])
  saved = model.flat_params.data.clone()
  model.flat_params.data.copy_(model.optimizer.ema)
  want = model.score(data)
  model.flat_params.data.copy_(saved)
  assert torch.equal(avg['nll'], want['nll']) and torch.equal(model.score(data)['nll'], raw['nll'])


def test_score_guard_trips_counts_a_forced_trip():
  """The input conv's bias puts the residual stream at +-1e5, beyond the range of the split-precision kernels, as in
  test_forward_range_guard_falls_back_to_exact_fp32: the pass is repeated with the exact-fp32 kernels and counted."""
  from wavenets_amd import _lib
  kw = _kw('cat_r64')
  ocfg, params, model = make_pair(seed=6, **kw)
  big = torch.where(torch.arange(params[1].numel()) % 2 == 0, 1.0e5, -1.0e5).to(params[1].dtype)
  params[1] = params[1] + big                                     # causal/bias
  model.set_weights([p.numpy() for p in params])
  x, _ = _inputs(kw, 2, 121, seed=3)
  ref = S.score(x, params, ocfg)
  model.compile()
  assert model.score_guard_trips == 0
  s = score_pass(model, x.to(_dev()), False, 2, 120)              # what is left behind is the exact-fp32 repeat: unfused
  assert model.score_guard_trips == 1 and _lib.lib().wn_debug_value(1) == 0
  rel = ((s['nll'].cpu().double() - ref['nll']).abs() / ref['nll'].abs()).max().item()
  print(f'score under a forced trip: nll worst relative {rel:.2e} (bar 2e-3: fp32 at a stream of 1e5 has an ulp of 8e-3)')
  assert bool(torch.isfinite(s['nll']).all()) and rel <= 2e-3
  ev = model.test_step(x.to(_dev()))['loss']
  assert model.test_guard_trips == 1 and abs(float(s['nll'].double().sum()) / 2 - ev) <= 2e-5 * abs(ev)
