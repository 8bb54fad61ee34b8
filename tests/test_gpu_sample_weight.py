"""sample_weight of train_step / test_step / loss_and_grads on the device, against the fp64
reference of tests/weighted_reference.py (pinned on the CPU in tests/test_sample_weight_cpu.py) and, where the statement is
about bits, against the device's own unweighted pass.

Standard batch: B = 3, T = 150 (T mod 32 = 22); utterance 0 weighs 1 everywhere, utterance 1 is length_weights(113),
utterance 2 is uniform in [0, 2) with every seventh entry exactly 0.  Which loss kernel ran is asserted first in every
case, with the logits-region sentinel of tests/test_gpu_head_tile_walk.py: the region is filled before the call and must
be untouched after a pass that fused the loss into the head's last conv, fully overwritten after any other; which
standalone kernel that other is follows from the head (route() of that file: 256 classes or fewer, more, a mixture).

Bars are the project's own: loss 2e-5 relative (section 24), every parameter gradient 1e-4 max|ref| + 1e-7
(test_loss_and_gradients_parity), range flag 0.  No row is excused: the reference's target probabilities are asserted to
lie far inside Keras's clip."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import weighted_reference as W
from test_gpu_parity import MODEL_CASES, make_pair, _inputs, math_mode  # noqa: F401  (math_mode: fixture)
from test_gpu_head_tile_walk import route, _full

pytestmark = pytest.mark.gpu

B, T = 3, 150
SENTINEL = 12345.0
# case id -> (name in MODEL_CASES, keywords on top, the last launch of the head in split mode)
NETS = {
    'cat_r64': ('cat_r64', {}, 'epilogue planes16s<1,8,-3>'),
    'cat_small_fused': ('cat_small_fused', {}, 'wn_cat_loss256_kernel'),
    'cat_noskipch': ('cat_noskipch', {}, 'wn_cat_loss256_kernel'),
    'cat_r64_c512': ('cat_r64', dict(bits=9), 'wn_cat_loss_kernel'),
    'mol': ('mol', {}, 'wn_mix_loss_kernel'),
    'gauss': ('gauss', {}, 'wn_mix_loss_kernel'),
    'cond': ('cond', {}, 'wn_cat_loss256_kernel'),
    'cat_lpb2_r64': ('cat_lpb2_r64', {}, None),          # (stacked convs: route() does not describe the blocks; head as below)
}
ONE_PER_KERNEL = ['cat_r64', 'cat_noskipch', 'cat_r64_c512', 'mol']


def _dev():
  return torch.device('cuda', 0)


def _kw(case):
  name, extra, _ = NETS[case]
  return dict(MODEL_CASES[name], **extra)


def _fusable(case):
  """loss_fusable (wn_forward.hip) and the streamed kernel's shape rule, restated by route() of the head tile-walk file."""
  kw = _full({k: v for k, v in _kw(case).items() if k != 'cond_inputs'})
  return route(kw)[-1].startswith('epilogue')


def test_the_cases_reach_the_kernels_they_are_there_for():
  for case, (_, _, last) in NETS.items():
    kw = _full({k: v for k, v in _kw(case).items() if k != 'cond_inputs'})
    if last is not None:
      assert route(kw)[-1] == last, (case, route(kw))
  assert _fusable('cat_r64') and _fusable('cat_lpb2_r64') and not _fusable('cat_small_fused')   # (40-wide operand: no image)
  assert T % 32 == 22


def _pair(case, seed=4):
  return make_pair(seed=seed, **_kw(case))


def _data(case, b=B, t=T, seed=8):
  x, cond = _inputs(_kw(case), b, t + 1, seed=seed)
  return x, cond


def _pack(x, cond):
  return (x.to(_dev()), cond.to(_dev())) if cond is not None else x.to(_dev())


def std_weights(b=B, t=T, seed=21):
  from wavenets_amd.data import length_weights
  assert b == 3
  g = torch.Generator().manual_seed(seed)
  w = torch.ones(b, t)
  w[1] = length_weights([113], t)[0]
  w[2] = torch.rand(t, generator=g) * 2
  w[2, ::7] = 0.0
  return w


def step(model, data, fused, b=B, t=T, **kwargs):
  """One loss_and_grads call with the logits region holding the sentinel beforehand; asserts which family of loss kernel
  ran.  Returns what loss_and_grads returns."""
  from wavenets_amd import _lib
  model._workspace('train', _lib.lib().wn_plan_workspace_floats(model._plan, b, t, 1))
  model.training_intermediate(5, 0, b, t).fill_(SENTINEL)
  out = model.loss_and_grads(data, global_batch=b, **kwargs)
  torch.cuda.synchronize()
  logits = model.training_intermediate(5, 0, b, t)
  if fused:
    assert bool((logits == SENTINEL).all()), 'the fused loss epilogue was expected and a logits tensor was written'
  else:
    assert not bool((logits == SENTINEL).any()), 'a standalone loss kernel was expected and the logits were not (all) written'
  return out


_REF = {}


def _reference(case, params, ocfg, x, cond, w):
  """fp64 reference of the standard batch, once a case (both math modes share it)."""
  if case not in _REF:
    _REF[case] = W.weighted_loss_and_grads(x, params, ocfg, w, cond, global_batch=x.shape[0])
  return _REF[case]


def _check_against(model, loss, ref, what):
  assert float(loss[2]) == 0.0, (what, 'range guard tripped')
  lr = float(ref['loss'])
  rel = abs(float(loss[0]) - lr) / abs(lr)
  print(f'{what}: loss {float(loss[0])!r} reference {lr!r} relative {rel:.2e}')
  assert rel <= 2e-5, (what, float(loss[0]), lr)
  worst = 0.0
  for n, g, r in zip(model.variable_names, model.gradients(), ref['grads']):
    assert bool(torch.isfinite(g).all()), (what, n)
    err = (g.cpu().double() - r).abs().max().item()
    bar = 1e-4 * r.abs().max().item() + 1e-7
    worst = max(worst, err / bar)
    assert err < bar, (what, n, err, bar)
  print(f'{what}: worst gradient err / bar {worst:.2e}')


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('case', list(NETS))
def test_weighted_step_against_the_fp64_reference(case, math_mode):
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  w = std_weights()
  ref = _reference(case, params, ocfg, x, cond, w)
  if ref['target_prob'] is not None:                       # far from Keras's clip: no row sits at the kink
    assert bool(((ref['target_prob'] > 1e-5) & (ref['target_prob'] < 1 - 1e-5)).all()), case
  fused = math_mode == 'split' and _fusable(case)
  if case in ('cat_r64', 'cat_lpb2_r64'):
    assert fused == (math_mode == 'split')
  loss, _, _ = step(model, _pack(x, cond), fused, sample_weight=w.to(_dev()))
  _check_against(model, loss, ref, f'{case} [{math_mode}]')


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('case', ONE_PER_KERNEL)
def test_all_ones_are_no_weights_bit_for_bit(case):
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  data = _pack(x, cond)
  got = []
  for sw in (None, torch.ones(B, T, device=_dev()), torch.ones(B, device=_dev()), torch.ones(B, T, 1, device=_dev())):
    model._sample_calls = 7
    model.set_drop_step(0)
    kw = {} if sw is None else {'sample_weight': sw}
    loss, samp, _ = step(model, data, _fusable(case), want_sample=True, **kw)
    assert model._sample_calls == 8 and samp.shape == (B, T, 1)
    got.append((loss.clone(), model.flat_grads.clone(), model.training_intermediate(12, 0, B, T).clone(), samp.clone()))
  for other in got[1:]:
    for name, a, b in zip(('loss', 'flat_grads', 'loss rows', 'sample'), got[0], other):
      assert torch.equal(a, b), (case, name, (a - b).abs().max().item())
  assert float(got[0][0][0]) > 0 and float(got[0][1].abs().max()) > 0


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('case', ['cat_r64', 'cat_noskipch', 'mol'])
def test_a_masked_region_does_not_exist_bit_for_bit(case):
  from wavenets_amd.data import length_weights
  ocfg, params, model = _pair(case)
  x, cond = _data(case)
  lengths = (150, 113, 40)
  w = length_weights(lengths, T).to(_dev())
  noise = torch.rand(x.shape, generator=torch.Generator().manual_seed(77)) * 2 - 1
  xa, xb = x.clone(), x.clone()
  for b, l in enumerate(lengths):
    xa[b, l + 1:] = 0.0
    xb[b, l + 1:] = noise[b, l + 1:]
    assert torch.equal(xa[b, :l + 1], xb[b, :l + 1])
  assert not torch.equal(xa, xb)
  got = []
  for xx in (xa, xb):
    loss, _, _ = step(model, _pack(xx, cond), _fusable(case), sample_weight=w)
    assert float(loss[2]) == 0.0
    got.append((loss[0].clone(), model.flat_grads.clone()))
  assert torch.equal(got[0][0], got[1][0]), (case, float(got[0][0]), float(got[1][0]))
  assert torch.equal(got[0][1], got[1][1]), (case, (got[0][1] - got[1][1]).abs().max().item())
  assert bool(torch.isfinite(got[0][1]).all()) and float(got[0][1].abs().max()) > 0
  # without the weights the two batches do differ
  l0 = model.loss_and_grads(_pack(xa, cond), global_batch=B)[0][0].item()
  l1 = model.loss_and_grads(_pack(xb, cond), global_batch=B)[0][0].item()
  assert l0 != l1


# ------------------------------------------------------------------------------------------ 4
def test_a_zero_weight_is_a_select_where_the_rows_own_loss_is_not_finite():
  """DESIGN.md section 17's open case reached by the data alone: every mean 1, every log-scale -7, a target of -1 lies
  2193 scales below: the bin mass underflows in float64, the row's loss is inf and its gradient NaN."""
  kw = dict(blocks=1, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[32], activation='leaky_relu',
            num_mixtures=10, sampling_function='logistic', bits=16)
  ocfg, params, model = make_pair(seed=4, **kw)
  M = 10
  params = [torch.zeros_like(p) for p in params]
  assert params[-1].shape == (3 * M,)
  params[-1][M:2 * M] = 1.0
  params[-1][2 * M:] = -7.0
  model.set_weights([p.numpy() for p in params])
  g = torch.Generator().manual_seed(5)
  w = torch.rand(B, T, generator=g) + 0.5
  zero = torch.rand(B, T, generator=g) < 0.3
  zero[0, 0] = zero[2, T - 1] = True
  w[zero] = 0.0
  x = torch.full((B, T + 1, 1), 0.999)
  x[:, 1:, 0][zero] = -1.0
  data = x.to(_dev())
  loss, _, _ = step(model, data, False)
  assert not bool(torch.isfinite(loss[0])), float(loss[0])
  ref = W.weighted_loss_and_grads(x, params, ocfg, w, None, global_batch=B)
  assert bool(torch.isfinite(ref['loss'])) and float(ref['grads'][-1].abs().max()) > 0
  loss, _, _ = step(model, data, False, sample_weight=w.to(_dev()))
  assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(model.flat_grads).all())
  _check_against(model, loss, ref, 'underflowing rows under weight 0')
  rows = model.training_intermediate(12, 0, B, T).reshape(B, T).cpu()
  assert bool((rows[zero] == 0).all()) and bool(torch.isfinite(rows).all())
  gp = model.training_intermediate(6, len(ocfg.final_layers_channels), B, T).reshape(B, T, -1).cpu()
  assert bool((gp[zero] == 0).all()) and float(gp.abs().max()) > 0


# ------------------------------------------------------------------------------------------ 5
WALK = {
    # fused epilogue: 3 x 688 = 2064 tiles of 32 rows against a grid of 2048 waves, T mod 32 = 17
    'cat_r64': (3, 22001),
    # a row a wave: 9003 rows against 8192 a pass
    'cat_noskipch': (3, 3001),
    'cat_r64_c512': (3, 3001),
    # a thread a row, no loop
    'mol': (3, 150),
}


def test_the_walk_shapes_reach_a_second_pass():
  b, t = WALK['cat_r64']
  assert -(-t // 32) == 688 and b * 688 == 2064 > 2048 and t % 32 == 17
  b, t = WALK['cat_noskipch']
  assert b * t == 9003 > 2048 * 4 and WALK['cat_r64_c512'] == (b, t)


@pytest.mark.parametrize('case', list(WALK))
def test_the_weight_is_read_from_the_right_row_in_every_tile_and_pass(case):
  from wavenets_amd.data import synthetic_waveforms
  b, t = WALK[case]
  ocfg, params, model = _pair(case)
  nf = len(ocfg.final_layers_channels)
  x = synthetic_waveforms(b, t + 1, seed=5, device=_dev())
  g = torch.Generator().manual_seed(31)
  w = torch.tensor([0.0, 1.0, 2.0, 4.0])[torch.randint(0, 4, (b, t), generator=g)].to(_dev())
  assert all(int((w == v).sum()) > 0 for v in (0.0, 1.0, 2.0, 4.0))
  fused = _fusable(case)

  def regions():
    return (model.training_intermediate(12, 0, b, t).reshape(b, t).clone(),
            model.training_intermediate(6, nf, b, t).reshape(b, t, -1).clone())
  loss0, _, _ = step(model, x, fused, b, t)
  rows0, gf0 = regions()
  assert float(loss0[2]) == 0.0 and bool(torch.isfinite(gf0).all()) and bool(torch.isfinite(rows0).all())
  nz = gf0[gf0 != 0].abs()
  assert nz.numel() > 0 and float(nz.min()) >= 2.0 ** -100, float(nz.min())      # nothing near the denormals: w * g is exact
  loss1, _, _ = step(model, x, fused, b, t, sample_weight=w)
  rows1, gf1 = regions()
  assert float(loss1[2]) == 0.0
  for name, got, want in (('loss rows', rows1, w * rows0), ('dL/dlogits', gf1, w[..., None] * gf0)):
    bad = (got != want).reshape(b, t, -1).any(dim=-1)
    if bool(bad.any()):
      u, tt = divmod(int(bad.flatten().nonzero()[0]), t)
      tile = u * -(-t // 32) + tt // 32
      raise AssertionError(f'{case} {name}: first differing row: utterance {u}, t {tt}, weight {float(w[u, tt])}; 32-row tile {tile} '
                           f'(pass {tile // 2048}), row-kernel pass {(u * t + tt) // 8192}; rows that differ: {int(bad.sum())}')


# ------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize('case', ['cat_r64', 'mol'])
def test_evaluation_weighs_its_rows(case):
  ocfg, params, model = _pair(case)
  model.compile()
  x, cond = _data(case)
  w = std_weights()
  ref = _reference(case, params, ocfg, x, cond, w)
  data = _pack(x, cond)
  plain = model.test_step(data)['loss']
  for m in model.metrics:
    m.reset_state()
  ev = model.test_step(data, sample_weight=w.to(_dev()))['loss']
  rel = abs(ev - float(ref['loss'])) / abs(float(ref['loss']))
  print(f'{case}: weighted evaluation loss {ev!r}, reference {float(ref["loss"])!r}, relative {rel:.2e}; unweighted {plain!r}')
  assert model.test_guard_trips == 0 and rel <= 2e-5
  assert abs(ev - plain) > 1e-3 * abs(plain)
  # and nothing stays armed behind it
  for m in model.metrics:
    m.reset_state()
  assert model.test_step(data)['loss'] == plain


# ------------------------------------------------------------------------------------------ 7
def _mse_bar(ref, n):
  # the reduction's own: two fp64 sums of n terms (numerator, denominator), one fp64 quotient, one fp32 store
  bar = 2.0 ** -24 * abs(ref) + 2 * (n + 2) * 2.0 ** -53 * abs(ref)
  assert bar < 1e-6 * abs(ref)
  return bar


@pytest.mark.parametrize('case', ['cat_r64', 'mol'])
def test_the_compiled_metric_is_the_weighted_mean(case):
  from wavenets_amd import Adam, MeanSquaredError
  ocfg, params, model = _pair(case, seed=40)
  model.compile(optimizer=Adam(learning_rate=1e-3, clipnorm=1.0), metrics=[MeanSquaredError()])
  x, cond = _data(case, seed=41)
  data = _pack(x, cond)
  w = std_weights().to(_dev())
  y = data[:, 1:, :] if cond is None else data[0][:, 1:, :]
  # train_step: the sample is drawn inside the step, from the weights before the update
  saved, calls = model.flat_params.detach().clone(), model._sample_calls
  logs = model.train_step(data, sample_weight=w)
  with torch.no_grad():
    model.flat_params.copy_(saved)
  model._sample_calls = calls
  _, samp, _ = model.loss_and_grads(data, want_sample=True, sample_weight=w)
  ref = W.weighted_mse(y.cpu(), samp.cpu(), w.cpu())
  err = abs(logs['mean_squared_error'] - ref)
  print(f'{case} train_step: metric {logs["mean_squared_error"]!r} reference {ref!r} err {err:.3e} bar {_mse_bar(ref, B * T):.3e}')
  assert ref > 0 and err <= _mse_bar(ref, B * T)
  plain = W.weighted_mse(y.cpu(), samp.cpu(), torch.ones(B, T))
  assert abs(plain - ref) > 1e-3 * ref                       # the weights matter to it
  # test_step: the sample is drawn from the evaluation's prediction
  for m in model.metrics:
    m.reset_state()
  calls = model._sample_calls
  logs = model.test_step(data, sample_weight=w)
  model._sample_calls = calls
  xin = data[:, :-1, :].contiguous() if cond is None else (data[0][:, :-1, :].contiguous(), data[1])
  samp = model.sample_waveform(model(xin))
  ref = W.weighted_mse(y.cpu(), samp.cpu(), w.cpu())
  err = abs(logs['mean_squared_error'] - ref)
  print(f'{case} test_step: metric {logs["mean_squared_error"]!r} reference {ref!r} err {err:.3e} bar {_mse_bar(ref, B * T):.3e}')
  assert ref > 0 and err <= _mse_bar(ref, B * T)
  # all weights 0: the metric is 0, not 0 / 0, and so is the loss
  for step_fn in (model.train_step, model.test_step):
    for m in model.metrics:
      m.reset_state()
    logs = step_fn(data, sample_weight=torch.zeros(B, T, device=_dev()))
    assert logs['mean_squared_error'] == 0.0 and logs['loss'] == 0.0, logs
  assert bool(torch.isfinite(model.flat_params).all())


# ------------------------------------------------------------------------------------------ 8
def _dp_weights():
  from test_gpu_dp import GLOBAL_B, T as DT
  g = torch.Generator().manual_seed(13)
  w = torch.rand(GLOBAL_B, DT, generator=g) * 2
  w[:, ::5] = 0.0
  w[1, 200:] = 0.0
  return w


def _dp_steps(model, x, w):
  from wavenets_amd import Adam, MeanSquaredError
  from test_gpu_dp import STEPS
  model.compile(optimizer=Adam(learning_rate=5e-4, clipnorm=1.0), metrics=[MeanSquaredError()])
  logs = None
  for _ in range(STEPS):
    logs = model.train_step(x, sample_weight=w)
  return logs


def _dp_worker(rank, world, port, out_dir):
  from test_gpu_dp import KW, GLOBAL_B, _data
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from wavenets_amd import WaveNet, dp
  model = WaveNet(**KW, device=dev, seed=7)
  rows = dp.shard_rows(GLOBAL_B, world, rank)
  logs = _dp_steps(model, _data('small')[rows].to(dev), _dp_weights()[rows].to(dev))
  torch.save({'params': model.flat_params.data.cpu(), 'logs': logs}, os.path.join(out_dir, f'rank{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


def test_two_rank_weighted_steps_equal_the_single_process(tmp_path):
  """Three weighted steps with rows and weights sharded by dp.shard_rows (gloo, both ranks on the one GPU) against the
  single-process weighted steps, at the bars of test_two_rank_train_step_equals_single_process."""
  from wavenets_amd import WaveNet
  from test_gpu_dp import KW, _data, _free_port
  mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
  r0, r1 = torch.load(tmp_path / 'rank0.pt'), torch.load(tmp_path / 'rank1.pt')
  assert torch.equal(r0['params'], r1['params'])
  assert r0['logs'] == r1['logs']
  dev = _dev()
  single = WaveNet(**KW, device=dev, seed=7)
  logs = _dp_steps(single, _data('small').to(dev), _dp_weights().to(dev))
  err = (single.flat_params.data.cpu() - r0['params']).abs().max().item()
  assert err < 1e-5, err
  assert abs(logs['loss'] - r0['logs']['loss']) < 1e-5 * abs(logs['loss'])
  assert abs(logs['reg_loss'] - r0['logs']['reg_loss']) < 1e-6 * max(1.0, abs(logs['reg_loss']))
  # the weights reached the ranks: the unweighted steps end elsewhere
  from test_gpu_dp import _run_steps
  plain = WaveNet(**KW, device=dev, seed=7)
  plain_logs = _run_steps(plain, _data('small').to(dev))
  assert abs(plain_logs['loss'] - logs['loss']) > 1e-3 * abs(logs['loss'])
