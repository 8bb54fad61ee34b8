"""Adam(use_ema=True): the exponential moving average of the weights, written by the Adam launch (wn_adam_kernel<true, false, false>),
and WaveNet.averaged_weights(), the scope that runs the model's passes on it.

The definition, with t the 1-based iteration, after the parameter update of step t:
  t == 1: a = p;   t > 1: a = a + (p - a) * (1 - ema_momentum), fp32;   t % ema_overwrite_frequency == 0: p = a.
The average observes: p, m, v of a run with the flag are those of a run without it, bit for bit.  The arithmetic is restated
here in numpy fp64 from the parameters read back after every step.
"""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# the networks of tests/test_gpu_clip_order.py
KW = dict(blocks=6, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[48, 40],
          activation='leaky_relu', bits=8, l2_reg_factor=0.001)
KW_CONFIGS1 = dict(blocks=30, channels=64, skip_channels=256, dilation_bound=1024, final_layers_channels=[128, 256],
                   activation='leaky_relu', bits=8)
KWS = {'small': KW, 'configs1': KW_CONFIGS1}
SHAPES = {'small': (4, 300), 'configs1': (2, 3500)}
LR, CLIPNORM, SEED = 5e-4, 1.0, 7
PARAM_BAR_SMALL = 4 * 4.710e-6       # tests/test_gpu_clip_order.py: PARAM_BAR['small'], its two-rank bar for the parameters


def dev():
  return torch.device('cuda', 0)


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _data(net, d=None):
  from wavenets_amd.data import synthetic_waveforms
  B, T = SHAPES[net]
  return synthetic_waveforms(B, T + 1, seed=99, device='cpu').to(d or dev())


def _model(net='small', d=None, **opt):
  from wavenets_amd import Adam, WaveNet
  model = WaveNet(**KWS[net], device=d or dev(), seed=SEED)
  model.build((1, 8, 1))
  model.compile(optimizer=Adam(learning_rate=LR, clipnorm=CLIPNORM, **opt))
  return model


def _bits(t):
  return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
  return torch.equal(_bits(a), _bits(b))


def _state(model):
  opt = model.optimizer
  torch.cuda.synchronize()
  out = {'p': model.flat_params.data.cpu().clone(), 'm': opt.m.cpu().clone(), 'v': opt.v.cpu().clone()}
  if opt.ema is not None:
    out['ema'] = opt.ema.cpu().clone()
  return out


def _restate(ps, momentum, overwrite_frequency=None):
  """numpy fp64: the average after every step from the parameters read back after every step.  ``momentum`` enters as the
  fp32 value the kernel is handed (a C float).  With an overwrite frequency the parameters read back after such a step ARE
  the average, and the recursion needs the updated parameters of that step, which were never stored: those steps take the
  device's value and the recursion goes on from it (their error is checked by the steps in between)."""
  mom = np.float64(np.float32(momentum))
  a = ps[0].astype(np.float64)
  out = [a]
  for t in range(2, len(ps) + 1):
    if overwrite_frequency and t % overwrite_frequency == 0:
      a = ps[t - 1].astype(np.float64)
    else:
      a = a + (ps[t - 1].astype(np.float64) - a) * (1.0 - mom)
    out.append(a)
  return out


# ------------------------------------------------------------------------------------------
# 1. the average observes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', ['small', 'configs1'])
def test_observer_parameters_and_moments_are_those_of_the_run_without_the_flag(net):
  x = _data(net)
  runs = {}
  for flag in (True, False):
    model = _model(net, use_ema=flag)
    logs = [dict(model.train_step(x)) for _ in range(20)]
    assert model.optimizer.iterations == 20
    runs[flag] = (_state(model), logs, model.train_guard_trips)
  for key in ('p', 'm', 'v'):
    assert _same(runs[True][0][key], runs[False][0][key]), key
  assert runs[True][1] == runs[False][1] and runs[True][2] == runs[False][2]
  assert 'ema' in runs[True][0] and 'ema' not in runs[False][0]
  assert not _same(runs[True][0]['ema'], runs[True][0]['p'])          # 20 steps in, the average trails the weights


# ------------------------------------------------------------------------------------------
# 2. first step
# ------------------------------------------------------------------------------------------
def test_first_step_copies_the_parameters():
  model = _model(use_ema=True)
  before = model.flat_params.data.clone()
  assert _same(model.optimizer.ema, before)                            # Adam.build: a copy of the current parameters
  model.optimizer.ema.fill_(float('nan'))                              # a copy, not a multiply by zero
  model.train_step(_data('small'))
  s = _state(model)
  assert _same(s['ema'], s['p']) and not _same(s['p'], before)
  assert model.optimizer.ema.data_ptr() != model.flat_params.data_ptr()


# ------------------------------------------------------------------------------------------
# 3. arithmetic
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('momentum,steps', [(0.9, 40), (0.99, 200)])
def test_average_follows_the_fp64_restatement(momentum, steps):
  """Bound: |a_gpu - a_ref| <= 2 * 2^-24 * max|a| / (1 - momentum): every step commits at most about 2^-24 |a| of rounding
  and the recursion damps earlier error by ``momentum`` (geometric sum 1 / (1 - momentum)); at 0.99 that is 1.2e-5 max|a|.
  An error beyond a quarter of the bound means that the expression is not the one specified."""
  model = _model(use_ema=True, ema_momentum=momentum)
  x = _data('small')
  ps, avs = [], []
  for _ in range(steps):
    model.train_step(x)
    s = _state(model)
    ps.append(s['p'].numpy())
    avs.append(s['ema'].numpy())
  ref = _restate(ps, momentum)
  worst = 0.0
  for t, (a, r) in enumerate(zip(avs, ref), 1):
    bound = 2.0 * 2.0 ** -24 * np.abs(r).max() / (1.0 - momentum)
    err = np.abs(a.astype(np.float64) - r).max()
    worst = max(worst, err / bound)
    assert err <= bound, (t, err, bound)
  print(f'momentum {momentum}, {steps} steps: worst error / bound = {worst:.4f} '
        f'(bound at the last step {bound:.3e}, max|a| {np.abs(ref[-1]).max():.4f}, error at the last step {err:.3e})')
  assert worst <= 0.25, worst
  assert np.abs(avs[-1] - ps[-1]).max() > 100 * bound                 # not vacuous: the average is far from the weights


# ------------------------------------------------------------------------------------------
# 4. skip flag, straight at the C-ABI
# ------------------------------------------------------------------------------------------
def test_skip_flag_leaves_the_average_untouched():
  from wavenets_amd import _lib
  model = _model(use_ema=True)
  n, nt = model.flat_params.numel(), len(model.variable_names)
  gen = torch.Generator().manual_seed(3)
  init = {k: torch.randn(n, generator=gen) * s for k, s in (('p', 0.1), ('g', 0.01), ('m', 0.01), ('a', 0.1))}
  init['v'] = torch.rand(n, generator=gen) * 1e-4

  def call(flag, step=5, overwrite=0):
    b = {k: t.clone().to(dev()) for k, t in init.items()}
    scratch = torch.zeros(nt + 8, dtype=torch.float32, device=dev())
    skip = None if flag is None else torch.tensor([flag], dtype=torch.float32, device=dev())
    _lib.check(_lib.lib().wn_adam_step_ema(model._plan, _lib.ptr(b['p']), _lib.ptr(b['g']), _lib.ptr(b['m']), _lib.ptr(b['v']),
                                           _lib.ptr(b['a']), step, LR, 0.9, 0.999, 1e-7, CLIPNORM, 0.99, overwrite,
                                           _lib.ptr(scratch), _lib.ptr(skip), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in b.items()}
  skipped, ran, plain = call(1.0), call(0.0), call(None)
  for k in ('p', 'm', 'v', 'a', 'g'):
    assert _same(skipped[k], init[k]), k
  for k in ('p', 'm', 'v', 'a'):
    assert _same(ran[k], plain[k]), k
    assert not _same(ran[k], init[k]), k
  # the unguarded call against the expression, and the old kernel for p, m, v
  b = {k: t.clone().to(dev()) for k, t in init.items()}
  scratch = torch.zeros(nt + 8, dtype=torch.float32, device=dev())
  _lib.check(_lib.lib().wn_adam_step_guarded(model._plan, _lib.ptr(b['p']), _lib.ptr(b['g']), _lib.ptr(b['m']), _lib.ptr(b['v']),
                                             5, LR, 0.9, 0.999, 1e-7, CLIPNORM, _lib.ptr(scratch), None, _lib.stream_ptr()))
  torch.cuda.synchronize()
  for k in ('p', 'm', 'v'):
    assert _same(b[k], plain[k]), k
  ref = init['a'].double() + (plain['p'].double() - init['a'].double()) * (1.0 - float(np.float32(0.99)))
  assert (plain['a'].double() - ref).abs().max().item() <= 2.0 * 2.0 ** -24 * ref.abs().max().item()
  # step 1 copies; overwrite hands the average back to the parameters
  first = call(None, step=1)
  assert _same(first['a'], first['p'])
  over = call(None, overwrite=1)
  assert _same(over['a'], plain['a']) and _same(over['p'], over['a']) and _same(over['m'], plain['m'])


# ------------------------------------------------------------------------------------------
# 5. overwrite
# ------------------------------------------------------------------------------------------
def test_overwrite_frequency_hands_the_average_back_every_third_step():
  momentum = 0.9
  model = _model(use_ema=True, ema_momentum=momentum, ema_overwrite_frequency=3)
  x = _data('small')
  ps, avs = [], []
  for t in range(1, 11):
    model.train_step(x)
    s = _state(model)
    # step 1 is the plain copy of the definition: a = p there as well
    assert _same(s['p'], s['ema']) == (t in (1, 3, 6, 9)), t
    ps.append(s['p'].numpy())
    avs.append(s['ema'].numpy())
  ref = _restate(ps, momentum, overwrite_frequency=3)
  for t, (a, r) in enumerate(zip(avs, ref), 1):
    bound = 2.0 * 2.0 ** -24 * np.abs(r).max() / (1.0 - momentum)
    assert np.abs(a.astype(np.float64) - r).max() <= 0.25 * bound, t
  # the overwritten run is a different trajectory from the observed one
  plain = _model(use_ema=True, ema_momentum=momentum)
  for _ in range(10):
    plain.train_step(x)
  assert not _same(plain.flat_params.data, model.flat_params.data)


# ------------------------------------------------------------------------------------------
# 6. the scope
# ------------------------------------------------------------------------------------------
def _trained(steps=6, **opt):
  model = _model(use_ema=True, ema_momentum=0.9, **opt)
  x = _data('small')
  for _ in range(steps):
    model.train_step(x)
  torch.cuda.synchronize()
  return model, x


def _twin_on(flat):
  """A second model of the same spec whose weights are set_weights-ed to ``flat``."""
  from wavenets_amd import WaveNet
  twin = WaveNet(**KW, device=dev(), seed=SEED + 1)
  twin.build((1, 8, 1))
  flat = flat.cpu()
  twin.set_weights([flat[o:o + int(np.prod(s))].view(*s).numpy() for o, s in zip(twin._offsets, twin._shapes)])
  return twin


def test_scope_runs_every_pass_on_the_average_and_restores():
  model, x = _trained()
  opt = model.optimizer
  raw, avg = model.flat_params.data.clone(), opt.ema.clone()
  raw_ptr, avg_ptr = model.flat_params.data_ptr(), opt.ema.data_ptr()
  assert not _same(raw, avg)
  twin = _twin_on(avg)
  xin = x[:, :-1, :]
  with model.averaged_weights() as scoped:
    assert scoped is model
    assert model.flat_params.data_ptr() == avg_ptr                     # a swap: no copy
    assert _same(model.call(xin), twin.call(xin))
    assert _same(model.logits(xin), twin.logits(xin))
    for queued in (True, False):
      assert _same(model.generate(64, use_queues=queued, seed=7), twin.generate(64, use_queues=queued, seed=7)), queued
    for a, b in zip(model.get_weights(), twin.get_weights()):
      assert np.array_equal(a.view(np.int32), b.view(np.int32))
    twin.compile()
    want = twin.test_step(x)
  assert model.flat_params.data_ptr() == raw_ptr and opt.ema.data_ptr() == avg_ptr
  assert _same(model.flat_params.data, raw) and _same(opt.ema, avg)
  assert model._averaged is None
  # outside, the passes are the raw weights' again, and those differ
  assert _same(model.call(xin), _twin_on(raw).call(xin)) and not _same(model.call(xin), twin.call(xin))
  # test_step inside the scope reports the twin's loss (the model's tracker holds the training steps: reset it first)
  for metric in model.metrics:
    metric.reset_state()
  with model.averaged_weights():
    got = model.test_step(x)
  assert got['loss'] == want['loss'], (got, want)


def test_scope_refuses_training_and_writes_and_restores_after_an_exception(tmp_path):
  from wavenets_amd import Adam, WaveNet, io
  model, x = _trained()
  raw = model.flat_params.data.clone()
  with model.averaged_weights():
    with pytest.raises(RuntimeError, match='averaged_weights'):
      model.train_step(x)
    with pytest.raises(RuntimeError, match='averaged_weights'):
      model.loss_and_grads(x)
    with pytest.raises(RuntimeError, match='averaged_weights'):
      model.set_weights(model.get_weights())
    with pytest.raises(RuntimeError, match='averaged_weights'):
      io.save_weights(model, str(tmp_path / 'ckpt.weights.npz'), model.optimizer)
    with pytest.raises(RuntimeError, match='averaged_weights'):
      with model.averaged_weights():
        pass
    assert model._averaged is not None                                 # the refused second entry did not end the first
  assert _same(model.flat_params.data, raw) and model.optimizer.iterations == 6
  assert not (tmp_path / 'ckpt.weights.npz').exists()
  # a pass that raises inside the scope still restores
  with pytest.raises(ValueError):
    with model.averaged_weights():
      model.generate(8, temperature=-1.0)
  assert _same(model.flat_params.data, raw) and model._averaged is None
  with pytest.raises(ZeroDivisionError):
    with model.averaged_weights():
      1 / 0
  assert _same(model.flat_params.data, raw) and model._averaged is None
  model.train_step(x)                                                  # and training goes on
  assert model.optimizer.iterations == 7
  # without an optimizer, or without the flag, entering names the flag
  for optimizer in (None, Adam(learning_rate=LR)):
    bare = WaveNet(**KW, device=dev(), seed=SEED)
    bare.build((1, 8, 1))
    bare.compile(optimizer=optimizer)
    with pytest.raises(RuntimeError, match='use_ema'):
      with bare.averaged_weights():
        pass


def test_finalize_variable_values():
  model, x = _trained()
  avg = model.optimizer.ema.clone()
  with model.averaged_weights():
    with pytest.raises(RuntimeError, match='averaged_weights'):
      model.optimizer.finalize_variable_values(model)
  model.optimizer.finalize_variable_values(model)
  assert _same(model.flat_params.data, avg) and _same(model.optimizer.ema, avg)
  plain = _model()
  plain.train_step(x)
  before = plain.flat_params.data.clone()
  assert plain.optimizer.finalize_variable_values(plain) is None and _same(plain.flat_params.data, before)


# ------------------------------------------------------------------------------------------
# 7. checkpoints
# ------------------------------------------------------------------------------------------
def test_checkpoint_resume_equals_the_uninterrupted_run(tmp_path):
  from wavenets_amd import io
  x = _data('small')
  opt = dict(use_ema=True, ema_momentum=0.9)
  whole = _model(**opt)
  for _ in range(10):
    whole.train_step(x)
  first = _model(**opt)
  for _ in range(5):
    first.train_step(x)
  path = str(tmp_path / 'weights-e0001-lr0.0005.weights.npz')
  io.save_weights(first, path, first.optimizer)
  with np.load(path) as d:
    assert 'adam_ema' in d and d['adam_ema'].shape == d['adam_m'].shape
  second = _model(**opt)
  io.load_weights(second, path, second.optimizer)
  assert second.optimizer.iterations == 5
  for key, t in _state(first).items():
    assert _same(_state(second)[key], t), key
  for _ in range(5):
    second.train_step(x)
  for key, t in _state(whole).items():
    assert _same(_state(second)[key], t), key

  # a file without an average (written by a plain optimizer) gives ema == loaded weights
  plain = _model()
  for _ in range(3):
    plain.train_step(x)
  bare = str(tmp_path / 'plain.weights.npz')
  io.save_weights(plain, bare, plain.optimizer)
  with np.load(bare) as d:
    assert 'adam_ema' not in d
  late = _model(**opt)
  late.train_step(x)                                                   # its own average, to be replaced
  io.load_weights(late, bare, late.optimizer)
  assert _same(late.optimizer.ema, plain.flat_params.data) and _same(late.flat_params.data, plain.flat_params.data)
  assert late.optimizer.iterations == 3
  late.train_step(x)                                                   # t = 4 > 1: averages from the loaded weights
  s = _state(late)
  ref = plain.flat_params.data.cpu().double()
  ref = ref + (s['p'].double() - ref) * (1.0 - float(np.float32(0.9)))
  assert (s['ema'].double() - ref).abs().max().item() <= 2.0 * 2.0 ** -24 * ref.abs().max().item()
  # a file with an average loaded into a plain optimizer: ignored
  other = _model()
  io.load_weights(other, path, other.optimizer)
  assert other.optimizer.ema is None and _same(other.optimizer.m, first.optimizer.m)

  # .weights.h5 stays weights-only; saved inside the scope it holds the average
  h5 = str(tmp_path / 'averaged.weights.h5')
  with first.averaged_weights():
    io.save_weights(first, h5)
  reader = _model()
  io.load_weights(reader, h5)
  assert _same(reader.flat_params.data, first.optimizer.ema)
  assert not _same(reader.flat_params.data, first.flat_params.data)


# ------------------------------------------------------------------------------------------
# 8. data parallel
# ------------------------------------------------------------------------------------------
DP_STEPS = 5


def _dp_train(model, x):
  for _ in range(DP_STEPS):
    model.train_step(x)
  out = _state(model)
  out['trips'] = model.train_guard_trips
  return out


def _worker(rank, world, port, backend, out_dir, net):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  torch.cuda.set_device(0)
  d = torch.device('cuda', 0)
  if backend == 'nccl':
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=d)
  else:
    dist.init_process_group('gloo', rank=rank, world_size=world)
  from wavenets_amd import dp
  assert dp.initialized() and dp.world_size() == world
  model = _model(net, d, use_ema=True, ema_momentum=0.9)
  B = SHAPES[net][0]
  x = _data(net, d)[dp.shard_rows(B, world, rank)]
  torch.save(_dp_train(model, x), os.path.join(out_dir, f'{backend}_rank{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


def test_two_ranks_one_gpu_gloo_hold_the_same_average(tmp_path):
  mp.spawn(_worker, args=(2, _free_port(), 'gloo', str(tmp_path), 'small'), nprocs=2, join=True)
  r0 = torch.load(tmp_path / 'gloo_rank0.pt')
  r1 = torch.load(tmp_path / 'gloo_rank1.pt')
  for key in ('p', 'm', 'v', 'ema'):                                   # nothing was added to the collective
    assert _same(r0[key], r1[key]), key
  assert r0['trips'] == r1['trips'] == 0
  single = _dp_train(_model('small', use_ema=True, ema_momentum=0.9), _data('small'))
  for key in ('p', 'ema'):
    err = (r0[key].double() - single[key].double()).abs().max().item()
    print(f'two ranks vs one process, same global batch: max |d {key}| = {err:.3e} (bar {PARAM_BAR_SMALL:.3e})')
    assert err <= PARAM_BAR_SMALL, (key, err)
  assert not _same(r0['ema'], r0['p'])


def test_nccl_world_size_one_equals_no_process_group(tmp_path):
  """The one-collective tail branch of the step (a process group of one rank over RCCL) against the early-logs branch (no
  process group), the configs[1] network: the reduce of one replica is the identity, the average is bit-equal."""
  if not dist.is_nccl_available():
    pytest.skip('no RCCL backend in this torch build')
  mp.spawn(_worker, args=(1, _free_port(), 'nccl', str(tmp_path), 'configs1'), nprocs=1, join=True)
  r = torch.load(tmp_path / 'nccl_rank0.pt')
  s = _dp_train(_model('configs1', use_ema=True, ema_momentum=0.9), _data('configs1'))
  for key in ('p', 'm', 'v', 'ema'):
    assert _same(s[key], r[key]), key
  assert s['trips'] == r['trips'] == 0
