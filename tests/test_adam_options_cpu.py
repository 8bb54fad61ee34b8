"""CPU-only checks of Adam's Keras keywords global_clipnorm, clipvalue, weight_decay and amsgrad: the known answers of
tests/adam_reference.py (the fp64 restatement the GPU tests compare with), the Python surface, and the C-ABI boundary --
wn_adam_step_ext and wn_clip_gradients_ext validate their arguments before anything touches the device, so every call
here hands them host memory (never dereferenced) and must come back with WN_E_INVALID."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import adam_reference as AR
from wavenets_amd import _lib, spec


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


# ------------------------------------------------------------------------------------------
# the restatement: hand-computable cases, three elements each
# ------------------------------------------------------------------------------------------
Z3 = np.zeros(3, dtype=np.float32)
KW = dict(lr=0.5, beta_1=0.5, beta_2=0.75, epsilon=0.0)       # all exact in fp32


def test_reference_global_norm_of_exactly_five():
  """Two tensors (3,) and (4, 0): N = 5, c = 2.5 -> one factor 0.5 for both (per tensor it would be 2.5/3 and 2.5/4)."""
  g = np.array([3.0, 4.0, 0.0], dtype=np.float32)
  tensors = [(0, 1), (1, 2)]
  assert AR.clip_factors(g, tensors, global_clipnorm=2.5) == [0.5, 0.5]
  assert AR.clip_factors(g, tensors, clipnorm=2.5) == [2.5 / 3, 2.5 / 4]
  assert AR.clip_factors(g, tensors, global_clipnorm=5.0) == [1.0, 1.0] == AR.clip_factors(g, tensors, global_clipnorm=7.0)
  r = AR.adam_step(Z3, Z3, Z3, None, g, 1, tensors, global_clipnorm=2.5, **KW)
  assert r['g'].tolist() == [1.5, 2.0, 0.0]
  assert r['m'].tolist() == [0.75, 1.0, 0.0]                       # (g' - 0) * (1 - 0.5)
  assert r['v'].tolist() == [0.5625, 1.0, 0.0]                     # g'^2 * (1 - 0.75)
  # alpha = 0.5 * sqrt(0.25) / 0.5 = 0.5;  p = 0 - 0.5 * m / sqrt(v) = -0.5 * 0.75 / 0.75, -0.5 * 1 / 1; 0/0 is NaN
  assert r['alpha'] == 0.5
  assert r['p'][:2].tolist() == [-0.5, -0.5] and np.isnan(r['p'][2])
  # a non-finite norm poisons every tensor
  bad = np.array([3.0, np.inf, 0.0], dtype=np.float32)
  assert all(np.isnan(s) for s in AR.clip_factors(bad, tensors, global_clipnorm=2.5))
  assert np.isnan(AR.adam_step(Z3, Z3, Z3, None, bad, 1, tensors, global_clipnorm=2.5, **KW)['m']).all()


def test_reference_value_clip_at_inside_and_beyond_the_bound():
  c = 0.5
  g = np.array([0.5, -0.5, 0.4999999701976776, -0.25, 7.0, -1e30, np.nan, 0.0, np.inf], dtype=np.float32)
  out = AR.clip(g, [(0, 9)], clipvalue=c)
  assert out[:6].tolist() == [0.5, -0.5, float(np.float32(0.4999999701976776)), -0.25, 0.5, -0.5]
  assert np.isnan(out[6]) and out[7] == 0.0 and out[8] == 0.5
  r = AR.adam_step(Z3, Z3, Z3, None, np.array([7.0, -0.25, np.nan], dtype=np.float32), 1, [(0, 3)], clipvalue=c, **KW)
  assert r['m'][:2].tolist() == [0.25, -0.125] and np.isnan(r['m'][2])


def test_reference_decay_comes_before_the_update_and_takes_lr():
  """p = 2, wd = 0.25, lr = 0.5: p0 = 2 - (2 * 0.25) * 0.5 = 1.75; step 1 of Adam with eps 0 moves by alpha = lr * sign(g)
  = 0.5 whatever |g|: p = 1.25.  After the update it would be 1.5 - 1.5 * 0.125 = 1.3125; with alpha in the decay's place
  the same here (alpha == lr at these betas), so step 2 tells them apart below; the L2 form would change m."""
  p = np.array([2.0, -2.0, 2.0], dtype=np.float32)
  g = np.array([1.0, 4.0, 0.0], dtype=np.float32)
  tensors = [(0, 2), (2, 1)]
  r = AR.adam_step(p, Z3, Z3, None, g, 1, tensors, weight_decay=0.25, **KW)
  assert r['p'][:2].tolist() == [1.25, -2.25]
  assert np.isnan(r['p'][2])                                       # zero gradient at eps 0: 0/0 (eps > 0 below)
  assert r['m'].tolist() == [0.5, 2.0, 0.0] and r['v'].tolist() == [0.25, 4.0, 0.0]       # the decay is not in the moments
  kw = dict(KW, epsilon=1.0)
  r = AR.adam_step(p, Z3, Z3, None, g, 1, tensors, weight_decay=0.25, **kw)
  assert r['p'][2] == 1.75                                         # a zero gradient still decays
  r = AR.adam_step(p, Z3, Z3, None, g, 1, tensors, weight_decay=0.25, decays=[True, False], **kw)
  assert r['p'][2] == 2.0 and r['p'][0] == 1.75 - 0.5 * 0.5 / (0.5 + 1.0)
  # step 2: alpha = 0.5 * sqrt(1 - 0.5625) / 0.75 differs from lr; the decay still takes lr
  r2 = AR.adam_step(p, Z3, Z3, None, np.zeros(3, dtype=np.float32), 2, tensors, weight_decay=0.25, **kw)
  assert r2['alpha'] != 0.5 and r2['p'].tolist() == [1.75, -1.75, 1.75]


def test_reference_vhat_holds_over_a_falling_v():
  v = np.array([4.0, 4.0, 0.0], dtype=np.float32)
  vhat = np.array([4.0, 9.0, 0.0], dtype=np.float32)
  g = np.array([0.0, 0.0, 2.0], dtype=np.float32)
  m = np.array([1.0, 1.0, 0.0], dtype=np.float32)
  r = AR.adam_step(Z3, m, v, vhat, g, 1, [(0, 3)], amsgrad=True, **KW)
  assert r['v'].tolist() == [3.0, 3.0, 1.0]                        # v's own recursion: 4 + (0 - 4) * 0.25
  assert r['vhat'].tolist() == [4.0, 9.0, 1.0]                     # held, held, risen
  assert r['m'].tolist() == [0.5, 0.5, 1.0]
  assert r['p'].tolist() == [-0.5 * 0.5 / 2.0, -0.5 * 0.5 / 3.0, -0.5 * 1.0 / 1.0]
  plain = AR.adam_step(Z3, m, v, None, g, 1, [(0, 3)], **KW)
  assert plain['vhat'] is None and plain['p'][0] == -0.5 * 0.5 / np.sqrt(3.0)


def test_reference_ema_follows_the_updated_parameters():
  p = np.array([1.0, 2.0, 3.0], dtype=np.float32)
  g = np.array([1.0, -1.0, 1.0], dtype=np.float32)
  r1 = AR.adam_step(p, Z3, Z3, None, g, 1, [(0, 3)], ema=np.full(3, 9.0, dtype=np.float32), ema_momentum=0.5, **KW)
  assert r1['ema'].tolist() == r1['p'].tolist() == [0.5, 2.5, 2.5]
  r2 = AR.adam_step(p, Z3, Z3, None, g, 2, [(0, 3)], ema=np.zeros(3, dtype=np.float32), ema_momentum=0.5, ema_overwrite=True, **KW)
  assert np.array_equal(r2['ema'], r2['p_step'] * 0.5) and np.array_equal(r2['p'], r2['ema'])


# ------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------
def test_keywords_defaults_and_validation():
  from wavenets_amd import Adam
  opt = Adam(clipnorm=1.0)
  assert opt.global_clipnorm is None and opt.clipvalue is None and opt.weight_decay is None and opt.amsgrad is False
  assert opt.vhat is None and not opt._extended()
  opt = Adam(global_clipnorm=2, weight_decay=0.01, amsgrad=True)
  assert opt.global_clipnorm == 2.0 and opt.weight_decay == 0.01 and opt.amsgrad is True and opt._extended()
  assert Adam(clipvalue=0.5).clipvalue == 0.5 and Adam(clipvalue=0.5)._extended()
  assert not Adam(weight_decay=0.0, amsgrad=False)._extended() and not Adam(weight_decay=0)._extended()
  for kw in (dict(clipnorm=1.0, global_clipnorm=1.0), dict(clipnorm=1.0, clipvalue=1.0), dict(global_clipnorm=1.0, clipvalue=1.0),
             dict(clipnorm=1.0, global_clipnorm=1.0, clipvalue=1.0)):
    with pytest.raises(ValueError, match='Only one of `clipnorm`, `clipvalue` and `global_clipnorm` can be set'):
      Adam(**kw)
  for name in ('global_clipnorm', 'clipvalue'):
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), -float('inf'), True, False, '1.0', [1.0]):
      with pytest.raises(ValueError, match=name):
        Adam(**{name: bad})
  for bad in (-0.01, float('nan'), float('inf'), -float('inf'), True, False, '0.1'):
    with pytest.raises(ValueError, match='weight_decay'):
      Adam(weight_decay=bad)
  for bad in (1, 0, 'true', None, 1.0):
    with pytest.raises(ValueError, match='amsgrad'):
      Adam(amsgrad=bad)


def test_options_struct_carries_the_keywords():
  from wavenets_amd import Adam
  o = Adam(learning_rate=1e-2, global_clipnorm=3.0, weight_decay=0.1, amsgrad=True)._options()
  assert (o.clip_mode, o.clip, o.amsgrad, o.ema_momentum, o.ema_overwrite) == (_lib.WN_CLIP_GLOBAL_NORM, 3.0, 1, 0.0, 0)
  assert o.weight_decay == np.float32(0.1) and o.lr == np.float32(1e-2) and o.decay_flags is None
  o = Adam(clipvalue=0.5, clip_before_reduce=True)._options()                      # clipped ahead of the reduce already
  assert (o.clip_mode, o.clip) == (_lib.WN_CLIP_NONE, 0.0)
  opt = Adam(clipnorm=1.0, amsgrad=True, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=2)
  opt.iterations = 4
  o = opt._options()
  assert (o.clip_mode, o.clip, o.ema_overwrite) == (_lib.WN_CLIP_NORM, 1.0, 1) and o.ema_momentum == np.float32(0.9)
  opt.iterations = 5
  assert opt._options().ema_overwrite == 0


def test_no_ops_without_the_flag_and_without_a_model():
  from wavenets_amd import Adam
  for kw in (dict(global_clipnorm=1.0), dict(clipvalue=1.0), dict(weight_decay=0.1), dict(amsgrad=True)):
    assert Adam(**kw).clip_local_gradients(None) is None


KW_SMALL = dict(blocks=6, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[48, 40],
                activation='leaky_relu', bits=8)


@pytest.fixture(scope='module')
def cpu_model(lib):
  from wavenets_amd import WaveNet
  model = WaveNet(**KW_SMALL, device=torch.device('cpu'), seed=3)
  model.build((1, 8, 1))
  return model


def test_exclude_from_weight_decay_matches_names_and_variables(cpu_model):
  from wavenets_amd import Adam
  names = cpu_model.variable_names
  assert any(n.endswith('bias') for n in names) and any(n.endswith('kernel') for n in names)
  assert Adam(weight_decay=0.1).decays(cpu_model) == [True] * len(names)
  assert Adam().decays(cpu_model) == [False] * len(names)
  opt = Adam(weight_decay=0.1)
  opt.exclude_from_weight_decay(var_names=['bias'])
  assert opt.decays(cpu_model) == [not re.search('bias', n) for n in names]
  opt = Adam(weight_decay=0.1)
  opt.exclude_from_weight_decay(var_names=['^' + re.escape(names[0]) + '$'])       # a pattern, not a substring list
  opt.exclude_from_weight_decay(var_list=[cpu_model.trainable_variables[2]])       # calls add up
  assert opt.decays(cpu_model) == [i not in (0, 2) for i in range(len(names))]
  opt = Adam(weight_decay=0.1)
  opt.exclude_from_weight_decay(var_list=[torch.zeros(3)])
  with pytest.raises(ValueError, match='not a trainable variable'):
    opt.decays(cpu_model)
  with pytest.raises(ValueError, match='var_names'):
    Adam(weight_decay=0.1).exclude_from_weight_decay(var_names=[3])
  with pytest.raises(ValueError, match='var_list'):
    Adam(weight_decay=0.1).exclude_from_weight_decay(var_list=['bias'])


def test_exclude_from_weight_decay_after_build_raises_and_build_makes_the_state(cpu_model):
  from wavenets_amd import Adam
  opt = Adam(weight_decay=0.1, amsgrad=True)
  opt.exclude_from_weight_decay(var_names=['bias'])
  opt.build(cpu_model)
  assert opt.vhat is not None and opt.vhat.shape == opt.v.shape and not opt.vhat.any()
  assert opt._decay_flags.dtype == torch.int32 and opt._decay_flags.tolist() == [int(d) for d in opt.decays(cpu_model)]
  with pytest.raises(ValueError, match='already been built'):
    opt.exclude_from_weight_decay(var_names=['kernel'])
  plain = Adam(weight_decay=0.1)
  plain.build(cpu_model)
  assert plain._decay_flags is None and plain.vhat is None          # no table: every tensor decays


def test_checkpoint_round_trip_of_vhat(cpu_model, tmp_path):
  """adam_vhat through io.save_weights / load_weights; a checkpoint without it starts an amsgrad optimizer from vhat = v,
  and an optimizer without amsgrad ignores a stored one."""
  from wavenets_amd import Adam, io
  gen = torch.Generator().manual_seed(5)
  opt = Adam(amsgrad=True)
  opt.build(cpu_model)
  opt.m.copy_(torch.randn(opt.m.shape, generator=gen))
  opt.v.copy_(torch.rand(opt.v.shape, generator=gen))
  opt.vhat.copy_(opt.v + torch.rand(opt.v.shape, generator=gen))
  opt.iterations = 2
  path = str(tmp_path / 'a.weights.npz')
  io.save_weights(cpu_model, path, opt)
  with np.load(path) as d:
    assert 'adam_vhat' in d and np.array_equal(d['adam_vhat'], opt.vhat.numpy())
  back = Adam(amsgrad=True)
  io.load_weights(cpu_model, path, back)
  assert back.iterations == 2
  for key in ('m', 'v', 'vhat'):
    assert torch.equal(getattr(back, key), getattr(opt, key)), key
  ignoring = Adam()
  io.load_weights(cpu_model, path, ignoring)
  assert ignoring.vhat is None and torch.equal(ignoring.v, opt.v)
  old = Adam()
  old.build(cpu_model)
  old.v.copy_(opt.v)
  old.iterations = 2
  path2 = str(tmp_path / 'b.weights.npz')
  io.save_weights(cpu_model, path2, old)
  with np.load(path2) as d:
    assert 'adam_vhat' not in d
  resumed = Adam(amsgrad=True)
  io.load_weights(cpu_model, path2, resumed)
  assert torch.equal(resumed.vhat, opt.v) and resumed.vhat.data_ptr() != resumed.v.data_ptr()


def test_driver_defaults_hold_the_keys():
  import importlib
  train = importlib.import_module('train')
  for key in ('global_clipnorm', 'clipvalue', 'weight_decay', 'exclude_from_weight_decay'):
    assert train.config[key] is None, key
  assert train.config['amsgrad'] is False


# ------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(lib):
  P = C.c_void_p
  assert _lib._SIGS['wn_adam_step_ext'] == (C.c_int, [P, P, P, P, P, P, P, C.c_int64, C.POINTER(_lib.WnAdamOptions), P, P, P])
  assert _lib._SIGS['wn_clip_gradients_ext'] == (C.c_int, [P, P, C.c_int32, C.c_float, P, P])
  assert 'wn_adam_step_ext' in _lib.EXPORTS and 'wn_clip_gradients_ext' in _lib.EXPORTS
  assert lib.wn_adam_step_ext.restype is C.c_int and lib.wn_clip_gradients_ext.restype is C.c_int
  header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wn_hip.h')
  with open(header) as f:
    text = f.read()
  assert 'int wn_adam_step_ext(wn_plan* p, float* params, const float* grads, float* m, float* v, float* vhat, float* ema,' in text
  assert 'int64_t step, const wn_adam_options* options, float* scratch, const float* skip_flag, void* stream);' in text
  assert 'int wn_clip_gradients_ext(wn_plan* p, float* grads, int32_t clip_mode, float clip, float* scratch, void* stream);' in text
  # the struct, field for field, and the mode bits
  body = re.search(r'typedef struct wn_adam_options \{(.*?)\} wn_adam_options;', text, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  fields = [f.strip() for decl in body.split(';') if decl.strip()
            for f in re.sub(r'^(const\s+)?\w+\s*\*?', '', decl.strip()).split(',')]
  assert fields == [n for n, _ in _lib.WnAdamOptions._fields_]
  assert C.sizeof(_lib.WnAdamOptions) == 48 and _lib.WnAdamOptions.decay_flags.offset == 40
  for name in ('WN_CLIP_NONE', 'WN_CLIP_NORM', 'WN_CLIP_GLOBAL_NORM', 'WN_CLIP_VALUE'):
    assert int(re.search(rf'#define {name} (\d+)', text).group(1)) == getattr(_lib, name)


def _plan(lib):
  s = spec.validate(kernel_size=2, channels=32, blocks=3, layers_per_block=1, activation=None, conditioning=None,
                    mapping_layers=None, mapping_activation=None, dropout=0, dilation_bound=4, num_mixtures=None,
                    sampling_function='categorical', bits=8, skip_channels=None, dilation_channels=None,
                    use_residual=True, use_skip=True, final_layers_channels=[32], l2_reg_factor=0)
  cfg = _lib.WnConfig()
  cfg.kernel_size, cfg.channels, cfg.blocks, cfg.layers_per_block = s.kernel_size, s.channels, s.blocks, s.layers_per_block
  cfg.activation = _lib.ACTIVATIONS[s.activation]
  cfg.dilation_bound = s.dilation_bound
  cfg.head = _lib.HEADS[s.sampling_function]
  cfg.bits = s.bits
  cfg.use_residual, cfg.use_skip = int(s.use_residual), int(s.use_skip)
  cfg.n_final = len(s.final_layers_channels)
  for i, c in enumerate(s.final_layers_channels):
    cfg.final_channels[i] = c
  plan = lib.wn_plan_create(C.byref(cfg))
  assert plan
  return C.c_void_p(plan)


@pytest.fixture()
def plan(lib):
  p = _plan(lib)
  yield p
  lib.wn_plan_destroy(p)


class _Host:
  """Host stand-ins for the device buffers of one call, filled with a value each so that a write would show."""
  NAMES = ('params', 'grads', 'm', 'v', 'vhat', 'ema', 'scratch')
  REQUIRED = ('params', 'grads', 'm', 'v', 'scratch')

  def __init__(self, lib, plan):
    n = lib.wn_plan_param_count(plan)
    self.fill = {'params': 1.0, 'grads': 3.0, 'm': 0.5, 'v': 0.25, 'vhat': 0.75, 'ema': 2.0, 'scratch': 0.0}
    self.buf = {k: (C.c_float * (lib.wn_plan_num_tensors(plan) if k == 'scratch' else n))() for k in self.NAMES}
    for k, b in self.buf.items():
      for i in range(len(b)):
        b[i] = self.fill[k]

  @staticmethod
  def options(**kw):
    o = _lib.WnAdamOptions()
    o.lr, o.beta1, o.beta2, o.eps = 5e-4, 0.9, 0.999, 1e-7
    o.clip_mode, o.clip, o.weight_decay, o.amsgrad = _lib.WN_CLIP_GLOBAL_NORM, 1.0, 0.1, 1
    o.ema_momentum, o.ema_overwrite = 0.99, 0
    for k, v in kw.items():
      setattr(o, k, v)
    return o

  def call(self, lib, plan, step=1, null=(), options=True, **kw):
    a = {k: (None if k in null else C.addressof(b)) for k, b in self.buf.items()}
    o = self.options(**kw)
    return lib.wn_adam_step_ext(plan, a['params'], a['grads'], a['m'], a['v'], a['vhat'], a['ema'], step,
                                C.byref(o) if options else None, a['scratch'], None, None)

  def untouched(self):
    return all(all(x == self.fill[k] for x in b) for k, b in self.buf.items())


def _invalid(lib, rc, word):
  assert rc == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert word in msg, msg


def test_step_ext_null_arguments_and_step_zero_are_invalid(lib, plan):
  h = _Host(lib, plan)
  a = {k: C.addressof(b) for k, b in h.buf.items()}
  o = h.options()
  _invalid(lib, lib.wn_adam_step_ext(None, a['params'], a['grads'], a['m'], a['v'], a['vhat'], a['ema'], 1, C.byref(o),
                                     a['scratch'], None, None), 'plan')
  for name in _Host.REQUIRED:
    _invalid(lib, h.call(lib, plan, null=(name,)), f'adam_step_ext: {name} is NULL')
  _invalid(lib, h.call(lib, plan, options=False), 'options')
  for step in (0, -1):
    _invalid(lib, h.call(lib, plan, step=step), 'step')
  assert h.untouched()


@pytest.mark.parametrize('mode', [3, 5, 6, 7, 8, -1, 16])
def test_step_ext_two_clip_modes_at_once_are_invalid(lib, plan, mode):
  h = _Host(lib, plan)
  _invalid(lib, h.call(lib, plan, clip_mode=mode), 'clip_mode')
  assert 'only one of clipnorm, clipvalue and global_clipnorm' in lib.wn_last_error_string().decode()
  assert h.untouched()


@pytest.mark.parametrize('mode', [_lib.WN_CLIP_NORM, _lib.WN_CLIP_GLOBAL_NORM, _lib.WN_CLIP_VALUE])
@pytest.mark.parametrize('clip', [0.0, -1.0, float('nan'), float('inf'), -float('inf')])
def test_step_ext_bad_clip_value_is_invalid(lib, plan, mode, clip):
  h = _Host(lib, plan)
  _invalid(lib, h.call(lib, plan, clip_mode=mode, clip=clip), 'clip must be finite and > 0')
  _invalid(lib, lib.wn_clip_gradients_ext(plan, C.addressof(h.buf['grads']), mode, clip, C.addressof(h.buf['scratch']), None),
           'clip must be finite and > 0')
  assert h.untouched()


@pytest.mark.parametrize('wd', [-0.1, -1e-30, float('nan'), float('inf'), -float('inf')])
def test_step_ext_bad_weight_decay_is_invalid(lib, plan, wd):
  h = _Host(lib, plan)
  _invalid(lib, h.call(lib, plan, weight_decay=wd), 'weight_decay')
  assert h.untouched()


def test_step_ext_amsgrad_without_vhat_and_bad_flag_are_invalid(lib, plan):
  h = _Host(lib, plan)
  _invalid(lib, h.call(lib, plan, null=('vhat',)), 'vhat')
  for bad in (2, -1, 256):
    _invalid(lib, h.call(lib, plan, amsgrad=bad), 'amsgrad')
  assert h.untouched()


def test_step_ext_ema_fields_out_of_range_are_invalid(lib, plan):
  h = _Host(lib, plan)
  for momentum in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
    _invalid(lib, h.call(lib, plan, ema_momentum=momentum), 'ema_momentum')
  for overwrite in (-1, 2, 3, 256):
    _invalid(lib, h.call(lib, plan, step=3, ema_overwrite=overwrite), 'ema_overwrite')
  _invalid(lib, h.call(lib, plan, null=('ema',)), 'without ema')                   # momentum 0.99 and no average
  _invalid(lib, h.call(lib, plan, null=('ema',), ema_momentum=0.0, ema_overwrite=1), 'without ema')
  assert h.untouched()


def test_clip_gradients_ext_null_arguments_and_modes_are_invalid(lib, plan):
  h = _Host(lib, plan)
  g, s = C.addressof(h.buf['grads']), C.addressof(h.buf['scratch'])
  _invalid(lib, lib.wn_clip_gradients_ext(None, g, _lib.WN_CLIP_VALUE, 1.0, s, None), 'plan')
  _invalid(lib, lib.wn_clip_gradients_ext(plan, None, _lib.WN_CLIP_VALUE, 1.0, s, None), 'grads')
  _invalid(lib, lib.wn_clip_gradients_ext(plan, g, _lib.WN_CLIP_VALUE, 1.0, None, None), 'scratch')
  for mode in (0, 3, 5, 6, 7, 8, -1):
    _invalid(lib, lib.wn_clip_gradients_ext(plan, g, mode, 1.0, s, None), 'clip_mode')
  assert h.untouched()
