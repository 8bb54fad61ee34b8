"""CPU-only checks of Adam(clip_before_reduce=...) -- the per-replica clipnorm ahead of the data-parallel all-reduce -- at
the C-ABI boundary and on the Python surface: wn_clip_gradients validates its arguments before anything touches the
device, so every call here hands it host memory (never dereferenced) and must come back with WN_E_INVALID."""
import ctypes as C
import os

import pytest

from wavenets_amd import _lib, spec


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


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
  return plan


def test_clip_gradients_is_exported_and_declared(lib):
  assert 'wn_clip_gradients' in _lib._SIGS and 'wn_clip_gradients' in _lib.EXPORTS
  res, args = _lib._SIGS['wn_clip_gradients']
  assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
  assert lib.wn_clip_gradients.restype is C.c_int
  header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wn_hip.h')
  with open(header) as f:
    assert 'int wn_clip_gradients(wn_plan* p, float* grads, float clipnorm, float* scratch, void* stream);' in f.read()


def test_clip_gradients_null_arguments_are_invalid(lib):
  plan = _plan(lib)
  try:
    n = lib.wn_plan_param_count(plan)
    grads = (C.c_float * n)()
    scratch = (C.c_float * lib.wn_plan_num_tensors(plan))()
    g, s = C.addressof(grads), C.addressof(scratch)
    assert lib.wn_clip_gradients(None, g, 1.0, s, None) == _lib.WN_E_INVALID
    assert lib.wn_clip_gradients(plan, None, 1.0, s, None) == _lib.WN_E_INVALID
    assert lib.wn_clip_gradients(plan, g, 1.0, None, None) == _lib.WN_E_INVALID
    assert 'clip_gradients' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


@pytest.mark.parametrize('clipnorm', [0.0, -0.0, -1.0, float('nan'), float('inf'), -float('inf')])
def test_clip_gradients_bad_clipnorm_is_invalid_before_the_device_is_touched(lib, clipnorm):
  plan = _plan(lib)
  try:
    n = lib.wn_plan_param_count(plan)
    grads = (C.c_float * n)(*([3.0] * n))
    scratch = (C.c_float * lib.wn_plan_num_tensors(plan))()
    assert lib.wn_clip_gradients(plan, C.addressof(grads), clipnorm, C.addressof(scratch), None) == _lib.WN_E_INVALID
    assert 'clipnorm' in lib.wn_last_error_string().decode()
    assert all(v == 3.0 for v in grads) and all(v == 0.0 for v in scratch)
  finally:
    lib.wn_plan_destroy(plan)


def test_adam_takes_the_flag_and_rejects_non_bools():
  from wavenets_amd import Adam
  assert Adam(clipnorm=1.0).clip_before_reduce is False                     # default: the reduced gradient is clipped
  opt = Adam(learning_rate=5e-4, clipnorm=1.0, clip_before_reduce=True)
  assert opt.clip_before_reduce is True and opt.clipnorm == 1.0
  assert Adam(clip_before_reduce=True).clipnorm is None                     # accepted; clip_local_gradients is then a no-op
  for bad in (1, 0, 'true', None, 1.0):
    with pytest.raises(ValueError, match='clip_before_reduce'):
      Adam(clipnorm=1.0, clip_before_reduce=bad)


def test_flag_without_clipnorm_launches_nothing():
  """No clipnorm: clip_local_gradients returns before it looks at the model (no plan, no device needed)."""
  from wavenets_amd import Adam
  assert Adam(clip_before_reduce=True).clip_local_gradients(None) is None
  assert Adam(clipnorm=1.0).clip_local_gradients(None) is None               # flag off: the clip stays in the Adam launch


def test_driver_defaults_hold_the_key():
  import importlib
  train = importlib.import_module('train')
  assert 'clip_before_reduce' in train.config and train.config['clip_before_reduce'] is False
