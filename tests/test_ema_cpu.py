"""CPU-only checks of Adam(use_ema=...) -- the exponential moving average of the weights, written by the Adam launch -- at
the C-ABI boundary and on the Python surface: wn_adam_step_ema validates its arguments before anything touches the
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


class _Host:
  """Host stand-ins for the device buffers of one call, filled with a value each so that a write would show."""
  NAMES = ('params', 'grads', 'm', 'v', 'ema', 'scratch')

  def __init__(self, lib, plan):
    n = lib.wn_plan_param_count(plan)
    self.fill = {'params': 1.0, 'grads': 3.0, 'm': 0.5, 'v': 0.25, 'ema': 2.0, 'scratch': 0.0}
    self.buf = {k: (C.c_float * (lib.wn_plan_num_tensors(plan) if k == 'scratch' else n))() for k in self.NAMES}
    for k, b in self.buf.items():
      for i in range(len(b)):
        b[i] = self.fill[k]

  def call(self, lib, plan, step=1, momentum=0.99, overwrite=0, null=None):
    a = {k: (None if k == null else C.addressof(b)) for k, b in self.buf.items()}
    return lib.wn_adam_step_ema(plan, a['params'], a['grads'], a['m'], a['v'], a['ema'], step, 5e-4, 0.9, 0.999, 1e-7, 1.0,
                                momentum, overwrite, a['scratch'], None, None)

  def untouched(self):
    return all(all(x == self.fill[k] for x in b) for k, b in self.buf.items())


def test_adam_step_ema_is_exported_and_declared(lib):
  assert 'wn_adam_step_ema' in _lib._SIGS and 'wn_adam_step_ema' in _lib.EXPORTS
  res, args = _lib._SIGS['wn_adam_step_ema']
  P = C.c_void_p
  assert res is C.c_int
  assert args == [P, P, P, P, P, P, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                  P, P, P]
  assert lib.wn_adam_step_ema.restype is C.c_int
  header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wn_hip.h')
  with open(header) as f:
    text = f.read()
  assert 'int wn_adam_step_ema(wn_plan* p, float* params, const float* grads, float* m, float* v, float* ema, int64_t step,' in text


def test_adam_step_ema_null_arguments_and_step_zero_are_invalid(lib):
  plan = _plan(lib)
  try:
    h = _Host(lib, plan)
    a = {k: C.addressof(b) for k, b in h.buf.items()}
    assert lib.wn_adam_step_ema(None, a['params'], a['grads'], a['m'], a['v'], a['ema'], 1, 5e-4, 0.9, 0.999, 1e-7, 1.0,
                                0.99, 0, a['scratch'], None, None) == _lib.WN_E_INVALID
    for name in _Host.NAMES:
      assert h.call(lib, plan, null=name) == _lib.WN_E_INVALID, name
      assert 'adam_step_ema' in lib.wn_last_error_string().decode()
    for step in (0, -1):
      assert h.call(lib, plan, step=step) == _lib.WN_E_INVALID
    assert h.untouched()
  finally:
    lib.wn_plan_destroy(plan)


@pytest.mark.parametrize('momentum', [-0.1, 1.5, float('nan'), float('inf'), -float('inf')])
def test_adam_step_ema_bad_momentum_is_invalid_before_the_device_is_touched(lib, momentum):
  plan = _plan(lib)
  try:
    h = _Host(lib, plan)
    assert h.call(lib, plan, momentum=momentum) == _lib.WN_E_INVALID
    assert 'ema_momentum' in lib.wn_last_error_string().decode()
    assert h.untouched()
  finally:
    lib.wn_plan_destroy(plan)


@pytest.mark.parametrize('overwrite', [-1, 2, 3, 256])
def test_adam_step_ema_bad_overwrite_is_invalid_before_the_device_is_touched(lib, overwrite):
  plan = _plan(lib)
  try:
    h = _Host(lib, plan)
    assert h.call(lib, plan, step=3, overwrite=overwrite) == _lib.WN_E_INVALID
    assert 'ema_overwrite' in lib.wn_last_error_string().decode()
    assert h.untouched()
  finally:
    lib.wn_plan_destroy(plan)


def test_adam_defaults_and_validation():
  from wavenets_amd import Adam
  opt = Adam(clipnorm=1.0)
  assert opt.use_ema is False and opt.ema_momentum == 0.99 and opt.ema_overwrite_frequency is None and opt.ema is None
  opt = Adam(use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=3)
  assert opt.use_ema is True and opt.ema_momentum == 0.9 and opt.ema_overwrite_frequency == 3
  assert Adam(use_ema=True, ema_momentum=0).ema_momentum == 0 and Adam(use_ema=True, ema_momentum=1.0).ema_momentum == 1.0
  for bad in (1, 0, 'true', None, 1.0):
    with pytest.raises(ValueError, match='use_ema'):
      Adam(use_ema=bad)
  for bad in (-0.1, 1.5, float('nan'), float('inf'), -float('inf'), '0.9', None, True):
    with pytest.raises(ValueError, match='ema_momentum'):
      Adam(use_ema=True, ema_momentum=bad)
  for bad in (0, -1, True, 2.5):
    with pytest.raises(ValueError, match='ema_overwrite_frequency'):
      Adam(use_ema=True, ema_overwrite_frequency=bad)
  # as in Keras: neither is looked at while use_ema is false
  opt = Adam(ema_momentum=1.5, ema_overwrite_frequency=0)
  assert opt.use_ema is False


def test_no_ops_without_the_flag_and_without_a_model():
  from wavenets_amd import Adam
  assert Adam(clipnorm=1.0).finalize_variable_values(None) is None
  assert Adam(ema_momentum=0.5).finalize_variable_values(None) is None
  assert Adam(use_ema=True).clip_local_gradients(None) is None
  assert Adam(clipnorm=1.0, use_ema=True).clip_local_gradients(None) is None


def test_driver_defaults_hold_the_keys():
  import importlib
  train = importlib.import_module('train')
  assert train.config['use_ema'] is False and train.config['ema_momentum'] == 0.99
  assert train.config['ema_overwrite_frequency'] is None and train.config['validation_utterances'] == 0


def test_averaged_file_name_is_not_a_resume_candidate(tmp_path):
  from wavenets_amd import io
  (tmp_path / 'averaged.weights.h5').write_bytes(b'x')
  assert io.find_resume(str(tmp_path)) is None
