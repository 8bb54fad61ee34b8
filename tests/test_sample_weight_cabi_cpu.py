"""CPU-only checks of sample_weight at the C-ABI boundary (include/wn_hip.h: wn_plan_arm_row_weights,
wn_weighted_squared_error) and of the Python surface's shape check, after the pattern of test_vjp_cabi_cpu.py: every
argument is validated before anything touches the device, so the calls here pass null pointers or addresses that are
never dereferenced and must come back with WN_E_INVALID and a message."""
import ctypes as C
import inspect

import numpy as np
import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan as _plan_of
from test_sampling_cabi_cpu import lib  # noqa: F401  (module fixture)

FAKE = C.c_void_p(4096)            # non-null, never dereferenced: the argument checks come first
P = C.c_void_p


@pytest.fixture
def plan(lib):
  p = C.c_void_p(_plan_of(lib, _cfg(blocks=3, channels=32, skip_channels=32, dilation_bound=4, final_layers_channels=[32])))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_arm_row_weights(p, None, 0)
  lib.wn_plan_destroy(p)


def test_the_binding_declares_both_prototypes(lib):
  for name, want in (('wn_plan_arm_row_weights', [P, P, C.c_int64]),
                     ('wn_weighted_squared_error', [P, P, P, C.c_int64, C.c_float, P, P, P])):
    res, args = _lib._SIGS[name]
    assert name in _lib.EXPORTS and res is C.c_int and args == want
    assert getattr(lib, name).argtypes == want


def test_arming_needs_a_plan(lib):
  assert lib.wn_plan_arm_row_weights(None, FAKE, 10) == _lib.WN_E_INVALID
  assert 'null plan' in lib.wn_last_error_string().decode()
  assert lib.wn_plan_arm_row_weights(None, None, 0) == _lib.WN_E_INVALID


def test_arm_and_disarm_on_a_plan_made_without_a_device(lib, plan):
  assert lib.wn_plan_arm_row_weights(plan, FAKE, 32) == _lib.WN_OK
  assert lib.wn_plan_arm_row_weights(plan, None, 0) == _lib.WN_OK
  assert lib.wn_plan_arm_row_weights(plan, None, 77) == _lib.WN_OK          # the count of a disarm is not looked at
  for rows in (0, -5):
    assert lib.wn_plan_arm_row_weights(plan, FAKE, rows) == _lib.WN_E_INVALID
    assert str(rows) in lib.wn_last_error_string().decode()


def _train(lib, plan, B, T, ws_floats):
  return lib.wn_train_fwd_bwd(plan, FAKE, FAKE, None, B, T, B, 1, FAKE, FAKE, None, FAKE, ws_floats, None)


def _eval(lib, plan, B, T, ws_floats):
  return lib.wn_eval_loss(plan, FAKE, FAKE, None, B, T, B, FAKE, None, FAKE, ws_floats, None)


def test_armed_for_other_rows_than_the_call_has_is_invalid_before_the_device(lib, plan):
  B, T = 2, 16
  big = max(lib.wn_plan_workspace_floats(plan, B, T, 1), lib.wn_plan_workspace_floats(plan, B, T, 0))
  assert big > 0
  assert lib.wn_plan_arm_row_weights(plan, FAKE, 10) == _lib.WN_OK
  for who, call in (('train_fwd_bwd', _train), ('eval_loss', _eval)):       # it stays armed from one call to the next
    assert call(lib, plan, B, T, big) == _lib.WN_E_INVALID
    msg = lib.wn_last_error_string().decode()
    assert msg.startswith(who + ':') and '10' in msg and '32' in msg and 'weights' in msg, msg
  # disarmed, the same calls get past that check: with a workspace that is too small they stop at the next one
  assert lib.wn_plan_arm_row_weights(plan, None, 0) == _lib.WN_OK
  for call in (_train, _eval):
    assert call(lib, plan, B, T, 0) == _lib.WN_E_INVALID
    assert 'workspace' in lib.wn_last_error_string().decode()


@pytest.mark.parametrize('missing', ['a', 'b', 'w', 'out', 'scratch', 'n'])
def test_weighted_squared_error_checks_its_arguments(lib, missing):
  kw = dict(a=FAKE, b=FAKE, w=FAKE, n=8, out=FAKE, scratch=FAKE)
  kw[missing] = 0 if missing == 'n' else None
  rc = lib.wn_weighted_squared_error(kw['a'], kw['b'], kw['w'], kw['n'], 1.0, kw['out'], kw['scratch'], None)
  assert rc == _lib.WN_E_INVALID
  assert lib.wn_last_error_string().decode().startswith('weighted_squared_error:')


class _Shape:
  """Stands in for a tensor: the check reads shapes only."""

  def __init__(self, *shape):
    self.shape = shape


@pytest.mark.parametrize('method', ['train_step', 'test_step', 'loss_and_grads'])
def test_python_surface_refuses_a_wrong_weight_shape_before_any_work(method):
  """sample_weight is checked first: on an object that has no plan, no parameters, no optimizer and no device."""
  from wavenets_amd import WaveNet
  m = WaveNet.__new__(WaveNet)
  B, T = 3, 20
  x = _Shape(B, T + 1, 1)
  for data in (x, (x, _Shape(B, 4))):
    for bad in (_Shape(B, T + 1), _Shape(B + 1), _Shape(B, T, 1, 1), np.zeros((B, T + 1), np.float32), np.zeros((B + 1,))):
      with pytest.raises(ValueError, match=rf'sample_weight must have shape \({B}, {T}\)'):
        getattr(m, method)(data, sample_weight=bad)
  assert inspect.signature(getattr(WaveNet, method)).parameters['sample_weight'].default is None
  for ok in (_Shape(B, T), _Shape(B, T, 1), _Shape(B), np.ones((B, T), np.float32)):
    assert WaveNet._check_sample_weight(x, ok) is ok
  assert WaveNet._check_sample_weight(x, None) is None


def test_the_metric_takes_the_keyword():
  from wavenets_amd import MeanSquaredError
  for name in ('update_state', 'update_state_device'):
    assert inspect.signature(getattr(MeanSquaredError, name)).parameters['sample_weight'].default is None
