"""CPU-only checks of wn_score and wn_debug_eval_region at the C-ABI boundary (include/wn_hip.h), after the pattern of
test_sample_weight_cabi_cpu.py: every argument is validated before anything touches the device, so the calls here pass
null pointers or addresses that are never dereferenced and must come back with WN_E_INVALID and a message."""
import ctypes as C
import inspect

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan as _plan_of
from test_sampling_cabi_cpu import lib  # noqa: F401  (module fixture)
from test_sample_weight_cabi_cpu import _Shape

FAKE = C.c_void_p(4096)            # non-null, never dereferenced: the argument checks come first
P = C.c_void_p
B, T = 2, 16


@pytest.fixture
def plan(lib):
  p = C.c_void_p(_plan_of(lib, _cfg(blocks=3, channels=32, skip_channels=32, dilation_bound=4, final_layers_channels=[32])))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_arm_row_weights(p, None, 0)
  lib.wn_plan_destroy(p)


@pytest.fixture
def cond_plan(lib):
  s = _cfg(blocks=2, channels=32, skip_channels=32, dilation_bound=2, final_layers_channels=[32], conditioning='global',
           mapping_layers=[8])
  p = C.c_void_p(_plan_of(lib, s, cond_inputs=4))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_destroy(p)


def test_the_binding_declares_both_prototypes(lib):
  for name, want in (('wn_score', [P, P, P, P, C.c_int32, C.c_int32, P, P, P, P, P, C.c_int64, P]),
                     ('wn_debug_eval_region', [P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])):
    res, args = _lib._SIGS[name]
    assert name in _lib.EXPORTS and res is C.c_int and args == want
    assert getattr(lib, name).argtypes == want


def _score(lib, the_plan, ws_floats, b=B, t=T, **kw):
  a = dict(plan=the_plan, params=FAKE, x_full=FAKE, cond=None, nll_out=FAKE, weight_out=None, rows_out=None, flag_out=FAKE,
           workspace=FAKE)
  a.update(kw)
  return lib.wn_score(a['plan'], a['params'], a['x_full'], a['cond'], b, t, a['nll_out'], a['weight_out'], a['rows_out'],
                      a['flag_out'], a['workspace'], ws_floats, None)


def _need(lib, plan, b=B, t=T):
  n = lib.wn_plan_workspace_floats(plan, b, t, 0)
  assert n > 0
  return n


@pytest.mark.parametrize('missing', ['plan', 'params', 'x_full', 'nll_out', 'flag_out', 'workspace'])
def test_a_null_pointer_is_invalid_and_named(lib, plan, missing):
  assert _score(lib, plan, _need(lib, plan), **{missing: None}) == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert msg.startswith('score:') and 'null' in msg and missing in msg, msg


def test_a_conditioned_plan_needs_its_condition(lib, cond_plan):
  assert _score(lib, cond_plan, _need(lib, cond_plan)) == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert msg.startswith('score:') and 'cond' in msg, msg
  # with one it gets past that check: a workspace that is too small stops it at the next
  assert _score(lib, cond_plan, 0, cond=FAKE) == _lib.WN_E_INVALID
  assert 'workspace' in lib.wn_last_error_string().decode()


@pytest.mark.parametrize('b,t', [(0, T), (-1, T), (B, 0), (B, -3)])
def test_an_empty_batch_is_invalid(lib, plan, b, t):
  assert _score(lib, plan, 1 << 40, b=b, t=t) == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert msg.startswith('score:') and str(b) in msg and str(t) in msg, msg


def test_a_small_workspace_is_invalid_and_both_sizes_are_named(lib, plan):
  need = _need(lib, plan)
  for have in (0, need - 1):
    assert _score(lib, plan, have) == _lib.WN_E_INVALID
    msg = lib.wn_last_error_string().decode()
    assert msg.startswith('score:') and 'workspace' in msg and str(have) in msg and str(need) in msg, msg
  # the inference size is what it asks for, not the training size
  assert need < lib.wn_plan_workspace_floats(plan, B, T, 1)


def test_armed_for_other_rows_than_the_call_has_is_invalid_before_the_device(lib, plan):
  need = _need(lib, plan)
  assert lib.wn_plan_arm_row_weights(plan, FAKE, 10) == _lib.WN_OK
  assert _score(lib, plan, need) == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert msg.startswith('score:') and '10' in msg and str(B * T) in msg and 'weights' in msg, msg
  # armed for the right rows, or disarmed, the call gets past that check
  for rows in (B * T, None):
    assert lib.wn_plan_arm_row_weights(plan, FAKE if rows else None, rows or 0) == _lib.WN_OK
    assert _score(lib, plan, 0) == _lib.WN_E_INVALID
    assert 'workspace' in lib.wn_last_error_string().decode()


def test_eval_region_describes_the_inference_layout(lib, plan):
  need = _need(lib, plan)
  off, ln = C.c_int64(), C.c_int64()
  spans = {}
  for what, want_len in ((5, B * T * 256), (12, B * T)):
    assert lib.wn_debug_eval_region(plan, B, T, what, C.byref(off), C.byref(ln)) == _lib.WN_OK
    assert ln.value == want_len and 0 <= off.value and off.value + ln.value <= need
    spans[what] = (off.value, off.value + ln.value)
  assert spans[5][1] <= spans[12][0] or spans[12][1] <= spans[5][0]
  # it is not the training layout under another name
  toff, tln = C.c_int64(), C.c_int64()
  assert lib.wn_debug_ws_region(plan, B, T, 5, 0, C.byref(toff), C.byref(tln)) == _lib.WN_OK
  assert tln.value == B * T * 256 and toff.value != spans[5][0]
  for what in (0, 4, 6, 10, 13, -1):
    assert lib.wn_debug_eval_region(plan, B, T, what, C.byref(off), C.byref(ln)) == _lib.WN_E_INVALID
    assert 'eval_region' in lib.wn_last_error_string().decode() and off.value == -1 and ln.value == 0
  assert lib.wn_debug_eval_region(None, B, T, 5, C.byref(off), C.byref(ln)) == _lib.WN_E_INVALID
  assert lib.wn_debug_eval_region(plan, 0, T, 5, C.byref(off), C.byref(ln)) == _lib.WN_E_INVALID
  assert lib.wn_debug_eval_region(plan, B, T, 5, None, C.byref(ln)) == _lib.WN_E_INVALID


def test_python_surface_refuses_a_wrong_weight_shape_before_any_work():
  """sample_weight is checked first: on an object that has no plan, no parameters and no device."""
  from wavenets_amd import WaveNet
  m = WaveNet.__new__(WaveNet)
  b, t = 3, 20
  x = _Shape(b, t + 1, 1)
  for data in (x, (x, _Shape(b, 4))):
    for bad in (_Shape(b, t + 1), _Shape(b + 1), _Shape(b, t, 1, 1)):
      with pytest.raises(ValueError, match=rf'sample_weight must have shape \({b}, {t}\)'):
        m.score(data, sample_weight=bad)
  sig = inspect.signature(WaveNet.score).parameters
  assert sig['sample_weight'].default is None and sig['per_sample'].default is False
