"""CPU-only checks of wn_vjp (include/wn_hip.h: the backward pass from a caller's gradient) at the C-ABI boundary, after
the pattern of test_sampling_cabi_cpu.py: every argument is validated before anything touches the device, so the calls
here pass null pointers or addresses that are never dereferenced and must come back with WN_E_INVALID and a message."""
import ctypes as C
import inspect

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan as _plan_of
from test_sampling_cabi_cpu import lib  # noqa: F401  (module fixture)

FAKE = C.c_void_p(4096)            # non-null, never dereferenced: the argument checks come first


def _vjp(lib, plan, params=FAKE, x=FAKE, cond=None, B=2, T=16, g_out=FAKE, g_kind=1, grads=FAKE, g_x=None, g_cond=None,
         ws=FAKE, ws_floats=0):
  return lib.wn_vjp(plan, params, x, cond, B, T, g_out, g_kind, grads, g_x, g_cond, ws, ws_floats, None)


@pytest.fixture
def plan(lib):
  p = C.c_void_p(_plan_of(lib, _cfg(blocks=3, channels=32, skip_channels=32, dilation_bound=4, final_layers_channels=[32])))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_destroy(p)


@pytest.fixture
def cond_plan(lib):
  p = C.c_void_p(_plan_of(lib, _cfg(blocks=3, channels=32, dilation_bound=4, final_layers_channels=[], conditioning='global',
                                    mapping_layers=[8]), 5))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_destroy(p)


def _invalid(lib, rc, *words):
  assert rc == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert msg.startswith('vjp:') and len(msg) > len('vjp: ')
  for w in words:
    assert w in msg, (w, msg)


def test_the_binding_declares_the_prototype(lib):
  res, args = _lib._SIGS['wn_vjp']
  assert 'wn_vjp' in _lib.EXPORTS and res is C.c_int
  P = C.c_void_p
  assert args == [P, P, P, P, C.c_int32, C.c_int32, P, C.c_int32, P, P, P, P, C.c_int64, P]
  assert lib.wn_vjp.argtypes == args


@pytest.mark.parametrize('missing', ['plan', 'params', 'x', 'g_out', 'grads', 'ws'])
def test_a_null_required_pointer_is_invalid(lib, plan, missing):
  kw = {missing: None} if missing != 'plan' else {}
  _invalid(lib, _vjp(lib, None if missing == 'plan' else plan, **kw), 'null')


def test_a_conditioned_plan_needs_the_condition(lib, cond_plan):
  _invalid(lib, _vjp(lib, cond_plan, cond=None), 'cond')


@pytest.mark.parametrize('B,T', [(0, 16), (-1, 16), (2, 0), (2, -3)])
def test_batch_and_length_below_one_are_invalid(lib, plan, B, T):
  _invalid(lib, _vjp(lib, plan, B=B, T=T), 'B', 'T')


@pytest.mark.parametrize('g_kind', [-1, 2, 7])
def test_a_gradient_kind_outside_0_1_is_invalid(lib, plan, g_kind):
  _invalid(lib, _vjp(lib, plan, g_kind=g_kind), 'g_kind', str(g_kind))


def test_a_condition_gradient_without_conditioning_is_invalid(lib, plan):
  _invalid(lib, _vjp(lib, plan, g_cond=FAKE), 'g_cond')


@pytest.mark.parametrize('g_kind', [0, 1])
def test_a_workspace_that_is_too_small_is_invalid(lib, plan, cond_plan, g_kind):
  need = lib.wn_plan_workspace_floats(plan, 2, 16, 1)
  assert need > 0
  for have in (0, need - 1):
    _invalid(lib, _vjp(lib, plan, g_kind=g_kind, g_x=FAKE, ws_floats=have), 'workspace', str(need))
  need = lib.wn_plan_workspace_floats(cond_plan, 2, 16, 1)
  _invalid(lib, _vjp(lib, cond_plan, cond=FAKE, g_kind=g_kind, g_cond=FAKE, ws_floats=need - 1), 'workspace', str(need))


def test_python_surface_refuses_a_wrong_output_before_any_work():
  """differentiable(output=...) is checked first: on an object that has no plan, no parameters and no device."""
  from wavenets_amd import WaveNet
  m = WaveNet.__new__(WaveNet)
  for bad in ('prob', 'LOGITS', None, 0):
    with pytest.raises(ValueError, match='output'):
      m.differentiable(None, output=bad)
  sig = inspect.signature(WaveNet.differentiable)
  assert sig.parameters['training'].default is False and sig.parameters['output'].default == 'probs'
