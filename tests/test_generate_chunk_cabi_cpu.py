"""CPU-only checks of wn_generate_chunk and wn_generate_state_range at the C-ABI boundary (include/wn_hip.h): the
arguments that say where in a sequence a call stands are validated before the device is touched, so every call here
passes null device pointers and must come back with WN_E_INVALID and a message naming the argument; the state range is
host arithmetic on the workspace layout."""
import ctypes as C
import os

import pytest

from wavenets_amd import _lib, spec


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


def _plan(lib, **kw):
  d = dict(kernel_size=2, channels=32, blocks=3, layers_per_block=1, activation=None, conditioning=None,
           mapping_layers=None, mapping_activation=None, dropout=0, dilation_bound=4, num_mixtures=None,
           sampling_function='categorical', bits=8, skip_channels=None, dilation_channels=None,
           use_residual=True, use_skip=True, final_layers_channels=[32], l2_reg_factor=0)
  d.update(kw)
  s = spec.validate(**d)
  cfg = _lib.WnConfig()
  cfg.kernel_size, cfg.channels, cfg.blocks, cfg.layers_per_block = s.kernel_size, s.channels, s.blocks, s.layers_per_block
  cfg.activation = _lib.ACTIVATIONS[s.activation]
  cfg.dilation_bound = s.dilation_bound
  cfg.num_mixtures = s.num_mixtures or 0
  cfg.head = _lib.HEADS[s.sampling_function]
  cfg.bits = s.bits
  cfg.skip_channels = s.skip_channels or 0
  cfg.dilation_channels = s.dilation_channels or 0
  cfg.use_residual, cfg.use_skip = int(s.use_residual), int(s.use_skip)
  cfg.n_final = len(s.final_layers_channels)
  for i, c in enumerate(s.final_layers_channels):
    cfg.final_channels[i] = c
  plan = lib.wn_plan_create(C.byref(cfg))
  assert plan
  return plan


# a host address that stands for "a window was given": the checks under test return before any pointer is used
_WINDOW = (C.c_float * 4)()


def _chunk(lib, plan, window, first, length, sampling=None, queued=1):
  s = sampling if sampling is not None else _lib.WnSampling(1.0, 0, 1, 1.0)
  return lib.wn_generate_chunk(plan, None, C.cast(_WINDOW, C.c_void_p) if window else None, None, 1, first, length, 0, queued,
                               C.byref(s), None, None, 0, None)


def _err(lib):
  return lib.wn_last_error_string().decode()


@pytest.mark.parametrize('queued', [0, 1])
def test_negative_first_is_invalid(lib, queued):
  plan = _plan(lib)
  try:
    for window in (False, True):
      assert _chunk(lib, plan, window, -1, 4, queued=queued) == _lib.WN_E_INVALID
      assert 'first must be >= 0' in _err(lib)
    assert _chunk(lib, None, False, -5, 4, queued=queued) == _lib.WN_E_INVALID      # (not even the plan is needed)
    assert 'first must be >= 0' in _err(lib) and '-5' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


def test_window_with_first_not_zero_is_invalid(lib):
  plan = _plan(lib)
  try:
    for first in (1, 7, 2 ** 40):
      assert _chunk(lib, plan, True, first, 4) == _lib.WN_E_INVALID
      assert 'window' in _err(lib) and 'requires first == 0' in _err(lib) and str(first) in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


def test_null_window_with_first_zero_is_invalid(lib):
  plan = _plan(lib)
  try:
    assert _chunk(lib, plan, False, 0, 4) == _lib.WN_E_INVALID
    assert 'window is null with first == 0' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


def test_first_plus_length_beyond_the_32_bit_step_range_is_invalid(lib):
  plan = _plan(lib)
  try:
    for first, length in ((2 ** 31 - 4, 4), (2 ** 31 - 1, 1), (2 ** 31, 1), (2 ** 40, 3), (1, 2 ** 31 - 1)):
      assert _chunk(lib, plan, False, first, length) == _lib.WN_E_INVALID
      assert 'first + length' in _err(lib) and str(first) in _err(lib)
    # the last step index that fits: the call gets past these checks, to the null pointers
    assert _chunk(lib, plan, False, 2 ** 31 - 5, 4) == _lib.WN_E_INVALID
    assert 'bad arguments' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


def test_checks_come_in_order_and_good_values_reach_the_pointer_check(lib):
  """The sampling controls are checked first (as for wn_generate_sampled), the place in the sequence next, the pointers
  last; wn_generate_sampled keeps its own answer to a null window."""
  plan = _plan(lib)
  try:
    assert _chunk(lib, plan, False, -1, 4, sampling=_lib.WnSampling(0.0, 0, 1, 1.0)) == _lib.WN_E_INVALID
    assert 'temperature' in _err(lib)
    for window, first in ((True, 0), (False, 1), (False, 12345)):
      assert _chunk(lib, plan, window, first, 4) == _lib.WN_E_INVALID
      assert 'bad arguments' in _err(lib)
    s = _lib.WnSampling(1.0, 0, 1, 1.0)
    assert lib.wn_generate_sampled(plan, None, None, None, 1, 4, 0, 1, C.byref(s), None, None, 0, None) == _lib.WN_E_INVALID
    assert 'bad arguments' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


STATE_PLANS = {
    'lpb3': dict(layers_per_block=3, skip_channels=32, dilation_bound=8),
    'k3': dict(kernel_size=3, blocks=4, skip_channels=32, dilation_bound=9, final_layers_channels=[]),
    'r128': dict(channels=128, blocks=5, skip_channels=256, dilation_bound=16, final_layers_channels=[128, 64]),
}


@pytest.mark.parametrize('B', [1, 33])
@pytest.mark.parametrize('name', list(STATE_PLANS))
def test_state_range_lies_inside_the_workspace(lib, name, B):
  plan = _plan(lib, **STATE_PLANS[name])
  try:
    rf = lib.wn_plan_receptive_field(plan)
    for queued in (1, 0):
      total = lib.wn_generate_workspace_floats(plan, B, queued)
      slot = lib.wn_generate_guard_slot(plan, B, queued)
      off, n = C.c_int64(-1), C.c_int64(-1)
      assert lib.wn_generate_state_range(plan, B, queued, C.byref(off), C.byref(n)) == _lib.WN_OK
      assert 0 <= off.value and n.value > 0 and off.value + n.value <= total
      if queued:
        # behind the guard and the relay's give-up word, up to the end of the layout; at least the raw-sample slots
        assert off.value >= slot + 2 and off.value + n.value == total
        assert n.value >= STATE_PLANS[name].get('kernel_size', 2) * B
      else:
        # the two window buffers, in front of the guard
        assert n.value >= 2 * B * rf and off.value + n.value <= slot
  finally:
    lib.wn_plan_destroy(plan)


def test_state_range_bad_arguments(lib):
  plan = _plan(lib)
  try:
    off, n = C.c_int64(), C.c_int64()
    assert lib.wn_generate_state_range(None, 1, 1, C.byref(off), C.byref(n)) == _lib.WN_E_INVALID
    assert 'generate_state_range' in _err(lib)
    for B in (0, -3):
      assert lib.wn_generate_state_range(plan, B, 1, C.byref(off), C.byref(n)) == _lib.WN_E_INVALID
      assert lib.wn_generate_state_range(plan, B, 0, C.byref(off), C.byref(n)) == _lib.WN_E_INVALID
    assert lib.wn_generate_state_range(plan, 1, 1, None, C.byref(n)) == _lib.WN_E_INVALID
    assert lib.wn_generate_state_range(plan, 1, 1, C.byref(off), None) == _lib.WN_E_INVALID
  finally:
    lib.wn_plan_destroy(plan)


def test_python_surface_checks_n_without_a_device():
  """GenerationSession.generate checks n before anything else."""
  from wavenets_amd import GenerationSession
  s = GenerationSession.__new__(GenerationSession)
  s.position = 0
  for n in (0, -1, 2.5, True, None):
    with pytest.raises(ValueError, match='n must be'):
      s.generate(n)
  assert s.position == 0
