"""CPU-only checks of the sampling controls at the C-ABI boundary (include/wn_hip.h, struct wn_sampling): temperature,
top_k and seed are validated before any other argument is looked at and before anything touches the device, so every
call here passes null device pointers and must come back with WN_E_INVALID and a message naming the argument."""
import ctypes as C
import os

import pytest

from wavenets_amd import _lib, spec

HEAD_CAT, HEAD_LOGISTIC, HEAD_GAUSSIAN = (_lib.HEADS[k] for k in ('categorical', 'logistic', 'gaussian'))


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


def _generate(lib, plan, sampling):
  return lib.wn_generate_sampled(plan, None, None, None, 1, 4, 0, 1, C.byref(sampling) if sampling is not None else None,
                                 None, None, 0, None)


def _sample(lib, head, sampling, C_=256, M=0):
  return lib.wn_sample_waveform_sampled(head, None, 4, C_, M, 8, 0, C.byref(sampling) if sampling is not None else None, 1,
                                        None, None)


# 1e-39 is a denormal float whose reciprocal (1e39) is not finite in fp32
BAD_T = [0.0, -0.0, -1.0, float('nan'), float('inf'), -float('inf'), 1e-39]


@pytest.mark.parametrize('T', BAD_T)
def test_bad_temperature_is_invalid_before_any_pointer_is_used(lib, T):
  plan = _plan(lib)
  try:
    s = _lib.WnSampling(T, 0, 1)
    if T == 1e-39:
      assert 0 < s.temperature < 2.0 ** -126                       # really a denormal in the struct's float
    assert _generate(lib, plan, s) == _lib.WN_E_INVALID
    assert 'temperature' in lib.wn_last_error_string().decode()
    assert _generate(lib, None, s) == _lib.WN_E_INVALID          # (not even the plan is needed)
    assert 'temperature' in lib.wn_last_error_string().decode()
    for head, M in ((HEAD_CAT, 0), (HEAD_LOGISTIC, 4), (HEAD_GAUSSIAN, 4)):
      assert _sample(lib, head, s, M=M) == _lib.WN_E_INVALID
      assert 'temperature' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


def test_negative_top_k_is_invalid(lib):
  plan = _plan(lib)
  try:
    s = _lib.WnSampling(1.0, -1, 1)
    assert _generate(lib, plan, s) == _lib.WN_E_INVALID
    assert 'top_k' in lib.wn_last_error_string().decode()
    assert _sample(lib, HEAD_CAT, s) == _lib.WN_E_INVALID
    assert 'top_k' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


@pytest.mark.parametrize('sampler', ['logistic', 'gaussian'])
def test_top_k_on_a_mixture_head_is_invalid(lib, sampler):
  plan = _plan(lib, num_mixtures=4, sampling_function=sampler, bits=16)
  try:
    s = _lib.WnSampling(1.0, 3, 1)
    assert _generate(lib, plan, s) == _lib.WN_E_INVALID
    assert 'top_k' in lib.wn_last_error_string().decode()
    assert _sample(lib, _lib.HEADS[sampler], s, C_=12, M=4) == _lib.WN_E_INVALID
    assert 'top_k' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


def test_null_sampling_is_invalid(lib):
  plan = _plan(lib)
  try:
    assert _generate(lib, plan, None) == _lib.WN_E_INVALID
    assert 'sampling' in lib.wn_last_error_string().decode()
    assert _sample(lib, HEAD_CAT, None) == _lib.WN_E_INVALID
    assert 'sampling' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


def test_valid_controls_pass_the_sampling_check(lib):
  """Good values get past the sampling check: the failure is then the null pointers' ('bad arguments'), not a control's;
  a sample_waveform call over zero rows returns WN_OK without touching the device.  top_k beyond 1024 classes is
  WN_E_UNSUPPORTED and names the limit; top_k >= classes is off, whatever the class count."""
  plan = _plan(lib)
  try:
    for T, k in ((1.0, 0), (0.7, 20), (1e-3, 1), (50.0, 256), (1.0, 10 ** 6)):
      assert _generate(lib, plan, _lib.WnSampling(T, k, 7)) == _lib.WN_E_INVALID
      assert 'bad arguments' in lib.wn_last_error_string().decode()
      assert lib.wn_sample_waveform_sampled(HEAD_CAT, None, 0, 256, 0, 8, 0, C.byref(_lib.WnSampling(T, k, 7)), 1, None,
                                            None) == _lib.WN_OK
    assert _sample(lib, HEAD_CAT, _lib.WnSampling(1.0, 5, 1), C_=65536) == _lib.WN_E_UNSUPPORTED
    assert '1024' in lib.wn_last_error_string().decode()
    assert lib.wn_sample_waveform_sampled(HEAD_CAT, None, 0, 65536, 0, 16, 0, C.byref(_lib.WnSampling(1.0, 65536, 1)), 1,
                                          None, None) == _lib.WN_OK
  finally:
    lib.wn_plan_destroy(plan)


def test_python_surface_checks_the_controls_without_a_device():
  """WaveNet._sampling mirrors the library's check (ValueError before any work is queued)."""
  from wavenets_amd import WaveNet
  cat = WaveNet.__new__(WaveNet)
  cat.sampling_function, cat.bits = 'categorical', 8
  mol = WaveNet.__new__(WaveNet)
  mol.sampling_function, mol.bits = 'logistic', 16
  for T in BAD_T:
    with pytest.raises(ValueError, match='temperature'):
      cat._sampling(T, 0, None, 256)
  with pytest.raises(ValueError, match='top_k'):
    cat._sampling(1.0, -1, None, 256)
  with pytest.raises(ValueError, match='top_k'):
    cat._sampling(1.0, 2.5, None, 256)
  with pytest.raises(ValueError, match='top_k'):
    mol._sampling(1.0, 3, None, 65536)
  with pytest.raises(ValueError, match='1024'):
    cat._sampling(1.0, 5, None, 65536)
  with pytest.raises(ValueError, match='seed'):
    cat._sampling(1.0, 0, 1.5, 256)
  s = cat._sampling(0.5, 300, None, 256)
  assert (s.temperature, s.top_k, s.seed) == (0.5, 300, 0x0402)
  assert cat._sampling(1.0, 0, 7, 256).seed == 7 and cat._sampling(1.0, 0, -1, 256).seed == 2 ** 64 - 1
