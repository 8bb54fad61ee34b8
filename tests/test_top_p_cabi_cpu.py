"""CPU-only checks of top_p (nucleus sampling; include/wn_hip.h, struct wn_sampling) at the C-ABI boundary, after the
pattern of test_sampling_cabi_cpu.py: the value is validated before any other argument is looked at and before anything
touches the device, so every call here passes null device pointers.  Also the fp64 reference of the nucleus that the GPU
tests (test_gpu_top_p.py) compare against, checked here on the dyadic row whose kept sets are known exactly."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from wavenets_amd import _lib
from test_sampling_cabi_cpu import HEAD_CAT, _generate, _plan, _sample, lib  # noqa: F401  (lib: module fixture)


# ------------------------------------------------------------------------------------------
# the reference: a few lines of torch in fp64
# ------------------------------------------------------------------------------------------
def f32(x):
  """The fp32 value the struct's float holds, as a Python float."""
  return float(np.float32(x))


def nucleus(probs, top_p, T=1.0, k=0):
  """probs (rows, C) fp32 -> bool (rows, C): the nucleus of every row.  Stable descending sort (probability descending,
  class index ascending), q = (p / p_max)^(1/T), zero beyond the first k (k = 0: all), normalised cumulative sum,
  n* = count(cum < top_p) + 1 classes kept."""
  rows, Cc = probs.shape
  order = torch.sort(probs, dim=-1, descending=True, stable=True)
  v = order.values.double()
  q = (v / v[:, :1]) ** (1.0 / T)
  if 0 < k < Cc:
    q[:, k:] = 0
  cum = q.cumsum(-1) / q.sum(-1, keepdim=True)
  n = ((cum < top_p).sum(-1) + 1).clamp(max=k if 0 < k < Cc else Cc)
  kept = torch.arange(Cc).unsqueeze(0) < n.unsqueeze(1)
  return torch.zeros(rows, Cc, dtype=torch.bool).scatter_(1, order.indices, kept)


def dyadic_row(Cc=256):
  """p[5] = 1/4, p[10] = p[70] = p[131] = p[200] = 1/8, 64 further classes at 1/256 (the first 64 of 140..205 without
  200), the rest 0: every partial sum and every p / p_max is exact in fp32."""
  row = torch.zeros(Cc)
  row[5] = 0.25
  row[[10, 70, 131, 200]] = 0.125
  small = [j for j in range(140, 206) if j != 200][:64]
  row[small] = 1.0 / 256
  assert float(row.double().sum()) == 1.0
  return row


TOP5 = [5, 10, 70, 131, 200]
# (top_k, top_p) -> the kept set
DYADIC_SETS = [
    (0, 0.25, [5]),                                   # equality suffices
    (0, 0.3, [5, 10]),
    (0, 0.375, [5, 10]),
    (0, 0.5, [5, 10, 70]),                            # ties by class index, not by lane
    (0, 0.75, TOP5),
    (0, float(np.nextafter(np.float32(0.75), np.float32(1.0))), TOP5 + [140]),
    (3, 0.5, [5]),
    (3, 0.6, [5, 10]),
]


@pytest.mark.parametrize('Cc', [256, 1000])
@pytest.mark.parametrize('k,top_p,expect', DYADIC_SETS)
def test_reference_nucleus_on_the_dyadic_row(k, top_p, expect, Cc):
  kept = nucleus(dyadic_row(Cc).unsqueeze(0), f32(top_p), 1.0, k)[0]
  assert sorted(kept.nonzero().reshape(-1).tolist()) == sorted(expect)


def test_reference_nucleus_tiny_top_p_is_the_first_maximum():
  row = torch.full((256,), 0.001); row[[17, 200]] = 0.3
  for T in (1.0, 0.3):
    assert nucleus(row.unsqueeze(0), 1e-6, T)[0].nonzero().reshape(-1).tolist() == [17]


# ------------------------------------------------------------------------------------------
# struct layout and argument checks
# ------------------------------------------------------------------------------------------
def test_struct_layout_top_p_is_the_last_member_and_defaults_to_zero():
  s = _lib.WnSampling(1.0, 0, 7)
  assert s.top_p == 0.0 and (s.temperature, s.top_k, s.seed) == (1.0, 0, 7)
  assert [f[0] for f in _lib.WnSampling._fields_] == ['temperature', 'top_k', 'seed', 'top_p']
  assert _lib.WnSampling.top_p.offset == 16 and C.sizeof(_lib.WnSampling) == 24
  assert _lib.WnSampling(1.0, 0, 7, 0.5).top_p == 0.5


@pytest.mark.parametrize('top_p', [-0.1, 1.5, float('nan'), float('inf')])
def test_bad_top_p_is_invalid_before_any_pointer_is_used(lib, top_p):
  plan = _plan(lib)
  try:
    s = _lib.WnSampling(1.0, 0, 1, top_p)
    assert _generate(lib, plan, s) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
    assert _generate(lib, None, s) == _lib.WN_E_INVALID            # (not even the plan is needed)
    assert 'top_p' in lib.wn_last_error_string().decode()
    assert _sample(lib, HEAD_CAT, s) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


@pytest.mark.parametrize('sampler', ['logistic', 'gaussian'])
def test_top_p_on_a_mixture_head_is_invalid(lib, sampler):
  plan = _plan(lib, num_mixtures=4, sampling_function=sampler, bits=16)
  try:
    s = _lib.WnSampling(1.0, 0, 1, 0.5)
    assert _generate(lib, plan, s) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
    assert _sample(lib, _lib.HEADS[sampler], s, C_=12, M=4) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
    # off is accepted with a mixture head: the failure is then the null pointers'
    for off in (0.0, 1.0):
      assert _generate(lib, plan, _lib.WnSampling(1.0, 0, 1, off)) == _lib.WN_E_INVALID
      assert 'bad arguments' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


def test_top_p_beyond_1024_classes_is_unsupported(lib):
  assert _sample(lib, HEAD_CAT, _lib.WnSampling(1.0, 0, 1, 0.5), C_=65536) == _lib.WN_E_UNSUPPORTED
  msg = lib.wn_last_error_string().decode()
  assert 'top_p' in msg and '1024' in msg
  plan = _plan(lib, bits=16)
  try:
    assert _generate(lib, plan, _lib.WnSampling(1.0, 0, 1, 0.5)) == _lib.WN_E_UNSUPPORTED
    assert 'top_p' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)
  # off: any class count
  for off in (0.0, 1.0):
    assert lib.wn_sample_waveform_sampled(HEAD_CAT, None, 0, 65536, 0, 16, 0, C.byref(_lib.WnSampling(1.0, 0, 1, off)), 1,
                                          None, None) == _lib.WN_OK


def test_valid_top_p_passes_the_sampling_check(lib):
  """0 and 1.0 (off) and values in (0, 1) get past the check: the failure is then the null pointers', and a
  sample_waveform call over zero rows returns WN_OK without touching the device.  A deterministic draw still checks."""
  plan = _plan(lib)
  try:
    for top_p in (0.0, 1.0, 0.5, 1e-6, f32(np.nextafter(np.float32(1.0), np.float32(0.0)))):
      for T, k in ((1.0, 0), (0.7, 20)):
        s = _lib.WnSampling(T, k, 7, top_p)
        assert _generate(lib, plan, s) == _lib.WN_E_INVALID
        assert 'bad arguments' in lib.wn_last_error_string().decode()
        assert lib.wn_sample_waveform_sampled(HEAD_CAT, None, 0, 256, 0, 8, 0, C.byref(s), 1, None, None) == _lib.WN_OK
    bad = _lib.WnSampling(1.0, 0, 7, 1.5)
    assert lib.wn_generate_sampled(plan, None, None, None, 1, 4, 1, 1, C.byref(bad), None, None, 0, None) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
    assert lib.wn_sample_waveform_sampled(HEAD_CAT, None, 0, 256, 0, 8, 1, C.byref(bad), 1, None, None) == _lib.WN_E_INVALID
    assert 'top_p' in lib.wn_last_error_string().decode()
  finally:
    lib.wn_plan_destroy(plan)


def test_python_surface_checks_top_p_without_a_device():
  from wavenets_amd import WaveNet
  cat = WaveNet.__new__(WaveNet)
  cat.sampling_function, cat.bits = 'categorical', 8
  mol = WaveNet.__new__(WaveNet)
  mol.sampling_function, mol.bits = 'logistic', 16
  for bad in (0, 0.0, -1, 1.01, float('nan'), float('inf'), True, False, '0.5', None, 1e-60):
    with pytest.raises(ValueError, match='top_p'):
      cat._sampling(1.0, 0, None, 256, top_p=bad)
  with pytest.raises(ValueError, match='top_p'):
    mol._sampling(1.0, 0, None, 65536, top_p=0.9)
  with pytest.raises(ValueError, match='1024'):
    cat._sampling(1.0, 0, None, 65536, top_p=0.9)
  # 1.0 is the default and is off: 1.0 in the struct, which the library reads as off; any head, any class count
  assert cat._sampling(1.0, 0, None, 256).top_p == 1.0
  assert mol._sampling(1.0, 0, None, 65536, top_p=1.0).top_p == 1.0 and mol._sampling(1.0, 0, None, 65536, top_p=1).top_p == 1.0
  s = cat._sampling(0.5, 20, 7, 256, top_p=0.3)
  assert (s.temperature, s.top_k, s.seed) == (0.5, 20, 7) and s.top_p == f32(0.3)
  assert math.isclose(cat._sampling(1.0, 0, None, 256, top_p=np.float32(0.9)).top_p, 0.9, rel_tol=1e-7)
