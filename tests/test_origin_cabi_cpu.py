"""CPU-only checks of the rows' own clocks (include/wn_hip.h, wn_generate_rows_chunk_origin / wn_generate_rows_begin_origin /
wn_generate_admit_origin) at the C-ABI boundary.  The three entry points are their parents with one
more argument, so the parents' argument-error cases run again through them: the test functions of
test_sampling_rows_cabi_cpu.py and test_admit_cabi_cpu.py are called with a library object whose parent symbols forward
to the new ones, with origin = NULL and with an aligned address.  Every call passes null or host pointers and comes back
before the device is touched."""
import ctypes as C
import inspect

import pytest

from wavenets_amd import _lib
import test_admit_cabi_cpu as admit_cases
import test_sampling_rows_cabi_cpu as rows_cases
from test_sampling_cabi_cpu import _plan, lib  # noqa: F401  (lib: module fixture)

_ORIGIN = (C.c_uint64 * 8)()              # an 8-byte aligned host address that stands for "an origin array was given"
_TABLE = (_lib.WnSamplingRow * 4)()
_BUF = (C.c_float * 8)()
NEW = ('wn_generate_rows_chunk_origin', 'wn_generate_rows_begin_origin', 'wn_generate_admit_origin')


def _err(lib):
  return lib.wn_last_error_string().decode()


def _addr(x, plus=0):
  return C.c_void_p(C.cast(x, C.c_void_p).value + plus)


class _Through:
  """The library with the three parent entry points routed through their *_origin forms: `origin` goes behind the flags,
  the eleventh argument of all three."""

  def __init__(self, lib, origin):
    self._lib, self._origin = lib, origin

  def __getattr__(self, name):
    return getattr(self._lib, name)

  def _call(self, name, a):
    assert len(a) == len(_lib._SIGS[name][1])
    return getattr(self._lib, name + '_origin')(*a[:11], self._origin, *a[11:])

  def wn_generate_rows_chunk(self, *a):
    return self._call('wn_generate_rows_chunk', a)

  def wn_generate_rows_begin(self, *a):
    return self._call('wn_generate_rows_begin', a)

  def wn_generate_admit(self, *a):
    return self._call('wn_generate_admit', a)


def test_the_three_symbols_bind(lib):
  for name in NEW:
    assert name in _lib.EXPORTS
    parent = name[:-len('_origin')]
    res, args = _lib._SIGS[name]
    pres, pargs = _lib._SIGS[parent]
    assert res is pres and args == pargs[:11] + [C.c_void_p] + pargs[11:]
    assert getattr(lib, name).argtypes == args


@pytest.mark.parametrize('origin', [None, 'aligned'])
def test_every_argument_error_of_the_parents_comes_back_unchanged(lib, origin):
  through = _Through(lib, _addr(_ORIGIN) if origin else None)
  rows_cases.test_generate_rows_chunk_argument_errors_come_back_before_the_device_is_touched(through)
  admit_cases.test_every_rows_begin_argument_error_comes_back_before_the_device_is_touched(through)
  admit_cases.test_every_admit_argument_error_comes_back_before_the_device_is_touched(through)


def _six(lib, plan, flags, origin=None):
  """(name, rc, error text) of the six entry points on arguments that are good up to the pointer check, with `flags`."""
  table, buf = _addr(_TABLE), _addr(_BUF)
  slots = (C.c_int32 * 1)(0)
  chunk = (plan, None, buf, None, 1, 0, 4, 0, 1, table, flags)
  begin = (plan, None, buf, None, 1, 5, 4, 0, 1, table, flags)
  admit = (plan, buf, buf, None, 1, slots, 5, 6, 0, table, flags)
  ctail, atail = (None, None, 0, None), (buf, buf, 0, buf, 0, None)
  calls = [('wn_generate_rows_chunk', chunk + ctail), ('wn_generate_rows_begin', begin + ctail), ('wn_generate_admit', admit + atail),
           ('wn_generate_rows_chunk_origin', chunk + (origin,) + ctail), ('wn_generate_rows_begin_origin', begin + (origin,) + ctail),
           ('wn_generate_admit_origin', admit + (origin,) + atail)]
  out = []
  for name, args in calls:
    rc = getattr(lib, name)(*args)
    out.append((name, rc, _err(lib)))
  return out


def test_rows_flags_4_is_still_invalid_on_all_six_entry_points(lib):
  """The origin does not travel as a flag bit."""
  plan = _plan(lib)
  try:
    for origin in (None, _addr(_ORIGIN)):
      for flags in (4, 5, 7):
        for name, rc, text in _six(lib, plan, flags, origin):
          assert rc == _lib.WN_E_INVALID and 'rows_flags' in text, (name, flags, text)
      # (the same arguments with good flags pass the flag check: they end at the pointers or the sizes)
      for name, rc, text in _six(lib, plan, 3, origin):
        assert rc == _lib.WN_E_INVALID and 'rows_flags' not in text, (name, text)
  finally:
    lib.wn_plan_destroy(plan)


def test_a_misaligned_origin_is_invalid_and_named(lib):
  """Before any other argument is looked at: everything else is null here."""
  plan = _plan(lib)
  try:
    for plus in (1, 2, 4, 7):
      bad = _addr(_ORIGIN, plus)
      for entry in (lib.wn_generate_rows_chunk_origin, lib.wn_generate_rows_begin_origin):
        assert entry(None, None, None, None, 0, 0, 0, 0, 1, None, 0, bad, None, None, 0, None) == _lib.WN_E_INVALID
        assert 'generate: origin must be aligned to 8 bytes' in _err(lib)
        # ... also on arguments that are good otherwise, deterministic or not, sliding window or queued
        for det in (0, 1):
          for queued in (0, 1):
            assert entry(plan, None, _addr(_BUF), None, 1, 0, 4, det, queued, _addr(_TABLE), 0, bad, None, None, 0, None) == _lib.WN_E_INVALID
            assert 'origin must be aligned' in _err(lib)
      assert lib.wn_generate_admit_origin(None, None, None, None, 0, None, 0, 0, 0, None, 0, bad, None, None, 0, None, 0,
                                          None) == _lib.WN_E_INVALID
      assert 'generate_admit: origin_k must be aligned to 8 bytes' in _err(lib)
    # 8 is aligned: the call goes on to the arguments behind it
    ok = _addr(_ORIGIN, 8)
    assert lib.wn_generate_rows_chunk_origin(None, None, None, None, 0, 0, 0, 0, 1, None, 0, ok, None, None, 0, None) == _lib.WN_E_INVALID
    assert 'rows is null' in _err(lib)
    assert lib.wn_generate_admit_origin(None, None, None, None, 0, None, 0, 0, 0, None, 0, ok, None, None, 0, None, 0,
                                        None) == _lib.WN_E_INVALID
    assert 'generate_admit: p is null' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


# ------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------
def test_python_signatures_take_own_clock():
  from wavenets_amd import WaveNet
  from wavenets_amd.model import GenerationSession
  assert inspect.signature(WaveNet.generation_session).parameters['own_clock'].default is False
  # admit keeps the parameter list of section 32; admit_own_clock is the same list under another name
  a, o = (inspect.signature(f).parameters for f in (GenerationSession.admit, GenerationSession.admit_own_clock))
  assert 'own_clock' not in a and list(a) == list(o) and [v.default for v in a.values()] == [v.default for v in o.values()]
  assert isinstance(GenerationSession.origins, property) and isinstance(GenerationSession.row_positions, property)


def test_python_surface_checks_own_clock_without_a_device(lib):
  from wavenets_amd import WaveNet
  from wavenets_amd.model import GenerationSession
  m = WaveNet.__new__(WaveNet)
  s = GenerationSession.__new__(GenerationSession)
  s._model = m
  for bad in (1, 0, None, 'yes', 1.0, [True]):
    with pytest.raises(ValueError, match='own_clock must be a bool'):
      m.generation_session(sample=None, stream=[0], own_clock=bad)
  # (start is looked at first, as ever)
  with pytest.raises(ValueError, match='start must be'):
    m.generation_session(start=-1, own_clock=1)
  # a session without a row table refuses the admission on either clock, with the text of before
  s._queued, s._rows = 1, None
  for admit in (s.admit, s.admit_own_clock):
    with pytest.raises(RuntimeError, match='admit needs per-row controls'):
      admit(0, None, stream=[0])
  s._queued = 0
  for admit in (s.admit, s.admit_own_clock):
    with pytest.raises(RuntimeError, match='use_queues=True'):
      admit(0, None, stream=[0])
  # origins and row_positions are host arithmetic
  s._origins, s.position = [0, 5, 13], 20
  assert s.origins == [0, 5, 13] and s.row_positions == [20, 15, 7]
  s.origins.append(1)
  assert s._origins == [0, 5, 13]
