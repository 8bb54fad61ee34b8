"""CPU-only checks of the sampling controls per utterance (include/wn_hip.h, struct wn_sampling_row)
at the C-ABI boundary, after the pattern of test_top_p_cabi_cpu.py: wn_sampling_rows_pack is host arithmetic and touches
no device, wn_generate_rows_chunk answers its argument errors before the device is touched (every call here passes null
or host pointers), and the Python layer checks its arguments before it queues any work."""
import ctypes as C

import numpy as np
import pytest

from wavenets_amd import _lib
from test_sampling_cabi_cpu import HEAD_CAT, HEAD_GAUSSIAN, HEAD_LOGISTIC, _plan, lib  # noqa: F401  (lib: module fixture)

B = 5
GOOD = (0.7, 20, 7, 0.9)          # temperature, top_k, seed, top_p


def _err(lib):
  return lib.wn_last_error_string().decode()


def _pack(lib, entries, head=HEAD_CAT, classes=256, stream=None):
  """-> (rc, rows, flags)"""
  n = len(entries)
  arr = (_lib.WnSampling * n)(*[_lib.WnSampling(*e) for e in entries])
  st = (C.c_uint64 * n)(*stream) if stream is not None else None
  rows = (_lib.WnSamplingRow * n)()
  flags = C.c_int32(-1)
  rc = lib.wn_sampling_rows_pack(arr, st, n, head, classes, rows, C.byref(flags))
  return rc, rows, flags.value


def _with(row, bad):
  entries = [GOOD] * B
  entries[row] = bad
  return entries


def test_struct_layout_is_eight_floats():
  assert C.sizeof(_lib.WnSamplingRow) == 32
  assert [f[0] for f in _lib.WnSamplingRow._fields_] == ['T', 'inv_T', 'top_k', 'top_p', 'seed', 'stream']
  assert (_lib.WnSamplingRow.seed.offset, _lib.WnSamplingRow.stream.offset) == (16, 24)


def test_table_size_in_floats(lib):
  assert [lib.wn_sampling_rows_floats(n) for n in (1, 5, 33, 4096)] == [8, 40, 264, 32768]
  assert lib.wn_sampling_rows_floats(0) == 0 and lib.wn_sampling_rows_floats(-3) == 0


# 1e-39: a denormal whose reciprocal is not finite in fp32
@pytest.mark.parametrize('row', [0, 2, 4])
@pytest.mark.parametrize('bad,word', [((0.0, 0, 1, 1.0), 'temperature'), ((-1.0, 0, 1, 1.0), 'temperature'),
                                      ((float('nan'), 0, 1, 1.0), 'temperature'), ((float('inf'), 0, 1, 1.0), 'temperature'),
                                      ((1e-39, 0, 1, 1.0), 'temperature'), ((1.0, -1, 1, 1.0), 'top_k'),
                                      ((1.0, 0, 1, -0.1), 'top_p'), ((1.0, 0, 1, 1.5), 'top_p'),
                                      ((1.0, 0, 1, float('nan')), 'top_p')])
def test_every_invalid_field_is_rejected_on_every_row_with_the_row_named(lib, row, bad, word):
  rc, rows, flags = _pack(lib, _with(row, bad))
  assert rc == _lib.WN_E_INVALID
  assert f'row {row}:' in _err(lib) and word in _err(lib)


@pytest.mark.parametrize('row', [0, 3])
@pytest.mark.parametrize('head', [HEAD_LOGISTIC, HEAD_GAUSSIAN])
def test_top_k_and_top_p_on_a_mixture_row_are_invalid(lib, head, row):
  entries = [(0.7, 0, 7, 1.0)] * B
  for bad, word in (((0.7, 3, 7, 1.0), 'top_k'), ((0.7, 0, 7, 0.5), 'top_p')):
    e = list(entries); e[row] = bad
    rc, rows, flags = _pack(lib, e, head=head, classes=30)
    assert rc == _lib.WN_E_INVALID
    assert f'row {row}:' in _err(lib) and word in _err(lib) and 'categorical head only' in _err(lib)
  rc, rows, flags = _pack(lib, entries, head=head, classes=30)
  assert rc == _lib.WN_OK and flags == _lib.WN_SAMPLING_ROWS_ON


@pytest.mark.parametrize('row', [1, 4])
def test_more_than_1024_classes_with_top_k_or_top_p_on_is_unsupported(lib, row):
  plain = [(0.7, 0, 7, 1.0)] * B
  for bad, word in (((1.0, 20, 7, 1.0), 'top_k'), ((1.0, 0, 7, 0.5), 'top_p')):
    e = list(plain); e[row] = bad
    rc, rows, flags = _pack(lib, e, classes=65536)
    assert rc == _lib.WN_E_UNSUPPORTED
    assert f'row {row}:' in _err(lib) and word in _err(lib) and '1024' in _err(lib)
  # temperature alone, and top_k >= classes (off), pass at any class count
  e = list(plain); e[row] = (1.0, 65536, 7, 1.0)
  rc, rows, flags = _pack(lib, e, classes=65536)
  assert rc == _lib.WN_OK and rows[row].top_k == 0


def test_valid_rows_are_packed_and_normalised(lib):
  entries = [(1.0, 0, 11, 0.0), (0.7, 0, 12, 1.0), (1.0, 20, 13, 1.0), (0.7, 256, 14, 0.9), (1.3, 300, 2 ** 64 - 1, 1.0)]
  rc, rows, flags = _pack(lib, entries)
  assert rc == _lib.WN_OK
  assert flags == _lib.WN_SAMPLING_ROWS_ON | _lib.WN_SAMPLING_ROWS_TOP_P
  for b, (T, k, seed, p) in enumerate(entries):
    r = rows[b]
    assert r.T == float(np.float32(T)) and r.inv_T == float(np.float32(1.0) / np.float32(T))
    assert r.top_k == (0 if k >= 256 else k)                       # top_k >= classes is off
    assert r.top_p == (float(np.float32(p)) if 0 < p < 1 else 0.0)   # top_p = 1 (and 0) is off
    assert r.seed == seed and r.stream == b
  # flags speak of the union of the rows
  assert _pack(lib, [(1.0, 0, 1, 1.0), (1.0, 256, 2, 0.0)])[2] == 0
  assert _pack(lib, [(1.0, 0, 1, 1.0), (1.0, 3, 2, 0.0)])[2] == _lib.WN_SAMPLING_ROWS_ON
  # streams
  rc, rows, flags = _pack(lib, entries, stream=[7, 7, 0, 2 ** 63 - 1, 3])
  assert rc == _lib.WN_OK and [r.stream for r in rows] == [7, 7, 0, 2 ** 63 - 1, 3]
  rc, rows, flags = _pack(lib, entries, stream=[0, 1, 2 ** 63, 3, 4])
  assert rc == _lib.WN_E_INVALID and 'row 2:' in _err(lib) and 'stream' in _err(lib)


@pytest.mark.parametrize('entry', [(1.0, 0, 5, 1.0), (0.7, 20, 5, 1.0), (0.7, 20, 5, 0.9), (1.3, 999, 5, 1.0)])
def test_a_table_of_equal_rows_is_copies_of_what_the_scalar_check_leaves(lib, entry):
  """WnSampleCtl of wn_sampling_check: T, 1 / T, the effective top_k and top_p; the key; stream b."""
  rc, rows, flags = _pack(lib, [entry] * B)
  assert rc == _lib.WN_OK
  T, k, seed, p = entry
  want = (float(np.float32(T)), float(np.float32(1.0) / np.float32(T)), 0 if k >= 256 else k,
          float(np.float32(p)) if p < 1 else 0.0, seed)
  for b in range(B):
    r = rows[b]
    assert (r.T, r.inv_T, r.top_k, r.top_p, r.seed) == want and r.stream == b
  first = bytes(rows)[:24]
  assert all(bytes(rows)[32 * b:32 * b + 24] == first for b in range(B))


def test_null_pointers_and_bad_batch_sizes_are_invalid(lib):
  arr = (_lib.WnSampling * B)(*[_lib.WnSampling(*GOOD)] * B)
  rows = (_lib.WnSamplingRow * B)()
  flags = C.c_int32()
  assert lib.wn_sampling_rows_pack(None, None, B, HEAD_CAT, 256, rows, C.byref(flags)) == _lib.WN_E_INVALID
  assert 'sampling_rows_pack' in _err(lib)
  assert lib.wn_sampling_rows_pack(arr, None, B, HEAD_CAT, 256, None, C.byref(flags)) == _lib.WN_E_INVALID
  assert lib.wn_sampling_rows_pack(arr, None, B, HEAD_CAT, 256, rows, None) == _lib.WN_E_INVALID
  for n in (0, -1):
    assert lib.wn_sampling_rows_pack(arr, None, n, HEAD_CAT, 256, rows, C.byref(flags)) == _lib.WN_E_INVALID
    assert 'B' in _err(lib)


_TABLE = (_lib.WnSamplingRow * 2)()      # a 16-byte aligned host address that stands for "a table was given"
_WINDOW = (C.c_float * 4)()


def _rows_chunk(lib, plan, table, flags, window, first, length, queued=1):
  return lib.wn_generate_rows_chunk(plan, None, C.cast(_WINDOW, C.c_void_p) if window else None, None, 1, first, length, 0,
                                    queued, table, flags, None, None, 0, None)


def test_generate_rows_chunk_argument_errors_come_back_before_the_device_is_touched(lib):
  plan = _plan(lib)
  try:
    table = C.cast(_TABLE, C.c_void_p)
    assert table.value % 16 == 0
    assert _rows_chunk(lib, plan, None, 0, True, 0, 4) == _lib.WN_E_INVALID
    assert 'rows is null' in _err(lib)
    assert _rows_chunk(lib, plan, C.c_void_p(table.value + 8), 0, True, 0, 4) == _lib.WN_E_INVALID
    assert 'aligned' in _err(lib)
    for flags in (4, -1, _lib.WN_SAMPLING_ROWS_TOP_P):       # top_p on without any control on: no pack call returns it
      assert _rows_chunk(lib, plan, table, flags, True, 0, 4) == _lib.WN_E_INVALID
      assert 'rows_flags' in _err(lib)
    # the rules of wn_generate_chunk for window / first, word for word
    for queued in (0, 1):
      assert _rows_chunk(lib, plan, table, 0, True, -1, 4, queued) == _lib.WN_E_INVALID
      assert 'first must be >= 0' in _err(lib)
      assert _rows_chunk(lib, plan, table, 0, True, 3, 4, queued) == _lib.WN_E_INVALID
      assert 'requires first == 0' in _err(lib)
      assert _rows_chunk(lib, plan, table, 0, False, 0, 4, queued) == _lib.WN_E_INVALID
      assert 'window is null with first == 0' in _err(lib)
      assert _rows_chunk(lib, plan, table, 0, False, 2 ** 31 - 4, 4, queued) == _lib.WN_E_INVALID
      assert 'first + length' in _err(lib)
    # good values reach the pointer check
    for flags in (0, 1, 3):
      for window, first in ((True, 0), (False, 1)):
        assert _rows_chunk(lib, plan, table, flags, window, first, 4) == _lib.WN_E_INVALID
        assert 'bad arguments' in _err(lib)
    assert _rows_chunk(lib, None, table, 0, True, 0, 4) == _lib.WN_E_INVALID
    assert 'bad arguments' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


# ------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------
def _models():
  from wavenets_amd import WaveNet
  cat = WaveNet.__new__(WaveNet)
  cat.sampling_function, cat.bits = 'categorical', 8
  mol = WaveNet.__new__(WaveNet)
  mol.sampling_function, mol.bits = 'logistic', 16
  return cat, mol


def _rows(model, batch, classes=256, have_sample=True, **kw):
  a = dict(temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None)
  a.update(kw)
  return model._sampling_rows(batch, a['temperature'], a['top_k'], a['seed'], a['top_p'], a['stream'], classes, have_sample)


def test_python_surface_checks_per_row_arguments_without_a_device(lib):
  import torch
  from wavenets_amd.model import _RowControls
  cat, mol = _models()
  # wrong length, of each argument
  for name, v in (('temperature', [1.0, 0.7]), ('top_k', (0, 1, 2, 3)), ('seed', np.arange(6)), ('top_p', torch.ones(2)),
                  ('stream', [0, 1])):
    with pytest.raises(ValueError, match=f'{name} has .* entries for a batch of 5'):
      _rows(cat, 5, **{name: v})
  with pytest.raises(ValueError, match='temperature'):
    _rows(cat, 4, temperature=np.ones((2, 2)))
  # a bool is no number here, on any row of any argument
  for name, v in (('temperature', [1.0, True, 1.0]), ('top_k', [0, 0, True]), ('seed', [False, 1, 2]), ('top_p', [1.0, True, 1.0]),
                  ('stream', [0, True, 2])):
    row = [isinstance(e, bool) for e in v].index(True)
    with pytest.raises(ValueError, match=f'row {row}: .*{name}'):
      _rows(cat, 3, **{name: v})
  # every entry is checked by the rules of the scalar, and the error names the row
  with pytest.raises(ValueError, match='row 1: temperature'):
    _rows(cat, 3, temperature=[1.0, 0.0, 1.0])
  with pytest.raises(ValueError, match='row 2: top_k'):
    _rows(cat, 3, top_k=[0, 5, -1])
  with pytest.raises(ValueError, match='row 0: top_p'):
    _rows(cat, 2, top_p=[1.5, 1.0])
  with pytest.raises(ValueError, match='row 1: top_k applies to the categorical head only'):
    _rows(mol, 2, 65536, top_k=[0, 3])
  with pytest.raises(ValueError, match='row 1: .*1024'):
    _rows(cat, 2, 65536, top_k=[0, 3])
  # streams: ints in [0, 2^63), a sequence, and only beside a sample
  for bad in ([0, -1, 2], [0, 1, 2 ** 63], [0, 1.5, 2], 7, 'abc'):
    with pytest.raises(ValueError, match='stream'):
      _rows(cat, 3, stream=bad)
  with pytest.raises(ValueError, match='stream requires `sample`'):
    _rows(cat, 3, stream=[0, 1, 2], have_sample=False)
  # equal rows and no stream: the one struct of the scalar entry points, whatever the spelling
  for kw in (dict(temperature=[0.7] * 3), dict(temperature=np.full(3, 0.7, np.float32), top_k=(20, 20, 20)),
             dict(temperature=torch.full((3,), 0.7), seed=[None, 0x0402, None], top_k=[0, 256, 300])):
    s = _rows(cat, 3, **kw)
    assert isinstance(s, _lib.WnSampling) and s.temperature == float(np.float32(0.7)) and s.seed == 0x0402
  # rows that differ, or a stream: the packed table
  r = _rows(cat, 3, temperature=[1.0, 0.7, 1.0], top_k=20, seed=np.array([1, 2, 3]), top_p=(1.0, 1.0, 0.9))
  assert isinstance(r, _RowControls) and r.flags == 3
  assert [(x.T, x.top_k, x.seed, x.stream) for x in r.host] == [(1.0, 20, 1, 0), (float(np.float32(0.7)), 20, 2, 1), (1.0, 20, 3, 2)]
  assert [x.top_p for x in r.host] == [0.0, 0.0, float(np.float32(0.9))]
  r = _rows(cat, 2, stream=np.array([5, 5]))
  assert isinstance(r, _RowControls) and r.flags == 0 and [x.stream for x in r.host] == [5, 5]
  assert tuple(r.device_table('cpu').shape) == (16,)
  r = _rows(mol, 2, 65536, temperature=[0.5, 1.0])
  assert isinstance(r, _RowControls) and r.flags == 1


def test_python_generate_signatures_take_stream():
  import inspect
  from wavenets_amd import WaveNet
  for f in (WaveNet.generate, WaveNet.generation_session):
    assert inspect.signature(f).parameters['stream'].default is None
