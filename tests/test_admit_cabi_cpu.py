"""CPU-only checks of admission into a running batch (include/wn_hip.h, wn_generate_rows_begin / wn_generate_admit;
DESIGN.md section 32) at the C-ABI boundary, after the pattern of test_sampling_rows_cabi_cpu.py: every argument error
comes back with its code and a text that names the argument before the device is touched (every call here passes null
or host pointers), the scratch size is the queued generation workspace of k rows, and wn_generate_admit_describe -- host
arithmetic over the two layouts -- lists segments that add up to the state of one utterance, lie inside the session's
state and do not overlap."""
import ctypes as C
import math
import re

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan as _plan_of
from test_sampling_cabi_cpu import _plan, lib  # noqa: F401  (lib: module fixture)

_TABLE = (_lib.WnSamplingRow * 4)()       # a 16-byte aligned host address that stands for "a table was given"
_BUF = (C.c_float * 8)()                  # ... and for any other pointer
BIG = 2 ** 40


def _err(lib):
  return lib.wn_last_error_string().decode()


def _p(x=_BUF):
  return C.cast(x, C.c_void_p)


def _admit(lib, plan, **kw):
  a = dict(p=plan, params=_p(), windows=_p(), cond=None, k=2, slots=[3, 0], B=5, position=6, det=0, rows_k=_p(_TABLE),
           flags=0, first_out=_p(), workspace=_p(), ws_floats=BIG, scratch=_p(), scratch_floats=BIG)
  a.update(kw)
  slots = None if a['slots'] is None else (C.c_int32 * len(a['slots']))(*a['slots'])
  return lib.wn_generate_admit(a['p'], a['params'], a['windows'], a['cond'], a['k'], slots, a['B'], a['position'], a['det'],
                               a['rows_k'], a['flags'], a['first_out'], a['workspace'], a['ws_floats'], a['scratch'],
                               a['scratch_floats'], None)


def _cond_plan(lib):
  kw = dict(blocks=3, channels=32, dilation_bound=8, final_layers_channels=[], conditioning='global', bits=6)
  p = C.c_void_p(_plan_of(lib, _cfg(**kw), 4))
  assert p.value
  return p


def test_every_admit_argument_error_comes_back_before_the_device_is_touched(lib):
  plan = _plan(lib)
  try:
    assert C.cast(_TABLE, C.c_void_p).value % 16 == 0
    for name in ('p', 'params', 'windows', 'slots', 'rows_k', 'first_out', 'workspace', 'scratch'):
      assert _admit(lib, plan, **{name: None}) == _lib.WN_E_INVALID
      assert f'generate_admit: {name} is null' in _err(lib)
    for k, B in ((0, 5), (-1, 5), (6, 5)):
      assert _admit(lib, plan, k=k, B=B, slots=[0] * max(k, 1)) == _lib.WN_E_INVALID
      assert 'k must lie in [1, B]' in _err(lib)
    for slots, idx in (([3, 5], 1), ([-1, 2], 0), ([0, 1, 2, 7], 3)):
      assert _admit(lib, plan, k=len(slots), slots=slots) == _lib.WN_E_INVALID
      assert f'slots[{idx}]' in _err(lib) and 'outside' in _err(lib)
    for slots, idx in (([3, 3], 1), ([0, 4, 2, 4], 3)):
      assert _admit(lib, plan, k=len(slots), slots=slots) == _lib.WN_E_INVALID
      assert f'slots[{idx}]' in _err(lib) and 'duplicate' in _err(lib)
    for position in (0, -4, 2 ** 31 - 1, 2 ** 40):
      assert _admit(lib, plan, position=position) == _lib.WN_E_INVALID
      assert 'position' in _err(lib)
    assert _admit(lib, plan, rows_k=C.c_void_p(C.cast(_TABLE, C.c_void_p).value + 8)) == _lib.WN_E_INVALID
    assert 'rows_k' in _err(lib) and 'aligned' in _err(lib)
    for flags in (4, -1, _lib.WN_SAMPLING_ROWS_TOP_P):
      assert _admit(lib, plan, flags=flags) == _lib.WN_E_INVALID
      assert 'rows_flags_k' in _err(lib)
    need = lib.wn_generate_workspace_floats(plan, 5, 1)
    assert _admit(lib, plan, ws_floats=need - 1) == _lib.WN_E_INVALID
    assert 'workspace too small' in _err(lib) and str(need) in _err(lib)
    need_k = lib.wn_generate_admit_scratch_floats(plan, 2)
    assert _admit(lib, plan, ws_floats=need, scratch_floats=need_k - 1) == _lib.WN_E_INVALID
    assert 'scratch too small' in _err(lib) and str(need_k) in _err(lib)
    # the largest position and every good value pass every check up to the sizes
    assert _admit(lib, plan, position=2 ** 31 - 2, flags=3, k=5, slots=[4, 3, 2, 1, 0], ws_floats=0) == _lib.WN_E_INVALID
    assert 'workspace too small' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)
  cond = _cond_plan(lib)
  try:
    assert _admit(lib, cond, cond=None) == _lib.WN_E_INVALID
    assert 'cond is null' in _err(lib)
  finally:
    lib.wn_plan_destroy(cond)


def _begin(lib, plan, table, flags, window, first, length, queued=1):
  return lib.wn_generate_rows_begin(plan, None, _p() if window else None, None, 1, first, length, 0, queued, table, flags,
                                    None, None, 0, None)


def test_every_rows_begin_argument_error_comes_back_before_the_device_is_touched(lib):
  plan = _plan(lib)
  try:
    table = _p(_TABLE)
    assert _begin(lib, plan, None, 0, True, 5, 4) == _lib.WN_E_INVALID
    assert 'rows is null' in _err(lib)
    assert _begin(lib, plan, C.c_void_p(table.value + 8), 0, True, 5, 4) == _lib.WN_E_INVALID
    assert 'aligned' in _err(lib)
    for flags in (4, -1, _lib.WN_SAMPLING_ROWS_TOP_P):
      assert _begin(lib, plan, table, flags, True, 5, 4) == _lib.WN_E_INVALID
      assert 'rows_flags' in _err(lib)
    for queued in (0, 1):
      assert _begin(lib, plan, table, 0, True, -1, 4, queued) == _lib.WN_E_INVALID
      assert 'first must be >= 0' in _err(lib)
      for first in (0, 5):
        assert _begin(lib, plan, table, 0, False, first, 4, queued) == _lib.WN_E_INVALID
        assert 'window is null' in _err(lib)
      assert _begin(lib, plan, table, 0, True, 2 ** 31 - 4, 4, queued) == _lib.WN_E_INVALID
      assert 'first + length' in _err(lib)
      # a window at first > 0 is what this entry point is for: it reaches the pointer check (out, workspace are null)
      for first in (0, 5, 2 ** 31 - 5):
        assert _begin(lib, plan, table, 3, True, first, 4, queued) == _lib.WN_E_INVALID
        assert 'bad arguments' in _err(lib)
    # ... and wn_generate_rows_chunk keeps its rule
    assert lib.wn_generate_rows_chunk(plan, None, _p(), None, 1, 5, 4, 0, 1, table, 0, None, None, 0, None) == _lib.WN_E_INVALID
    assert 'requires first == 0' in _err(lib)
  finally:
    lib.wn_plan_destroy(plan)


def test_scratch_is_the_queued_workspace_of_k_rows(lib):
  plan = _plan(lib)
  try:
    for k in (1, 2, 5, 33):
      assert lib.wn_generate_admit_scratch_floats(plan, k) == lib.wn_generate_workspace_floats(plan, k, 1) > 0
    assert lib.wn_generate_admit_scratch_floats(plan, 0) == 0 and lib.wn_generate_admit_scratch_floats(None, 1) == 0
  finally:
    lib.wn_plan_destroy(plan)


def _describe(lib, plan, k, B, n=1 << 16):
  buf = C.create_string_buffer(n)
  rc = lib.wn_generate_admit_describe(plan, k, B, buf, n)
  return rc, buf.value.decode()


def _parse(text):
  """-> ([(name, block, slots, width, src, dst)], floats per utterance)"""
  items = text.split(' | ')
  m = re.fullmatch(r'floats_per_utterance=(\d+)', items[-1])
  assert m, items[-1]
  segs = []
  for it in items[:-1]:
    s = re.fullmatch(r'(\S+) block=(-?\d+) slots=(\d+) width=(\d+) src=(\d+) dst=(\d+)', it)
    assert s, it
    segs.append((s.group(1),) + tuple(int(v) for v in s.groups()[1:]))
  return segs, int(m.group(1))


@pytest.mark.parametrize('k,B', [(1, 5), (2, 5), (5, 5), (2, 33)])
@pytest.mark.parametrize('name', ['cat_r64', 'cat_lpb3', 'cat_k3', 'cond'])
def test_describe_lists_the_state_of_one_utterance(lib, name, k, B):
  from test_gpu_parity import MODEL_CASES
  kw = dict(MODEL_CASES[name])
  cond_inputs = kw.pop('cond_inputs', 0)
  plan = C.c_void_p(_plan_of(lib, _cfg(**kw), cond_inputs))
  assert plan.value, _err(lib)
  try:
    rc, text = _describe(lib, plan, k, B)
    assert rc == _lib.WN_OK, _err(lib)
    segs, per = _parse(text)
    # the floats of one utterance, from the constructor arguments: dilation of conv i of block b is KS ^ ((b * LPB + i) mod
    # log_KS(bound)), a ring of a conv's inputs has (KS - 1) * dilation + 1 slots
    KS, N, LPB = kw.get('kernel_size', 2), kw['blocks'], kw.get('layers_per_block', 1)
    R = kw['channels']
    D = kw.get('dilation_channels') or R
    power = round(math.log(kw['dilation_bound'], KS))
    slots = lambda b, i: (KS - 1) * KS ** ((b * LPB + i) % power) + 1
    want = KS + sum(slots(b, 0) * R for b in range(N)) + sum(slots(b, i) * D for b in range(N) for i in range(1, LPB))
    if cond_inputs:
      want += N * 2 * D
    assert per == want == sum(s[2] * s[3] for s in segs)
    names = [s[0] for s in segs]
    assert names[0] == 'xin' and names.count('xin') == 1 and len(set(names)) == len(names)
    assert sum(n.startswith('ring[') for n in names) == N and sum(n.startswith('ringp[') for n in names) == N * (LPB - 1)
    assert sum(n.startswith('cb[') for n in names) == (N if cond_inputs else 0)
    # where they lie: the destinations inside the session's state (cb: inside the priming layout in front of it), the
    # sources inside the scratch's; no two overlap on either side
    off, n = C.c_int64(), C.c_int64()
    assert lib.wn_generate_state_range(plan, B, 1, C.byref(off), C.byref(n)) == 0
    offk, nk = C.c_int64(), C.c_int64()
    assert lib.wn_generate_state_range(plan, k, 1, C.byref(offk), C.byref(nk)) == 0
    rf = lib.wn_plan_receptive_field(plan)
    prime, prime_k = (lib.wn_plan_workspace_floats(plan, b, rf, 0) for b in (B, k))
    assert 0 < prime <= off.value and 0 < prime_k <= offk.value
    for side, rows, (lo, hi), plo in ((5, B, (off.value, off.value + n.value), prime), (4, k, (offk.value, offk.value + nk.value), prime_k)):
      spans = []
      for s in segs:
        a, b = s[side], s[side] + s[2] * rows * s[3]
        if s[0].startswith('cb['):
          assert 0 <= a and b <= plo, s
        else:
          assert lo <= a and b <= hi, s
        spans.append((a, b))
      spans.sort()
      assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)), spans
    assert hi <= lib.wn_generate_admit_scratch_floats(plan, k)
  finally:
    lib.wn_plan_destroy(plan)


def test_describe_argument_errors(lib):
  plan = _plan(lib)
  try:
    assert lib.wn_generate_admit_describe(plan, 1, 5, None, 100) == _lib.WN_E_INVALID
    assert _describe(lib, None, 1, 5)[0] == _lib.WN_E_INVALID
    for k, B in ((0, 5), (6, 5), (1, 0)):
      assert _describe(lib, plan, k, B)[0] == _lib.WN_E_INVALID
    rc, text = _describe(lib, plan, 1, 5, 16)
    assert rc == _lib.WN_E_INVALID and 'bytes' in _err(lib) and len(text) == 15
  finally:
    lib.wn_plan_destroy(plan)


def test_python_signatures():
  import inspect
  from wavenets_amd import WaveNet
  from wavenets_amd.model import GenerationSession
  assert inspect.signature(WaveNet.generation_session).parameters['start'].default == 0
  sig = inspect.signature(GenerationSession.admit).parameters
  assert list(sig)[1:] == ['slots', 'sample', 'condition', 'temperature', 'top_k', 'seed', 'top_p', 'stream']
  assert sig['stream'].default is None and sig['condition'].default is None
