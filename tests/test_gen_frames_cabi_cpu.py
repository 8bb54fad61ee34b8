"""Frame schedules of queued generation at the C-ABI boundary, without a device (include/wn_hip.h: wn_generate_frames_floats,
wn_generate_frames_build, struct wn_frame_row, wn_plan_arm_gen_frames).  Every call below must come
back before the device is touched: the pointers are host addresses that would fault if anything were read or launched."""
import ctypes as C

import pytest

from test_cabi_cpu import _cfg, _plan, lib  # noqa: F401  (lib: fixture)
from test_local_cond_cpu import _conditioned_plan
from wavenets_amd import _lib

ONE = C.c_void_p(64)            # never dereferenced; aligned to 16 bytes
BIG = 1 << 40
N, D2 = 3, 64                   # _conditioned_plan: 3 blocks of 32 channels


@pytest.fixture
def plan(lib):
  p = _conditioned_plan(lib)
  yield p
  lib.wn_plan_arm_gen_frames(p, None, 0)
  lib.wn_plan_destroy(p)


@pytest.fixture
def bare(lib):
  u = C.c_void_p(_plan(lib, _cfg(blocks=3, dilation_bound=8)))
  yield u
  lib.wn_plan_destroy(u)


def _records(*rows):
  """rows: per batch row None (off the schedule) or (pointer, block_stride, origin, frames, hop)."""
  recs = (_lib.WnFrameRow * len(rows))()
  for b, r in enumerate(rows):
    if r is not None:
      recs[b] = _lib.WnFrameRow(*r)
  return recs


def _msg(lib):
  return lib.wn_last_error_string()


def test_the_symbols_resolve_with_their_signatures(lib):
  P = C.c_void_p
  want = {'wn_generate_frames_floats': (C.c_int64, [P, C.c_int64]),
          'wn_generate_frames_build': (C.c_int, [P, P, P, C.c_int32, C.c_int32, P, C.c_int64, P, C.c_int64, C.c_int32, P]),
          'wn_plan_arm_gen_frames': (C.c_int, [P, C.POINTER(_lib.WnFrameRow), C.c_int32])}
  for name, sig in want.items():
    assert name in _lib.EXPORTS and _lib._SIGS[name] == sig and hasattr(lib, name)
  assert C.sizeof(_lib.WnFrameRow) == 32            # pointer, two int64, two int32: no padding


def test_frames_floats_holds_the_bias_rows_and_grows(lib, plan, bare):
  sizes = [lib.wn_generate_frames_floats(plan, rows) for rows in (1, 3, 12, 400)]
  for rows, n in zip((1, 3, 12, 400), sizes):
    assert n >= N * rows * D2, (rows, n)
  assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[3]
  assert lib.wn_generate_frames_floats(plan, 0) == 0 and lib.wn_generate_frames_floats(None, 4) == 0
  assert lib.wn_generate_frames_floats(bare, 4) == 0            # a plan without conditioning has no table


def test_frames_build_argument_checks(lib, plan, bare):
  need = lib.wn_generate_frames_floats(plan, 2 * 3)
  ws_need = lib.wn_generate_workspace_floats(plan, 2, 1)

  def call(pp=plan, params=ONE, cond=ONE, k=2, F=3, table=ONE, tf=BIG, ws=ONE, wf=BIG, B=2):
    return lib.wn_generate_frames_build(pp, params, cond, k, F, table, tf, ws, wf, B, None)
  cases = ((dict(pp=None), b'null plan'), (dict(params=None), b'null params'), (dict(cond=None), b'null cond'),
           (dict(table=None), b'null table'), (dict(ws=None), b'null workspace'),
           (dict(k=0), b'k = 0, F = 3'), (dict(F=-1), b'k = 2, F = -1'),
           (dict(k=1 << 20, F=1 << 10), b'must not exceed 2147483647'),
           (dict(table=C.c_void_p(68)), b'table must be aligned to 16 bytes'),
           (dict(tf=need - 1), f'table too small ({need - 1} floats, wn_generate_frames_floats(p, 6) is {need})'.encode()),
           (dict(B=0), b'B must be >= 1 (got 0)'),
           (dict(wf=ws_need - 1), f'workspace too small ({ws_need - 1} < {ws_need} floats)'.encode()))
  for kw, text in cases:
    assert call(**kw) == _lib.WN_E_INVALID, kw
    assert _msg(lib).startswith(b'generate_frames_build:') and text in _msg(lib), (kw, _msg(lib))
  assert call(pp=bare) == _lib.WN_E_INVALID and b'no conditioning' in _msg(lib)
  assert lib.wn_plan_set_cond_frames(plan, 3) == _lib.WN_OK
  assert call() == _lib.WN_E_INVALID and b'3 condition frames are armed' in _msg(lib)
  assert lib.wn_plan_set_cond_frames(plan, 0) == _lib.WN_OK


def test_arm_gen_frames_argument_checks(lib, plan, bare):
  good = (64, 4 * D2, 0, 4, 5)
  assert lib.wn_plan_arm_gen_frames(None, _records(good), 1) == _lib.WN_E_INVALID and b'null plan' in _msg(lib)
  assert lib.wn_plan_arm_gen_frames(plan, _records(good), -1) == _lib.WN_E_INVALID and b'B must be >= 0 (got -1)' in _msg(lib)
  for bad, text in (((64, 4 * D2, 0, 0, 5), b'row 1: frames and hop must be >= 1 (got frames = 0, hop = 5)'),
                    ((64, 4 * D2, 0, 4, 0), b'row 1: frames and hop must be >= 1 (got frames = 4, hop = 0)'),
                    ((64, 4 * D2 - 1, 0, 4, 5), b'row 1: block_stride = 255 is below frames * 2D = 4 * 64'),
                    ((66, 4 * D2, 0, 4, 5), b'row 1: rows must be aligned to 4 bytes')):
    assert lib.wn_plan_arm_gen_frames(plan, _records(None, bad), 2) == _lib.WN_E_INVALID, bad
    assert text in _msg(lib), (bad, _msg(lib))
  # a record that is off the schedule is not looked at
  assert lib.wn_plan_arm_gen_frames(plan, _records((None, 0, 0, 0, 0), good), 2) == _lib.WN_OK
  # a null pointer or B = 0 disarms, on any plan
  assert lib.wn_plan_arm_gen_frames(plan, None, 2) == _lib.WN_OK
  assert lib.wn_plan_arm_gen_frames(plan, _records(good), 0) == _lib.WN_OK
  assert lib.wn_plan_arm_gen_frames(bare, None, 0) == _lib.WN_OK
  assert lib.wn_plan_arm_gen_frames(bare, _records(good), 1) == _lib.WN_E_INVALID
  assert b'1 frame schedules on a plan without conditioning' in _msg(lib)
  assert lib.wn_plan_set_cond_frames(plan, 3) == _lib.WN_OK
  assert lib.wn_plan_arm_gen_frames(plan, _records(good), 1) == _lib.WN_E_INVALID
  assert b'3 condition frames are armed' in _msg(lib)
  assert lib.wn_plan_set_cond_frames(plan, 0) == _lib.WN_OK


def _rows_chunk(lib, p, B, first, length, queued=1, ws_floats=BIG):
  return lib.wn_generate_rows_chunk(p, ONE, None, ONE, B, first, length, 1, queued, ONE, 0, ONE, ONE, ws_floats, None)


def test_a_schedule_that_ends_inside_a_call_is_refused_before_anything_is_read(lib, plan):
  # row 1: 4 frames of hop 5 from origin 3: samples 3 .. 22.  The call makes samples 20 .. 23.
  recs = _records(None, (64, 4 * D2, 3, 4, 5), (64, 8 * D2, 0, 8, 5))
  assert lib.wn_plan_arm_gen_frames(plan, recs, 3) == _lib.WN_OK
  assert _rows_chunk(lib, plan, 3, 20, 4) == _lib.WN_E_INVALID
  msg = _msg(lib)
  assert b'row 1 runs past its condition frames' in msg and b'frames = 4 of hop = 5' in msg and b'origin 3' in msg, msg
  assert b'sample 23' in msg and b'its last sample is 22' in msg, msg
  # one sample fewer fits: the next check of the call is the one that answers (the workspace is too small on purpose)
  assert _rows_chunk(lib, plan, 3, 20, 3, ws_floats=8) == _lib.WN_E_INVALID and b'workspace too small' in _msg(lib)
  # armed for another B than the call's, and on the sliding window
  assert _rows_chunk(lib, plan, 2, 20, 3) == _lib.WN_E_INVALID
  assert b'armed for B = 3 rows, the call has B = 2' in _msg(lib)
  assert _rows_chunk(lib, plan, 3, 20, 3, queued=0) == _lib.WN_E_INVALID
  assert b'the sliding window takes none' in _msg(lib)
  # the scalar entry point and the begin form see the same schedule
  sp = _lib.WnSampling(1.0, 0, 0, 0.0)
  assert lib.wn_generate_chunk(plan, ONE, None, ONE, 3, 20, 4, 1, 1, C.byref(sp), ONE, ONE, BIG, None) == _lib.WN_E_INVALID
  assert b'row 1 runs past' in _msg(lib)
  assert lib.wn_generate_rows_begin(plan, ONE, ONE, ONE, 3, 20, 4, 1, 1, ONE, 0, ONE, ONE, BIG, None) == _lib.WN_E_INVALID
  assert b'row 1 runs past' in _msg(lib)
  # the admission's scratch pass at k rows does not look at it: its own checks answer
  slots = (C.c_int32 * 1)(1)
  rc = lib.wn_generate_admit(plan, ONE, ONE, ONE, 1, slots, 3, 20, 1, ONE, 0, ONE, ONE, 8, ONE, BIG, None)
  assert rc == _lib.WN_E_INVALID and b'generate_admit: workspace too small' in _msg(lib)


def test_arm_then_disarm_leaves_the_argument_checks_as_they_were(lib, plan):
  sp = _lib.WnSampling(1.0, 0, 0, 0.0)
  calls = (lambda: lib.wn_generate_chunk(plan, ONE, None, ONE, 3, -1, 4, 1, 1, C.byref(sp), ONE, ONE, BIG, None),
           lambda: lib.wn_generate_chunk(plan, ONE, None, ONE, 3, 0, 4, 1, 1, C.byref(sp), ONE, ONE, BIG, None),
           lambda: lib.wn_generate_chunk(plan, ONE, ONE, ONE, 3, 5, 4, 1, 1, C.byref(sp), ONE, ONE, BIG, None),
           lambda: lib.wn_generate_chunk(plan, ONE, None, ONE, 3, 20, 40, 1, 1, C.byref(sp), ONE, ONE, 8, None),
           lambda: lib.wn_generate_chunk(plan, ONE, None, ONE, 3, 20, 40, 1, 0, C.byref(sp), ONE, ONE, 8, None),
           lambda: lib.wn_generate_chunk(plan, None, None, ONE, 3, 20, 40, 1, 1, C.byref(sp), ONE, ONE, BIG, None))

  def answers():
    return [(c(), _msg(lib)) for c in calls]
  before = answers()
  assert all(rc == _lib.WN_E_INVALID for rc, _ in before)
  assert lib.wn_plan_arm_gen_frames(plan, _records(None, (64, 4 * D2, 3, 4, 5), None), 3) == _lib.WN_OK
  armed = answers()
  assert armed != before and b'runs past' in armed[3][1] and b'sliding window' in armed[4][1]
  assert lib.wn_plan_arm_gen_frames(plan, None, 0) == _lib.WN_OK
  assert answers() == before
