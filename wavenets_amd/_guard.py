"""What stands around a pass of the library: the range-guard protocol every user-facing call ends
with, and the two arm / run / disarm scopes.  Host code only; nothing here launches."""
from __future__ import annotations

import contextlib

from . import _lib


def guarded(model, run, tripped, skip=False, after_first=None, before_rerun=None, counter=None, count_first=False):
  """The range-guard protocol: ``run()``; if ``tripped()`` -- the site's host read of the pass's range flag -- says that
  the pass left the range of the split-precision kernels, ``run()`` again under ``model.exact_fp32()``.  Returns whether
  it ran again.

  skip: the site's condition under which nothing is checked; ``tripped`` is then never called (its read is the host
  synchronisation that ``range_check = False``, exact-fp32 mode and ``length == 0`` exist to avoid).
  after_first: queued behind the first run whether or not anything is checked (``call`` keeps its guard float there).
  before_rerun: the site's way back to the state in front of the first run.
  counter: the attribute of ``model`` that counts the reruns, or None; count_first: it is bumped ahead of
  ``before_rerun`` and the rerun (a rerun that raises is then counted), otherwise behind the rerun (it is then not)."""
  run()
  if after_first is not None:
    after_first()
  if skip or not tripped():
    return False
  if counter is not None and count_first:
    setattr(model, counter, getattr(model, counter) + 1)
  if before_rerun is not None:
    before_rerun()
  with model.exact_fp32():
    run()
  if counter is not None and not count_first:
    setattr(model, counter, getattr(model, counter) + 1)
  return True


@contextlib.contextmanager
def row_weights(plan, weights, rows):
  """The ``(B, T)`` row weights of ``sample_weight`` armed in the plan for the passes of the scope and disarmed whatever
  happens (``weights`` None: nothing is armed, nothing disarmed)."""
  L = _lib.lib()
  try:
    if weights is not None:
      _lib.check(L.wn_plan_arm_row_weights(plan, _lib.ptr(weights), rows))
    yield
  finally:
    if weights is not None:
      L.wn_plan_arm_row_weights(plan, None, 0)


@contextlib.contextmanager
def kept_pass(model, frames, mode=None, drop_state=None):
  """The state of a pass that was kept, for the scope, whatever the calling thread's is now: its condition frames armed,
  its math mode (knob 1; None: the caller's) and its dropout (rate, step) (None: as armed); what the model holds is
  back whatever happens."""
  L = _lib.lib()
  prev = L.wn_debug_value(1)
  if mode is not None:
    L.wn_debug_set(1, mode)
  if drop_state is not None:
    model._set_dropout_state(*drop_state)
  try:
    model._arm_frames(frames)
    yield
  finally:
    if mode is not None:
      L.wn_debug_set(1, prev)
    if drop_state is not None:
      model._set_dropout_state(model.dropout, model._drop_armed_step)
    model._arm_frames(0)
