"""CPU-only checks of what stands around a pass in the Python driver: the one range-guard protocol
(wavenets_amd/_guard.py::guarded) with recording stubs, the scope that arms the row weights, the function that reads the
two guard words of a generation pass, and the choice of the generation entry point.  wn_debug_set / wn_debug_value and the
arming calls are host only; objects are made with ``__new__`` and the few attributes a helper reads."""
import ctypes as C

import pytest
import torch

from wavenets_amd import WaveNet, _guard, _lib, generation
from test_cabi_cpu import _cfg, _plan as _plan_of
from test_sample_weight_cabi_cpu import _eval
from test_sampling_cabi_cpu import lib  # noqa: F401  (module fixture)

COUNTER = 'generation_guard_trips'


class _Site:
  """A guard site made of recording stubs: what ran, in which order, under which value of knob 1."""

  def __init__(self, lib, trips, rerun_raises=False):
    self.lib, self.trips, self.rerun_raises = lib, trips, rerun_raises
    self.events, self.model = [], WaveNet.__new__(WaveNet)
    setattr(self.model, COUNTER, 7)

  def run(self):
    self.events.append(('run', self.lib.wn_debug_value(1), getattr(self.model, COUNTER)))
    if self.rerun_raises and len(self.events) > 1:
      raise KeyError('rerun')

  def tripped(self):
    self.events.append('tripped')
    return self.trips

  def before_rerun(self):
    self.events.append(('before_rerun', self.lib.wn_debug_value(1), getattr(self.model, COUNTER)))

  def never(self):
    raise AssertionError('the host read was made although the skip condition holds')


@pytest.fixture(params=[0, 1])
def knob(lib, request, monkeypatch):
  """Knob 1 at a previous value of 0 and of 1, its writes recorded; back to 0 afterwards."""
  lib.wn_debug_set(1, request.param)
  writes, real = [], lib.wn_debug_set
  monkeypatch.setattr(lib, 'wn_debug_set', lambda k, v: (writes.append((k, v)), real(k, v))[1])
  yield request.param, writes
  real(1, 0)


def test_a_pass_in_range_runs_once_and_writes_nothing(lib, knob):
  prev, writes = knob
  s = _Site(lib, trips=False)
  assert _guard.guarded(s.model, s.run, s.tripped, before_rerun=s.before_rerun, counter=COUNTER) is False
  assert s.events == [('run', prev, 7), 'tripped']
  assert getattr(s.model, COUNTER) == 7 and writes == [] and lib.wn_debug_value(1) == prev


@pytest.mark.parametrize('count_first', [False, True])
def test_a_tripped_pass_runs_again_in_exact_fp32(lib, knob, count_first):
  prev, writes = knob
  s = _Site(lib, trips=True)
  assert _guard.guarded(s.model, s.run, s.tripped, before_rerun=s.before_rerun, counter=COUNTER,
                        count_first=count_first) is True
  counted = 8 if count_first else 7                # what the hook and the rerun see
  assert s.events == [('run', prev, 7), 'tripped', ('before_rerun', prev, counted), ('run', 1, counted)]
  assert getattr(s.model, COUNTER) == 8
  assert writes == [(1, 1), (1, prev)] and lib.wn_debug_value(1) == prev


def test_after_first_is_queued_behind_the_first_run_only(lib, knob):
  prev, _ = knob
  for skip in (False, True):
    s = _Site(lib, trips=True)
    assert _guard.guarded(s.model, s.run, s.never if skip else s.tripped, skip=skip,
                          after_first=lambda: s.events.append('after_first')) is (not skip)
    assert s.events[:2] == [('run', prev, 7), 'after_first'] and s.events.count('after_first') == 1
    assert getattr(s.model, COUNTER) == 7          # no counter named: none bumped


@pytest.mark.parametrize('count_first', [False, True])
def test_a_rerun_that_raises_leaves_the_knob_restored_and_the_count_where_its_placement_says(lib, knob, count_first):
  prev, writes = knob
  s = _Site(lib, trips=True, rerun_raises=True)
  with pytest.raises(KeyError, match='rerun'):
    _guard.guarded(s.model, s.run, s.tripped, before_rerun=s.before_rerun, counter=COUNTER, count_first=count_first)
  assert [e[0] for e in s.events if e != 'tripped'] == ['run', 'before_rerun', 'run']
  assert getattr(s.model, COUNTER) == (8 if count_first else 7)
  assert writes == [(1, 1), (1, prev)] and lib.wn_debug_value(1) == prev


def test_the_skip_condition_spares_the_host_read(lib, knob):
  prev, writes = knob
  s = _Site(lib, trips=True)
  assert _guard.guarded(s.model, s.run, s.never, skip=True, before_rerun=s.never, counter=COUNTER) is False
  assert s.events == [('run', prev, 7)] and getattr(s.model, COUNTER) == 7 and writes == []


# ------------------------------------------------------------------------------------------ row weights
@pytest.fixture
def plan(lib):
  p = C.c_void_p(_plan_of(lib, _cfg(blocks=3, channels=32, skip_channels=32, dilation_bound=4, final_layers_channels=[32])))
  assert p.value, lib.wn_last_error_string()
  yield p
  lib.wn_plan_arm_row_weights(p, None, 0)
  lib.wn_plan_destroy(p)


def _armed(lib, plan):
  """As tests/test_sample_weight_cabi_cpu.py observes it: weights armed for 10 rows stop a (2, 16) pass at its row check,
  in front of the workspace check that stops it otherwise; nothing reaches the device."""
  assert _eval(lib, plan, 2, 16, 0) == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert ('weights' in msg) != ('workspace' in msg), msg
  return 'weights' in msg


@pytest.mark.parametrize('body_raises', [False, True])
def test_row_weights_are_armed_for_the_body_and_disarmed_whatever_happens(lib, plan, body_raises):
  weights, seen = torch.zeros(10), []
  try:
    with _guard.row_weights(plan, weights, 10):
      seen.append(_armed(lib, plan))
      if body_raises:
        raise KeyError('body')
  except KeyError:
    assert body_raises
  assert seen == [True] and not _armed(lib, plan)


def test_no_row_weights_arm_nothing_and_a_refused_arming_raises_disarmed(lib, plan):
  with _guard.row_weights(plan, None, 10):
    assert not _armed(lib, plan)
  with pytest.raises(ValueError, match='0'):
    with _guard.row_weights(plan, torch.zeros(10), 0):
      raise AssertionError('the body ran behind a refused arming')
  assert not _armed(lib, plan)


# ------------------------------------------------------------------------------------------ generation guard words
def _words(guard, watchdog):
  return torch.cat([torch.tensor([guard], dtype=torch.float32), torch.tensor([watchdog], dtype=torch.int32).view(torch.float32)])


def test_guard_words(lib):
  assert generation._guard_words(_words(0.0, 0), 'call') is False
  assert generation._guard_words(_words(1e9, 0), 'call') is True
  assert generation._guard_words(_words(float('nan'), 0), 'chunk') is True        # not (g < limit)
  limit = lib.wn_range_limit()
  assert generation._guard_words(_words(limit, 0), 'call') is True and limit > 0
  for noun in ('call', 'chunk'):
    for guard in (0.0, 1e9):                       # the watchdog is looked at ahead of the guard
      with pytest.raises(RuntimeError) as e:
        generation._guard_words(_words(guard, 3), noun)
      assert str(e.value) == generation._RELAY_GAVE_UP.format(3, noun)
      assert 'gave up waiting' in str(e.value) and f'of this {noun} are invalid' in str(e.value)
  marked = []
  with pytest.raises(RuntimeError):
    generation._guard_words(_words(0.0, 1), 'chunk', lambda: marked.append(1))
  assert marked == [1] and generation._guard_words(_words(0.0, 0), 'chunk', lambda: marked.append(2)) is False and marked == [1]


# ------------------------------------------------------------------------------------------ generation entry point
class _Rows:
  flags = 5


@pytest.mark.parametrize('phase,rows,origin,name,args', [
    ('call', False, False, 'wn_generate_sampled', 'abcde' + 'gh' + 'S' + 'yz'),       # no `first`
    ('call', True, False, 'wn_generate_rows_chunk', 'abcdefgh' + 'R5' + 'yz'),
    ('chunk', False, False, 'wn_generate_chunk', 'abcdefgh' + 'S' + 'yz'),
    ('begin', False, False, 'wn_generate_chunk', 'abcdefgh' + 'S' + 'yz'),
    ('chunk', True, False, 'wn_generate_rows_chunk', 'abcdefgh' + 'R5' + 'yz'),
    ('begin', True, False, 'wn_generate_rows_begin', 'abcdefgh' + 'R5' + 'yz'),
    ('chunk', True, True, 'wn_generate_rows_chunk_origin', 'abcdefgh' + 'R5O' + 'yz'),
    ('begin', True, True, 'wn_generate_rows_begin_origin', 'abcdefgh' + 'R5O' + 'yz'),
    ('admit', True, False, 'wn_generate_admit', 'abcdefgh' + 'R5' + 'yz'),
    ('admit', True, True, 'wn_generate_admit_origin', 'abcdefgh' + 'R5O' + 'yz'),
])
def test_generation_entry(lib, monkeypatch, phase, rows, origin, name, args):
  """Every combination names the entry the three sites named before, with the controls between head and tail."""
  monkeypatch.setattr(_lib, 'ptr', lambda t: t)                  # the stand-ins are their own pointers
  monkeypatch.setattr(generation.C, 'byref', lambda s: 'S')
  entry, got = generation._generation_entry(phase, tuple('abcdefgh'), _Rows if rows else object(), 'R' if rows else None,
                                            'O' if origin else None, tuple('yz'))
  assert entry.__name__ == name and entry is getattr(lib, name)
  assert ''.join(str(a) for a in got) == args
