"""A row's own clock (semantics in include/wn_hip.h, the *_origin entry points) on the GPU.  Every
stochastic draw that reads a row's record uses the counter (stream, t - origin[row]).  The defining property: a request
admitted by admit_own_clock gives the same samples in any slot of any batch at any position -- from its first sample on
it is bit for bit model.generate(n, sample=prompt, ..., use_queues=True) of that request alone, from position 0.  Every
comparison is torch.equal; the networks, rows and admissions are those of test_gpu_sampling_rows.py and test_gpu_admit.py."""
import functools

import pytest
import torch

from test_gpu_parity import MODEL_CASES, O, dev, make_pair
from test_gpu_sampling_rows import MIX_ROWS, OFF, ROWS, ROWS_NO_P, SA, SC, _kw, _net
from test_gpu_admit import CHUNKS, _admissions_of, _form, _inputs, _rows_of

pytestmark = pytest.mark.gpu


def _diff(a, b):
  return (a != b).nonzero()[:4].tolist()


# ------------------------------------------------------------------------------------------
# 1. a sequence that begins at a position, on its own clock, is the sequence from position 0
# ------------------------------------------------------------------------------------------
NETS_BEGIN = [('cat_r64', True, None), ('cat_r64', False, None), ('mix_32', True, None), ('mix_32', False, None),
              ('r128', True, 'relay'), ('r128', True, 'one_workgroup')]


@functools.lru_cache(maxsize=None)
def _from_zero(name, queued, form):
  kw, model = _net(name)
  w, cond = _inputs(model, kw, 5, 12)
  args = dict(sample=w, use_queues=queued, stream=[0, 1, 2, 3, 4], **_kw(_rows_of(model, name)))
  with _form(form):
    return args, model.generation_session(start=0, **args).generate(11)


@pytest.mark.parametrize('q', [5, 37])
@pytest.mark.parametrize('name,queued,form', NETS_BEGIN, ids=lambda v: str(v))
def test_begin_at_a_position_on_its_own_clock_equals_position_0(name, queued, form, q):
  """test_begin_at_a_position_stochastic_chunks_equal_the_one_chunk shows that the two differ without own_clock."""
  kw, model = _net(name)
  args, want = _from_zero(name, queued, form)
  with _form(form):
    s = model.generation_session(start=q, own_clock=True, **args)
    assert s.position == q and s.origins == [q] * 5 and s.row_positions == [0] * 5
    got = torch.cat([s.generate(n) for n in (1, 1, 2, 7)], 1)
  assert s.position == q + 11 and s.row_positions == [11] * 5
  assert torch.equal(got, want), _diff(got, want)


# ------------------------------------------------------------------------------------------
# 2. the admission oracle: an admitted request is the request alone, from position 0
# ------------------------------------------------------------------------------------------
def _alone(model, n, nw, ncond, sid, ctl, **more):
  return model.generate(n, sample=nw, condition=ncond, use_queues=True, stream=[sid], **_kw([ctl]), **more)[0]


def _run_admissions(model, kw, rows, admissions, own, chunks=CHUNKS, B=5, seed=12, **more):
  """test_gpu_admit._check_admissions' scenario: a session of B rows in `chunks`, admission i after chunk i with
  admit_own_clock where own[i], else admit.  Returns (session, its samples, the samples without admissions, {row: (q, own, first sample, window,
  condition, stream id, controls)} of the row's present request, q the index of its first sample)."""
  w, cond = _inputs(model, kw, B, seed)
  args = dict(sample=w, condition=cond, use_queues=True, stream=list(range(B)), **_kw(rows), **more)
  total = sum(chunks)
  base = model.generation_session(**args).generate(total)
  s = model.generation_session(**args)
  pieces, req = [], {}
  for i, n in enumerate(chunks):
    pieces.append(s.generate(n))
    if i < len(admissions):
      slots, streams, ctl = admissions[i]
      nw, ncond = _inputs(model, kw, len(slots), 100 + i)
      prompt = torch.cat([torch.zeros(len(slots), 3, 1, device=dev()), nw], 1)
      pos = s.position
      first = (s.admit_own_clock if own[i] else s.admit)(slots, prompt, condition=ncond, stream=streams, **_kw(ctl))
      assert first.shape == (len(slots), 1, 1) and s.position == pos
      for j, b in enumerate(slots):
        req[b] = (pos - 1, own[i], first[j], nw[j:j + 1].contiguous(), None if ncond is None else ncond[j:j + 1].contiguous(),
                  streams[j], ctl[j])
  assert s.position == total
  return s, torch.cat(pieces, 1), base, req


def _check_rows(model, s, got, base, req, **more):
  """Every admitted request against its reference (own clock: model.generate of the request alone; session clock: its B = 1
  session begun at its position), every other sample against the session without admissions."""
  total = got.shape[1]
  for b in range(got.shape[0]):
    if b not in req:
      assert torch.equal(got[b], base[b]), (b, _diff(got[b], base[b]))
      continue
    q, own, first, nw, ncond, sid, ctl = req[b]
    assert torch.equal(got[b, :q + 1], base[b, :q + 1]), (b, 'before its replacement')
    if own:
      want = _alone(model, total - q, nw, ncond, sid, ctl, **more)
    else:
      want = model.generation_session(sample=nw, condition=ncond, use_queues=True, stream=[sid], start=q, **_kw([ctl]),
                                      **more).generate(total - q)[0]
    have = torch.cat([first, got[b, q + 1:]], 0)
    assert torch.equal(have, want), (b, q, own, _diff(have, want))
    assert s.origins[b] == (q if own else 0) and s.row_positions[b] == total - s.origins[b]


@pytest.mark.parametrize('name,form', [('cat_r64', None), ('cat_lpb3', None), ('cat_k3', None), ('cond', None), ('mix_64', None),
                                       ('r128', 'relay'), ('r128', 'one_workgroup')], ids=lambda v: str(v))
def test_admission_oracle_own_clock(name, form):
  """Admissions at positions 6 and 14.  ADMIT_CAT has a top_p row: until it is admitted cat_r64 draws in the head launch
  (tail 2), afterwards in the sampler launch; mix_64 and r128 draw in the head launch's tail 4 / the sampler launch."""
  kw, model = _net(name)
  with _form(form):
    s, got, base, req = _run_admissions(model, kw, _rows_of(model, name), _admissions_of(model, name), own=(True, True))
    assert sorted(req) == [0, 3, 4] and s.origins == [13, 0, 0, 5, 13]
    _check_rows(model, s, got, base, req)
  assert s.exact is False and model.generation_guard_trips == 0


# ------------------------------------------------------------------------------------------
# 3. independence of when, where and with whom
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cat_r64', 'mix_64'])
def test_a_request_draws_the_same_at_any_position_in_any_slot_of_any_batch(name):
  kw, model = _net(name)
  rows = _rows_of(model, name)
  ctl = (0.8, 10 if model.sampling_function == 'categorical' else 0, OFF, SC)
  nw, _ = _inputs(model, kw, 1, 77)
  takes = []
  for B, position, slot, seed in ((5, 6, 3, 12), (3, 14, 0, 31)):
    w, _ = _inputs(model, kw, B, seed)
    s = model.generation_session(sample=w, use_queues=True, stream=list(range(10, 10 + B)), **_kw(rows[:B]))
    s.generate(position)
    first = s.admit_own_clock(slot, nw, stream=[100], **_kw([ctl]))
    assert s.origins[slot] == position - 1
    takes.append(torch.cat([first[0], s.generate(4)[slot], s.generate(8)[slot]], 0))
  assert torch.equal(takes[0], takes[1]), _diff(takes[0], takes[1])
  assert torch.equal(takes[0], _alone(model, 13, nw, None, 100, ctl))


# ------------------------------------------------------------------------------------------
# 4. mixed clocks in one session
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,own', [('cat_r64', (True, False)), ('cat_r64', (False, True)), ('mix_64', (True, False))],
                         ids=lambda v: str(v))
def test_mixed_clocks_in_one_session(name, own):
  """One admission on its own clock, one on the session's: the second is section 32's property, a B = 1 session begun at
  start = position - 1.  (False, True): the first admission runs before the session has an origin array."""
  kw, model = _net(name)
  s, got, base, req = _run_admissions(model, kw, _rows_of(model, name), _admissions_of(model, name), own=own)
  assert s.origins == ([0, 0, 0, 5, 0] if own[0] else [13, 0, 0, 0, 13])
  assert s.row_positions == [24 - o for o in s.origins]
  _check_rows(model, s, got, base, req)
  # the two clocks do give different draws: row 3's request on the other clock is not this row
  q, own3, first, nw, ncond, sid, ctl = req[3]
  other = (model.generation_session(sample=nw, use_queues=True, stream=[sid], start=q, **_kw([ctl])).generate(24 - q)[0]
           if own3 else _alone(model, 24 - q, nw, None, sid, ctl))
  assert not torch.equal(torch.cat([first, got[3, q + 1:]], 0), other)


# ------------------------------------------------------------------------------------------
# 5. an origin array of zeros is the path without one
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,rows,queued', [('cat_r64', ROWS, True), ('cat_r64', ROWS_NO_P, True), ('cat_r64', ROWS, False),
                                              ('mix_64', MIX_ROWS, True), ('mix_32', MIX_ROWS, False)],
                         ids=['top_p_rows', 'top_p_off', 'top_p_rows_window', 'mix_64', 'mix_32_window'])
def test_zeros_are_the_path_without_origins(name, rows, queued):
  kw, model = _net(name)
  w, _ = _inputs(model, kw, 5, 12)
  args = dict(sample=w, use_queues=queued, stream=[0, 1, 2, 3, 4], **_kw(rows))
  want = model.generation_session(**args).generate(14)
  s = model.generation_session(start=0, own_clock=True, **args)
  assert s._origin is not None and s.origins == [0] * 5
  got = torch.cat([s.generate(n) for n in (1, 6, 7)], 1)
  assert torch.equal(got, want), _diff(got, want)
  s.reset()
  assert s.origins == [0] * 5 and torch.equal(s.generate(14), want)


# ------------------------------------------------------------------------------------------
# 6. deterministic=True ignores the origins
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cat_r64', 'mix_64'])
def test_deterministic_ignores_origins(name):
  kw, model = _net(name)
  rows, adm = _rows_of(model, name), _admissions_of(model, name)
  _, got, _, _ = _run_admissions(model, kw, rows, adm, own=(True, True), deterministic=True)
  _, want, _, _ = _run_admissions(model, kw, rows, adm, own=(False, False), deterministic=True)
  assert torch.equal(got, want), _diff(got, want)
  w, _ = _inputs(model, kw, 5, 12)
  args = dict(sample=w, use_queues=True, deterministic=True, stream=[0, 1, 2, 3, 4], **_kw(rows))
  a = model.generation_session(start=5, own_clock=True, **args).generate(9)
  assert torch.equal(a, model.generation_session(start=5, **args).generate(9))


# ------------------------------------------------------------------------------------------
# 7. the guard repeat keeps the clock
# ------------------------------------------------------------------------------------------
def test_guard_trip_at_an_own_clock_admission_repeats_it_with_the_same_origins():
  """The recipe of test_guard_trip_at_admission_repeats_it_in_exact_fp32 (causal/kernel = 6e5 everywhere, the session's
  rows begun from zero windows, the admitted window O.synthetic_waveform(1, rf, seed=9) with max |x[t] + x[t-1]| = 1.75, so
  |H[0]| reaches 1.05e6 in the admission's priming pass and far beyond the range limit of 30000), with stochastic draws
  and the session begun at start = 5: its priming pass sees zeros at any start, and the admission at position 6 gets the
  origin 5, which a repeat that dropped the origins would draw from counter (100, 5) instead of (100, 0)."""
  from wavenets_amd import _lib
  kw = dict(MODEL_CASES['cat_r64'])
  ocfg, params, model = make_pair(seed=11, bias_range=0.1, **kw)
  ws = [p.clone() for p in params]
  ck = model.variable_names.index('causal/kernel')
  ws[ck] = torch.full_like(ws[ck], 6.0e5)
  model.set_weights([w.numpy() for w in ws])
  w0 = torch.zeros(2, model.receptive_field, 1, device=dev())
  nw = O.synthetic_waveform(1, model.receptive_field, seed=9)
  assert 6.0e5 * float((nw[:, 1:] + nw[:, :-1]).abs().max()) >= 2 * _lib.lib().wn_range_limit()
  nw = nw.to(dev())
  with model.exact_fp32():
    want = model.generate(7, sample=nw, use_queues=True, stream=[100], seed=[SA])[0]
  assert model.generation_guard_trips == 0
  S = model.generation_session(sample=w0, use_queues=True, stream=[0, 1], start=5)
  S.generate(1)
  assert model.generation_guard_trips == 0 and S.exact is False
  first = S.admit_own_clock(1, nw, stream=[100], seed=[SA])
  assert model.generation_guard_trips == 1 and S.exact is True and S.origins == [0, 5]
  have = torch.cat([first[0], S.generate(3)[1], S.generate(3)[1]], 0)
  assert model.generation_guard_trips == 1 and S.position == 12 and S.row_positions == [12, 7]
  assert torch.equal(have, want), _diff(have, want)
  on_session_clock = model.generation_session(sample=nw, use_queues=True, stream=[100], seed=[SA], start=5)
  with model.exact_fp32():
    assert not torch.equal(have, on_session_clock.generate(7)[0])
