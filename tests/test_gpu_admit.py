"""Admission into a running batch (semantics in include/wn_hip.h, wn_generate_rows_begin /
wn_generate_admit) on the GPU.  A sequence may begin at a position other than 0, and GenerationSession.admit primes new
requests alone, at the session's time, and moves their state rows into rows of the session.  The defining property:
an admitted row, from its first sample on, is bit for bit a session of B = 1 begun with start = position - 1 from the
request's own window, condition and record, and every other row is what it is without the admission.  Every comparison
is torch.equal; the networks and rows are those of test_gpu_sampling_rows.py."""
import contextlib
import functools

import pytest
import torch

from test_gpu_parity import MODEL_CASES, O, dev, make_pair
from test_gpu_sampling_rows import MIX_ROWS, OFF, ROWS, ROWS_NO_P, SA, SB, SC, _kw, _net

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _form(form):
  """The 128-channel chain as the relay over one workgroup per block, or as one workgroup (knob 2)."""
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(2, 1 if form == 'one_workgroup' else 0)
  try:
    yield
  finally:
    _lib.lib().wn_debug_set(2, 0)


def _inputs(model, kw, B, seed):
  """B windows and, on a conditioned net, B conditions, both drawn from `seed`."""
  w = O.synthetic_waveform(B, model.receptive_field, seed=seed).to(dev())
  cond = None
  if kw.get('conditioning') is not None:
    cond = torch.rand(B, kw['cond_inputs'], generator=torch.Generator().manual_seed(seed)).to(dev())
  return w, cond


def _rows_of(model, name):
  if model.sampling_function != 'categorical':
    return MIX_ROWS
  return ROWS_NO_P if name == 'cond' else ROWS


NETS_BEGIN = [('cat_r64', True, None), ('cat_r64', False, None), ('cat_lpb3', True, None), ('cat_k3', True, None),
              ('cond', True, None), ('mix_64', True, None), ('r128', True, 'relay'), ('r128', True, 'one_workgroup')]


# ------------------------------------------------------------------------------------------
# 1. a sequence that begins at a position: deterministic samples do not depend on it
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _det_reference(name, queued, form):
  kw, model = _net(name)
  w, cond = _inputs(model, kw, 3, 4)
  args = dict(sample=w, condition=cond, use_queues=queued, deterministic=True, stream=[7, 8, 9])
  with _form(form):
    return args, model.generation_session(start=0, **args).generate(20)


@pytest.mark.parametrize('q', [5, 37])
@pytest.mark.parametrize('name,queued,form', NETS_BEGIN, ids=lambda v: str(v))
def test_begin_at_a_position_deterministic(name, queued, form, q):
  """The arg max / mode sequence of a window is the same at every position: this pins the capture origin of xin and of
  every ring (window index t at slot (t + q) % nslots), tau and the window parity of the steps behind it.  5 and 37 are
  odd, and no multiple of 3, 9 or 17 (the rings of dilation 2, 8 and 16) or 7 (kernel size 3, dilation 3)."""
  kw, model = _net(name)
  args, want = _det_reference(name, queued, form)
  with _form(form):
    s = model.generation_session(start=q, **args)
    assert s.position == q
    got = [s.generate(n) for n in (1, 6, 13)]
    assert s.position == q + 20
  got = torch.cat(got, 1)
  assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()


# ------------------------------------------------------------------------------------------
# 2. ... and stochastic ones do, through the counter (stream, t) alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q', [5, 37])
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'mix_32'])
def test_begin_at_a_position_stochastic_chunks_equal_the_one_chunk(name, queued, q):
  kw, model = _net(name)
  rows = _rows_of(model, name)
  w, cond = _inputs(model, kw, 5, 12)
  args = dict(sample=w, use_queues=queued, stream=[0, 1, 2, 3, 4], **_kw(rows))
  one = model.generation_session(start=q, **args).generate(11)
  s = model.generation_session(start=q, **args)
  pieces = torch.cat([s.generate(n) for n in (1, 1, 2, 7)], 1)
  assert s.position == q + 11
  assert torch.equal(pieces, one), (pieces != one).nonzero()[:4].tolist()
  at0 = model.generation_session(start=0, **args).generate(11)
  for b in range(5):
    assert not torch.equal(one[b], at0[b]), b


# ------------------------------------------------------------------------------------------
# 3. the admission oracle
# ------------------------------------------------------------------------------------------
CHUNKS = (6, 8, 10)
# (slots, stream ids, controls (T, top_k, top_p, seed)) of the admissions after chunk 1 and after chunk 2
ADMIT_CAT = [([3], [100], [(0.8, 10, OFF, SC)]), ([4, 0], [101, 102], [(1.2, 0, 0.7, SA), (0.9, 30, OFF, SB)])]
ADMIT_CAT_NO_P = [([3], [100], [(0.8, 10, OFF, SC)]), ([4, 0], [101, 102], [(1.2, 0, OFF, SA), (0.9, 30, OFF, SB)])]
ADMIT_MIX = [([3], [100], [(0.8, 0, OFF, SC)]), ([4, 0], [101, 102], [(1.2, 0, OFF, SA), (0.6, 0, OFF, SB)])]


def _admissions_of(model, name):
  if model.sampling_function != 'categorical':
    return ADMIT_MIX
  return ADMIT_CAT_NO_P if name == 'cond' else ADMIT_CAT


def _check_admissions(model, kw, rows, admissions, chunks=CHUNKS, B=5, seed=12, slots_arg=lambda slots: slots):
  """A session of B rows in `chunks`, with admission i after chunk i; every admitted request against its own B = 1
  session, every other sample against the same session without admissions.  Returns the session."""
  w, cond = _inputs(model, kw, B, seed)
  args = dict(sample=w, condition=cond, use_queues=True, stream=list(range(B)), **_kw(rows))
  total = sum(chunks)
  base = model.generation_session(**args).generate(total)
  s = model.generation_session(**args)
  pieces, firsts, since = [], {}, {}       # since[b]: the position row b's present request made its first sample at
  for i, n in enumerate(chunks):
    pieces.append(s.generate(n))
    if i < len(admissions):
      slots, streams, ctl = admissions[i]
      nw, ncond = _inputs(model, kw, len(slots), 100 + i)
      # (a longer prompt than the receptive field: its last receptive_field samples are the window)
      prompt = torch.cat([torch.zeros(len(slots), 3, 1, device=dev()), nw], 1)
      pos = s.position
      first = s.admit(slots_arg(slots), prompt, condition=ncond, stream=streams, **_kw(ctl))
      assert first.shape == (len(slots), 1, 1) and s.position == pos
      for j, b in enumerate(slots):
        since[b] = pos - 1
        firsts[b] = (first[j], nw[j:j + 1].contiguous(), None if ncond is None else ncond[j:j + 1].contiguous(), streams[j], ctl[j])
  got = torch.cat(pieces, 1)
  assert s.position == total
  for b in range(B):
    if b not in since:
      assert torch.equal(got[b], base[b]), (b, (got[b] != base[b]).nonzero()[:4].tolist())
      continue
    q = since[b]
    assert torch.equal(got[b, :q + 1], base[b, :q + 1]), (b, 'before its replacement')
    first, nw, ncond, sid, ctl = firsts[b]
    alone = model.generation_session(sample=nw, condition=ncond, use_queues=True, stream=[sid], start=q, **_kw([ctl]))
    want = alone.generate(total - q)[0]
    have = torch.cat([first, got[b, q + 1:]], 0)
    assert torch.equal(have, want), (b, q, (have != want).nonzero()[:4].tolist())
    assert not torch.equal(have, base[b, q:]), (b, 'the admission changed nothing')
  return s


@pytest.mark.parametrize('name,form', [('cat_r64', None), ('cat_small_fused', None), ('cat_lpb3', None), ('cond', None),
                                       ('mix_64', None), ('mol', None), ('r128', 'relay'), ('r128', 'one_workgroup')],
                         ids=lambda v: str(v))
def test_admission_oracle(name, form):
  """Admissions at positions 6 and 14: the priming draws are samples 5 and 13 -- odd, no multiple of 3 or 9."""
  kw, model = _net(name)
  with _form(form):
    s = _check_admissions(model, kw, _rows_of(model, name), _admissions_of(model, name))
  assert s.exact is False and model.generation_guard_trips == 0
  with pytest.raises(RuntimeError, match='reset after admit'):
    s.reset()


# ------------------------------------------------------------------------------------------
# 4. the union of the flags changes with the admission
# ------------------------------------------------------------------------------------------
def test_admitting_a_top_p_row_moves_every_row_to_the_sampler_launch():
  """No row of ROWS_NO_P has top_p on, so the five rows draw in the head launch; the admitted request has, and from then on
  the step takes the sampler launch for every row.  The untouched rows stay bit for bit (they are compared with the
  session that never left the head launch)."""
  kw, model = _net('cat_r64')
  s = _check_admissions(model, kw, ROWS_NO_P, [([2], [100], [(0.9, 0, 0.8, SC)])], chunks=(6, 8))
  assert s._sampling.flags == 3


# ------------------------------------------------------------------------------------------
# 5. the second workgroup / tile
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cat_r64', 'r128'])
def test_admission_into_the_second_workgroup_at_33_utterances(name):
  kw, model = _net(name)
  rows = [(1.0, 0, OFF, SA)] * 33
  rows[0], rows[31], rows[32] = (0.7, 0, OFF, SB), (1.3, 20, OFF, SC), (0.5, 0, OFF, SA)
  _check_admissions(model, kw, rows, [([32, 0], [100, 101], [(0.8, 10, OFF, SC), (1.2, 0, OFF, SB)])], chunks=(6, 8), B=33,
                    slots_arg=lambda slots: torch.tensor(slots))


# ------------------------------------------------------------------------------------------
# 6. exact fp32
# ------------------------------------------------------------------------------------------
def test_admission_oracle_in_exact_fp32():
  kw, model = _net('cat_r64')
  with model.exact_fp32():
    s = _check_admissions(model, kw, ROWS, ADMIT_CAT)
  assert s.exact is True and model.generation_guard_trips == 0


# ------------------------------------------------------------------------------------------
# 7. a range-guard trip in the admission's priming pass
# ------------------------------------------------------------------------------------------
def test_guard_trip_at_admission_repeats_it_in_exact_fp32():
  """The set-up of test_guard_trip_in_a_later_chunk_restores_the_state (causal/kernel = 6e5 everywhere): the session's two
  rows have zero windows, so its priming pass (chunk 1) stays in range.  The admitted window is not zero: the input conv
  of ITS priming pass gives |H[0]| = 6e5 * |x[t] + x[t-1]| (+ a bias below 0.1), far beyond the range limit of 30000 --
  for O.synthetic_waveform(1, 17, seed=9) max |x[t] + x[t-1]| is 1.75, i.e. |H[0]| up to 1.05e6 (the window alone decides
  it on the CPU; no generate_naive run is needed for the first activation).  So S trips at the admission, repeats it in
  exact fp32 and stays there; R is told to run the admission and everything behind it in exact fp32."""
  from wavenets_amd import _lib
  kw = dict(MODEL_CASES['cat_r64'])
  ocfg, params, model = make_pair(seed=11, bias_range=0.1, **kw)
  ws = [p.clone() for p in params]
  ck = model.variable_names.index('causal/kernel')
  ws[ck] = torch.full_like(ws[ck], 6.0e5)
  model.set_weights([w.numpy() for w in ws])
  w0 = torch.zeros(2, model.receptive_field, 1, device=dev())
  nw = O.synthetic_waveform(1, model.receptive_field, seed=9)
  reach = 6.0e5 * float((nw[:, 1:] + nw[:, :-1]).abs().max())
  if reach < 2 * _lib.lib().wn_range_limit():
    pytest.skip(f'the priming pass of this window stays in range (|H[0]| up to {reach:g})')
  nw = nw.to(dev())
  args = dict(sample=w0, deterministic=True, use_queues=True, stream=[0, 1])
  R = model.generation_session(**args)
  r = [R.generate(1)]
  with model.exact_fp32():
    ra = R.admit(1, nw, stream=[100])
    r += [R.generate(3), R.generate(3)]
  assert model.generation_guard_trips == 0 and R.exact is False
  S = model.generation_session(**args)
  s = [S.generate(1)]
  assert model.generation_guard_trips == 0 and S.exact is False
  sa = S.admit(1, nw, stream=[100])
  assert model.generation_guard_trips == 1 and S.exact is True
  s += [S.generate(3), S.generate(3)]
  assert model.generation_guard_trips == 1 and S.position == 7
  r, s = torch.cat(r, 1), torch.cat(s, 1)
  assert torch.isfinite(s).all() and torch.isfinite(sa).all() and torch.isfinite(r).all()
  assert torch.equal(sa, ra) and torch.equal(s, r), (s != r).nonzero()[:4].tolist()


# ------------------------------------------------------------------------------------------
# 8. the surface
# ------------------------------------------------------------------------------------------
def test_admit_and_start_surface():
  kw = dict(MODEL_CASES['cat_small_fused'])
  ocfg, params, model = make_pair(seed=7, bias_range=0.3, **kw)
  rf = model.receptive_field
  w = O.synthetic_waveform(3, rf, seed=4).to(dev())
  nw = O.synthetic_waveform(2, rf, seed=5).to(dev())
  args = dict(sample=w, use_queues=True, stream=[0, 1, 2])
  # start
  for bad in (-1, 1.5, True, None):
    with pytest.raises(ValueError, match='start must be'):
      model.generation_session(start=bad, **args)
  with pytest.raises(ValueError, match='start > 0 needs'):
    model.generation_session(sample=w, use_queues=True, seed=5, start=4)
  s = model.generation_session(start=9, **args)
  assert s.position == 9
  a = s.generate(4)
  assert s.position == 13
  s.reset()
  assert s.position == 9
  assert torch.equal(s.generate(4), a) and s.position == 13
  # admit: what the session must be
  with pytest.raises(RuntimeError, match='use_queues'):
    sw = model.generation_session(sample=w, use_queues=False, stream=[0, 1, 2])
    sw.generate(2)
    sw.admit(0, nw[:1], stream=[9])
  with pytest.raises(RuntimeError, match='per-row controls'):
    sc = model.generation_session(sample=w, use_queues=True, seed=5)
    sc.generate(2)
    sc.admit(0, nw[:1], stream=[9])
  for start in (0, 9):
    fresh = model.generation_session(start=start, **args)
    with pytest.raises(RuntimeError, match='position'):
      fresh.admit(0, nw[:1], stream=[9])
  # ... and its arguments; a refused admission leaves the session as it was
  for slots, word in (([0, 0], 'duplicate'), ([0, 3], r'slots\[1\]'), (-1, r'slots\[0\]'), (True, r'slots\[0\]'), ([], 'slots'),
                      ([0.5, 1], r'slots\[0\]')):
    with pytest.raises(ValueError, match=word):
      s.admit(slots, nw, stream=[8, 9])
  with pytest.raises(ValueError, match='stream is required'):
    s.admit([0, 1], nw)
  with pytest.raises(ValueError, match='stream has 1 entries for a batch of 2'):
    s.admit([0, 1], nw, stream=[9])
  with pytest.raises(ValueError, match='sample must have shape'):
    s.admit([0, 1], nw[:1], stream=[8, 9])
  with pytest.raises(ValueError, match='sample must have shape'):
    s.admit([0, 1], nw[:, 1:], stream=[8, 9])
  with pytest.raises(ValueError, match='row 1: temperature'):
    s.admit([0, 1], nw, stream=[8, 9], temperature=[1.0, 0.0])
  with pytest.raises(ValueError, match='row 0: top_k'):
    s.admit([2, 1], nw, stream=[8, 9], top_k=[-1, 0])
  with pytest.raises(ValueError, match='condition must have shape'):
    s.admit([0, 1], nw, stream=[8, 9], condition=torch.zeros(2, 4))
  assert s.position == 13 and s._admitted is False and s._sampling.flags == 0
  b = s.generate(3)
  # a good one: position stays, the table and its flags follow, reset is over
  first = s.admit([2, 0], nw, stream=[8, 9], temperature=[0.7, 1.0], top_p=[1.0, 0.9])
  assert first.shape == (2, 1, 1) and s.position == 16
  assert s._sampling.flags == 3 and [r.stream for r in s._sampling.host] == [9, 1, 8]
  assert [e.temperature for e in s._sampling.entries] == [1.0, 1.0, float(torch.tensor(0.7))]
  assert len(s._scratch) == 1 and 2 in s._scratch
  s.admit(1, nw[1:], stream=[3])
  assert sorted(s._scratch) == [1, 2]
  c = s.generate(2)
  assert s.position == 18 and c.shape == (3, 2, 1)
  with pytest.raises(RuntimeError, match='reset after admit'):
    s.reset()
  # a failed session, and changed weights (the text of generate)
  s._failed = True
  with pytest.raises(RuntimeError, match='earlier chunk failed'):
    s.admit(0, nw[:1], stream=[9])
  s._failed = False
  model.set_weights(model.get_weights())
  with pytest.raises(RuntimeError, match='weights changed'):
    s.admit(0, nw[:1], stream=[9])
  # a conditioned net asks for the condition
  ckw = dict(MODEL_CASES['cond'])
  cmodel = make_pair(seed=7, bias_range=0.3, **ckw)[2]
  cw = O.synthetic_waveform(2, cmodel.receptive_field, seed=4).to(dev())
  cs = cmodel.generation_session(sample=cw, condition=torch.rand(2, ckw['cond_inputs']), use_queues=True, stream=[0, 1])
  cs.generate(2)
  with pytest.raises(ValueError, match='Conditioning must be provided'):
    cs.admit(0, cw[:1], stream=[5])
  with pytest.raises(ValueError, match='condition must have shape'):
    cs.admit(0, cw[:1], stream=[5], condition=torch.rand(2, ckw['cond_inputs']))
