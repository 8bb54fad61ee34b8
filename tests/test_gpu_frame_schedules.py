"""Frame schedules per request in queued generation: a request admitted into a session on a frame
schedule keeps its own frames, counted from its own first sample; the rows' frames are advanced inside a chunk by the copy
kernel, so a chunk is one call whatever boundaries it crosses.  The nets of tests/test_gpu_local_cond_generation.py (r64:
the chain kernels, r128: the relay) and two more of the same size: 48 channels (one launch per block) and a logistic
mixture head.  B = 3, hop 5 and 32, 3 or 4 frames.  Every comparison is torch.equal."""
import functools

import pytest
import torch

import local_reference as LR
from test_gpu_local_cond_generation import _model as _lr_model
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

B, CIN = LR.GEN_B, 3
MORE_NETS = {
    'b48': dict(blocks=3, channels=48, skip_channels=64, dilation_bound=4, final_layers_channels=[64], activation='relu',
                mapping_layers=[8], mapping_activation='tanh', bits=6),
    'mol': dict(blocks=3, channels=64, skip_channels=64, dilation_bound=4, final_layers_channels=[64, 64],
                activation='leaky_relu', num_mixtures=4, sampling_function='logistic', bits=8),
}
NETS = list(LR.GEN_NETS) + list(MORE_NETS)
STREAM = 40                                    # the admitted request's Philox stream
# per hop: the session's position at the admission (mid-frame), the two chunks behind it, the position on a session boundary
PLAN = {5: (7, 3, 6, 10), 32: (45, 25, 45, 64)}


@functools.lru_cache(maxsize=None)
def _pair(name):
  """(the local model, the global model with the same weights)."""
  if name in LR.GEN_NETS:
    return _lr_model(name), _lr_model(name, 'global')
  from wavenets_amd import WaveNet
  local = WaveNet(**MORE_NETS[name], conditioning='local', device=dev(), seed=31)
  local.build([(1, 8, 1), (1, 2, CIN)])
  glob = WaveNet(**MORE_NETS[name], conditioning='global', device=dev(), seed=31)
  glob.build([(1, 8, 1), (1, CIN)])
  # (a (1, cin, w) mapping kernel and a (cin, w) one hold the same floats in the same order)
  glob.set_weights([w.reshape(g.shape) for w, g in zip(local.get_weights(), glob.get_weights())])
  return local, glob


@functools.lru_cache(maxsize=None)
def _inputs(name, F=4):
  """The session's prompts (B, RF, 1) and frames (B, F, Cin); a request's prompt (1, RF, 1) and frames (1, 3, Cin)."""
  rf = _pair(name)[0].receptive_field
  g = torch.Generator().manual_seed(77)
  rnd = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).to(dev())
  return rnd(B, rf, 1), rnd(B, F, CIN), rnd(1, rf, 1), rnd(1, 3, CIN)


def _session_kw(name, hop, **more):
  w, fr, _, _ = _inputs(name)
  return dict(sample=w, condition=fr, hop=hop, use_queues=True, seed=[5, 6, 7], stream=[0, 1, 2], **more)


def _request_kw(more):
  return dict(stream=[STREAM], **({} if more.get('deterministic') else dict(temperature=0.8)))


@pytest.mark.parametrize('variant,slot', [('mid', 0), ('mid', 2), ('boundary', 2), ('deterministic', 0), ('exact', 2)])
@pytest.mark.parametrize('hop', [5, 32])
@pytest.mark.parametrize('name', NETS)
def test_an_admitted_request_keeps_its_own_frames(name, hop, variant, slot):
  """admit_own_clock with (1, 3, Cin) frames into a session of 4 frames that stands mid-frame (or on a boundary): the two
  chunks behind it cross boundaries of both schedules, which do not coincide.  The admitted row is model.generate of the
  request alone; the other rows are the session without the admission."""
  import contextlib
  local, _ = _pair(name)
  _, _, prompt, req = _inputs(name)
  p0, c1, c2, on = PLAN[hop]
  if variant == 'boundary':
    p0, c2 = on, c2 if hop == 5 else 38
  more = dict(deterministic=True) if variant == 'deterministic' else {}
  with (local.exact_fp32() if variant == 'exact' else contextlib.nullcontext()):
    base = local.generation_session(**_session_kw(name, hop, **more)).generate(p0 + c1 + c2)
    s = local.generation_session(**_session_kw(name, hop, **more))
    a = s.generate(p0)
    first = s.admit_own_clock(slot, prompt, condition=req, **_request_kw(more))
    b, c = s.generate(c1), s.generate(c2)
    alone = local.generate(1 + c1 + c2, sample=prompt, condition=req, hop=hop, use_queues=True, **more, **_request_kw(more))
    held = local.generate(1 + c1 + c2, sample=prompt, condition=req[:, :1], use_queues=True, **more, **_request_kw(more))
  assert s.position == p0 + c1 + c2 and (s.exact or variant != 'exact')
  got = torch.cat([a, b, c], 1)
  row = torch.cat([first[0], b[slot], c[slot]], 0)
  assert torch.equal(row, alone[0]), (row != alone[0]).nonzero()[:4].tolist()
  for r in range(B):
    if r != slot:
      assert torch.equal(got[r], base[r]), r
  assert torch.equal(got[slot, :p0], base[slot, :p0])
  if hop == 32 and name in LR.GEN_NETS and variant != 'deterministic':
    assert not torch.equal(alone, held)                   # the request's frames matter (71 or 64 stochastic draws)


@pytest.mark.parametrize('hop', [5, 32])
@pytest.mark.parametrize('name', NETS)
def test_a_plain_admission_with_frames_is_the_request_begun_alone_at_that_position(name, hop):
  """admit draws on the session's clock, and the frames still count from the request's own first sample, position - 1: the
  row is a B = 1 session begun with start = position - 1 from the request's arguments and frames."""
  local, _ = _pair(name)
  _, _, prompt, req = _inputs(name)
  p0, c1, c2, _ = PLAN[hop]
  s = local.generation_session(**_session_kw(name, hop))
  s.generate(p0)
  first = s.admit([1], prompt, condition=req, stream=[STREAM], temperature=0.8)
  b, c = s.generate(c1), s.generate(c2)
  one = local.generation_session(sample=prompt, condition=req, hop=hop, use_queues=True, stream=[STREAM], temperature=0.8,
                                 start=p0 - 1).generate(1 + c1 + c2)
  assert torch.equal(torch.cat([first[0], b[1], c[1]], 0), one[0])


@pytest.mark.parametrize('hop', [5, 32])
@pytest.mark.parametrize('name', NETS)
def test_a_whole_sequence_is_one_chunk_and_no_conditioning_phase(name, hop, monkeypatch):
  from wavenets_amd import _lib
  from wavenets_amd.generation import GenerationSession
  local, _ = _pair(name)
  w, fr, _, _ = _inputs(name)
  kw = dict(sample=w, condition=fr, hop=hop, use_queues=True, seed=7)
  total = fr.shape[1] * hop
  pieces, left, k = [], total, 0
  s = local.generation_session(**kw)
  while left > 0:                                         # 3, 7, 4, 11, ...: no size divides hop = 5 or 32
    n = min((3, 7, 4, 11, 2, 13, 6)[k % 7], left)
    pieces.append(s.generate(n))
    left -= n
    k += 1
  calls = {'chunk': 0, 'set_condition': 0}
  chunk, setc = GenerationSession._generate_chunk, _lib.lib().wn_generate_set_condition

  def counted_chunk(self, n):
    calls['chunk'] += 1
    return chunk(self, n)

  def counted_setc(*args):
    calls['set_condition'] += 1
    return setc(*args)
  monkeypatch.setattr(GenerationSession, '_generate_chunk', counted_chunk)
  monkeypatch.setattr(_lib.lib(), 'wn_generate_set_condition', counted_setc)
  one = local.generation_session(**kw).generate(total)
  assert calls == {'chunk': 1, 'set_condition': 0}
  call = local.generate(total, **kw)
  assert calls['set_condition'] == 0
  assert torch.equal(one, torch.cat(pieces, 1)) and torch.equal(one, call)


@pytest.mark.parametrize('name', NETS)
def test_a_chunk_past_an_admitted_rows_frames_is_refused_and_changes_nothing(name):
  local, _ = _pair(name)
  _, _, prompt, req = _inputs(name)
  hop, slot = 5, 2

  def begun():
    s = local.generation_session(**_session_kw(name, hop))
    s.generate(7)
    s.admit_own_clock(slot, prompt, condition=req[:, :2], stream=[STREAM], temperature=0.8)     # samples 6 .. 15
    return s
  want = begun().generate(9)
  s = begun()
  with pytest.raises(ValueError, match=f'row {slot}: .* run past the 2 condition frames of hop 5'):
    s.generate(10)
  assert s.position == 7
  assert torch.equal(s.generate(9), want)
  with pytest.raises(ValueError, match=f'row {slot}'):
    s.generate(1)


@pytest.mark.parametrize('name', NETS)
def test_set_condition_ends_an_admitted_rows_schedule(name):
  """The row follows the held condition across its former boundaries (11 and 16): it is the global model's B = 1 session
  begun at the admission's position and rewritten by hand at the same step; the other rows are the session without any of it."""
  local, glob = _pair(name)
  _, _, prompt, req = _inputs(name)
  hop, slot = 5, 1
  held = (torch.rand(1, CIN, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(dev())
  base = local.generation_session(**_session_kw(name, hop)).generate(18)
  s = local.generation_session(**_session_kw(name, hop))
  a = s.generate(7)
  first = s.admit([slot], prompt, condition=req, stream=[STREAM], temperature=0.8)
  b = s.generate(2)
  s.set_condition(held, slots=[slot])
  c = s.generate(9)                                       # crosses 10 and 15 (the session's), 11 and 16 (the request's former ones)
  sg = glob.generation_session(sample=prompt, condition=req[:, 0].contiguous(), use_queues=True, stream=[STREAM], temperature=0.8,
                               start=6)
  hand = [sg.generate(3)]
  sg.set_condition(held)
  hand.append(sg.generate(9))
  assert torch.equal(torch.cat([first[0], b[slot], c[slot]], 0), torch.cat(hand, 1)[0])
  got = torch.cat([a, b, c], 1)
  for r in (0, 2):
    assert torch.equal(got[r], base[r]), r


def test_a_session_without_hop_refuses_frames():
  local, _ = _pair('r64')
  w, fr, prompt, req = _inputs('r64')
  s = local.generation_session(sample=w, condition=fr[:, :1], use_queues=True, seed=[5, 6, 7], stream=[0, 1, 2])
  s.generate(3)
  with pytest.raises(ValueError, match='the session needs hop='):
    s.admit([1], prompt, condition=req, stream=[STREAM])
  assert s.position == 3
  s.admit([1], prompt, condition=req[:, :1], stream=[STREAM])          # one frame is a held condition, as ever
  assert s.generate(2).shape == (B, 2, 1)


@pytest.mark.parametrize('name', ['r64', 'b48'])
def test_tables_off_the_float4_alignment_give_the_same_samples(name, monkeypatch):
  """The copy kernel's one-float-per-lane form (a table that is not 16-byte aligned) against its float4 form."""
  from wavenets_amd import _lib
  from wavenets_amd.generation import _FrameSchedule
  local, _ = _pair(name)
  w, fr, _, _ = _inputs(name)
  kw = dict(sample=w, condition=fr, hop=5, use_queues=True, seed=3)
  want = local.generate(20, **kw)
  record, shifted = _FrameSchedule.record, []

  def off_by_one_float(self, j, width):
    r = record(self, j, width)
    if not hasattr(self, 'moved'):
      self.moved = torch.empty(self.table.numel() + 1, dtype=torch.float32, device=self.table.device)
    self.moved[1:].copy_(self.table)
    shifted.append(self.moved.data_ptr() + 4)
    return _lib.WnFrameRow(r.rows - self.table.data_ptr() + shifted[-1], r.block_stride, r.origin, r.frames, r.hop)
  monkeypatch.setattr(_FrameSchedule, 'record', off_by_one_float)
  assert torch.equal(local.generate(20, **kw), want)
  assert shifted and all(p % 16 == 4 for p in shifted)


@pytest.mark.parametrize('name', NETS)
def test_a_table_of_hundreds_of_rows_holds_the_rows_set_condition_writes(name):
  """A served request has hundreds of condition rows: k * F = 3 * 150 = 450, many 32-row tiles of the small product and a
  long walk of the rows GEMM.  Row (j, f) of every block is bit for bit what wn_generate_set_condition writes into cb for
  frame f alone (B = 3 rows), read back from the workspace at the offsets wn_generate_admit_describe names."""
  import ctypes as C
  import re
  from wavenets_amd import _lib
  from wavenets_amd.generation import _FrameSchedule
  local, _ = _pair(name)
  w, fr, _, _ = _inputs(name)
  F = 150
  frames = (torch.rand(B, F, CIN, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(dev())
  s = local.generation_session(sample=w, condition=fr[:, :1], use_queues=True, seed=[5, 6, 7], stream=[0, 1, 2])
  s.generate(2)                                           # primed: the weight images are in the workspace
  sch = _FrameSchedule(frames, 0, 5)
  sch.build(s, False)
  buf = C.create_string_buffer(1 << 16)
  _lib.check(_lib.lib().wn_generate_admit_describe(local._plan, 1, B, buf, len(buf)))
  offs = [int(v) for v in re.findall(r'cb\[\d+\] block=\d+ slots=1 width=\d+ src=\d+ dst=(\d+)', buf.value.decode())]
  width = 2 * local.spec.D
  assert len(offs) == 3 and sch.table.numel() >= len(offs) * B * F * width
  table = sch.table[:len(offs) * B * F * width].view(len(offs), B, F, width)
  for f in list(range(0, F, 7)) + [F - 1]:
    s.set_condition(frames[:, f])
    for n, off in enumerate(offs):
      assert torch.equal(s._ws[off:off + B * width].view(B, width), table[n, :, f]), (n, f)
  assert not torch.equal(table[:, :, 0], table[:, :, F - 1])


def test_a_first_chunk_that_raises_behind_its_priming_step_leaves_position_at_the_start(monkeypatch):
  """The chunk that begins a scheduled sequence is the priming step and the rest as two library calls: when something
  raises between them nothing is committed, and the next chunk begins the sequence again."""
  from wavenets_amd.generation import _FrameSchedule
  local, _ = _pair('r64')
  w, fr, _, _ = _inputs('r64')
  kw = dict(sample=w, condition=fr, hop=5, use_queues=True, seed=7)
  want = local.generation_session(**kw).generate(12)
  s = local.generation_session(**kw)
  build = _FrameSchedule.build

  def failing(self, session, exact):
    raise RuntimeError('no table today')
  monkeypatch.setattr(_FrameSchedule, 'build', failing)
  with pytest.raises(RuntimeError, match='no table today'):
    s.generate(12)
  assert s.position == 0
  monkeypatch.setattr(_FrameSchedule, 'build', build)
  assert torch.equal(s.generate(12), want) and s.position == 12
