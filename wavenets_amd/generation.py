"""Generation on the host side: the argument handling of WaveNet.generate / generation_session (a mixin of WaveNet), the
per-utterance sampling controls, the choice of the library's entry point, and GenerationSession."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _guard, _lib


_RELAY_GAVE_UP = ('wn_generate: a workgroup of the generation relay gave up waiting for its predecessor '
                  '(code {}); the samples of this {} are invalid')


def _guard_words(words, noun, gave_up=None):
  """The two words at wn_generate_guard_slot -- the pass's range-guard float and the relay's watchdog word -- read to the
  host (one blocking copy): did the pass leave the range of the split-precision kernels?  A non-zero watchdog word comes
  first: the samples of this `noun` ('call', 'chunk') are invalid and RuntimeError says so, behind `gave_up()` where the
  site has something to mark.  (A NaN guard counts as tripped.)"""
  guard, watchdog = words.cpu()
  if int(watchdog.view(torch.int32)) != 0:
    if gave_up is not None:
      gave_up()
    raise RuntimeError(_RELAY_GAVE_UP.format(int(watchdog.view(torch.int32)), noun))
  return not (float(guard) < _lib.lib().wn_range_limit())


def _generation_entry(phase, head, sampling, rows, origin, tail):
  """The library's entry point of a generation pass with its arguments.  phase: 'call' (generate: a whole sequence from
  its window), 'begin' (the chunk that begins a session's sequence at start > 0), 'chunk' (every other chunk; start = 0
  runs the call it always ran) or 'admit' (per-row controls only).  sampling: the struct wn_sampling of the scalar entry
  points (rows None), or the _RowControls whose device table `rows` is.  origin: the rows' clock origins on the device,
  or None -- the entry points without the argument.  head / tail: the site's arguments in front of and behind the
  controls."""
  L = _lib.lib()
  if rows is None:
    if phase == 'call':                     # (wn_generate_sampled takes no `first`: head[5])
      return L.wn_generate_sampled, (*head[:5], *head[6:], C.byref(sampling), *tail)
    return L.wn_generate_chunk, (*head, C.byref(sampling), *tail)
  if phase == 'admit':
    entry = L.wn_generate_admit if origin is None else L.wn_generate_admit_origin
  elif phase == 'begin':
    entry = L.wn_generate_rows_begin if origin is None else L.wn_generate_rows_begin_origin
  else:
    entry = L.wn_generate_rows_chunk if origin is None else L.wn_generate_rows_chunk_origin
  controls = (_lib.ptr(rows), sampling.flags) + (() if origin is None else (_lib.ptr(origin),))
  return entry, (*head, *controls, *tail)


class _RowControls:
  """Sampling controls per utterance: B checked struct wn_sampling entries and their Philox streams,
  packed by wn_sampling_rows_pack (host only) into the table of struct wn_sampling_row that wn_generate_rows_chunk reads
  from device memory, and the flags that say what the union of the rows asks for."""

  def __init__(self, entries, streams, head, classes):
    B = len(entries)
    self.entries, self.streams = list(entries), (list(streams) if streams is not None else None)
    arr = (_lib.WnSampling * B)(*[_lib.WnSampling(e.temperature, e.top_k, e.seed, e.top_p) for e in entries])
    st = (C.c_uint64 * B)(*streams) if streams is not None else None
    self.host = (_lib.WnSamplingRow * B)()
    flags = C.c_int32(0)
    _lib.check(_lib.lib().wn_sampling_rows_pack(arr, st, B, head, classes, self.host, C.byref(flags)))
    self.flags = int(flags.value)

  def __len__(self):
    return len(self.entries)

  def device_table(self, device):
    """The table as a float tensor on `device`: one copy, made once per call or session."""
    return torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.float32).to(device)


class _FrameSchedule:
  """The frame schedule of one request: its condition frames (k, F, Cin), kept for the rebuild of
  an exact-fp32 turn, and the table of its bias rows for every frame (wn_generate_frames_build), made once.  Row j of the
  request uses frame (t - origin) // hop at the step that emits sample t."""

  def __init__(self, cond, origin, hop):
    self.cond, self.origin, self.hop = cond.contiguous(), int(origin), int(hop)
    self.k, self.frames = int(cond.shape[0]), int(cond.shape[1])
    self.table = None

  def build(self, session, exact):
    """The table, in exact-fp32 mode or the calling context's, from the weight images of the session's primed workspace
    (read only).  In place once it exists: the records keep pointing at it."""
    m, L = session._model, _lib.lib()
    if self.table is None:
      self.table = torch.empty(int(L.wn_generate_frames_floats(m._plan, self.k * self.frames)), dtype=torch.float32,
                               device=m._device)

    def run():
      _lib.check(L.wn_generate_frames_build(m._plan, _lib.ptr(m.flat_params), _lib.ptr(self.cond), self.k, self.frames,
                                            _lib.ptr(self.table), self.table.numel(), _lib.ptr(session._ws), session._ws.numel(),
                                            session._B, _lib.stream_ptr()))
    if exact:
      with m.exact_fp32():
        run()
    else:
      run()

  def record(self, j, width):
    """struct wn_frame_row of the request's row j (width = 2 * dilation channels floats per bias row)."""
    return _lib.WnFrameRow(self.table.data_ptr() + 4 * j * self.frames * width, self.k * self.frames * width, self.origin,
                           self.frames, self.hop)


def _as_rows(name, v):
  """None for a scalar argument, else the entries of a list, tuple, numpy array or 1-D tensor as Python values."""
  if isinstance(v, torch.Tensor):
    v = v.detach().cpu().numpy()
  if isinstance(v, np.ndarray):
    if v.ndim == 0:
      return None
    if v.ndim != 1:
      raise ValueError(f'{name} must be a scalar or a sequence of one entry per utterance (got shape {tuple(v.shape)})')
    return v.tolist()
  if isinstance(v, (list, tuple)):
    return [e.item() if isinstance(e, (np.generic, torch.Tensor)) else e for e in v]
  return None


class GenerationSession:
  """One sequence of WaveNet.generation_session(...), continued chunk by chunk (wn_generate_chunk).

  position: samples emitted so far.  exact: the session runs under exact_fp32() from here on (a chunk left the range
  of the split-precision kernels, or the sequence was begun in exact-fp32 mode, whose priming pass does not prepare
  what a split-precision step reads).  Otherwise a chunk runs in the math mode of the calling context.

  start: the index of the sequence's first sample; position begins there, the first chunk is
  wn_generate_rows_begin.  admit() puts new requests into rows of the running batch.

  origins: per row, the index its clock counts from -- row b draws sample t from the Philox counter
  (stream[b], t - origins[b]).  All zero unless the session was created with own_clock=True or a request admitted by admit_own_clock;
  row_positions is position - origins[b], the number of samples row b's present clock has counted."""

  def __init__(self, model, sampling, condition, window, batch_size, use_queues, deterministic, start=0, own_clock=False,
               frames=None, hop=None):
    L = _lib.lib()
    self._model, self._sampling, self._cond, self._window = model, sampling, condition, window
    # local conditioning (DESIGN.md sections 36 and 42): frames (B, F, Cin) and the samples per frame.  The step that emits
    # sample g, counted from `start`, uses frame g // hop; the priming pass uses frame 0 (`condition`).  Every row has a
    # schedule of its own: _sched[b] is (schedule, its row of that schedule) or None -- a row admitted with a held condition,
    # or taken off by set_condition(slots=), keeps the condition set_condition gives it.  The schedules are armed around every
    # chunk (wn_plan_arm_gen_frames) and advanced by the copy kernel inside it.
    self._hop = hop
    self._own = None if frames is None else _FrameSchedule(frames, start, hop)     # of the rows the session begins with
    self._sched = [None if self._own is None else (self._own, b) for b in range(int(batch_size))]
    # set_condition on a scheduled row: the row keeps that condition until the position held here, its next frame boundary
    self._held = {}
    # per-row controls: the device table of the session, read by every chunk (and by the exact-fp32 rerun of one)
    self._rows = sampling.device_table(model._device) if isinstance(sampling, _RowControls) else None
    self._B, self._queued, self._det = int(batch_size), int(bool(use_queues)), int(bool(deterministic))
    # its own workspace (never model._workspace('gen')): other sessions and one-shot generate calls leave it alone
    self._ws = torch.zeros(int(L.wn_generate_workspace_floats(model._plan, self._B, self._queued)), dtype=torch.float32,
                           device=model._device)
    off, n = C.c_int64(), C.c_int64()
    _lib.check(L.wn_generate_state_range(model._plan, self._B, self._queued, C.byref(off), C.byref(n)))
    # what steps write and a continuation reads, and where a chunk's range-guard trip restores it from
    self._state = self._ws[off.value:off.value + n.value]
    self._shadow = torch.empty_like(self._state)
    self._slot = int(L.wn_generate_guard_slot(model._plan, self._B, self._queued))
    self._weights = (model.flat_params.data_ptr(), model._train_gen)
    self._failed = False
    self._start = int(start)
    self._admitted = False                 # admit() has replaced rows: the window no longer begins this batch
    self._scratch = {}                     # admit(): the scratch workspace of k rows, kept per k
    self.position = self._start
    self.exact = False
    # the rows' clock origins: None (every origin 0, the entry points without the argument) or B uint64 on the device,
    # read by every chunk like the table; own_clock: every row counts from `start`
    self._origin = None
    if own_clock:
      self._origin = torch.full((self._B,), self._start, dtype=torch.int64, device=model._device)
    self._origins = [self._start if own_clock else 0] * self._B

  @property
  def origins(self):
    return list(self._origins)

  @property
  def row_positions(self):
    return [self.position - o for o in self._origins]

  def generate(self, n):
    """The next (B, n, 1) samples, n >= 1.  A chunk that raises leaves position where it was.  With a frame schedule
    (local conditioning) the chunk is split at the frame boundaries and the condition table rewritten there; a chunk that
    would run past the last frame raises ValueError before anything is made."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
      raise ValueError(f'n must be an int >= 1 (got {n!r})')
    n = int(n)
    for b, entry in enumerate(self._sched):
      if entry is None:
        continue
      sch, done = entry[0], self.position - entry[0].origin
      if done + n > sch.frames * sch.hop:
        raise ValueError(f'generation session: row {b}: {done} + {n} samples run past the {sch.frames} condition frames '
                         f'of hop {sch.hop} ({sch.frames * sch.hop} samples)')
    # (one chunk whatever frame boundaries it crosses: the copy kernel advances the rows inside it.  Only a row that
    # set_condition holds until its next boundary ends a chunk there: it goes back on its schedule between two calls)
    pieces = []
    while n > 0:
      self._held = {b: end for b, end in self._held.items() if end > self.position}
      take = min([n] + [end - self.position for end in self._held.values()])
      pieces.append(self._generate_chunk(take))
      n -= take
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces, 1)

  def _build_tables(self, exact):
    """Every schedule's table (again): in the math mode the session runs in from here on."""
    for sch in {id(e[0]): e[0] for e in self._sched if e is not None}.values():
      sch.build(self, exact)

  def _frame_records(self):
    """The B struct wn_frame_row of the next chunk, or None when no row is on a schedule with a table (nothing is armed
    then, and the chunk queues what it queues without schedules)."""
    width = 2 * self._model.spec.D
    recs = (_lib.WnFrameRow * self._B)()
    some = False
    for b, entry in enumerate(self._sched):
      if entry is not None and entry[0].table is not None and self._held.get(b, 0) <= self.position:
        recs[b] = entry[0].record(entry[1], width)
        some = True
    return recs if some else None

  def _write_condition(self, cond):
    """self._cond = cond, and into the bias table of the workspace when the sequence has begun (the priming pass of a
    sequence that has not takes it from self._cond)."""
    m, L = self._model, _lib.lib()
    cond = cond.contiguous()
    if self.position > self._start:
      if not self._queued:
        raise NotImplementedError('set_condition needs use_queues=True: the sliding window maps the condition in every step')

      def run():
        _lib.check(L.wn_generate_set_condition(m._plan, _lib.ptr(m.flat_params), _lib.ptr(cond), self._B, 1, _lib.ptr(self._ws),
                                               self._ws.numel(), _lib.stream_ptr()))
      if self.exact:
        with m.exact_fp32():
          run()
      else:
        run()
    self._cond = cond

  def set_condition(self, condition, slots=None):
    """A new condition for running rows, from the next step on: (B, Cin), or (k, Cin) for the k rows `slots`.  Works on a
    globally conditioned model too.  On a session with a frame schedule the rows still on the schedule are rewritten at
    the next frame boundary; rows an admission replaced are driven by this call alone."""
    m = self._model
    self._check_usable()
    if self._cond is None:
      raise ValueError('set_condition: the model has no conditioning')
    condition = torch.as_tensor(condition, dtype=torch.float32, device=m._device)
    if condition.dim() == 3 and condition.shape[1] == 1:
      condition = condition[:, 0, :]
    cond = self._cond.clone()
    if slots is None:
      if tuple(condition.shape) != tuple(cond.shape):
        raise ValueError(f'condition must have shape {tuple(cond.shape)} (got {tuple(condition.shape)})')
      cond.copy_(condition)
    else:
      slot_list = [int(slots)] if isinstance(slots, (int, np.integer)) else [int(v) for v in slots]
      if any(v < 0 or v >= self._B for v in slot_list) or len(set(slot_list)) != len(slot_list):
        raise ValueError(f'slots must be distinct ints in [0, {self._B}) (got {slot_list})')
      if tuple(condition.shape) != (len(slot_list), cond.shape[1]):
        raise ValueError(f'condition must have shape {(len(slot_list), cond.shape[1])} (got {tuple(condition.shape)})')
      cond[torch.tensor(slot_list, device=m._device)] = condition
    # (the table of the workspace again for all B rows: the rows on a schedule take their frames back at the first step of
    # the next chunk, which always runs the copy kernel)
    self._write_condition(cond)
    for b in (range(self._B) if slots is None else slot_list):
      if self._sched[b] is None:
        continue
      sch = self._sched[b][0]
      if sch is not self._own:
        self._sched[b] = None                 # a request admitted on a schedule: this call ends it
      else:
        # a row the session began with: the condition stands until the row's next frame boundary, as it did when a
        # boundary was a rewrite of the table between two chunks
        g = self.position - sch.origin
        self._held[b] = sch.origin + (((g - 1) // sch.hop + 1) if g > 0 else 1) * sch.hop

  def _generate_chunk(self, n):
    if self.position != self._start or self._own is None or not self._queued:
      return self._chunk(n)
    # The chunk that begins a sequence on a frame schedule: the tables are built from the weight images its priming pass
    # leaves, in the math mode that pass ended in, so the priming step is a call of its own and the steps behind it the
    # next one (the chunks of a sequence, concatenated, are the one call bit for bit: DESIGN.md section 23).
    # Nothing is committed until both have returned: if the table build or the second call raises, position is back at
    # the start, where the next chunk begins the sequence again from the window (a chunk that raises leaves position where
    # it was).
    try:
      head = self._chunk(1)
      self._build_tables(self.exact)
      return head if n == 1 else torch.cat([head, self._chunk(n - 1)], 1)
    except BaseException:
      self.position = self._start
      raise

  def _chunk(self, n):
    m, L, first = self._model, _lib.lib(), self.position
    self._check_usable()
    out = torch.empty(self._B, n, 1, dtype=torch.float32, device=m._device)
    begins = first == self._start            # the chunk that begins the sequence from the window

    def run():
      window = _lib.ptr(self._window) if begins else None
      # (start = 0 runs the call it always ran; the range-guard rerun below repeats with the same origins)
      entry, args = _generation_entry(
          'begin' if begins and first > 0 else 'chunk',
          (m._plan, _lib.ptr(m.flat_params), window, _lib.ptr(self._cond), self._B, first, n, self._det, self._queued),
          self._sampling, self._rows, self._origin, (_lib.ptr(out), _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr()))
      # the rows' frame schedules, armed for this call alone (the rerun arms the tables the exact-fp32 turn rebuilt)
      records = None if begins else self._frame_records()
      try:
        if records is not None:
          _lib.check(L.wn_plan_arm_gen_frames(m._plan, records, self._B))
        _lib.check(entry(*args))
      finally:
        if records is not None:
          L.wn_plan_arm_gen_frames(m._plan, None, 0)

    def tripped():
      return _guard_words(self._ws[self._slot:self._slot + 2], 'chunk', lambda: setattr(self, '_failed', True))

    def restore():
      # the tripped run has overwritten the raw-sample slots and ring slots of its steps: back to the state in front
      # of the chunk, the chunk again and everything after it on the exact-fp32 kernels (same seed: same draws); the
      # samples already handed out stand
      if not begins:
        self._state.copy_(self._shadow)
        # the tables were built in split precision: again from the kept frames, in the mode the session is turning to
        # (the compact table needs no place in the shadow: the rerun's first step runs the copy kernel)
        self._build_tables(True)
    if self.exact or L.wn_debug_value(1) == 1:
      # exact fp32 cannot trip: no shadow copy, no host read
      with m.exact_fp32():
        run()
      if begins:
        self.exact = True
    else:
      if not begins:
        self._shadow.copy_(self._state)              # device to device, on the call's stream
      if _guard.guarded(m, run, tripped, before_rerun=restore, counter='generation_guard_trips'):
        self.exact = True
    self.position = first + n
    return out

  def _check_usable(self):
    m = self._model
    if self._failed:
      raise RuntimeError('generation session: an earlier chunk failed; its state is invalid')
    if (m.flat_params.data_ptr(), m._train_gen) != self._weights:
      raise RuntimeError('generation session: the weights changed since the session was created (optimizer step, '
                         'set_weights, finalize_variable_values, or an averaged_weights() boundary); start a new session')

  def admit(self, slots, sample, condition=None, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None):
    """New requests into rows of the running batch (wn_generate_admit).  slots: an int or k distinct
    ints in [0, B); sample: (k, >= receptive_field, 1), the prompts; condition: (k, cond_inputs) on a conditioned net;
    the controls as in generate, scalars or k-sequences; stream: k ints, required.  Returns (k, 1, 1): every request's
    first sample, index position - 1 of the session; from the next chunk on row slots[j] is request j.  That row, from
    the returned sample on, is bit for bit a session of B = 1 begun with start = position - 1 from the request's own
    arguments; every other row is what it is without the admission.  Queued sessions with per-row controls only, after
    their first chunk.  The admitted rows draw on the session's clock; admit_own_clock gives them their own."""
    return self._admit(slots, sample, condition, temperature, top_k, seed, top_p, stream, False)

  def admit_own_clock(self, slots, sample, condition=None, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None):
    """admit, with the admitted rows on their own clock: they count from their own first sample --
    origin position - 1, so the returned sample is drawn from counter (stream, 0).  Such a row is then bit for bit
    model.generate(n, sample=prompt, use_queues=True, stream=[id], <its controls>) of the request alone, whichever slot,
    batch and position it was admitted at.  The other rows keep their clocks.  (A method of its own: admit's parameter
    list is what section 32 fixed.)"""
    return self._admit(slots, sample, condition, temperature, top_k, seed, top_p, stream, True)

  def _admit(self, slots, sample, condition, temperature, top_k, seed, top_p, stream, own_clock):
    m, L = self._model, _lib.lib()
    if not self._queued:
      raise RuntimeError('generation session: admit needs a session with use_queues=True (the sliding window has no '
                         'state rows to move)')
    if self._rows is None:
      raise RuntimeError('generation session: admit needs per-row controls (create the session with stream=)')
    if self.position < 1 or self.position == self._start:
      raise RuntimeError(f'generation session: admit needs position >= 1 and a begun sequence (position is {self.position}); '
                         'generate the first chunk before admitting')
    self._check_usable()
    one = not isinstance(slots, (list, tuple, np.ndarray, torch.Tensor))
    slot_list = [slots] if one else _as_rows('slots', slots)
    if slot_list is None or len(slot_list) < 1:
      raise ValueError(f'slots must be an int or a sequence of distinct ints (got {slots!r})')
    for j, v in enumerate(slot_list):
      if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < self._B:
        raise ValueError(f'slots[{j}] must be an int in [0, {self._B}) (got {v!r})')
      if v in slot_list[:j]:
        raise ValueError(f'slots[{j}] = {v} is a duplicate (the slots must be distinct)')
    slot_list = [int(v) for v in slot_list]
    k, rf = len(slot_list), m.receptive_field
    sample = torch.as_tensor(sample, dtype=torch.float32, device=m._device)
    if sample.dim() != 3 or sample.shape[0] != k or sample.shape[2] != 1 or sample.shape[1] < rf:
      raise ValueError(f'sample must have shape ({k}, >= {rf}, 1) for {k} slots (got {tuple(sample.shape)})')
    sample = sample[:, -rf:, :].contiguous()
    if m.conditioning is not None and condition is None:
      raise ValueError('Conditioning must be provided.')
    req_frames = None                        # (k, F, Cin), F > 1: the requests bring a frame schedule of their own
    if condition is not None:
      condition = torch.as_tensor(condition, dtype=torch.float32, device=m._device).contiguous()
      if m.conditioning == 'local' and self._cond is not None:
        cin = int(self._cond.shape[1])
        if condition.dim() == 2 and cin == 1 and condition.shape[1] > 1:
          condition = condition[:, :, None].contiguous()     # (k, F) frames of one input
        if condition.dim() == 3 and condition.shape[1] == 1:
          condition = condition[:, 0, :].contiguous()        # a held condition as one frame, (k, 1, Cin)
        elif condition.dim() == 3 and condition.shape[1] > 1 and tuple(condition.shape[::2]) == (k, cin):
          if self._hop is None:
            raise ValueError(f'condition holds {int(condition.shape[1])} frames per request: the session needs hop= '
                             '(generation_session(..., hop=h): the samples generated per frame)')
          req_frames = condition
          condition = req_frames[:, 0, :].contiguous()       # the priming pass takes frame 0, as in generate
      if self._cond is None or tuple(condition.shape) != (k,) + tuple(self._cond.shape[1:]):
        want = None if self._cond is None else (k,) + tuple(self._cond.shape[1:])
        raise ValueError(f'condition must have shape {want} (got {tuple(condition.shape)})')
    if stream is None:
      raise ValueError('stream is required: one Philox stream id per admitted request')
    new = m._sampling_rows(k, temperature, top_k, seed, top_p, stream, 2 ** m.bits, True)
    # the whole table again: the error text names the session's row, the flags are the new union
    old = self._sampling
    entries = list(old.entries)
    streams = list(old.streams) if old.streams is not None else list(range(self._B))
    for j, b in enumerate(slot_list):
      entries[b], streams[b] = new.entries[j], new.streams[j]
    table = _RowControls(entries, streams, _lib.HEADS[m.sampling_function], 2 ** m.bits)
    rows_k = new.device_table(m._device)
    if k not in self._scratch:
      self._scratch[k] = torch.zeros(int(L.wn_generate_admit_scratch_floats(m._plan, k)), dtype=torch.float32, device=m._device)
    scratch = self._scratch[k]
    first_out = torch.empty(k, 1, 1, dtype=torch.float32, device=m._device)
    slots_c = (C.c_int32 * k)(*slot_list)
    # a session without an origin array gets one of zeros at its first admit_own_clock, and keeps it
    origin = self._origin
    if origin is None and own_clock:
      origin = torch.zeros(self._B, dtype=torch.int64, device=m._device)
    origin_k = None if origin is None else torch.full((k,), self.position - 1 if own_clock else 0, dtype=torch.int64,
                                                      device=m._device)

    def run():
      # (the range-guard rerun below repeats with the same origins)
      entry, args = _generation_entry(
          'admit',
          (m._plan, _lib.ptr(m.flat_params), _lib.ptr(sample), _lib.ptr(condition), k, slots_c, self._B, self.position, self._det),
          new, rows_k, origin_k,
          (_lib.ptr(first_out), _lib.ptr(self._ws), self._ws.numel(), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()))
      _lib.check(entry(*args))

    def tripped():                            # (the admission's scratch has a guard float and no watchdog word to read)
      slot = int(L.wn_generate_guard_slot(m._plan, k, 1))
      return not (float(scratch[slot]) < L.wn_range_limit())
    if self.exact or L.wn_debug_value(1) == 1:
      with m.exact_fp32():
        run()
    elif _guard.guarded(m, run, tripped, counter='generation_guard_trips'):
      # the admission's priming pass left the range of the split-precision kernels: it ran again on the exact-fp32 kernels
      # (the move overwrites the same rows: nothing to restore), and the session stays there, with its tables built again
      self.exact = True
      self._build_tables(True)
    # the session's own records: rows slots[j] of the device table (in place: the chunks read this tensor) and of the condition
    self._sampling = table
    self._rows.copy_(table.device_table(m._device))
    if origin is not None:
      origin[torch.tensor(slot_list, device=m._device)] = origin_k
      self._origin = origin
      for b in slot_list:
        self._origins[b] = self.position - 1 if own_clock else 0
    if condition is not None:
      if not self._admitted:
        self._cond = self._cond.clone()          # (the caller's tensor stays as it is)
      self._cond[torch.tensor(slot_list, device=m._device)] = condition
      # the rows leave whatever schedule they were on: a held condition is driven by set_condition alone, frames go on a
      # schedule of the request's own that counts from its first sample, index position - 1, whichever clock its draws follow
      sch = None
      if req_frames is not None:
        sch = _FrameSchedule(req_frames, self.position - 1, self._hop)
        sch.build(self, self.exact)
      for j, b in enumerate(slot_list):
        self._sched[b] = None if sch is None else (sch, j)
        self._held.pop(b, None)
    self._admitted = True
    return first_out

  def reset(self):
    """Back to the start: the next chunk begins the sequence again from the window, on the same workspace (and with the
    same origins)."""
    if self._admitted:
      raise RuntimeError('generation session: reset after admit is not possible (the rows the window began are gone); '
                         'start a new session')
    self.position = self._start
    self._failed = False
    self._held = {}


class _Generation:
  def _sampling(self, temperature, top_k, seed, classes, top_p=1.0):
    """The sampling controls of a stochastic draw as the C struct (semantics: include/wn_hip.h, struct wn_sampling),
    checked as the library checks them, before any work is queued.  classes: row length of a categorical prediction.
    top_p: a real number in (0, 1]; 1.0 is off."""
    if isinstance(top_k, bool) or not isinstance(top_k, int):
      raise ValueError(f'top_k must be an int (got {top_k!r})')
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
      raise ValueError(f'seed must be an int or None (got {seed!r})')
    t = np.float32(temperature)
    with np.errstate(all='ignore'):
      if not (t > 0 and np.isfinite(t) and np.isfinite(np.float32(1.0) / t)):
        raise ValueError(f'temperature must be finite and > 0 with a finite reciprocal (got {temperature!r})')
    if not 0 <= top_k < 2**31:
      raise ValueError(f'top_k must be >= 0 (got {top_k})')
    if top_k > 0 and self.sampling_function != 'categorical':
      raise ValueError(f'top_k applies to the categorical head only (got top_k = {top_k} with {self.sampling_function})')
    if 0 < top_k < classes and classes > _lib.WN_TOP_K_MAX_CLASSES:
      raise ValueError(f'top_k is offered for up to {_lib.WN_TOP_K_MAX_CLASSES} classes (got {classes})')
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float, np.integer, np.floating)):
      raise ValueError(f'top_p must be a real number in (0, 1] (got {top_p!r})')
    tp = np.float32(top_p)
    if not (float(top_p) > 0 and tp > 0 and tp <= 1):        # NaN fails; so does a value that rounds to 0 in fp32
      raise ValueError(f'top_p must lie in (0, 1] (got {top_p!r})')
    if tp < 1 and self.sampling_function != 'categorical':
      raise ValueError(f'top_p applies to the categorical head only (got top_p = {top_p} with {self.sampling_function})')
    if tp < 1 and classes > _lib.WN_TOP_K_MAX_CLASSES:
      raise ValueError(f'top_p is offered for up to {_lib.WN_TOP_K_MAX_CLASSES} classes (got {classes})')
    key = 0x0402 if seed is None else seed & 0xFFFFFFFFFFFFFFFF
    return _lib.WnSampling(float(t), top_k, key, float(tp))

  def _sampling_rows(self, batch_size, temperature, top_k, seed, top_p, stream, classes, have_sample=True):
    """Sampling controls given per utterance.  Each of temperature, top_k, seed and top_p is a
    scalar or a sequence (list, tuple, numpy array, 1-D tensor) of batch_size entries, entry b for utterance b; scalars
    beside sequences are broadcast.  Every row is checked by _sampling, and the error names the row.  stream: None, or
    batch_size ints in [0, 2**63), the row word of utterance b's Philox counter (None: b).
    Returns the one struct wn_sampling of today's scalar entry points when every row is equal and stream is None --
    such a call runs exactly the code it ran before -- and a _RowControls otherwise."""
    B = int(batch_size)
    cols = {}
    for name, v in (('temperature', temperature), ('top_k', top_k), ('seed', seed), ('top_p', top_p)):
      rows = _as_rows(name, v)
      if rows is not None and len(rows) != B:
        raise ValueError(f'{name} has {len(rows)} entries for a batch of {B} utterances')
      cols[name] = rows if rows is not None else [v] * B
    entries = []
    for b in range(B):
      T = cols['temperature'][b]
      if isinstance(T, bool):
        raise ValueError(f'row {b}: temperature must be a real number (got {T!r})')
      try:
        entries.append(self._sampling(T, cols['top_k'][b], cols['seed'][b], classes, cols['top_p'][b]))
      except ValueError as e:
        raise ValueError(f'row {b}: {e}') from None
    streams = None
    if stream is not None:
      streams = _as_rows('stream', stream)
      if streams is None:
        raise ValueError(f'stream must be None or a sequence of one int per utterance (got {stream!r})')
      if len(streams) != B:
        raise ValueError(f'stream has {len(streams)} entries for a batch of {B} utterances')
      for b, v in enumerate(streams):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 63:
          raise ValueError(f'row {b}: stream must be an int in [0, 2**63) (got {v!r})')
      if not have_sample:
        raise ValueError('stream requires `sample`: a caller who names the Philox streams owns the prompt')
    # (compared as the library reads them: top_k >= classes and top_p = 1 are off)
    key = lambda e: (e.temperature, 0 if e.top_k >= classes else e.top_k, e.seed, 0.0 if e.top_p >= 1 else e.top_p)
    if streams is None and all(key(e) == key(entries[0]) for e in entries):
      return entries[0]
    return _RowControls(entries, streams, _lib.HEADS[self.sampling_function], classes)

  def generate(self, length, batch_size: int = 1, condition=None, sample=None,
               use_queues=False, deterministic=False, temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None, hop=None):
    """src/model.py:258-307 (intended semantics; the reference's kwarg / rank bugs are not
    reproduced).  Returns (B, length, 1).
    temperature / top_k / seed / top_p (additions) as in sample_waveform; an int seed is the Philox key of
    the draws and seeds the initial noise window when `sample` is None.  seed=None is seed=0x0402.
    Per utterance: each of the four may be a sequence of B entries (list, tuple, numpy array, 1-D
    tensor), entry b for utterance b; a scalar beside sequences is broadcast.  Row b of the result is bit for bit row b
    of the call at the same B whose scalar controls are row b's.  Without `sample`, row b of the noise window is row b
    of the window the scalar call with seed[b] draws.  stream: None, or B ints in [0, 2**63) -- utterance b draws from
    the Philox counter row stream[b] instead of b, so a request keeps its draws whichever batch slot it lands in
    (requires `sample`).  deterministic stays one flag for the call."""
    condition, frames, hop = self._local_frames(condition, hop, use_queues, length)
    if frames is not None:
      # a frame schedule (local conditioning): the sequence as a session, split at the frame boundaries -- the chunks of a
      # sequence, concatenated, are the one call bit for bit
      session = self.generation_session(batch_size=batch_size, condition=frames, sample=sample, use_queues=use_queues,
                                        deterministic=deterministic, temperature=temperature, top_k=top_k, seed=seed,
                                        top_p=top_p, stream=stream, hop=hop)
      if int(length) < 1:
        return torch.empty(session._B, 0, 1, dtype=torch.float32, device=self._device)
      return session.generate(int(length))
    sampling, condition, sample, batch_size = self._generation_args(batch_size, condition, sample, deterministic,
                                                                    temperature, top_k, seed, top_p, stream)
    L = _lib.lib()
    ws = self._workspace('gen', L.wn_generate_workspace_floats(self._plan, batch_size, int(bool(use_queues))))
    out = torch.empty(batch_size, int(length), 1, dtype=torch.float32, device=self._device)
    rows = sampling.device_table(self._device) if isinstance(sampling, _RowControls) else None
    def run():                              # (the range-guard rerun below repeats with the same table)
      entry, args = _generation_entry(
          'call',
          (self._plan, _lib.ptr(self.flat_params), _lib.ptr(sample), _lib.ptr(condition), batch_size, 0, int(length),
           int(bool(deterministic)), int(bool(use_queues))),
          sampling, rows, None, (_lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
      _lib.check(entry(*args))

    def tripped():
      slot = L.wn_generate_guard_slot(self._plan, batch_size, int(bool(use_queues)))
      return _guard_words(ws[slot:slot + 2], 'call')
    # range guard (one host read; the caller reads the samples anyway): an activation beyond the fp16 range of the
    # split-precision kernels -> the whole call again on the exact-fp32 kernels (same seed: same draws)
    _guard.guarded(self, run, tripped, skip=not length > 0 or L.wn_debug_value(1) == 1, counter='generation_guard_trips',
                   count_first=True)
    return out

  def _local_frames(self, condition, hop, use_queues, length=None):
    """Local conditioning in generation: condition (B, F) or (B, F, Cin) and hop, the samples per
    frame.  Returns (the priming pass's condition = frame 0 as (B, Cin), frames (B, F, Cin) or None, hop): None is a held
    condition with no end (F == 1 without hop).  Other models: (condition, None, None)."""
    if self.conditioning != 'local' or condition is None:
      if hop is not None:
        raise ValueError('hop belongs to conditioning=\'local\' with a condition of frames')
      return condition, None, None
    condition = torch.as_tensor(condition, dtype=torch.float32, device=self._device)
    if condition.dim() == 2:
      condition = condition[:, :, None]
    if condition.dim() != 3 or condition.shape[1] < 1:
      raise ValueError('condition must have shape (batch, frames) or (batch, frames, n_cond)')
    F = int(condition.shape[1])
    first = condition[:, 0, :].contiguous()
    if hop is None:
      if F > 1:
        raise ValueError(f'hop is required with {F} condition frames: the samples generated per frame')
      return first, None, None
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 1:
      raise ValueError(f'hop must be an int >= 1 (got {hop!r})')
    if F > 1 and not use_queues:
      raise NotImplementedError('a frame schedule needs use_queues=True: the reference\'s sliding window re-upsamples the whole '
                                'condition onto the window at every step, which defines nothing usable')
    if length is not None and int(length) > F * int(hop):
      raise ValueError(f'length {int(length)} runs past the {F} condition frames of hop {int(hop)} ({F * int(hop)} samples)')
    return first, condition.contiguous(), int(hop)

  def _generation_args(self, batch_size, condition, sample, deterministic, temperature, top_k, seed, top_p, stream=None):
    """The argument handling of generate and generation_session: the sampling controls checked, condition and sample on
    the device, the batch size they imply, the initial window (the last receptive_field samples of `sample`, or zeros /
    seeded noise), the model built.  Returns (sampling, condition, window, batch_size); sampling is the struct
    wn_sampling of the call, or a _RowControls when the controls differ between utterances or `stream` is given."""
    per_row = stream is not None or any(_as_rows(n, v) is not None for n, v in (
        ('temperature', temperature), ('top_k', top_k), ('seed', seed), ('top_p', top_p)))
    # (scalars: checked first, as ever; per utterance: once the batch size is known, below)
    sampling = None if per_row else self._sampling(temperature, top_k, seed, 2 ** self.bits, top_p)
    if self.conditioning is not None and condition is None:
      raise ValueError('Conditioning must be provided.')
    if condition is not None:
      condition = torch.as_tensor(condition, dtype=torch.float32, device=self._device).contiguous()
    if sample is not None:
      sample = torch.as_tensor(sample, dtype=torch.float32, device=self._device).contiguous()
    if condition is not None and sample is not None:
      if condition.shape[0] != sample.shape[0]:
        raise ValueError('Condition and sample must have same batch size.')
    if condition is not None:
      batch_size = condition.shape[0]
    if sample is not None:
      batch_size = sample.shape[0]
    rf = self.receptive_field
    if per_row:
      sampling = self._sampling_rows(batch_size, temperature, top_k, seed, top_p, stream, 2 ** self.bits, sample is not None)
    if sample is None:
      if deterministic:
        sample = torch.zeros(batch_size, rf, 1, device=self._device)
      elif isinstance(sampling, _RowControls):
        # row b of the (B, rf, 1) noise the scalar call with seed[b] draws: one host randn per distinct seed
        noise = {}
        for e in sampling.entries:
          if e.seed not in noise:
            noise[e.seed] = torch.randn(batch_size, rf, 1, generator=torch.Generator(device='cpu').manual_seed(int(e.seed)))
        sample = torch.stack([noise[e.seed][b] for b, e in enumerate(sampling.entries)]).to(self._device)
      else:
        g = torch.Generator(device='cpu').manual_seed(int(sampling.seed))
        sample = torch.randn(batch_size, rf, 1, generator=g).to(self._device)
    if sample.shape[1] != rf:
      if sample.shape[1] < rf:
        raise ValueError('sample must hold at least receptive_field samples')
      sample = sample[:, -rf:, :].contiguous()
    if not self.built:
      self.build([tuple(sample.shape), tuple(condition.shape)] if condition is not None else tuple(sample.shape))
    return sampling, condition, sample, batch_size

  def generation_session(self, batch_size: int = 1, condition=None, sample=None, use_queues=False, deterministic=False,
                         temperature=1.0, top_k=0, seed=None, top_p=1.0, stream=None, start=0, own_clock=False, hop=None):
    """A sequence made in pieces: the arguments of generate without `length`, with the same checks (per-utterance
    controls and `stream` included: the session keeps the device table of its rows).  The chunks of
    session.generate(n), concatenated, are bit for bit generate(total, same arguments).  The
    session owns its workspace and is bound to the weights as they are now: after an optimizer step, set_weights,
    finalize_variable_values, or entering / leaving averaged_weights() its generate raises RuntimeError.
    start: an int >= 0, the index of the sequence's first sample -- the draw of sample t uses the
    Philox counter (stream, t), so a sequence begun at `start` draws what a request admitted at that position draws
    (GenerationSession.admit).  start > 0 needs per-row controls: passing stream= is enough.
    own_clock=True: every row counts from `start` -- sample t is drawn from counter (stream, t - start),
    so the session is bit for bit the session with start=0, stochastic draws included.  Needs per-row controls too.
    hop (conditioning='local'): the samples per condition frame; session.generate splits its chunks at
    the frame boundaries and raises ValueError at the chunk that would run past the last frame."""
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
      raise ValueError(f'start must be an int >= 0 (got {start!r})')
    if not isinstance(own_clock, bool):
      raise ValueError(f'own_clock must be a bool (got {own_clock!r})')
    condition, frames, hop = self._local_frames(condition, hop, use_queues)
    sampling, condition, window, batch_size = self._generation_args(batch_size, condition, sample, deterministic,
                                                                    temperature, top_k, seed, top_p, stream)
    if start > 0 and not isinstance(sampling, _RowControls):
      raise ValueError('start > 0 needs per-row sampling controls: pass stream= (one Philox stream id per utterance)')
    if own_clock and not isinstance(sampling, _RowControls):
      raise RuntimeError('generation session: own_clock needs per-row controls (create the session with stream=)')
    return GenerationSession(self, sampling, condition, window, batch_size, use_queues, deterministic, int(start), own_clock,
                             frames, hop)

  def generate_stream(self, length, chunk, **kwargs):
    """Generator over a generation_session(**kwargs): yields (B, min(chunk, rest), 1) tensors until `length` samples are
    out; concatenated they are generate(length, **kwargs).  The arguments are checked here, not at the first next()."""
    length, chunk = int(length), int(chunk)
    if chunk < 1:
      raise ValueError(f'chunk must be >= 1 (got {chunk})')
    session = self.generation_session(**kwargs)

    def pieces():
      while session.position < length:
        yield session.generate(min(chunk, length - session.position))
    return pieces()

