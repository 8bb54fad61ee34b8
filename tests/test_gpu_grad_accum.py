"""Adam(gradient_accumulation_steps=k) on the GPU: wn_grad_accumulate alone against
tests/accum_reference.py bit for bit, the cycle as the plain step on the mean bit for bit, the mean against the oracle on the
concatenated rows, a forced trip of the range guard on a storing and on the final micro-step, a checkpoint in mid-cycle, the
default optimizer as it was, and two ranks with one gradient-sized collective per cycle.

The network is the `small` one of tests/test_gpu_adam_options.py (44 tensors, 59 640 parameters); helpers follow that file."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import accum_reference as AC
import adam_reference as AR

pytestmark = pytest.mark.gpu

KW = dict(blocks=6, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[48, 40],
          activation='leaky_relu', bits=8, l2_reg_factor=0.001)
SEED, MICRO_B, T = 7, 2, 96
U = AR.U


def dev():
  return torch.device('cuda', 0)


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  """Both contraction modes of the passes, as tests/test_gpu_parity.py switches them (debug knob 1)."""
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


def _bits(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _tensors(model):
  return [(o, int(np.prod(s))) for o, s in zip(model._offsets, model._shapes)]


def _state(model, opt):
  torch.cuda.synchronize()
  s = {'p': model.flat_params.data, 'm': opt.m, 'v': opt.v, 'vhat': opt.vhat, 'ema': opt.ema, 'accum': opt.accum}
  return {k: (None if t is None else t.detach().cpu().numpy().copy()) for k, t in s.items()}


def _grads(model):
  torch.cuda.synchronize()
  return model.flat_grads.detach().cpu().numpy().copy()


def _micro_batches(count, rows=MICRO_B, seed=99):
  """``count`` different micro-batches of ``rows`` utterances."""
  from wavenets_amd.data import synthetic_waveforms
  x = synthetic_waveforms(count * rows, T + 1, seed=seed, device='cpu')
  return [x[i * rows:(i + 1) * rows].contiguous() for i in range(count)]


def _model(seed=SEED):
  from wavenets_amd import WaveNet
  m = WaveNet(**KW, device=dev(), seed=seed)
  m.build((1, 8, 1))
  return m


# ------------------------------------------------------------------------------------------
# 1. the kernel alone
# ------------------------------------------------------------------------------------------
PAD = 32
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.0], dtype=np.float32)


def _values(n, seed):
  """fp32 over 40 binades (2^-20 .. 2^20), random sign; the specials paired with each other and with ordinary values at
  the front and at random places.  No sum or quotient is subnormal: two such floats add to 0 or to at least an ulp of the
  smaller, 2^-43, and the quotients by 2, 3, 7 stay above 2^-46."""
  rng = np.random.RandomState(seed)
  v = (np.ldexp(1.0 + rng.rand(n), rng.randint(-20, 21, size=n)) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)
  for i in range(min(n, 2 * len(SPECIALS))):                   # the second round shifted by the seed: other pairings
    v[i] = SPECIALS[(i + (seed if i >= len(SPECIALS) else 0)) % len(SPECIALS)]
  if n > 64:
    where = rng.randint(0, n, size=max(8, n // 64))
    v[where] = SPECIALS[rng.randint(0, len(SPECIALS), size=where.size)]
  return v


def _place(values, shift):
  """[32 + shift sentinels | values | 32 sentinels] on the device, the values ``shift`` floats behind a 16-byte boundary."""
  n = values.size
  host = np.empty(PAD + shift + n + PAD, dtype=np.float32)
  host[:PAD + shift] = np.arange(PAD + shift, dtype=np.float32) * 1.25 + 1000.5
  host[PAD + shift + n:] = np.arange(PAD, dtype=np.float32) * 1.25 + 2000.5
  host[PAD + shift:PAD + shift + n] = values
  buf = torch.from_numpy(host).to(dev())
  assert buf.data_ptr() % 16 == 0
  return host, buf, buf[PAD + shift:PAD + shift + n]


def _call(acc_in, g_in, sa, sg, mode, k, flag):
  """One wn_grad_accumulate on fresh buffers; returns (acc, g) afterwards.  The sentinels on both sides of both buffers must
  not have moved."""
  from wavenets_amd import _lib
  n = g_in.size
  out = []
  ha, ba, va = _place(acc_in, sa)
  hg, bg, vg = _place(g_in, sg)
  assert (va.data_ptr() % 16) // 4 == sa and (vg.data_ptr() % 16) // 4 == sg
  _lib.check(_lib.lib().wn_grad_accumulate(_lib.ptr(va), _lib.ptr(vg), n, mode, k, _lib.ptr(flag), _lib.stream_ptr()))
  torch.cuda.synchronize()
  for host, buf, shift in ((ha, ba, sa), (hg, bg, sg)):
    got = buf.cpu().numpy()
    lo, hi = PAD + shift, PAD + shift + n
    assert _bits(got[:lo], host[:lo]) and _bits(got[hi:], host[hi:]), 'a sentinel moved'
    out.append(got[lo:hi].copy())
  return out


@pytest.fixture(scope='module')
def flags():
  return {0: torch.zeros(1, dtype=torch.float32, device=dev()), 1: torch.ones(1, dtype=torch.float32, device=dev())}


def _one_pass():
  from wavenets_amd import _lib
  return _lib.WN_ACCUM_ONE_PASS


@pytest.mark.parametrize('n', [1, 3, 4, 5, 7, 1023, 59641, 'one pass + 5'])
def test_kernel_alone_bit_for_bit(n, flags):
  """Every pairing of the two buffers' offsets from a 16-byte boundary (0/0 moves float4, the fifteen others run scalar),
  the three modes, k in {2, 3, 7}: the restatement's bits, NaN as NaN; FIRST overwrites an accumulator full of NaN and
  garbage; a raised flag leaves every bit of both buffers alone in every mode; a second run gives the same bits.  The last
  size lies 5 floats above what one pass of the largest grid covers, so the grid strides and an odd tail remains."""
  big = n == 'one pass + 5'
  n = _one_pass() + 5 if big else n
  assert n % 4 != 0 or not big
  g1, g2 = _values(n, 1), _values(n, 2)
  stale = _values(n, 3)
  stale[::2] = np.nan
  ks = (3,) if big else (2, 3, 7)
  for sa in range(4):
    for sg in range(4):
      more = not big or (sa, sg) in ((0, 0), (1, 2))          # the large size repeats and skips at two pairings only
      # FIRST: acc = g, whatever acc held; g stays
      acc, g = _call(stale, g1, sa, sg, AC.FIRST, 0, flags[0])
      want_acc, want_g = AC.accumulate(stale, g1, AC.FIRST)
      assert AC.same_bits(acc, want_acc) and AC.same_bits(g, want_g), ('FIRST', sa, sg)
      assert AC.same_bits(acc, g1)
      # ADD
      acc2, g = _call(want_acc, g2, sa, sg, AC.ADD, 0, None if (sa + sg) % 2 else flags[0])
      want_acc2, want_g = AC.accumulate(want_acc, g2, AC.ADD)
      assert AC.same_bits(acc2, want_acc2) and AC.same_bits(g, want_g), ('ADD', sa, sg)
      if more:
        again, _ = _call(want_acc, g2, sa, sg, AC.ADD, 0, flags[0])
        assert AC.same_bits(again, acc2)
      # FINISH: g = (g + acc) / k, acc stays
      for k in ks:
        acc3, mean = _call(want_acc2, g1, sa, sg, AC.FINISH, k, flags[0])
        want_acc3, want_mean = AC.accumulate(want_acc2, g1, AC.FINISH, k)
        assert AC.same_bits(mean, want_mean), ('FINISH', k, sa, sg)
        assert AC.same_bits(acc3, want_acc3) and AC.same_bits(acc3, want_acc2)
      # a raised flag: nothing moves, in any mode
      for mode in (AC.FIRST, AC.ADD, AC.FINISH) if more else ():
        acc4, g4 = _call(stale, g2, sa, sg, mode, 3, flags[1])
        assert AC.same_bits(acc4, stale) and AC.same_bits(g4, g2), ('skip', mode, sa, sg)
  # the quotient by 3 and by 7 is inexact somewhere, so a product with a reciprocal would show
  if n >= 1023:
    with np.errstate(all='ignore'):
      s = (g1 + want_acc2).astype(np.float32)
      s = s[np.isfinite(s)]
      for k in (3, 7):
        assert np.any(s * (np.float32(1.0) / np.float32(k)) != s / np.float32(k))


# ------------------------------------------------------------------------------------------
# 2. the cycle is the plain step on the mean
# ------------------------------------------------------------------------------------------
def _norm(x):
  return float(np.sqrt(np.sum(np.asarray(x, dtype=np.float64) ** 2)))


def _clip_choice(name, grads, tensors):
  """The clip of case ``name`` from the three micro-gradients of the first cycle, chosen so that every single micro-gradient
  is over the bound where their mean is not; returns (keywords, a host check of that condition for any later cycle)."""
  mean = AC.mean64(grads)
  if name == 'clipnorm':
    ratios = [min(_norm(g[o:o + n]) for g in grads) / max(_norm(mean[o:o + n]), 1e-300) for o, n in tensors]
    t = int(np.argmax(ratios))
    o, n = tensors[t]
    c = float(np.sqrt(min(_norm(g[o:o + n]) for g in grads) * _norm(mean[o:o + n])))
    assert min(_norm(g[o:o + n]) for g in grads) > 1.001 * c and c > 1.001 * _norm(mean[o:o + n]), ratios[t]
    # ... while other tensors are clipped either way and others never: the bound is not trivial
    assert any(_norm(mean[o:o + n]) > c for o, n in tensors) and any(max(_norm(g[o:o + n]) for g in grads) < c for o, n in tensors)
    return dict(clipnorm=c)
  if name == 'global_clipnorm':
    lo, hi = _norm(mean), min(_norm(g) for g in grads)
    assert hi > 1.002 * lo, (lo, hi)
    c = float(np.sqrt(lo * hi))
    assert hi > 1.001 * c and c > 1.001 * lo
    return dict(global_clipnorm=c)
  if name == 'clipvalue':
    c = float(np.median(np.abs(grads[0])))
    differs = (np.min(np.abs(np.stack(grads)), axis=0) > c) & (np.abs(mean) < c)
    assert differs.sum() > 100 and (np.abs(mean) > c).sum() > 100, differs.sum()
    return dict(clipvalue=c, weight_decay=0.05)
  return dict(amsgrad=True, use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=1)


@pytest.mark.parametrize('name', ['clipnorm', 'global_clipnorm', 'clipvalue', 'amsgrad_ema'])
def test_cycle_is_the_plain_step_on_the_mean_bit_for_bit(name, math_mode):
  """k = 3, two cycles of three different micro-batches.  Model A: Adam(k=3, clip) and train_step.  Model B, same weights,
  the plain Adam(clip): its three flat_grads from loss_and_grads, combined on the host by the restatement, written to
  flat_grads, one apply_gradients.  p, m, v (vhat, ema) of A are untouched after calls 1 and 2 of a cycle and equal B's bit
  for bit after call 3, A's flat_grads then holds the restated mean, and the counters follow.  The second cycle starts on an
  accumulator that still holds the first one's sums: FIRST overwrites it.  The clip is chosen (on the host, from the
  gradients) so that it acts on every single micro-gradient where it does not act on the mean."""
  from wavenets_amd import Adam
  k = 3
  xs = [x.to(dev()) for x in _micro_batches(10 if name == 'global_clipnorm' else 2 * k)]
  A, B = _model(), _model(seed=SEED + 1)
  B.flat_params.data.copy_(A.flat_params.data)
  tensors = _tensors(A)
  first = []
  for x in xs:
    loss, _, _ = B.loss_and_grads(x)
    first.append(_grads(B))
    assert float(loss[2]) == 0
  if name == 'global_clipnorm':
    # Whole gradients of different utterances are nearly parallel and of different length, so the mean of three is usually
    # longer than the shortest of them.  From ten micro-batches take the three of most equal length, where the mean is
    # shortest against them (the inputs are chosen, from gradients at the starting weights; the bound follows below).
    import itertools
    norms = [_norm(g) for g in first]
    best = max(itertools.combinations(range(len(xs)), k),
               key=lambda t: min(norms[i] for i in t) / _norm(AC.mean64([first[i] for i in t])))
    rest = [i for i in range(len(xs)) if i not in best][:k]
    xs, first = [xs[i] for i in best] + [xs[i] for i in rest], [first[i] for i in best]
  first = first[:k]
  kw = _clip_choice(name, first, tensors)
  print(name, math_mode, kw)
  optA, optB = Adam(learning_rate=5e-3, gradient_accumulation_steps=k, **kw), Adam(learning_rate=5e-3, **kw)
  A.compile(optimizer=optA)
  B.compile(optimizer=optB)
  optB.build(B)
  keys = ['p', 'm', 'v'] + (['vhat', 'ema'] if name == 'amsgrad_ema' else [])
  assert optA.accum is not None and optB.accum is None
  for cycle in range(2):
    grads = []
    for j in range(k):
      x = xs[cycle * k + j]
      loss, _, _ = B.loss_and_grads(x)
      grads.append(_grads(B))
      before = _state(A, optA)
      gen = A._train_gen
      A.train_step(x)
      after = _state(A, optA)
      assert A._train_gen == gen + (1 if j < k - 1 else 2)       # the pass counts one; the optimizer only when weights move
      if j < k - 1:
        for key in keys:
          assert _bits(after[key], before[key]), (cycle, j, key)
        assert (optA.iterations, optA.accumulated) == (cycle, j + 1)
        assert _bits(_grads(A), grads[j])                                          # a storing micro-step leaves g alone
        assert AC.same_bits(after['accum'], AC.accumulate(before['accum'], grads[j], AC.ADD if j else AC.FIRST)[0])
      else:
        assert (optA.iterations, optA.accumulated) == (cycle + 1, 0)
    mean = AC.cycle_mean(grads)
    assert _bits(_grads(A), mean), cycle                                           # what Adam was given
    B.flat_grads.copy_(torch.from_numpy(mean).to(dev()))
    optB.apply_gradients(B)
    sB = _state(B, optB)
    for key in keys:
      assert _bits(after[key], sB[key]), (cycle, key)
      assert not _bits(after[key], before[key]), (cycle, key)
    assert optB.iterations == cycle + 1
  assert optA.ext_steps == (0 if name == 'clipnorm' else 2)                        # updates that took the ext entry


# ------------------------------------------------------------------------------------------
# 3. against the oracle
# ------------------------------------------------------------------------------------------
def test_accumulated_mean_against_the_oracle_on_the_concatenated_rows(math_mode):
  """k = 2, two micro-batches of 2 rows, l2_reg_factor > 0: flat_grads after the cycle is the oracle's gradient of the 4
  concatenated rows.

  The bar is the one tests/test_gpu_parity.py applies to parameter gradients, in test_loss_and_gradients_parity and, with
  the regulariser, in test_l2_regulariser, per tensor:

      err = (g.cpu().double() - r).abs().max().item()
      assert err < 1e-4 * max(r.abs().max().item(), 1e-6) + 1e-7
  """
  from oracle import wavenet_oracle as O
  from wavenets_amd import Adam, WaveNet
  ocfg = O.OracleConfig(**KW)
  assert KW['l2_reg_factor'] > 0
  params = O.init_params(ocfg, seed=4)
  model = WaveNet(**KW, device=dev())
  model.set_weights([p.numpy() for p in params])
  opt = Adam(learning_rate=5e-4, clipnorm=1.0, gradient_accumulation_steps=2)
  model.compile(optimizer=opt)
  x = O.synthetic_waveform(2 * MICRO_B, T + 1, seed=8)
  _, _, grads_ref, _ = O.loss_and_grads(x.double(), [p.double() for p in params], ocfg)
  model.train_step(x[:MICRO_B].to(dev()))
  model.train_step(x[MICRO_B:].to(dev()))
  assert (opt.iterations, opt.accumulated) == (1, 0)
  for name, g, r in zip(model.variable_names, model.gradients(), grads_ref):
    scale = max(r.abs().max().item(), 1e-6)
    err = (g.cpu().double() - r).abs().max().item()
    assert err < 1e-4 * scale + 1e-7, (name, err, scale)


# ------------------------------------------------------------------------------------------
# 4. a forced trip of the range guard
# ------------------------------------------------------------------------------------------
def _trip_run(xs, k, trip_at, exact_at):
  """``len(xs)`` train_steps of Adam(k, clipnorm=1.0).  ``trip_at``: the call (0-based) whose first pass gets its range flag
  raised on the device behind the step's own kernels, as test_train_step_with_global_clipnorm_and_a_forced_skip does.
  ``exact_at``: the call the caller itself runs under exact_fp32(), without any trip."""
  from wavenets_amd import Adam
  m = _model()
  opt = Adam(learning_rate=5e-3, clipnorm=1.0, gradient_accumulation_steps=k)
  m.compile(optimizer=opt)
  m.early_logs = False                               # the step's scalars are read behind the (here absent) all-reduce
  n = m.flat_params.numel()
  inner = m.loss_and_grads
  seen = {'calls': 0, 'force': False, 'at_repeat': None}

  def loss_and_grads(*a, **kw):
    out = inner(*a, **kw)
    seen['calls'] += 1
    if seen['force']:
      seen['force'] = False
      m._grad_bucket[n + 2] = 1.0                    # the range flag of this pass
    elif seen['at_repeat'] == 'next':
      seen['at_repeat'] = _state(m, opt)
    return out
  m.loss_and_grads = loss_and_grads
  record = {'pairs': [], 'last_update': None}
  for i, x in enumerate(xs):
    before = _state(m, opt)
    calls = seen['calls']
    if i == trip_at:
      seen['force'], seen['at_repeat'] = True, 'next'
    if i == exact_at:
      with m.exact_fp32():
        m.train_step(x)
    else:
      m.train_step(x)
    assert seen['calls'] - calls == (2 if i == trip_at else 1)
    record['pairs'].append((opt.iterations, opt.accumulated))
    if i == trip_at:
      assert m.train_guard_trips == 1
      for key in ('p', 'm', 'v', 'accum'):           # the skipped launches moved nothing, the accumulator included
        assert _bits(seen['at_repeat'][key], before[key]), key
    if opt.accumulated == 0:
      record['last_update'] = (before, _grads(m), opt.iterations)
  record['trips'] = m.train_guard_trips
  record['end'] = _state(m, opt)
  record['model'], record['opt'] = m, opt
  return record


@pytest.mark.parametrize('where', ['storing', 'final'])
def test_forced_trip_reaches_neither_the_accumulator_nor_the_state(where, math_mode):
  """k = 3, two cycles; the trip falls on call 5 (the ADD micro-step of the second cycle, an accumulator in use) or on call
  6 (FINISH and the Adam launch).  Across the skipped launches accum, p, m and v keep their bits, train_guard_trips counts
  one, and (iterations, accumulated) are right after every call.

  The repeat runs the exact-fp32 kernels, so the run it has to equal is the run without a trip in which the caller runs
  that same micro-step under exact_fp32() -- in split mode the plain run differs from both by the split-precision error of
  one gradient, which is not the subject here (its distance is printed).  The bars are those of the pattern test after its
  tripped step: elementwise, tests/adam_reference.py's, taken from the fp64 restatement of the last update from the state
  before it and the mean left in flat_grads.  The distance to that restatement itself is printed and not asserted: the
  bar on p was derived for gradients that keep their sign from step to step (tests/test_gpu_adam_options.py's docstring),
  which three different micro-batches per cycle do not (measured on p: 1.11 bars split / storing, 1.66 split / final, 1.12
  in fp32 mode; m 0.12, v 0.08: the plain Adam launch against fp64, nothing of the accumulation).  Measured against the
  untripped run: 0.000 bars everywhere; against the plain split run 41 - 270 bars on m."""
  k = 3
  xs = [x.to(dev()) for x in _micro_batches(2 * k)]
  at = 4 if where == 'storing' else 5
  tripped = _trip_run(xs, k, trip_at=at, exact_at=None)
  untripped = _trip_run(xs, k, trip_at=None, exact_at=at)
  plain = _trip_run(xs, k, trip_at=None, exact_at=None)
  want = [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0)]
  assert tripped['pairs'] == untripped['pairs'] == plain['pairs'] == want
  assert tripped['trips'] == 1 and untripped['trips'] == 0 and plain['trips'] == 0
  before, g, t = tripped['last_update']
  m, opt = tripped['model'], tripped['opt']
  ref = AR.adam_step(before['p'], before['m'], before['v'], None, g, t, _tensors(m), lr=opt.learning_rate, clipnorm=1.0)
  bars = AR.bars(ref)
  for key in ('m', 'v', 'p'):
    got = tripped['end'][key].astype(np.float64)
    for what, other in (('restated', ref[key]), ('untripped', untripped['end'][key].astype(np.float64)),
                        ('plain', plain['end'][key].astype(np.float64))):
      err = np.abs(got - other)
      ratio = float(np.max(err / np.maximum(bars[key], 1e-300)))
      print(f'{where} {math_mode} {key}: tripped - {what}: worst error / bar = {ratio:.3f}')
      if what == 'untripped':
        assert np.all(err <= bars[key]), (key, what, ratio)
  assert _bits(tripped['end']['accum'], untripped['end']['accum'])


# ------------------------------------------------------------------------------------------
# 5. a checkpoint in mid-cycle
# ------------------------------------------------------------------------------------------
def test_checkpoint_in_mid_cycle_resumes_bit_for_bit(tmp_path, math_mode):
  """k = 2: three train_steps, save (one micro-step of the second cycle is held), the fourth; a fresh model and optimizer
  load the file and take the fourth: bit for bit the same p, m, v."""
  from wavenets_amd import Adam, io
  xs = [x.to(dev()) for x in _micro_batches(4)]
  kw = dict(learning_rate=5e-3, clipnorm=1.0, gradient_accumulation_steps=2)
  a, opt = _model(), Adam(**kw)
  a.compile(optimizer=opt)
  for x in xs[:3]:
    a.train_step(x)
  assert (opt.iterations, opt.accumulated) == (1, 1)
  path = str(tmp_path / 'mid.weights.npz')
  io.save_weights(a, path, opt)
  held = _state(a, opt)['accum']
  a.train_step(xs[3])
  whole = _state(a, opt)
  with np.load(path) as d:
    assert int(d['adam_accumulated']) == 1 and int(d['adam_iterations']) == 1 and _bits(d['adam_accum'], held)
  b, resumed = _model(seed=SEED + 1), Adam(**kw)
  b.compile(optimizer=resumed)
  io.load_weights(b, path, resumed)
  assert (resumed.iterations, resumed.accumulated) == (1, 1)
  b.train_step(xs[3])
  assert (resumed.iterations, resumed.accumulated) == (2, 0)
  part = _state(b, resumed)
  for key in ('p', 'm', 'v'):
    assert _bits(part[key], whole[key]), key


# ------------------------------------------------------------------------------------------
# 6. k = None is the optimizer as it was
# ------------------------------------------------------------------------------------------
def test_default_optimizer_never_accumulates(monkeypatch):
  from wavenets_amd import Adam, _lib
  L = _lib.lib()
  calls = []

  class Spy:
    def __getattr__(self, name):
      fn = getattr(L, name)
      if name.startswith('wn_adam_step') or name == 'wn_grad_accumulate':
        if name == 'wn_grad_accumulate':
          return lambda *a: (calls.append((name, a[3])), fn(*a))[1]
        calls.append((name, None))
      return fn
  monkeypatch.setattr(_lib, 'lib', lambda: Spy())
  xs = [x.to(dev()) for x in _micro_batches(2)]
  m, opt = _model(), Adam(learning_rate=5e-4, clipnorm=1.0)
  m.compile(optimizer=opt)
  for x in xs:
    m.train_step(x)
  assert calls == [('wn_adam_step_guarded', None)] * 2
  assert opt.accum is None and opt.gradient_accumulation_steps is None and (opt.iterations, opt.accumulated) == (2, 0)
  del calls[:]
  m, opt = _model(), Adam(learning_rate=5e-4, clipnorm=1.0, gradient_accumulation_steps=2)
  m.compile(optimizer=opt)
  for x in xs:
    m.train_step(x)
  assert calls == [('wn_grad_accumulate', _lib.WN_ACCUM_FIRST), ('wn_grad_accumulate', _lib.WN_ACCUM_FINISH),
                   ('wn_adam_step_guarded', None)]
  assert opt.accum.numel() == m.flat_params.numel() and opt.accum.dtype == torch.float32


# ------------------------------------------------------------------------------------------
# 7. two ranks
# ------------------------------------------------------------------------------------------
DP_K, DP_CYCLES = 2, 2


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _dp_steps(model, xs, trip_on_first=False):
  """DP_CYCLES cycles of Adam(k=2, clipnorm=1.0) with a compiled metric; ``trip_on_first``: this process raises the range
  flag of its first pass (a storing micro-step)."""
  from wavenets_amd import Adam, MeanSquaredError, dp
  opt = Adam(learning_rate=5e-4, clipnorm=1.0, gradient_accumulation_steps=DP_K)
  model.compile(optimizer=opt, metrics=[MeanSquaredError()])
  model.build((1, 8, 1))
  n = model.flat_params.numel()
  numels, passes, inner_reduce, inner_pass = [], [0], dp.allreduce_bucket, model.loss_and_grads

  def allreduce_bucket(bucket, group=None):
    numels.append(int(bucket.numel()))
    return inner_reduce(bucket, group)

  def loss_and_grads(*a, **kw):
    out = inner_pass(*a, **kw)
    passes[0] += 1
    if trip_on_first and passes[0] == 1:
      model._grad_bucket[n + 2] = 1.0
    return out
  dp.allreduce_bucket = allreduce_bucket
  model.loss_and_grads = loss_and_grads
  try:
    logs, pairs, per_step = [], [], []
    for x in xs:
      seen = len(numels)
      logs.append(model.train_step(x))
      pairs.append((opt.iterations, opt.accumulated))
      per_step.append(numels[seen:])
  finally:
    dp.allreduce_bucket = inner_reduce
  torch.cuda.synchronize()
  return {'params': model.flat_params.data.cpu(), 'm': opt.m.cpu(), 'v': opt.v.cpu(), 'accum': opt.accum.cpu(), 'logs': logs,
          'pairs': pairs, 'numels': per_step, 'passes': passes[0], 'trips': model.train_guard_trips, 'n': n}


def _dp_worker(rank, world, port, out_dir, trip_rank):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from wavenets_amd import WaveNet, _lib, dp
  out = {}
  for mode in ('split', 'fp32'):
    _lib.lib().wn_debug_set(1, 1 if mode == 'fp32' else 0)
    model = WaveNet(**KW, device=dev(), seed=SEED)
    xs = [x[dp.shard_rows(2 * MICRO_B, world, rank)].to(dev()) for x in _micro_batches(DP_K * DP_CYCLES, rows=2 * MICRO_B)]
    out[mode] = _dp_steps(model, xs, trip_on_first=(rank == trip_rank))
  _lib.lib().wn_debug_set(1, 0)
  torch.save(out, os.path.join(out_dir, f'trip{trip_rank}_rank{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('trip_rank', [-1, 1])
def test_two_ranks_one_gradient_sized_collective_per_cycle(tmp_path, trip_rank):
  """Two ranks on one GPU over gloo, k = 2, two cycles, both math modes in the same processes.  Replicas are bit-identical
  (parameters, moments, logs); they equal the single process on the concatenated micro-batches within the bars of
  tests/test_gpu_dp.py::test_two_rank_train_step_equals_single_process (parameters 1e-5 absolute on this network after
  three updates there, two here; loss 1e-5 relative; reg_loss 1e-6); per cycle dp.allreduce_bucket sees one call of at
  least param_count elements and k - 1 calls of 3 + metrics elements, in that order from the storing micro-steps to the
  last.  trip_rank = 1: the first pass of rank 1 alone raises its range flag, on a storing micro-step: the reduced clone
  carries it to rank 0, both skip the store and both repeat the micro-step."""
  from wavenets_amd import WaveNet, _lib
  mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path), trip_rank), nprocs=2, join=True)
  r0 = torch.load(tmp_path / f'trip{trip_rank}_rank0.pt', weights_only=False)
  r1 = torch.load(tmp_path / f'trip{trip_rank}_rank1.pt', weights_only=False)
  for mode in ('split', 'fp32'):
    a, b = r0[mode], r1[mode]
    for key in ('params', 'm', 'v'):
      assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (mode, key)
    assert a['logs'] == b['logs'] and set(a['logs'][0]) == {'loss', 'reg_loss', 'mean_squared_error'}
    assert a['pairs'] == b['pairs'] == [(0, 1), (1, 0), (1, 1), (2, 0)]
    n, small = a['n'], 3 + 1
    if trip_rank < 0:
      assert a['trips'] == b['trips'] == 0 and a['passes'] == b['passes'] == DP_K * DP_CYCLES
      for rec in (a, b):
        assert len(rec['numels']) == DP_K * DP_CYCLES
        for i, calls in enumerate(rec['numels']):
          storing = i % DP_K != DP_K - 1
          assert calls == ([small] if storing else [n + 3 + 5]), (mode, i, calls)       # the bucket: gradient + tail
          assert storing or calls[0] >= n
    else:
      assert a['trips'] == b['trips'] == 1 and a['passes'] == b['passes'] == DP_K * DP_CYCLES + 1
      assert a['numels'][0] == b['numels'][0] == [small, small]                          # the skipped store and its repeat
      assert not torch.equal(a['accum'], b['accum'])                                     # each replica's own sums
      continue                      # (the repeat ran exact-fp32 kernels: not the single process's arithmetic in split mode)
    # the single process on the concatenated micro-batches
    _lib.lib().wn_debug_set(1, 1 if mode == 'fp32' else 0)
    try:
      single = WaveNet(**KW, device=dev(), seed=SEED)
      s = _dp_steps(single, [x.to(dev()) for x in _micro_batches(DP_K * DP_CYCLES, rows=2 * MICRO_B)])
    finally:
      _lib.lib().wn_debug_set(1, 0)
    assert s['pairs'] == a['pairs']
    err = (s['params'] - a['params']).abs().max().item()
    print(f'{mode}: two ranks against one process, max |dp| = {err:.3e}')
    assert err < 1e-5, err
    for ls, la in zip(s['logs'], a['logs']):
      assert abs(ls['loss'] - la['loss']) < 1e-5 * abs(ls['loss'])
      assert abs(ls['reg_loss'] - la['reg_loss']) < 1e-6 * max(1.0, abs(ls['reg_loss']))
