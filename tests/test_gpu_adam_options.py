"""Adam(global_clipnorm / clipvalue / weight_decay / amsgrad) on the GPU against tests/adam_reference.py, the fp64
restatement of one step.

The tests write ``model.flat_grads`` themselves and call ``optimizer.apply_gradients(model)``, so the gradient is known
exactly; every step is compared, elementwise, with the restatement of that step from the state read back before it:

    m        8u (|m| + |g'|)                       u = 2^-24
    v, vhat  12u (|v| + g'^2)
    p        4u |p| + 24u alpha |m| / (sqrt(v or vhat) + eps)

Roundings the kernel actually makes in the specified expressions (first order, each at most u relative):
  g'    global norm: per-tensor sum to float, (float)N^2, sqrtf, the division, the product: 4u |g'| (N^2 carries 2u, the root
        halves it and adds its own).  Value clip and no clip: none.
  m     g' - m and the fused multiply-add: (4u |g'| + u |g' - m|)(1 - beta_1) + u |m| <= 1.6u |m| + 0.5u |g'| at beta_1 = 0.9.
  v     g' g' (8u + u), the difference, the fused multiply-add: (9u g'^2 + u |g'^2 - v|)(1 - beta_2) + u v <= 1.1u v + 0.01u g'^2.
  p     decay: p wd, the product with lr, the difference (the first two weigh wd lr): <= 1.01u |p|; update: sqrtf (u/2 from
        v, u of its own), the sum with eps, alpha m (u, and m's own error), the division, the difference: about
        (1.6 + 0.5 |g'|/|m| + 4) u of the update, and u |p|.  2u |p| + (6 + 0.5 |g'|/|m|) u update: inside the bar while
        |g'| <= 36 |m|, which the crafted gradients keep (the same sign from step to step: no cancellation in m).
  ema   (no bar in the issue) p's error, p - a, the fused multiply-add: p's bar + 4u (|a| + |p|).
So the bars hold with room; they stay as the issue states them, only the denominator of p's takes vhat under amsgrad (what
the step divided by; vhat >= v, so this is the tighter bar).

Every case is also sensitive: the nearest wrong candidate named in its docstring lies at least 100 bars away somewhere."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import adam_reference as AR

pytestmark = pytest.mark.gpu

# the `small` network of tests/test_gpu_clip_order.py: the 40 x 256 output kernel (10240 floats) is longer than the 32 x 256
# threads of one grid row, so the grid-stride loop wraps; the biases are short tensors at offsets that are no multiple of a wave
KW = dict(blocks=6, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[48, 40],
          activation='leaky_relu', bits=8, l2_reg_factor=0.001)
GLOBAL_B, T, SEED = 4, 300, 7
U = AR.U


def dev():
  return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def model():
  from wavenets_amd import WaveNet
  m = WaveNet(**KW, device=dev(), seed=SEED)
  m.build((1, 8, 1))
  lens = [int(np.prod(s)) for s in m._shapes]
  assert max(lens) == 40 * 256 > 32 * 256 and any(o % 64 for o in m._offsets) and min(lens) < 64
  return m


def _tensors(model):
  return [(o, int(np.prod(s))) for o, s in zip(model._offsets, model._shapes)]


def _rand(n, lo, hi, seed):
  """fp32 values of magnitude in [lo, hi] and random sign: nothing near zero, so relative statements hold everywhere."""
  gen = torch.Generator().manual_seed(seed)
  mag = lo + (hi - lo) * torch.rand(n, generator=gen)
  sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
  return (mag * sign).float()


@pytest.fixture(scope='module')
def p_init(model):
  return _rand(model.flat_params.numel(), 0.05, 0.2, 11)


def _fresh(model, p_init, **kw):
  """The model at p_init with a new optimizer (not compiled: apply_gradients is called directly)."""
  from wavenets_amd import Adam
  model.flat_params.data.copy_(p_init.to(dev()))
  opt = Adam(**kw)
  opt.build(model)
  return opt


def _state(model, opt):
  torch.cuda.synchronize()
  s = {'p': model.flat_params.data, 'm': opt.m, 'v': opt.v, 'vhat': opt.vhat, 'ema': opt.ema}
  return {k: (None if t is None else t.detach().cpu().numpy().copy()) for k, t in s.items()}


def _apply(model, opt, g, skip=None):
  model.flat_grads.copy_(torch.as_tensor(g).to(dev()))
  opt.apply_gradients(model, skip_flag=skip)
  return _state(model, opt)


def _ref(model, opt, before, g, t, **over):
  f = opt.ema_overwrite_frequency
  kw = dict(lr=opt.learning_rate, beta_1=opt.beta_1, beta_2=opt.beta_2, epsilon=opt.epsilon, clipnorm=opt.clipnorm,
            global_clipnorm=opt.global_clipnorm, clipvalue=opt.clipvalue, weight_decay=opt.weight_decay,
            decays=opt.decays(model) if opt.weight_decay else None, amsgrad=opt.amsgrad,
            ema=before['ema'] if opt.use_ema else None, ema_momentum=opt.ema_momentum,
            ema_overwrite=bool(opt.use_ema and f is not None and t % f == 0))
  kw.update(over)
  return AR.adam_step(before['p'], before['m'], before['v'], before['vhat'], np.asarray(g), t, _tensors(model), **kw)


def _bars(ref, before=None):
  b = AR.bars(ref)
  b['vhat'] = b['v']
  if ref['ema'] is not None:
    b['ema'] = b['p'] + 4 * U * (np.abs(before['ema'].astype(np.float64)) + np.abs(ref['p_step']))
  return b


def _check(got, ref, before=None, keys=('m', 'v', 'p'), what=''):
  """Elementwise |got - ref| <= bar; prints the worst ratio per quantity before asserting."""
  bars = _bars(ref, before)
  for k in keys:
    r, g = ref[k], got[k].astype(np.float64)
    assert np.array_equal(np.isnan(r), np.isnan(g)), (what, k, 'NaN pattern')
    ok = ~np.isnan(r)
    bar = bars[k][ok]
    if k == 'p' and ref['ema'] is not None and not np.array_equal(ref['p'], ref['p_step']):
      bar = bars['ema'][ok]                                  # p overwritten by the average carries the average's bar
    err = np.abs(g[ok] - r[ok])
    ratio = float(np.max(err / np.maximum(bar, 1e-300))) if err.size else 0.0
    print(f'{what} {k}: worst error / bar = {ratio:.3f}')
    assert np.all(err <= bar), (what, k, ratio)


def _far(cand, ref_value, bar, what, bars_away=100.0):
  """A wrong candidate must lie >= 100 bars from the restatement somewhere (else the case could not tell them apart)."""
  ok = ~(np.isnan(cand) | np.isnan(ref_value))
  ratio = float(np.max(np.abs(cand[ok] - ref_value[ok]) / np.maximum(bar[ok], 1e-300)))
  print(f'candidate "{what}": {ratio:.4g} bars away')
  assert ratio >= bars_away, (what, ratio)


def _bits(a, b):
  return a is None and b is None or np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------
# 1. global norm
# ------------------------------------------------------------------------------------------
def _heavy_gradient(model, seed=21):
  """The output kernel (the longest tensor) carries almost all of the norm: magnitudes ~1 there, ~0.1 elsewhere."""
  n = model.flat_params.numel()
  tensors = _tensors(model)
  big = max(range(len(tensors)), key=lambda i: tensors[i][1])
  g = _rand(n, 0.05, 0.15, seed)
  o, ln = tensors[big]
  g[o:o + ln] = _rand(ln, 0.5, 1.5, seed + 1)
  return g.numpy(), big


def test_global_norm_scales_all_tensors_by_one_factor(model, p_init):
  """global_clipnorm = half the fp64 norm, two steps.  Candidates: the per-tensor factor (clipnorm's); the factor of the
  largest tensor alone (its norm in place of the whole gradient's)."""
  g, big = _heavy_gradient(model)
  tensors = _tensors(model)
  N = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
  o, ln = tensors[big]
  Nbig = float(np.sqrt(np.sum(g[o:o + ln].astype(np.float64) ** 2)))
  assert 0.9 < Nbig / N < 0.999
  c = N / 2
  opt = _fresh(model, p_init, learning_rate=1e-2, global_clipnorm=c)
  for t in (1, 2):
    before = _state(model, opt)
    got = _apply(model, opt, g)
    ref = _ref(model, opt, before, g, t)
    if t == 1:
      assert np.allclose(ref['g'], g.astype(np.float64) * (f32c := AR.f32(c)) / N, rtol=1e-12)
    _check(got, ref, what=f'global norm step {t}')
    bars = _bars(ref)
    per_tensor = _ref(model, opt, before, g, t, global_clipnorm=None, clipnorm=c)
    _far(per_tensor['m'], ref['m'], bars['m'], 'per-tensor factor')
    lone = g.astype(np.float64) * (f32c / Nbig)
    _far(before['m'] + (lone - before['m']) * (1.0 - AR.f32(0.9)), ref['m'], bars['m'], 'factor of the largest tensor alone')
  assert opt.ext_steps == 2


def test_global_norm_inside_the_bound_is_the_run_without_clipping(model, p_init):
  g, _ = _heavy_gradient(model, seed=31)
  N = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
  runs = {}
  for name, kw in (('bound', dict(global_clipnorm=2 * N)), ('at', dict(global_clipnorm=float(np.float32(N) * np.float32(1.000001)))),
                   ('none', {})):
    opt = _fresh(model, p_init, learning_rate=1e-2, **kw)
    for _ in range(2):
      runs[name] = _apply(model, opt, g)
    assert opt.ext_steps == (0 if name == 'none' else 2)
  for name in ('bound', 'at'):
    for k in ('p', 'm', 'v'):
      assert _bits(runs[name][k], runs['none'][k]), (name, k)


def test_global_norm_with_an_inf_poisons_every_tensor_and_the_skip_flag_holds(model, p_init):
  g, big = _heavy_gradient(model, seed=41)
  g = g.copy()
  g[_tensors(model)[3][0] + 1] = np.inf
  opt = _fresh(model, p_init, learning_rate=1e-2, global_clipnorm=1.0)
  before = _state(model, opt)
  skipped = _apply(model, opt, g, skip=torch.ones(1, device=dev()))
  for k in ('p', 'm', 'v'):
    assert _bits(skipped[k], before[k]), k
  opt.iterations -= 1
  got = _apply(model, opt, g, skip=torch.zeros(1, device=dev()))
  assert np.isnan(got['m']).all() and np.isnan(got['v']).all() and np.isnan(got['p']).all()
  assert np.isnan(_ref(model, opt, before, g, 1)['m']).all()


# ------------------------------------------------------------------------------------------
# 2. value clip
# ------------------------------------------------------------------------------------------
def test_value_clip_clamps_and_keeps_nan(model, p_init):
  """Elements at +-c exactly, just inside, far outside, and one NaN, in a short bias and in the wrapped output kernel.
  Candidate: the clamp by fminf(fmaxf()), which turns the NaN into +-c."""
  c = 0.5
  n = model.flat_params.numel()
  g = _rand(n, 0.1, 1.5, 51).numpy()                                  # both sides of c
  tensors = _tensors(model)
  big = max(range(len(tensors)), key=lambda i: tensors[i][1])
  short = min(range(len(tensors)), key=lambda i: tensors[i][1])
  inside = np.nextafter(np.float32(c), np.float32(0))
  special = np.array([c, -c, inside, -inside, 1e30, -1e30, np.inf, np.nan], dtype=np.float32)
  spots = []
  for o in (tensors[short][0], tensors[big][0] + 32 * 256 + 5, tensors[big][0] + tensors[big][1] - len(special)):
    g[o:o + len(special)] = special
    spots.append(o)
  opt = _fresh(model, p_init, learning_rate=1e-2, clipvalue=c)
  before = _state(model, opt)
  got = _apply(model, opt, g)
  ref = _ref(model, opt, before, g, 1)
  assert np.count_nonzero(np.abs(ref['g']) == c) > n // 2 and np.count_nonzero(np.abs(ref['g']) < c) > n // 10
  _check(got, ref, what='value clip')
  b1 = 1.0 - AR.f32(0.9)
  for o in spots:
    want = np.array([c, -c, inside, -inside, c, -c, c], dtype=np.float64) * b1
    assert np.all(np.abs(got['m'][o:o + 7] - want) <= 8 * U * 11 * np.abs(want))
    assert got['m'][o + 2] != got['m'][o] and np.isnan(got['m'][o + 7]) and np.isnan(got['p'][o + 7])   # fminf(fmaxf()) gives +-c * b1
  assert np.count_nonzero(np.isnan(got['m'])) == len(spots)


# ------------------------------------------------------------------------------------------
# 3. decay
# ------------------------------------------------------------------------------------------
def test_decay_before_the_update_scaled_by_lr_and_not_on_excluded_tensors(model, p_init):
  """lr = 1e-2, weight_decay = 0.1, biases excluded, one tensor with a zero gradient; two steps.  Candidates: decay after
  the update; scaled by alpha; added to the gradient (the L2 form); unscaled."""
  lr, wd = 1e-2, 0.1
  n = model.flat_params.numel()
  tensors = _tensors(model)
  g = _rand(n, 0.5, 1.5, 61).numpy()
  zero = next(i for i, nm in enumerate(model.variable_names) if nm.endswith('kernel') and tensors[i][1] > 1000)
  zo, zl = tensors[zero]
  g[zo:zo + zl] = 0.0
  opt = _fresh(model, p_init, learning_rate=lr)
  plain = [_apply(model, opt, g) for _ in range(2)]
  assert opt.ext_steps == 0
  from wavenets_amd import Adam
  model.flat_params.data.copy_(p_init.to(dev()))
  opt = Adam(learning_rate=lr, weight_decay=wd)
  opt.exclude_from_weight_decay(var_names=['bias'])
  decays = opt.decays(model)
  assert not all(decays) and any(decays) and decays[zero]
  lr32, wd32 = AR.f32(lr), AR.f32(wd)
  for t in (1, 2):
    before = _state(model, opt) if t > 1 else {'p': p_init.numpy(), 'm': np.zeros(n, np.float32), 'v': np.zeros(n, np.float32),
                                               'vhat': None, 'ema': None}
    got = _apply(model, opt, g)
    ref = _ref(model, opt, before, g, t)
    _check(got, ref, what=f'decay step {t}')
    bars = _bars(ref)
    p, upd = before['p'].astype(np.float64), None
    dec = np.zeros(n, dtype=bool)
    for (o, ln), d in zip(tensors, decays):
      dec[o:o + ln] = d
    upd = ref['alpha'] * ref['m'] / (np.sqrt(ref['v']) + ref['eps'])
    cands = {'after the update': np.where(dec, (p - upd) - ((p - upd) * wd32) * lr32, p - upd),
             'scaled by alpha': np.where(dec, p - (p * wd32) * ref['alpha'], p) - upd,
             'unscaled': np.where(dec, p - p * wd32, p) - upd}
    for name, cand in cands.items():
      _far(cand, ref['p'], bars['p'], name)
    gl2 = np.where(dec, g + wd32 * p, g)
    _far(before['m'] + (gl2 - before['m']) * (1.0 - AR.f32(0.9)), ref['m'], bars['m'], 'added to the gradient (L2)')
    # excluded tensors: the run without decay, bit for bit; a zero gradient still decays (and moves nothing else)
    for (o, ln), d in zip(tensors, decays):
      if not d:
        for k in ('p', 'm', 'v'):
          assert _bits(got[k][o:o + ln], plain[t - 1][k][o:o + ln]), (k, o)
    assert not got['m'][zo:zo + zl].any() and not got['v'][zo:zo + zl].any()
    assert np.all(got['p'][zo:zo + zl] != before['p'][zo:zo + zl])
    assert np.all(np.abs(got['p'][zo:zo + zl] - (p[zo:zo + zl] - (p[zo:zo + zl] * wd32) * lr32)) <= 4 * U * np.abs(p[zo:zo + zl]))
  assert opt.ext_steps == 2 and opt._decay_flags is not None


# ------------------------------------------------------------------------------------------
# 4. amsgrad
# ------------------------------------------------------------------------------------------
def test_amsgrad_vhat_holds_while_v_falls(model, p_init):
  """Gradient x10 at step 1, x0.1 at steps 2-3: v falls, vhat holds and is the denominator.  Candidates: v overwritten by
  vhat; vhat not fed to the denominator."""
  n = model.flat_params.numel()
  base = _rand(n, 0.5, 1.5, 71).numpy()
  opt = _fresh(model, p_init, learning_rate=1e-2, amsgrad=True)
  assert opt.vhat is not None and not opt.vhat.any()
  for t, f in ((1, 10.0), (2, 0.1), (3, 0.1)):
    g = (base * np.float32(f)).astype(np.float32)
    before = _state(model, opt)
    got = _apply(model, opt, g)
    ref = _ref(model, opt, before, g, t)
    _check(got, ref, keys=('m', 'v', 'vhat', 'p'), what=f'amsgrad step {t}')
    if t > 1:
      bars = _bars(ref)
      assert np.all(got['v'] < before['v']) and _bits(got['vhat'], before['vhat'])
      _far(ref['vhat'], ref['v'], bars['v'], 'v overwritten by vhat')
      _far(before['p'] - ref['alpha'] * ref['m'] / (np.sqrt(ref['v']) + ref['eps']), ref['p'], bars['p'],
           'vhat not fed to the denominator')
    else:
      assert _bits(got['vhat'], got['v'])
  assert opt.ext_steps == 3


# ------------------------------------------------------------------------------------------
# 5. combinations
# ------------------------------------------------------------------------------------------
def _steps_gradients(model, seed):
  base = _heavy_gradient(model, seed)[0]
  return [(base * np.float32(f)).astype(np.float32) for f in (10.0, 0.1, 0.1)]        # the same signs: no cancellation in m


COMBOS = {'global_clipnorm': dict(global_clipnorm=20.0), 'clipvalue': dict(clipvalue=0.5), 'weight_decay': dict(weight_decay=0.1),
          'amsgrad': dict(amsgrad=True),
          'all': dict(global_clipnorm=20.0, weight_decay=0.1, amsgrad=True)}


@pytest.mark.parametrize('name', list(COMBOS))
def test_use_ema_with_each_keyword(model, p_init, name):
  """Three steps with the keyword alone, with use_ema, and with ema_overwrite_frequency=2.  The average follows the p of the
  update; without an overwrite p, m, v (and vhat) are bit for bit those of the run without use_ema; every run follows its
  restatement.  `all`: the four families -- a clip, the decay (biases excluded), amsgrad, the average -- at once."""
  from wavenets_amd import Adam
  gs = _steps_gradients(model, 81)
  runs = {}
  for ema_kw in ({}, dict(use_ema=True, ema_momentum=0.9), dict(use_ema=True, ema_momentum=0.9, ema_overwrite_frequency=2)):
    model.flat_params.data.copy_(p_init.to(dev()))
    opt = Adam(learning_rate=1e-2, **COMBOS[name], **ema_kw)
    if opt.weight_decay:
      opt.exclude_from_weight_decay(var_names=['bias'])
    opt.build(model)
    if opt.use_ema:
      assert _bits(_state(model, opt)['ema'], p_init.numpy())
    states = []
    for t, g in enumerate(gs, 1):
      before = _state(model, opt)
      got = _apply(model, opt, g)
      ref = _ref(model, opt, before, g, t)
      keys = ('m', 'v', 'p') + (('vhat',) if opt.amsgrad else ()) + (('ema',) if opt.use_ema else ())
      _check(got, ref, before, keys=keys, what=f'{name} {sorted(ema_kw)} step {t}')
      if opt.ema_overwrite_frequency and t == 2:
        assert _bits(got['p'], got['ema']) and not np.array_equal(ref['p'], ref['p_step'])
      states.append(got)
    assert opt.ext_steps == 3
    runs[len(ema_kw)] = states
  for t in range(3):
    for k in ('p', 'm', 'v', 'vhat'):
      assert _bits(runs[2][t][k], runs[0][t][k]), (t, k)                    # the average observes
  for k in ('p', 'm', 'v', 'vhat', 'ema'):
    assert _bits(runs[3][0][k], runs[2][0][k]), k                           # the same until the first overwrite
  assert not _bits(runs[3][1]['p'], runs[2][1]['p'])


# ------------------------------------------------------------------------------------------
# 6. default path
# ------------------------------------------------------------------------------------------
def _data():
  from wavenets_amd.data import synthetic_waveforms
  return synthetic_waveforms(GLOBAL_B, T + 1, seed=99, device='cpu')


def test_default_path_is_the_existing_entry_point_bit_for_bit():
  """Adam(clipnorm=1.0), three real train_steps: after every step p, m, v equal the existing wn_adam_step_guarded called
  directly on a clone of the state before it, with the step's gradient (the step leaves it in flat_grads)."""
  from wavenets_amd import Adam, WaveNet, _lib
  m = WaveNet(**KW, device=dev(), seed=SEED)
  opt = Adam(learning_rate=5e-4, clipnorm=1.0)
  m.compile(optimizer=opt)
  x = _data().to(dev())
  logs = []
  for t in (1, 2, 3):
    if t == 1:
      m.build((1, 8, 1))
    clone = {'p': m.flat_params.data.clone(), 'm': opt.m.clone(), 'v': opt.v.clone()}
    logs.append(m.train_step(x))
    scratch = torch.zeros(len(m.variable_names) + 8, device=dev())
    _lib.check(_lib.lib().wn_adam_step_guarded(m._plan, _lib.ptr(clone['p']), _lib.ptr(m.flat_grads), _lib.ptr(clone['m']),
                                               _lib.ptr(clone['v']), t, 5e-4, 0.9, 0.999, 1e-7, 1.0, _lib.ptr(scratch), None,
                                               _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, got in (('p', m.flat_params.data), ('m', opt.m), ('v', opt.v)):
      assert torch.equal(got.view(torch.int32), clone[k].view(torch.int32)), (t, k)
  assert opt.ext_steps == 0 and opt.iterations == 3 and opt.vhat is None and opt._decay_flags is None
  assert all(np.isfinite(l['loss']) for l in logs) and m.train_guard_trips == 0


def test_keywords_at_their_off_values_take_the_old_entry_points(model, p_init, monkeypatch):
  from wavenets_amd import _lib
  g = _rand(model.flat_params.numel(), 0.5, 1.5, 91).numpy()
  L = _lib.lib()
  calls = []

  class Spy:
    def __getattr__(self, name):
      fn = getattr(L, name)
      if name.startswith('wn_adam_step') or name.startswith('wn_clip_gradients'):
        calls.append(name)
      return fn
  monkeypatch.setattr(_lib, 'lib', lambda: Spy())
  for kw, want in ((dict(clipnorm=1.0, weight_decay=0.0, amsgrad=False), 'wn_adam_step_guarded'),
                   (dict(weight_decay=0.0, use_ema=True), 'wn_adam_step_ema'),
                   (dict(weight_decay=None), 'wn_adam_step_guarded'),
                   (dict(weight_decay=1e-3), 'wn_adam_step_ext'), (dict(amsgrad=True), 'wn_adam_step_ext'),
                   (dict(clipvalue=1.0), 'wn_adam_step_ext'), (dict(global_clipnorm=1.0, use_ema=True), 'wn_adam_step_ext')):
    del calls[:]
    opt = _fresh(model, p_init, **kw)
    _apply(model, opt, g)
    assert calls == [want], (kw, calls)
    assert opt.ext_steps == int(want == 'wn_adam_step_ext')


# ------------------------------------------------------------------------------------------
# 7. the fused step
# ------------------------------------------------------------------------------------------
def test_train_step_with_global_clipnorm_and_a_forced_skip():
  """Three train_steps with global_clipnorm: flat_grads (left in place by the step) restated in fp64 into p, m, v.  Step 2
  is forced to skip: the range flag in the bucket's tail is raised behind the step's own loss kernels, so the Adam launch
  must leave the state alone, the host sees the flag, and the repeat (exact-fp32 kernels) lands on the same iteration."""
  from wavenets_amd import Adam, WaveNet
  m = WaveNet(**KW, device=dev(), seed=SEED)
  c = 0.05
  opt = Adam(learning_rate=5e-4, global_clipnorm=c)
  m.compile(optimizer=opt)
  m.build((1, 8, 1))
  m.early_logs = False                             # the step's scalars are read behind the (here absent) all-reduce
  x = _data().to(dev())
  n = m.flat_params.numel()
  inner = m.loss_and_grads
  seen = {'calls': 0, 'force': False, 'at_repeat': None}

  def loss_and_grads(*a, **kw):
    out = inner(*a, **kw)
    seen['calls'] += 1
    if seen['force']:
      seen['force'] = False
      m._grad_bucket[n + 2] = 1.0                  # the range flag of this pass
    elif seen['at_repeat'] == 'next':
      seen['at_repeat'] = _state(m, opt)
    return out
  m.loss_and_grads = loss_and_grads
  for t in (1, 2, 3):
    before = _state(m, opt)
    if t == 2:
      seen['force'], seen['at_repeat'] = True, 'next'
    calls = seen['calls']
    m.train_step(x)
    assert opt.iterations == t and seen['calls'] - calls == (2 if t == 2 else 1)
    if t == 2:
      assert m.train_guard_trips == 1
      for k in ('p', 'm', 'v'):
        assert _bits(seen['at_repeat'][k], before[k]), k                  # the skipped launch moved nothing
    got = _state(m, opt)
    g = m.flat_grads.detach().cpu().numpy().copy()
    N = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    print(f'step {t}: gradient norm {N:.4f}, global_clipnorm {c}')
    assert N > 2 * c                                                      # the clip acts
    ref = _ref(m, opt, before, g, t)
    _check(got, ref, what=f'train_step {t}')
    _far(_ref(m, opt, before, g, t, global_clipnorm=None, clipnorm=c)['m'], ref['m'], _bars(ref)['m'], 'per-tensor factor')
  assert opt.ext_steps == 4                        # three steps and the skipped launch


# ------------------------------------------------------------------------------------------
# 8. data parallel
# ------------------------------------------------------------------------------------------
DP_C, DP_STEPS = 0.05, 2


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _worker(rank, world, port, out_dir, flag):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  torch.cuda.set_device(0)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from wavenets_amd import Adam, WaveNet, dp
  m = WaveNet(**KW, device=dev(), seed=SEED)
  opt = Adam(learning_rate=5e-4, global_clipnorm=DP_C, clip_before_reduce=flag)
  m.compile(optimizer=opt)
  m.build((1, 8, 1))
  x = _data()[dp.shard_rows(GLOBAL_B, world, rank)].to(dev())
  local, clipped, inner = [], [], opt.clip_local_gradients

  def clip_local_gradients(model):
    torch.cuda.synchronize()
    local.append(model.flat_grads.detach().cpu().numpy().copy())          # this replica's own gradient, unclipped
    inner(model)
    torch.cuda.synchronize()
    clipped.append(model.flat_grads.detach().cpu().numpy().copy())        # ... and as it goes into the all-reduce
  opt.clip_local_gradients = clip_local_gradients
  steps = []
  for _ in range(DP_STEPS):
    before = _state(m, opt)
    m.train_step(x)
    steps.append({'before': before, 'after': _state(m, opt), 'local': local[-1], 'sent': clipped[-1]})
  torch.save({'steps': steps, 'trips': m.train_guard_trips, 'ext': opt.ext_steps}, os.path.join(out_dir, f'flag{int(flag)}_rank{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


def test_two_ranks_global_clipnorm_in_both_orders(tmp_path, model):
  """Two ranks on one GPU over gloo.  clip_before_reduce off: the summed gradient is clipped inside the step; on: each
  replica's own gradient is clipped ahead of the sum and the step clips nothing.  Replicas are bit-equal; each order follows
  the restatement of that order from the two shards' gradients gathered here -- on: every shard's clip against fp64, then the
  step from the fp32 sum of the clipped shards (what the kernel is handed); off: the step, clip included, from the fp32 sum
  of the shards -- and the two orders lie far apart."""
  tensors = _tensors(model)
  got, refs = {}, {}
  for flag in (False, True):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), flag), nprocs=2, join=True)
    r0 = torch.load(tmp_path / f'flag{int(flag)}_rank0.pt', weights_only=False)
    r1 = torch.load(tmp_path / f'flag{int(flag)}_rank1.pt', weights_only=False)
    assert r0['trips'] == r1['trips'] == 0 and r0['ext'] == r1['ext'] == DP_STEPS
    for s0, s1 in zip(r0['steps'], r1['steps']):
      for k in ('p', 'm', 'v'):
        assert _bits(s0['after'][k], s1['after'][k]), (flag, k)
      assert not np.array_equal(s0['local'], s1['local'])
    for t, (s0, s1) in enumerate(zip(r0['steps'], r1['steps']), 1):
      shards = [s0['local'], s1['local']]
      for sh in shards:
        assert np.sqrt(np.sum(sh.astype(np.float64) ** 2)) > 2 * DP_C
      b = s0['before']
      if flag:
        # each replica's own gradient against the fp64 clip of it (4u |g'|, as in the pre-reduce test below); the step is
        # then handed the fp32 sum of the two clipped gradients (two ranks: one addition, the same on both) and clips nothing
        for sh, sent in zip(shards, (s0['sent'], s1['sent'])):
          want = AR.clip(sh, tensors, global_clipnorm=DP_C)
          assert np.all(np.abs(sent - want) <= 4 * U * np.abs(want)) and not np.array_equal(sent, sh)
        ref = AR.adam_step(b['p'], b['m'], b['v'], None, s0['sent'] + s1['sent'], t, tensors, lr=5e-4)
        order = sum(AR.clip(sh, tensors, global_clipnorm=DP_C) for sh in shards)
      else:
        for sh, sent in zip(shards, (s0['sent'], s1['sent'])):
          assert np.array_equal(sent, sh)                                     # nothing is clipped ahead of the sum
        ref = AR.adam_step(b['p'], b['m'], b['v'], None, shards[0] + shards[1], t, tensors, lr=5e-4, global_clipnorm=DP_C)
        order = AR.clip(shards[0].astype(np.float64) + shards[1], tensors, global_clipnorm=DP_C)
      _check(s0['after'], ref, what=f'clip_before_reduce={flag} step {t}')
      # the gradient the step saw is the fp64 gradient of this order: 4u per clipped part and u of the sum, 5u of the parts
      # (off: u of the sum, and as much through N), asked with 6u
      parts = sum(np.abs(AR.clip(sh, tensors, global_clipnorm=DP_C)) for sh in shards) if flag else np.abs(order)
      assert np.all(np.abs(ref['g'] - order) <= 6 * U * parts)
      if t == 1:
        got[flag], refs[flag] = s0['after'], ref
  _far(refs[True]['m'], refs[False]['m'], _bars(refs[False])['m'], 'the other order')
  _far(got[True]['m'].astype(np.float64), refs[False]['m'], _bars(refs[False])['m'], 'the other order, as run')


@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_pre_reduce_clips_stay_inside_the_gradient(model, shift):
  """wn_clip_gradients_ext alone on a gradient that starts ``shift`` floats behind a 16-byte boundary, sentinels on both
  sides: the global form against fp64 within 4u |g'| (roundings: the stored sum, (float)N^2 and sqrtf leave 2u on N, the
  division 3u on the factor, the product 4u), bit-identical inside the bound; the value form exact, NaN kept."""
  from wavenets_amd import _lib
  n, nt = model.flat_params.numel(), len(model.variable_names)
  tensors = _tensors(model)
  flat = torch.from_numpy(_heavy_gradient(model, seed=101)[0]).clone()
  flat[n - 1] = float('nan') if shift == 3 else flat[n - 1]
  pad = 32
  sentinel = torch.arange(2 * pad + shift, dtype=torch.float32) * 1.25 + 1000.5

  def run(mode, c, g_in):
    buf = torch.empty(pad + shift + n + pad, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    buf[:pad + shift] = sentinel[:pad + shift].to(dev())
    buf[pad + shift + n:] = sentinel[pad + shift:].to(dev())
    g_dev = buf[pad + shift:pad + shift + n]
    g_dev.copy_(g_in.to(dev()))
    scratch = torch.full((nt + 8,), -1.0, dtype=torch.float32, device=dev())
    _lib.check(_lib.lib().wn_clip_gradients_ext(model._plan, _lib.ptr(g_dev), mode, c, _lib.ptr(scratch), _lib.stream_ptr()))
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.equal(out[:pad + shift], sentinel[:pad + shift])
    assert torch.equal(out[pad + shift + n:], sentinel[pad + shift:])
    assert torch.equal(scratch.cpu()[nt:], torch.full((8,), -1.0))              # num_tensors floats of scratch, no more
    return out[pad + shift:pad + shift + n].numpy(), scratch.cpu()[:nt].numpy()

  clean = flat.clone()
  clean[n - 1] = 0.25
  N = float(np.sqrt(np.sum(clean.numpy().astype(np.float64) ** 2)))
  out, norms2 = run(_lib.WN_CLIP_GLOBAL_NORM, N / 2, clean)
  ref = AR.clip(clean.numpy(), tensors, global_clipnorm=N / 2)
  assert np.all(np.abs(out - ref) <= 4 * U * np.abs(ref)) and not np.array_equal(out, clean.numpy())
  assert abs(float(np.sum(norms2.astype(np.float64))) - N * N) <= 1e-6 * N * N
  inside, _ = run(_lib.WN_CLIP_GLOBAL_NORM, 2 * N, clean)
  assert _bits(inside, clean.numpy())
  vals, _ = run(_lib.WN_CLIP_VALUE, 0.1, flat)
  want = AR.clip(flat.numpy(), tensors, clipvalue=0.1).astype(np.float32)
  assert np.array_equal(np.isnan(vals), np.isnan(want)) and np.array_equal(np.nan_to_num(vals, nan=7.0), np.nan_to_num(want, nan=7.0))
  assert np.count_nonzero(vals != flat.numpy()) > n // 10 and np.count_nonzero(vals == flat.numpy()) > n // 10


# ------------------------------------------------------------------------------------------
# 9. checkpoint
# ------------------------------------------------------------------------------------------
def test_checkpoint_carries_vhat(model, p_init, tmp_path):
  """Two amsgrad steps, save, load into a fresh model and optimizer, a third step: bit for bit the uninterrupted run."""
  from wavenets_amd import Adam, WaveNet, io
  gs = _steps_gradients(model, 111)
  kw = dict(learning_rate=1e-2, amsgrad=True, weight_decay=0.1)
  opt = _fresh(model, p_init, **kw)
  model.compile(optimizer=opt)
  try:
    for g in gs[:2]:
      _apply(model, opt, g)
    path = str(tmp_path / 'ck.weights.npz')
    io.save_weights(model, path, opt)
    whole = _apply(model, opt, gs[2])
  finally:
    model.optimizer = None
  with np.load(path) as d:
    assert 'adam_vhat' in d and d['adam_vhat'].any()
  other = WaveNet(**KW, device=dev(), seed=SEED + 1)
  other.build((1, 8, 1))
  resumed = Adam(**kw)
  io.load_weights(other, path, resumed)
  assert resumed.iterations == 2
  part = _apply(other, resumed, gs[2])
  for k in ('p', 'm', 'v', 'vhat'):
    assert _bits(part[k], whole[k]), k
  assert not _bits(whole['vhat'], whole['v'])
