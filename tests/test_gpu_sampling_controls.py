"""Sampling controls of generation and sample_waveform -- temperature, top_k, seed (semantics in
include/wn_hip.h, struct wn_sampling) -- on the GPU: exact properties first (identities, queued == sliding window, top_k = 1
is arg max, the tie rule, support, seed), then bounds derived from the number formats, then the laws against the oracle."""
import math

import pytest
import torch

from test_gpu_parity import MODEL_CASES, O, dev, make_pair

pytestmark = pytest.mark.gpu

SEED = 0x5EED1234ABCD          # a non-default Philox key with bits in both halves


def _mix128():
  return dict(blocks=6, channels=128, skip_channels=256, dilation_bound=32, final_layers_channels=[128, 128],
              activation='leaky_relu', num_mixtures=5, sampling_function='logistic', bits=16)


def _model(**kw):
  """A model that only samples (sample_waveform needs no weights)."""
  from wavenets_amd import WaveNet
  base = dict(blocks=2, channels=32, dilation_bound=2, final_layers_channels=[])
  base.update(kw)
  return WaveNet(**base, device=dev())


# ------------------------------------------------------------------------------------------
# 2. defaults and identities, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'mix128', 'cat_lpb3'])
def test_defaults_and_identities_are_bit_exact(name, queued):
  kw = _mix128() if name == 'mix128' else dict(MODEL_CASES[name])
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **kw)
  w = O.synthetic_waveform(3, model.receptive_field, seed=12).to(dev())
  n = 16
  base = model.generate(n, sample=w, use_queues=queued)
  assert torch.equal(base, model.generate(n, sample=w, use_queues=queued, temperature=1.0, top_k=0, seed=None))
  assert torch.equal(base, model.generate(n, sample=w, use_queues=queued, seed=0x0402))
  if model.sampling_function == 'categorical':
    assert torch.equal(base, model.generate(n, sample=w, use_queues=queued, top_k=2 ** kw['bits']))
    assert torch.equal(base, model.generate(n, sample=w, use_queues=queued, top_k=2 ** kw['bits'] + 5))
  # ... and without a window: seed=None draws the window of seed=0x0402
  assert torch.equal(model.generate(n, batch_size=3, use_queues=queued),
                     model.generate(n, batch_size=3, use_queues=queued, seed=0x0402))
  # the controls do something
  assert not torch.equal(base, model.generate(n, sample=w, use_queues=queued, temperature=0.5))


# ------------------------------------------------------------------------------------------
# 3. queued == sliding window under the controls (kernel_size = 2), 5 utterances, non-default seed
# ------------------------------------------------------------------------------------------
CAT_CONTROLS = [(0.7, 0), (1.0, 20), (0.7, 20)]
MIX_T = [0.5, 1.3]


def _both_forms(model, n, B, seed_w, **controls):
  w = O.synthetic_waveform(B, model.receptive_field, seed=seed_w).to(dev())
  naive = model.generate(n, sample=w, use_queues=False, seed=SEED, **controls)
  queued = model.generate(n, sample=w, use_queues=True, seed=SEED, **controls)
  plain = model.generate(n, sample=w, use_queues=True, seed=SEED)
  return naive, queued, plain


@pytest.mark.parametrize('T,k', CAT_CONTROLS)
@pytest.mark.parametrize('name', ['cat_r64', 'cat_small_fused', 'cat_lpb3'])
def test_queued_equals_sliding_window_categorical(name, T, k):
  """Chain + fused categorical tail (cat_r64: head launch with tail 2), sampler + emit from the logits behind the per-layer
  head (cat_small_fused) and the composed path (cat_lpb3, layers_per_block = 3, 64 classes)."""
  kw = dict(MODEL_CASES[name])
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **kw)
  naive, queued, plain = _both_forms(model, 14, 5, 12, temperature=T, top_k=k)
  assert torch.equal(naive, queued), (naive - queued).abs().max()
  assert not torch.equal(queued, plain)


@pytest.mark.parametrize('T,k', CAT_CONTROLS)
@pytest.mark.parametrize('form', ['relay', 'one_workgroup'])
def test_queued_equals_sliding_window_128_channel_chain(form, T, k):
  from wavenets_amd import _lib
  kw = dict(blocks=5, channels=128, skip_channels=256, dilation_bound=16, final_layers_channels=[128, 64],
            activation='leaky_relu', bits=8, use_skip=True)
  ocfg, params, model = make_pair(seed=17, bias_range=0.3, **kw)
  w = O.synthetic_waveform(5, model.receptive_field, seed=3).to(dev())
  naive = model.generate(40, sample=w, use_queues=False, seed=SEED, temperature=T, top_k=k)
  _lib.lib().wn_debug_set(2, 1 if form == 'one_workgroup' else 0)
  try:
    queued = model.generate(40, sample=w, use_queues=True, seed=SEED, temperature=T, top_k=k)
  finally:
    _lib.lib().wn_debug_set(2, 0)
  assert torch.equal(naive, queued), (naive - queued).abs().max()


@pytest.mark.parametrize('T', MIX_T)
@pytest.mark.parametrize('channels,sampler,mix,finals', [(64, 'logistic', 10, [128, 256]), (32, 'gaussian', 8, [64, 64]),
                                                         (128, 'logistic', 5, [128, 128])])
def test_queued_equals_sliding_window_mixture_head_in_one_launch(channels, sampler, mix, finals, T):
  kw = dict(blocks=6, channels=channels, skip_channels=256, dilation_bound=32, final_layers_channels=finals,
            activation='leaky_relu', num_mixtures=mix, sampling_function=sampler, bits=16)
  ocfg, params, model = make_pair(seed=23, bias_range=0.3, **kw)
  naive, queued, plain = _both_forms(model, 30, 5, 6, temperature=T)
  assert torch.equal(naive, queued), (naive - queued).abs().max()
  assert not torch.equal(queued, plain)


@pytest.mark.parametrize('T', MIX_T)
def test_queued_equals_sliding_window_mixture_sampler_launch(T):
  """'mol': the head's layers as separate launches, mixture sampler + emit in one (wn_sample_rand_mix_kernel<true>)."""
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES['mol']))
  naive, queued, plain = _both_forms(model, 14, 5, 12, temperature=T)
  assert torch.equal(naive, queued), (naive - queued).abs().max()
  assert not torch.equal(queued, plain)


# ------------------------------------------------------------------------------------------
# 4. top_k = 1 is arg max
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('B', [3, 9])          # 9 utterances: the sampler runs as its own launch behind the head
def test_top_k_1_is_arg_max_in_generation(queued, B):
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES['cat_r64']))
  w = O.synthetic_waveform(B, model.receptive_field, seed=12).to(dev())
  det = model.generate(200, sample=w, use_queues=queued, deterministic=True)
  for T in (1.0, 0.6):
    top1 = model.generate(200, sample=w, use_queues=queued, deterministic=False, top_k=1, temperature=T, seed=SEED)
    assert torch.equal(det, top1), (T, (det - top1).abs().max())
  assert det.unique().numel() >= 2


def test_top_k_1_is_arg_max_in_sample_waveform():
  ocfg, params, model = make_pair(seed=4, **dict(MODEL_CASES['cat_small_fused']))
  g = torch.Generator().manual_seed(0)
  probs = torch.softmax(torch.randn(3, 40, 256, generator=g) * 2, -1)
  probs[0, 0, 17] = probs[0, 0, 200] = probs[0, 0].max() * 2          # an exact tie at the top: the first one wins
  s = model.sample_waveform(probs.to(dev()), top_k=1)
  assert torch.equal(s.cpu(), O.sample_waveform_deterministic(probs, ocfg))
  s = model.sample_waveform(probs.to(dev()), top_k=1, temperature=0.3, seed=5)
  assert torch.equal(s.cpu(), O.sample_waveform_deterministic(probs, ocfg))


# ------------------------------------------------------------------------------------------
# 5. tie rule: (probability descending, class index ascending)
# ------------------------------------------------------------------------------------------
def _classes(samples, bits):
  return torch.round((samples.cpu().reshape(-1).double() + 1.0) * 2 ** (bits - 1)).long()


def test_top_k_tie_rule():
  model = _model(bits=8)
  row = torch.zeros(256); row[:4] = 0.25
  big = row.expand(1, 4000, 256).contiguous().to(dev())
  assert _classes(model.sample_waveform(big, top_k=2), 8).unique().tolist() == [0, 1]
  assert _classes(model.sample_waveform(big, top_k=3), 8).unique().tolist() == [0, 1, 2]
  assert _classes(model.sample_waveform(big, top_k=3, temperature=0.5), 8).unique().tolist() == [0, 1, 2]
  # ties that sit in different lanes and different register slots of the wave (class = lane + 64 slot): index order, not
  # lane order -- class 70 (lane 6) ranks behind class 10 (lane 10) and before class 131 (lane 3)
  row = torch.full((256,), 0.001); row[[10, 70, 131, 200]] = 0.2; row[5] = 0.19
  big = row.expand(1, 4000, 256).contiguous().to(dev())
  assert _classes(model.sample_waveform(big, top_k=1), 8).unique().tolist() == [10]
  assert _classes(model.sample_waveform(big, top_k=2), 8).unique().tolist() == [10, 70]
  assert _classes(model.sample_waveform(big, top_k=3), 8).unique().tolist() == [10, 70, 131]
  assert _classes(model.sample_waveform(big, top_k=4), 8).unique().tolist() == [10, 70, 131, 200]
  assert _classes(model.sample_waveform(big, top_k=5), 8).unique().tolist() == [5, 10, 70, 131, 200]
  # ... and beyond 256 classes (the row is read from memory, 64 classes a round)
  model = _model(bits=10)
  row = torch.full((1000,), 1e-4); row[[999, 640, 70, 300]] = 0.2
  big = row.expand(1, 4000, 1000).contiguous().to(dev())
  assert _classes(model.sample_waveform(big, top_k=2), 10).unique().tolist() == [70, 300]
  assert _classes(model.sample_waveform(big, top_k=4), 10).unique().tolist() == [70, 300, 640, 999]


# ------------------------------------------------------------------------------------------
# 6. support of the top-k draw
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits,C', [(4, 16), (8, 256), (10, 1024), (10, 1000), (7, 100)])
def test_top_k_support(bits, C):
  """Every draw lies in the set torch.sort(descending=True, stable=True)[:k] names.  Rows whose k-th and (k+1)-th
  probabilities are closer than 2 ulp are left out (none with these generator seeds, checked on the CPU); at most 1 % may
  be."""
  model = _model(bits=bits)
  g = torch.Generator().manual_seed(100 + C)
  rows = 2000
  probs = torch.softmax(torch.randn(1, rows, C, generator=g) * 2, -1)
  order = torch.sort(probs[0], dim=-1, descending=True, stable=True)
  for k in [k for k in (1, 2, 5, 15, 64, 255, 999) if k < C]:
    kth, nxt = order.values[:, k - 1], order.values[:, k]
    ulp = torch.nextafter(kth, torch.full_like(kth, math.inf)) - kth
    clear = (kth - nxt) >= 2 * ulp
    assert (~clear).float().mean().item() <= 0.01
    allowed = torch.zeros(rows, C, dtype=torch.bool)
    allowed.scatter_(1, order.indices[:, :k], True)
    for T in (1.0, 0.7):
      cls = _classes(model.sample_waveform(probs.to(dev()), top_k=k, temperature=T, seed=k), bits)
      assert cls.min() >= 0 and cls.max() < C
      ok = allowed[torch.arange(rows), cls]
      assert ok[clear].all(), (k, T, int((~ok[clear]).sum()))
      if k > 1:
        assert (cls != order.indices[:, 0]).any()          # not just the arg max


# ------------------------------------------------------------------------------------------
# 7. seed
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'mol'])
def test_seed_selects_the_take(name, queued):
  """Same seed, same audio; another seed, another take.  With sample=None the seed also draws the initial noise window.
  (A deterministic=True call without a window starts from silence, today as before, so it cannot show the window; the
  arg-max draw of a stochastic call can: with top_k=1 nothing depends on the Philox key, and the first sample differs
  between two seeds only through their windows.)"""
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES[name]))
  w = O.synthetic_waveform(5, model.receptive_field, seed=12).to(dev())
  a = model.generate(24, sample=w, use_queues=queued, seed=7)
  assert torch.equal(a, model.generate(24, sample=w, use_queues=queued, seed=7))
  b = model.generate(24, sample=w, use_queues=queued, seed=8)
  assert not torch.equal(a, b)
  # no window given: the seed draws it
  rf = model.receptive_field
  for s in (7, 8):
    win = torch.randn(5, rf, 1, generator=torch.Generator(device='cpu').manual_seed(s)).to(dev())
    assert torch.equal(model.generate(12, batch_size=5, use_queues=queued, seed=s),
                       model.generate(12, sample=win, use_queues=queued, seed=s))
  assert torch.equal(model.generate(12, batch_size=5, use_queues=queued, deterministic=True, seed=7),
                     model.generate(12, batch_size=5, use_queues=queued, deterministic=True))
  if name == 'cat_r64':
    first7 = model.generate(1, batch_size=5, use_queues=queued, top_k=1, seed=7)
    first8 = model.generate(1, batch_size=5, use_queues=queued, top_k=1, seed=8)
    assert not torch.equal(first7, first8)


def test_seed_in_sample_waveform():
  model = _model(bits=8)
  probs = torch.softmax(torch.randn(2, 500, 256, generator=torch.Generator().manual_seed(1)), -1).to(dev())
  model._sample_calls = 10
  a = model.sample_waveform(probs, seed=7)
  model._sample_calls = 10
  assert torch.equal(a, model.sample_waveform(probs, seed=7))
  model._sample_calls = 10
  assert not torch.equal(a, model.sample_waveform(probs, seed=8))
  model._sample_calls = 10
  d = model.sample_waveform(probs)
  model._sample_calls = 10
  assert torch.equal(d, model.sample_waveform(probs, seed=0x0402, temperature=1.0, top_k=0))
  model._sample_calls = 10
  assert torch.equal(d, model.sample_waveform(probs, top_k=256))


# ------------------------------------------------------------------------------------------
# 8. small-T bound for mixtures (derived, not measured)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mol', 'gauss'])
def test_mixture_small_temperature_bound(name):
  """With 24-bit uniforms the logistic noise ln z - ln(1 - z) is bounded by ln(2^25) and the Box-Muller noise by
  sqrt(2 ln 2^25).  At T = 1e-3 and a leading component logit >= 1 ahead, the other weights are e^-1000 = 0 in fp32, so
  |draw - deterministic draw| <= T e^s bound (1 + 1e-5) + 1 ulp."""
  kw = dict(MODEL_CASES[name])
  ocfg, params, model = make_pair(seed=4, **kw)
  M = kw['num_mixtures']
  g = torch.Generator().manual_seed(8)
  rows = 20000
  wl = torch.randn(rows, M, generator=g)
  lead = torch.randint(0, M, (rows,), generator=g)
  wl[torch.arange(rows), lead] = wl.max(-1).values + 1.0 + torch.rand(rows, generator=g)
  top2 = wl.topk(2, -1).values
  assert (top2[:, 0] - top2[:, 1]).min() >= 1.0
  mu = torch.rand(rows, M, generator=g) * 1.9 - 0.95
  s = torch.rand(rows, M, generator=g) * 3.0 - 4.0
  pred = torch.cat([wl, mu, s], -1).unsqueeze(0)
  T = 1e-3
  det = model.sample_waveform(pred.to(dev()), deterministic=True).cpu().reshape(-1)
  assert torch.equal(det, O.sample_waveform_deterministic(pred, ocfg).reshape(-1))
  draw = model.sample_waveform(pred.to(dev()), temperature=T, seed=3).cpu().reshape(-1)
  bound = math.log(2.0 ** 25) if name == 'mol' else math.sqrt(2.0 * math.log(2.0 ** 25))
  scale = torch.exp(s[torch.arange(rows), lead].double())
  big = torch.maximum(det.abs(), draw.abs())
  ulp = (torch.nextafter(big, torch.full_like(big, math.inf)) - big).double()
  err = (draw.double() - det.double()).abs()
  lim = T * scale * bound * (1 + 1e-5) + ulp
  print('max |draw - det| / limit:', (err / lim).max().item())
  assert (err <= lim).all(), (err / lim).max().item()
  assert (err > 0).float().mean() > 0.5              # the noise is there, T times smaller


# ------------------------------------------------------------------------------------------
# 9. 65536 classes
# ------------------------------------------------------------------------------------------
def test_temperature_at_65536_classes():
  model = _model(bits=16)
  g = torch.Generator().manual_seed(2)
  C = 65536
  logits = torch.randn(6, C, generator=g)
  top = torch.tensor([0, 1, 63, 4097, 40000, C - 1])
  logits[torch.arange(6), top] = logits.max(-1).values + 2.0 + torch.rand(6, generator=g)
  rest = logits.clone(); rest[torch.arange(6), top] = -math.inf
  assert (logits[torch.arange(6), top] - rest.max(-1).values).min() >= 2.0
  probs = torch.softmax(logits, -1).unsqueeze(0)
  for seed in (1, 2, 3):
    s = model.sample_waveform(probs.to(dev()), temperature=0.05, seed=seed).cpu().reshape(-1)
    assert torch.isfinite(s).all() and s.min() >= -1.0 and s.max() < 1.0
    assert _classes(s, 16).tolist() == top.tolist()
  # flat-ish rows: finite samples in [-1, 1), not all alike
  flat = torch.softmax(torch.randn(1, 64, C, generator=g) * 0.01, -1)
  s = model.sample_waveform(flat.to(dev()), temperature=0.05, seed=1).cpu().reshape(-1)
  assert torch.isfinite(s).all() and s.min() >= -1.0 and s.max() < 1.0 and s.unique().numel() > 32
  with pytest.raises(ValueError, match='1024'):
    model.sample_waveform(probs.to(dev()), top_k=5)


# ------------------------------------------------------------------------------------------
# 10. / 11. laws (construction, n and failure probabilities of test_mixture_stochastic_sampler_distribution and
# test_categorical_samplers)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [0.5, 1.5])
@pytest.mark.parametrize('name', ['mol', 'gauss'])
def test_mixture_law_at_temperature(name, T):
  """Empirical CDF of n draws at temperature T against the oracle's law of the row [w / T | mu | s + ln T].
  Dvoretzky-Kiefer-Wolfowitz: P(sup|F_n - F| > eps) <= 2 exp(-2 n eps^2) = 1.1e-6 at these sizes."""
  kw = dict(MODEL_CASES[name])
  ocfg, params, model = make_pair(seed=4, **kw)
  M = kw['num_mixtures']
  g = torch.Generator().manual_seed(3)
  row = torch.cat([torch.randn(M, generator=g), torch.rand(M, generator=g) * 1.6 - 0.8,
                   torch.rand(M, generator=g) * 3.0 - 4.0])
  row_T = torch.cat([row[:M] / T, row[M:2 * M], row[2 * M:] + math.log(T)])
  n = 200000
  eps = math.sqrt(math.log(2 / 1.1e-6) / (2 * n))
  big = row.expand(1, n, 3 * M).contiguous()
  draws = model.sample_waveform(big.to(dev()), temperature=T, seed=21).cpu().reshape(-1).double()
  assert draws.abs().max() <= 1.0
  v = torch.linspace(-1.0, 0.9999, 400, dtype=torch.float64)
  Fn = (draws.unsqueeze(0) <= v.unsqueeze(1)).double().mean(1)
  F = O.mixture_sample_cdf(row_T, ocfg, v)
  print('sup |Fn - F| =', (Fn - F).abs().max().item(), 'eps =', eps)
  assert (Fn - F).abs().max().item() < eps, (Fn - F).abs().max().item()
  # the T = 1 law is a different one at this resolution (the test can tell them apart)
  assert (O.mixture_sample_cdf(row, ocfg, v) - F).abs().max().item() > 2 * eps
  # component pick ~ softmax(w / T): with tiny scales every draw sits on its component's mean
  tight = torch.cat([row[:M], row[M:2 * M], torch.full((M,), -12.0)])
  d2 = model.sample_waveform(tight.expand(1, n, 3 * M).contiguous().to(dev()), temperature=T, seed=22).cpu().reshape(-1)
  comp = (d2.unsqueeze(1) - row[M:2 * M].unsqueeze(0)).abs().argmin(1)
  counts = torch.bincount(comp, minlength=M).double()
  w = torch.softmax(row[:M].double() / T, -1)
  chi2 = (((counts - n * w) ** 2) / (n * w)).sum().item()
  print('chi2 =', chi2)
  assert chi2 < 70.0, chi2                                # M-1 <= 9 dof: P(chi2 > 70) < 1e-10


def _chi2(counts, p, n):
  live = p > 0
  assert counts[~live].sum() == 0
  return (((counts[live] - n * p[live]) ** 2) / (n * p[live])).sum().item()


@pytest.mark.parametrize('T,k', [(0.5, 0), (1.5, 0), (1.0, 5), (0.5, 5), (1.5, 5)])
def test_categorical_law_under_the_controls(T, k):
  """16 live classes of 256, one row repeated n times: chi-square of the bin counts against softmax(log p / T), against
  the renormalised top-5 law, and against both together."""
  model = _model(bits=8)
  g = torch.Generator().manual_seed(0)
  row = torch.softmax(torch.randn(16, generator=g), -1)
  p16 = torch.zeros(256); p16[:16] = row
  law = row.double() ** (1.0 / T)
  if k:
    keep = torch.sort(row, descending=True, stable=True).indices[:k]
    mask = torch.zeros(16, dtype=torch.bool); mask[keep] = True
    law = torch.where(mask, law, torch.zeros_like(law))
  law = law / law.sum()
  n = 200000
  big = p16.expand(1, n, 256).contiguous()
  draws = model.sample_waveform(big.to(dev()), temperature=T, top_k=k, seed=31).cpu().reshape(-1)
  idx = _classes(draws, 8)
  assert idx.max() < 16
  counts = torch.bincount(idx, minlength=16).double()[:16]
  chi2 = _chi2(counts, law, n)                      # (classes outside the kept set: never drawn)
  print('chi2 =', chi2)
  if k:
    assert chi2 < 36.0, chi2        # 4 dof: P(chi2 > 36) = e^-18 (1 + 18) = 2.9e-7
  else:
    assert chi2 < 60.0, chi2        # 15 dof: P(chi2 > 60) ~ 2e-7
  if not k:       # the law without the controls is a different one at this sample size
    assert _chi2(n * law, row.double(), n) > 1000.0
