"""top_p (nucleus sampling) of generation and sample_waveform on the GPU (semantics in
include/wn_hip.h, struct wn_sampling): off is the draw of before bit for bit, exact kept sets on rows whose sums are exact
in fp32, tiny top_p is the arg max, two-sided support and the law against the fp64 reference of
test_top_p_cabi_cpu.py, and queued == sliding window."""
import math

import pytest
import torch

from test_gpu_parity import MODEL_CASES, O, dev, make_pair
from test_gpu_sampling_controls import SEED, _chi2, _classes, _model
from test_top_p_cabi_cpu import DYADIC_SETS, dyadic_row, f32, nucleus

pytestmark = pytest.mark.gpu

# Slack of the reference nucleus, in normalised mass; a condition, not a measurement.  fp32 summation of up to 1024
# non-negative terms in any order is off by at most 1023 * 2^-24 = 6.1e-5 of the sum; a tempered term
# expf(logf(r) / T) is off by a few 2^-23 q |ln q| / T, under 1e-4 summed over 1024 classes for T >= 0.5.
DELTA = 2.5e-4


# ------------------------------------------------------------------------------------------
# 1. off is bit-exact; the domain
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'cat_lpb3'])
def test_top_p_off_is_bit_exact(name, queued):
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES[name]))
  w = O.synthetic_waveform(3, model.receptive_field, seed=12).to(dev())
  base = model.generate(16, sample=w, use_queues=queued)
  assert torch.equal(base, model.generate(16, sample=w, use_queues=queued, top_p=1.0))
  assert torch.equal(base, model.generate(16, sample=w, use_queues=queued, top_p=1))
  assert not torch.equal(base, model.generate(16, sample=w, use_queues=queued, top_p=0.5))
  for bad in (0, -1, 1.01, float('nan'), True):
    with pytest.raises(ValueError, match='top_p'):
      model.generate(16, sample=w, use_queues=queued, top_p=bad)


def test_top_p_on_a_mixture_model_raises():
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES['mol']))
  w = O.synthetic_waveform(3, model.receptive_field, seed=12).to(dev())
  with pytest.raises(ValueError, match='top_p'):
    model.generate(8, sample=w, use_queues=True, top_p=0.9)
  pred = torch.zeros(1, 4, 30, device=dev())
  with pytest.raises(ValueError, match='top_p'):
    model.sample_waveform(pred, top_p=0.9)
  assert torch.equal(model.generate(8, sample=w, use_queues=True), model.generate(8, sample=w, use_queues=True, top_p=1.0))


# ------------------------------------------------------------------------------------------
# 2. exact sets on dyadic rows
# ------------------------------------------------------------------------------------------
def _drawn_set(model, row, bits, **controls):
  big = row.expand(1, 4000, row.numel()).contiguous().to(dev())
  return _classes(model.sample_waveform(big, **controls), bits).unique().tolist()


@pytest.mark.parametrize('k,top_p,expect', DYADIC_SETS)
def test_top_p_exact_sets_on_the_dyadic_row(k, top_p, expect):
  """One row repeated 4000 times, T = 1: every sum and every p / p_max is exact in fp32, so the kept set is exact.  The
  rarest kept class is 140 in the last case, mass 1/193 of its nucleus: P(never drawn in 4000) = (1 - 1/193)^4000 = 1e-9;
  every other kept class has at least 1/6."""
  model = _model(bits=8)
  assert _drawn_set(model, dyadic_row(), 8, top_k=k, top_p=top_p, seed=9) == sorted(expect)


def test_top_p_exact_sets_beyond_256_classes():
  """1000 classes: the row is re-read from memory, 64 classes a round."""
  model = _model(bits=10)
  row = dyadic_row(1000)
  assert _drawn_set(model, row, 10, top_p=0.5, seed=9) == [5, 10, 70]
  assert _drawn_set(model, row, 10, top_p=0.25, seed=9) == [5]
  assert _drawn_set(model, row, 10, top_p=0.6, top_k=3, seed=9) == [5, 10]
  # ties in different rounds of the re-read
  row = torch.zeros(1000); row[[999, 640, 70, 300]] = 0.125; row[400:464] = 1.0 / 128
  assert _drawn_set(model, row, 10, top_p=0.25, seed=9) == [70, 300]
  assert _drawn_set(model, row, 10, top_p=0.375, seed=9) == [70, 300, 640]


# ------------------------------------------------------------------------------------------
# 3. tiny top_p is arg max
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('B', [3, 9])          # 9 utterances: the sampler runs as its own launch behind the head
def test_tiny_top_p_is_arg_max_in_generation(queued, B):
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES['cat_r64']))
  w = O.synthetic_waveform(B, model.receptive_field, seed=12).to(dev())
  det = model.generate(200, sample=w, use_queues=queued, deterministic=True)
  for T in (1.0, 0.6):
    top1 = model.generate(200, sample=w, use_queues=queued, deterministic=False, top_p=1e-6, temperature=T, seed=SEED)
    assert torch.equal(det, top1), (T, (det - top1).abs().max())
  assert det.unique().numel() >= 2


def test_tiny_top_p_is_arg_max_in_sample_waveform():
  ocfg, params, model = make_pair(seed=4, **dict(MODEL_CASES['cat_small_fused']))
  g = torch.Generator().manual_seed(0)
  probs = torch.softmax(torch.randn(3, 40, 256, generator=g) * 2, -1)
  probs[0, 0, 17] = probs[0, 0, 200] = probs[0, 0].max() * 2          # an exact tie at the top: the first one wins
  want = O.sample_waveform_deterministic(probs, ocfg)
  assert torch.equal(model.sample_waveform(probs.to(dev()), top_p=1e-6).cpu(), want)
  assert torch.equal(model.sample_waveform(probs.to(dev()), top_p=2.0 ** -11, temperature=0.3, seed=5).cpu(), want)
  assert torch.equal(model.sample_waveform(probs.to(dev()), top_p=1e-6, top_k=7, seed=5).cpu(), want)


# ------------------------------------------------------------------------------------------
# 4. support, two-sided and without exclusions
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bits,C', [(4, 16), (8, 256), (10, 1000), (10, 1024)])
def test_top_p_support(bits, C):
  """Every drawn class lies in the reference nucleus at top_p + DELTA, for every row; and the control is not silently
  top-1: some draw differs from the arg max, and some drawn class lies outside the nucleus at top_p / 2."""
  model = _model(bits=bits)
  g = torch.Generator().manual_seed(100 + C)
  rows = 2000
  probs = torch.softmax(torch.randn(1, rows, C, generator=g) * 2, -1)
  first = torch.sort(probs[0], dim=-1, descending=True, stable=True).indices[:, 0]
  on_dev = probs.to(dev())
  r = torch.arange(rows)
  for T, k in ((1.0, 0), (0.7, 0), (1.0, 15), (0.7, 15)):
    for top_p in (0.3, 0.9, 0.99):
      tp = f32(top_p)
      cls = _classes(model.sample_waveform(on_dev, temperature=T, top_k=k, top_p=top_p, seed=int(1000 * top_p) + k), bits)
      assert cls.min() >= 0 and cls.max() < C
      ok = nucleus(probs[0], tp + DELTA, T, k)[r, cls]
      assert ok.all(), (T, k, top_p, int((~ok).sum()))
      assert (cls != first).any(), (T, k, top_p)
      assert (~nucleus(probs[0], 0.5 * tp, T, k)[r, cls]).any(), (T, k, top_p)


# ------------------------------------------------------------------------------------------
# 5. law
# ------------------------------------------------------------------------------------------
def _chi2_tail_even(x, m):
  """P(chi-square with 2 m degrees of freedom > x) = e^(-x/2) sum_{i < m} (x/2)^i / i!"""
  return math.exp(-x / 2) * sum((x / 2) ** i / math.factorial(i) for i in range(m))


@pytest.mark.parametrize('T,k,top_p', [(1.0, 0, 0.575), (0.5, 0, 0.6), (1.0, 8, 0.8)])
def test_categorical_law_under_top_p(T, k, top_p):
  """The 16-live-classes row of test_categorical_law_under_the_controls, n draws: chi-square of the bin counts against the
  renormalised nucleus law.  top_p sits >= 100 DELTA of normalised mass from the cumulative sums on both sides of the cut
  (asserted), so the reference nucleus is the kernel's.  Bound: degrees of freedom d = nucleus size - 1; the tail of
  chi-square with d degrees lies below that with d + 1, so with 2 m = d rounded up to even the bound is the smallest
  integer x with e^(-x/2) sum_{i < m} (x/2)^i / i! < 1e-6 (d = 2: 28; d = 4: 34; d = 5 -> 6: 39)."""
  model = _model(bits=8)
  g = torch.Generator().manual_seed(0)
  row = torch.softmax(torch.randn(16, generator=g), -1)
  p16 = torch.zeros(256); p16[:16] = row
  tp = f32(top_p)
  v = torch.sort(row, descending=True, stable=True).values.double()
  q = (v / v[0]) ** (1.0 / T)
  if k:
    q[k:] = 0
  cum = q.cumsum(0) / q.sum()
  assert (cum - tp).abs().min().item() >= 100 * DELTA
  keep = nucleus(row.unsqueeze(0), tp, T, k)[0]
  size = int(keep.sum())
  assert 3 <= size < (k or 16)
  law = torch.where(keep, (row.double() / row.max().double()) ** (1.0 / T), torch.zeros(16, dtype=torch.float64))
  law = law / law.sum()
  n = 200000
  big = p16.expand(1, n, 256).contiguous()
  draws = model.sample_waveform(big.to(dev()), temperature=T, top_k=k, top_p=top_p, seed=31).cpu().reshape(-1)
  idx = _classes(draws, 8)
  assert idx.max() < 16
  counts = torch.bincount(idx, minlength=16).double()[:16]
  assert counts[~keep].sum() == 0                     # classes outside the nucleus: never drawn
  chi2 = _chi2(counts, law, n)
  m = size // 2                                       # 2 m = (size - 1) rounded up to even
  bound = next(x for x in range(1, 200) if _chi2_tail_even(x, m) < 1e-6)
  print('nucleus size', size, 'chi2 =', chi2, 'bound', bound)
  assert chi2 < bound, (chi2, bound)
  # the law without top_p is a different one at this sample size
  full = q / q.sum()
  order = torch.sort(row, descending=True, stable=True).indices
  full_law = torch.zeros(16, dtype=torch.float64); full_law[order] = full
  assert full_law[~keep].sum() * n > 1000.0


# ------------------------------------------------------------------------------------------
# 6. queued == sliding window, bit for bit
# ------------------------------------------------------------------------------------------
TOP_P_CONTROLS = [(1.0, 0), (0.7, 20)]


@pytest.mark.parametrize('T,k', TOP_P_CONTROLS)
@pytest.mark.parametrize('name', ['cat_r64', 'cat_small_fused', 'cat_lpb3'])
def test_queued_equals_sliding_window_under_top_p(name, T, k):
  ocfg, params, model = make_pair(seed=11, bias_range=0.3, **dict(MODEL_CASES[name]))
  w = O.synthetic_waveform(5, model.receptive_field, seed=12).to(dev())
  naive = model.generate(14, sample=w, use_queues=False, seed=SEED, temperature=T, top_k=k, top_p=0.8)
  queued = model.generate(14, sample=w, use_queues=True, seed=SEED, temperature=T, top_k=k, top_p=0.8)
  assert torch.equal(naive, queued), (naive - queued).abs().max()
  assert not torch.equal(queued, model.generate(14, sample=w, use_queues=True, seed=SEED, temperature=T, top_k=k))


@pytest.mark.parametrize('T,k', TOP_P_CONTROLS)
@pytest.mark.parametrize('form', ['relay', 'one_workgroup'])
def test_queued_equals_sliding_window_128_channel_chain_under_top_p(form, T, k):
  from wavenets_amd import _lib
  kw = dict(blocks=5, channels=128, skip_channels=256, dilation_bound=16, final_layers_channels=[128, 64],
            activation='leaky_relu', bits=8, use_skip=True)
  ocfg, params, model = make_pair(seed=17, bias_range=0.3, **kw)
  w = O.synthetic_waveform(5, model.receptive_field, seed=3).to(dev())
  naive = model.generate(40, sample=w, use_queues=False, seed=SEED, temperature=T, top_k=k, top_p=0.8)
  _lib.lib().wn_debug_set(2, 1 if form == 'one_workgroup' else 0)
  try:
    queued = model.generate(40, sample=w, use_queues=True, seed=SEED, temperature=T, top_k=k, top_p=0.8)
    plain = model.generate(40, sample=w, use_queues=True, seed=SEED, temperature=T, top_k=k)
  finally:
    _lib.lib().wn_debug_set(2, 0)
  assert torch.equal(naive, queued), (naive - queued).abs().max()
  assert not torch.equal(queued, plain)
