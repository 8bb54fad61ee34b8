"""The loss kernels where training takes them: categorical rows with probabilities beyond both
ends of Keras's clip range [1e-7, 1 - 1e-7], mixture rows at the -7 floor of the log-scales, at the 1e8 cap of the
Gaussian argument and in both far tails of sharp components.

The references hold no device input: a head whose last kernel is zero outputs its bias on every row in both math
modes (0 * a + bias is exact), so the logits / mixture parameters of every row are known on the CPU and the fp64 oracle
(categorical) or the exact-in-both-tails fp64 functions pinned by tests/test_loss_reference_cpu.py against 50-digit
arithmetic (mixtures) give loss rows and dL/dlogits outright.  Every test prints its worst figures before it asserts."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu

EPS = 1e-7                   # keras.backend.epsilon()
B, T = 2, 133                # 266 rows: 2 mod 4 (a ragged last workgroup of the row kernels), no multiple of the epilogue's 32-row tile
SENTINEL = 12345.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mix_tails.npz')


def dev():
  return torch.device('cuda', 0)


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  """Both contraction modes: 'split' = fp16 hi/lo 3-product MFMA (default), 'fp32' = exact-fp32 MFMA (debug knob 1)."""
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


# ------------------------------------------------------------------------------------------
# helpers: a model with a constant head, the training workspace's regions
# ------------------------------------------------------------------------------------------
def constant_head_params(ocfg, bias_row, seed=6):
  """Oracle parameters with the last conv's kernel zeroed and its bias set to bias_row."""
  params = O.init_params(ocfg, seed=seed)
  assert O.param_shapes(ocfg)[-2][0].startswith('final') and O.param_shapes(ocfg)[-1][0].endswith('bias')
  params[-2] = torch.zeros_like(params[-2])
  params[-1] = torch.as_tensor(bias_row, dtype=torch.float32).clone()
  return params


@functools.lru_cache(maxsize=None)
def _model(items):
  from wavenets_amd import WaveNet
  return WaveNet(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in items}, device=dev())


def model_for(kw, params):
  model = _model(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
  model.set_weights([p.numpy() for p in params])
  return model


def region_span(model, what, idx):
  from wavenets_amd import _lib
  off, ln = C.c_int64(), C.c_int64()
  _lib.check(_lib.lib().wn_debug_ws_region(model._plan, B, T, what, idx, C.byref(off), C.byref(ln)))
  return off.value, ln.value


def train_ws(model):
  """The training workspace of a (B, T) call, allocated as loss_and_grads allocates it (a sentinel goes in before the
  first call)."""
  from wavenets_amd import _lib
  return model._workspace('train', _lib.lib().wn_plan_workspace_floats(model._plan, B, T, 1))


def run_step(model, x, nf, want_pred, expect_fused):
  """One loss_and_grads call with the logits region holding a sentinel beforehand: the fused loss epilogue of the head's
  last conv never forms a logits tensor, the standalone loss kernels read one.  Returns (loss[3], loss rows, dL/dlogits,
  logits region, pred, max-abs slot of dL/dlogits)."""
  train_ws(model)
  o5, n5 = region_span(model, 5, 0)
  o6, n6 = region_span(model, 6, nf)
  assert n5 == n6 and (o5 + n5 <= o6 or o6 + n6 <= o5)       # two regions, not one under two names
  model.training_intermediate(5, 0, B, T).fill_(SENTINEL)
  loss, pred, _ = model.loss_and_grads(x.to(dev()), want_pred=want_pred)
  logits = model.training_intermediate(5, 0, B, T).clone().cpu()
  if expect_fused:
    assert torch.all(logits == SENTINEL), 'the fused loss epilogue was expected and a logits tensor was written'
  else:
    assert not torch.any(logits == SENTINEL), 'the standalone loss kernel was expected and no logits tensor was written'
  rows = model.training_intermediate(12, 0, B, T).clone().cpu().double().reshape(B, T)
  g = model.training_intermediate(6, nf, B, T).clone().cpu().double()
  amax = model.training_intermediate(10, 0, B, T)[nf].item()
  return loss.cpu(), rows, g, logits, (pred.cpu() if pred is not None else None), amax


# ------------------------------------------------------------------------------------------
# categorical head: the clip regimes on all three row kernels and the fused epilogue
# ------------------------------------------------------------------------------------------
# (a hidden width of 48 is the narrowest operand the fused loss epilogue takes -- three 16-wide k steps,
# wn_gemm_planes16s_supported; under a 32-wide hidden layer a 256-class head runs the standalone kernel in both modes)
CAT_KW = dict(blocks=3, channels=32, skip_channels=32, dilation_bound=4, final_layers_channels=[48])
CAT_BIASES = ['flat', 'peak30', 'peak14', 'straddle', 'ramp', 'twin']


def c_star(Cn):
  return (5 * Cn) // 8 + 1


def cat_input(bits):
  """(B, T + 1, 1), piecewise constant in runs of 19 samples: both ends of the range and beyond them (classes 0 and
  C - 1), the centre of class c*, two more."""
  Cn = 1 << bits
  vals = torch.tensor([-1.0, 1.0, 1.5, -1.5, (c_star(Cn) + 0.5) * 2.0 / Cn - 1.0, 0.1, -0.6], dtype=torch.float32)
  t = torch.arange(T + 1)
  return torch.stack([vals[((t // 19) + 3 * b) % 7] for b in range(B)]).unsqueeze(-1)


def cat_bias(bits, name):
  Cn, cs = 1 << bits, c_star(1 << bits)
  b = torch.zeros(Cn, dtype=torch.float32)
  if name == 'peak30':          # q_c* > 1 - 1e-7, every other class below 1e-7
    b[cs] = 30.0
  elif name == 'peak14':        # everything inside the clip
    b[cs] = 14.0
  elif name == 'straddle':      # the other classes on both sides of 1e-7; the classes that occur as targets 0.4 off it
    b = (torch.rand(Cn, generator=torch.Generator().manual_seed(bits)) * 2 - 1) * 0.4
    tc = [c for c in torch.unique(O.quantize(cat_input(bits), bits)).tolist() if c != cs]
    for i, c in enumerate(tc):
      b[c] = 0.4 if i % 2 == 0 else -0.4
    b[cs] = math.log(1e7)
  elif name == 'ramp':          # a long tail below the clip, the maximum inside
    b = 0.5 * torch.arange(Cn, dtype=torch.float32)
  elif name == 'twin':          # two equal maxima 25 above the rest
    b[cs] = 25.0
    b[cs + 1] = 25.0
  else:
    assert name == 'flat'
  return b


@functools.lru_cache(maxsize=None)
def cat_reference(bits, name):
  """Everything the device is compared with, from the bias row and the waveform alone (fp64)."""
  Cn = 1 << bits
  ocfg = O.OracleConfig(**CAT_KW, bits=bits)
  params = constant_head_params(ocfg, cat_bias(bits, name))
  x = cat_input(bits)
  target = O.quantize(x[:, 1:, 0], bits)
  logits = params[-1].double().expand(B, T, Cn).clone().requires_grad_(True)
  q = torch.softmax(logits, dim=-1)
  rows = O.loss_categorical(target, q)
  gl, = torch.autograd.grad(rows.sum() / B, logits)
  loss, _, grads, pred = O.loss_and_grads(x.double(), [p.double() for p in params], ocfg)
  assert torch.equal(pred, q.detach())                       # the oracle's head is the bias row too
  q = q.detach()
  qt = torch.gather(q, -1, target.unsqueeze(-1))[..., 0]
  others = ((q < EPS) | (q > 1 - EPS)).any(-1)
  regime = torch.where(qt > 1 - EPS, 1, torch.where(qt < EPS, 2, torch.where(others, 3, 4)))
  return dict(params=params, x=x, target=target, q=q, rows=rows.detach(), gl=gl, loss=loss, grads=grads, regime=regime)


@pytest.mark.parametrize('bits', [4, 8, 9])
def test_categorical_regimes_hold_on_the_reference(bits):
  """Conditions, not measurements: asserted on the fp64 reference before anything runs on the device."""
  Cn = 1 << bits
  regimes = torch.cat([cat_reference(bits, n)['regime'].reshape(-1) for n in CAT_BIASES])
  counts = torch.bincount(regimes, minlength=5)[1:]
  print(f'bits={bits}: rows with target above 1-eps / below eps / inside with others clipped / nothing clipped:', counts.tolist())
  assert torch.all(counts >= 32)
  tg = cat_reference(bits, 'flat')['target']
  assert (tg == 0).sum() >= 32 and (tg == Cn - 1).sum() >= 32 and (tg == c_star(Cn)).sum() >= 32
  # no target sits at a threshold: its own indicator moves its gradient by gscale (test_loss_reference_cpu.py)
  for n in CAT_BIASES:
    r = cat_reference(bits, n)
    qt = torch.gather(r['q'], -1, r['target'].unsqueeze(-1))
    assert torch.all(((qt / EPS - 1).abs() > 0.3) & (((1 - qt) / EPS - 1).abs() > 0.3)), n


def check_probs(tag, got, logits64):
  """Returned probabilities against the fp64 softmax of the same logits.  fp32 evaluates expf(l - m) / z: the difference
  l - m is rounded to half a unit of its own last place, <= |l - m| 2^-24, and that absolute error of the argument is a
  relative one of the exponential (2.1e-6 for logits 36 apart: the largest term by far); expf, the 2^bits-term sum,
  the reciprocal and the product stay under 16 units of 2^-24 together.  Below the smallest normal fp32 number
  (2^-126) a probability is denormal or 0."""
  q = torch.softmax(logits64, -1)
  gap = logits64.max(-1, keepdim=True).values - logits64
  bar = q * 2.0 ** -24 * (gap + 16.0) + 2.0 ** -126
  ratio = ((got.double().reshape(q.shape) - q).abs() / bar).max().item()
  rel = ((got.double().reshape(q.shape) - q).abs() / q)[q > 1e-30].max().item()
  print(f'{tag} returned probabilities: worst err / bar {ratio:.3e}, worst relative error {rel:.3e} (largest logit gap {gap.max().item():.1f})')
  assert ratio <= 1.0


def check_cat_step(tag, got, ref_rows, ref_gl, fused):
  loss, rows, g, _, _, amax = got
  assert loss[2].item() == 0
  e_rows = (rows - ref_rows).abs().max().item()
  e_g = (g.reshape(ref_gl.shape) - ref_gl).abs().max().item()
  bar_g = 1e-4 * ref_gl.abs().max().item() + 1e-7
  print(f'{tag} [{"fused epilogue" if fused else "row kernel"}] loss rows max|err| {e_rows:.3e} (bar 1e-5)  '
        f'dL/dlogits max|err| {e_g:.3e} (bar {bar_g:.3e}, max|ref| {ref_gl.abs().max().item():.3e})')
  assert e_rows <= 1e-5
  assert abs(loss[0].item() - ref_rows.sum().item() / B) <= 1e-5 * T
  assert e_g <= bar_g
  assert amax >= g.abs().max().item()                        # what the range guard of the backward pass reads


@pytest.mark.parametrize('name', CAT_BIASES)
@pytest.mark.parametrize('bits', [4, 8, 9])
def test_categorical_constant_head(bits, name, math_mode):
  """C = 16 (persistent kernel, three of four register slots empty), 256 (persistent kernel; in split mode without
  want_pred the fused epilogue of the head's last conv), 512 (loop kernel).  Bars: loss rows 1e-5 absolute, dL/dlogits
  and every parameter gradient 1e-4 max|ref| + 1e-7 per tensor; no element is excused near the clip thresholds."""
  Cn = 1 << bits
  r = cat_reference(bits, name)
  model = model_for(dict(CAT_KW, bits=bits), r['params'])
  nf = len(CAT_KW['final_layers_channels'])
  tag = f'cat bits={bits} {name} {math_mode}'
  for want_pred in (False, True):
    fused = bits == 8 and math_mode == 'split' and not want_pred
    got = run_step(model, r['x'], nf, want_pred, fused)
    check_cat_step(tag, got, r['rows'], r['gl'], fused)
    if not fused:
      assert torch.equal(got[3].reshape(B, T, Cn), r['params'][-1].expand(B, T, Cn))    # 0 * a + bias, exactly
    worst = 0.0
    for n, gd, gr in zip(model.variable_names, model.gradients(), r['grads']):
      err = (gd.cpu().double() - gr).abs().max().item()
      worst = max(worst, err / (1e-4 * gr.abs().max().item() + 1e-7))
      assert err <= 1e-4 * gr.abs().max().item() + 1e-7, (n, err)
    print(f'{tag} parameter gradients: worst err / bar {worst:.3e}')
    if want_pred:
      check_probs(tag, got[4], r['params'][-1].double().expand(B, T, Cn))


def test_categorical_scaled_head_per_row_variety(math_mode):
  """The last kernel times 60 instead of zero: every row its own logits, |logit| up to 15..30, about half of all class
  probabilities below the clip.  The standalone kernel is compared with the fp64 evaluation of the device's own logits
  (region 5), the fused epilogue with the standalone result of the same model and input, at the same bars."""
  kw = dict(blocks=4, channels=64, skip_channels=256, dilation_bound=1024, final_layers_channels=[128, 256],
            activation='leaky_relu', bits=8)
  ocfg = O.OracleConfig(**kw)
  params = O.init_params(ocfg, seed=4)
  params[-2] = params[-2] * 60.0
  x = O.synthetic_waveform(B, T + 1, seed=8)
  lg = O.model_forward(x[:, :-1].double(), [p.double() for p in params], ocfg, return_logits=True)
  qo = torch.softmax(lg, -1)
  print(f'oracle: max|logit| {lg.abs().max().item():.2f}, share of class probabilities below the clip '
        f'{(qo < EPS).double().mean().item():.3f}')
  assert 15.0 <= lg.abs().max().item() <= 30.0 and (qo < EPS).double().mean().item() >= 0.25
  model = model_for(kw, params)
  nf = len(kw['final_layers_channels'])
  alone = run_step(model, x, nf, True, False)
  logits = alone[3].double().reshape(B, T, 256).requires_grad_(True)
  assert (logits.detach() - lg).abs().max().item() < 1e-4 * 60
  target = O.quantize(x[:, 1:, 0], 8)
  q = torch.softmax(logits, -1)
  rows = O.loss_categorical(target, q)
  gl, = torch.autograd.grad(rows.sum() / B, logits)
  qt = torch.gather(q.detach(), -1, target.unsqueeze(-1))
  clipped_t = ((qt < EPS) | (qt > 1 - EPS)).sum().item()
  print(f'targets clipped: {clipped_t} of {B * T}')
  assert clipped_t >= 32
  # a target within 1e-3 of a threshold could take either side of it in fp32 (its gradient then moves by gscale)
  assert torch.all(((qt / EPS - 1).abs() > 1e-3) & (((1 - qt) / EPS - 1).abs() > 1e-3))
  check_cat_step(f'cat_r64 x60 {math_mode}', alone, rows.detach(), gl, False)
  check_probs(f'cat_r64 x60 {math_mode}', alone[4], logits.detach())
  if math_mode == 'split':
    fused = run_step(model, x, nf, False, True)
    check_cat_step('cat_r64 x60 split, against the standalone result', fused, alone[1], alone[2].reshape(gl.shape), True)


@pytest.mark.parametrize('rows', [1, 5, 257])
@pytest.mark.parametrize('Cn', [16, 100, 256, 1000])
def test_categorical_loss_of_probabilities(Cn, rows):
  """wn_cat_loss_probs_kernel (WaveNet.loss_fn): every row holds exact 0 and 1, 1e-7f and 1 - 1e-7 rounded to fp32 with
  their fp32 neighbours and a denormal; three rows in four do not sum to 1 (Keras renormalises by S).  The output
  buffer is one element longer than the rows and that element must survive."""
  from wavenets_amd import _lib
  f = np.float32
  lo, hi = f(1e-7), f(1.0) - f(1e-7)
  special = np.array([0.0, 1.0, lo, np.nextafter(lo, f(0)), np.nextafter(lo, f(1)), hi, np.nextafter(hi, f(0)),
                      np.nextafter(hi, f(2)), 1e-40], dtype=f)
  assert special[-1] > 0 and special[-1] < np.finfo(f).tiny
  g = torch.Generator().manual_seed(Cn * 1000 + rows)
  p = torch.softmax(torch.randn(rows, Cn, generator=g) * 3, -1)
  p = p * torch.tensor([1.0, 0.5, 3.0, 0.01])[torch.arange(rows) % 4].unsqueeze(-1)
  target = torch.randint(0, Cn, (rows,), generator=g)
  for r in range(rows):
    pos = [(r * 7 + k) % Cn for k in range(len(special))]
    p[r, pos] = torch.from_numpy(special)
    # targets: each special value in turn, then class 0, class C - 1 and a random class
    target[r] = pos[r % 9] if r % 12 < 9 else [0, Cn - 1, int(target[r])][r % 12 - 9]
  ref = O.loss_categorical(target.reshape(1, rows), p.double().reshape(1, rows, Cn))[0]
  out = torch.full((rows + 1,), SENTINEL, dtype=torch.float32, device=dev())
  pd, td = p.to(dev()).contiguous(), target.to(dev()).to(torch.int32).contiguous()
  _lib.check(_lib.lib().wn_loss_fn(_lib.HEADS['categorical'], _lib.ptr(td), _lib.ptr(pd), rows, Cn, 0, 8, _lib.ptr(out),
                                   _lib.stream_ptr()))
  out = out.cpu()
  err = (out[:rows].double() - ref).abs().max().item()
  print(f'probs kernel C={Cn} rows={rows}: max|err| {err:.3e} (bar 1e-5), loss range {ref.min().item():.3f} .. {ref.max().item():.3f}')
  assert out[rows].item() == SENTINEL
  assert err <= 1e-5
  if Cn == 256:
    model = model_for(dict(CAT_KW, bits=8), constant_head_params(O.OracleConfig(**CAT_KW, bits=8), torch.zeros(256)))
    got = model.loss_fn(td.reshape(1, rows, 1), pd.reshape(1, rows, Cn)).cpu()
    assert torch.equal(got.reshape(-1), out[:rows])


# ------------------------------------------------------------------------------------------
# mixture heads: the floor, the cap, both tails
# ------------------------------------------------------------------------------------------
def mix_groups():
  z = np.load(GOLDEN)
  out = []
  for k in sorted(z.files):
    if k.endswith('_pred'):
      key = k[:-5]
      kind, m, b = key.split('_')
      out.append(dict(key=key, kind=kind, M=int(m[1:]), bits=int(b[1:]),
                      **{f: z[f'{key}_{f}'] for f in ('pred', 'y', 'loss', 'grad', 'exp10')}))
  return out


MIX_GROUPS = mix_groups()


def mix_loss_rows(kind, M, bits, pred, y):
  """wn_loss_fn on (rows, 3M) fp32 parameters and (rows,) fp32 targets; one more output element than rows, which must
  survive."""
  from wavenets_amd import _lib
  rows = len(y)
  out = torch.full((rows + 1,), SENTINEL, dtype=torch.float32, device=dev())
  pd, yd = torch.from_numpy(pred).to(dev()).contiguous(), torch.from_numpy(y).to(dev()).contiguous()
  _lib.check(_lib.lib().wn_loss_fn(_lib.HEADS[kind], _lib.ptr(yd), _lib.ptr(pd), rows, 3 * M, M, bits, _lib.ptr(out),
                                   _lib.stream_ptr()))
  out = out.cpu()
  assert out[rows].item() == SENTINEL
  return out[:rows].double()


def check_mix_rows(tag, got, exact, exp10):
  """One fp32 rounding of a double evaluation: |loss - exact| <= 1e-6 max(1, |exact|) (6e-8 with a margin of 16) where
  the exact likelihood is above 1e-280; +inf on both sides where it is below 1e-320."""
  exact = torch.from_numpy(exact)
  fin = torch.from_numpy(exp10 > -280)
  assert torch.all(fin | torch.from_numpy(exp10 < -320))
  err = (got[fin] - exact[fin]).abs() / exact[fin].abs().clamp(min=1.0)
  bad = (~(err <= 1e-6)).nonzero().reshape(-1).tolist()      # (a NaN or an inf on the device counts as a miss)
  print(f'{tag}: {int(fin.sum())} finite rows, worst |err| / max(1, |exact|) {err.max().item() if len(err) else 0.0:.3e} (bar 1e-6), '
        f'{int((~fin).sum())} underflowed rows')
  fin_idx = fin.nonzero().reshape(-1)
  assert not bad, [(int(fin_idx[i]), got[fin][i].item(), exact[fin][i].item()) for i in bad[:8]]
  assert torch.all(got[~fin] == float('inf'))


@pytest.mark.parametrize('g', MIX_GROUPS, ids=[g['key'] for g in MIX_GROUPS])
def test_mixture_loss_rows_floor_cap_and_tails(g):
  """The rows of tests/golden/mix_tails.npz through wn_mix_loss_kernel: the same fp32 inputs the 50-digit evaluation
  read.  257 rows (the group's rows repeated: a second, one-thread workgroup), one row alone, and the mirrored rows
  (-y; -mu), whose exact loss is the same."""
  n = len(g['y'])
  idx = np.arange(257) % n
  got = mix_loss_rows(g['kind'], g['M'], g['bits'], g['pred'][idx], g['y'][idx])
  check_mix_rows(f'{g["key"]} 257 rows', got, g['loss'][idx], g['exp10'][idx])
  one = int(np.argmax(np.where(g['exp10'] > -280, g['y'] - g['pred'][:, g['M']], -np.inf)))   # deepest finite upper side of component 0
  got1 = mix_loss_rows(g['kind'], g['M'], g['bits'], g['pred'][one:one + 1], g['y'][one:one + 1])
  check_mix_rows(f'{g["key"]} row {one} alone', got1, g['loss'][one:one + 1], g['exp10'][one:one + 1])
  assert got1[0] == got[one]
  M = g['M']
  mirrored = g['pred'][idx].copy()
  mirrored[:, M:2 * M] = -mirrored[:, M:2 * M]
  gotm = mix_loss_rows(g['kind'], M, g['bits'], mirrored, -g['y'][idx])
  check_mix_rows(f'{g["key"]} mirrored', gotm, g['loss'][idx], g['exp10'][idx])
  if g['key'] == 'logistic_M10_b16':
    from test_gpu_parity import MODEL_CASES
    kw = dict(MODEL_CASES['mol'])
    model = model_for(kw, O.init_params(O.OracleConfig(**kw), seed=1))
    via = model.loss_fn(torch.from_numpy(g['y'][idx]).reshape(1, 257, 1), torch.from_numpy(g['pred'][idx]).reshape(1, 257, 30))
    assert torch.equal(via.cpu().reshape(-1).double(), got)


@pytest.mark.parametrize('M', [0, 33])
@pytest.mark.parametrize('kind', ['logistic', 'gaussian'])
def test_mixture_loss_rejects_unsupported_mixture_counts(kind, M):
  from wavenets_amd import _lib
  out = torch.full((4,), SENTINEL, dtype=torch.float32, device=dev())
  pred = torch.zeros(3, 3 * max(M, 1), dtype=torch.float32, device=dev())
  y = torch.zeros(3, dtype=torch.float32, device=dev())
  rc = _lib.lib().wn_loss_fn(_lib.HEADS[kind], _lib.ptr(y), _lib.ptr(pred), 3, 3 * M, M, 16, _lib.ptr(out), _lib.stream_ptr())
  assert rc == _lib.WN_E_UNSUPPORTED
  torch.cuda.synchronize()
  assert torch.all(out.cpu() == SENTINEL)                     # refused before any launch


def mix_bias_rows(kind):
  """Fixture rows that serve as the constant head's output: (name, pred row)."""
  if kind == 'logistic':
    g = next(g for g in MIX_GROUPS if g['key'] == 'logistic_M10_b16')
    p = g['pred']
    broad = next(r for r in p if r[20 + 3] == 0 and r[20] == -9 and r[:10].max() < 1)       # one broad component, the rest below the floor
    sharp = next(r for r in p if np.all(r[20:] == -7) and r[:10].max() > 30)                 # all at the floor, one weight 40 above
    return [('one broad, the rest below the floor', broad), ('all at the floor, one weight raised', sharp)]
  g = next(g for g in MIX_GROUPS if g['key'] == 'gaussian_M8_b16')
  p = g['pred']
  return [('broad and floor-sharp', next(r for r in p if r[8] > -1e4)), ('one component beyond the cap', next(r for r in p if r[8] < -1e4))]


MIX_GRAD_CASES = [(n, i) for n in ('mol', 'gauss') for i in (0, 1)]


@pytest.mark.parametrize('name,which', MIX_GRAD_CASES)
def test_mixture_gradients_constant_head(name, which, math_mode):
  """dL/dpred of the mixture kernel inside a training step: the 'mol' / 'gauss' networks of the parity suite (M = 10 and
  8) with a zero last kernel and a fixture row as its bias, the targets from a waveform that sweeps both sides of every
  mean.  Reference: gscale times the fp64 autograd gradient of O.loss_logistic_exact / O.loss_gaussian, row by row.
  Bar: 1e-6 of the reference row's largest |entry| + 1e-30; no row excused (asserted: every likelihood above 1e-280)."""
  from test_gpu_parity import MODEL_CASES
  kw = dict(MODEL_CASES[name])
  kind, M = kw['sampling_function'], kw['num_mixtures']
  label, bias = mix_bias_rows(kind)[which]
  ocfg = O.OracleConfig(**kw)
  params = constant_head_params(ocfg, bias, seed=4)
  t = torch.arange(T + 1, dtype=torch.float64)
  x = torch.stack([0.98 * torch.sin(2 * math.pi * (t / 61.0 + 0.37 * b)) for b in range(B)]).float().unsqueeze(-1)
  y = x[:, 1:, :].double()
  pred = torch.from_numpy(bias).double().expand(B, T, 3 * M).clone().requires_grad_(True)
  rows = O.loss_logistic_exact(y, pred, M, kw['bits']) if kind == 'logistic' else O.loss_gaussian(y, pred, M)
  ref, = torch.autograd.grad(rows.sum() / B, pred)
  rows = rows.detach()
  assert torch.all(torch.isfinite(rows)) and torch.all(-rows / math.log(10.0) > -280)
  mu = pred.detach()[..., M:2 * M]
  assert ((y - mu) > 0.03).any(0).any(0).sum() >= M - 1 and ((y - mu) < -0.03).any(0).any(0).sum() >= M - 1
  model = model_for(kw, params)
  nf = len(kw['final_layers_channels'])
  loss, got_rows, g, logits, out, amax = run_step(model, x, nf, True, False)
  assert loss[2].item() == 0
  assert torch.equal(out.reshape(B, T, 3 * M), torch.from_numpy(bias).expand(B, T, 3 * M))      # the bias row, exactly
  e_rows = ((got_rows - rows).abs() / rows.abs().clamp(min=1.0)).max().item()
  g = g.reshape(B, T, 3 * M)
  bar = 1e-6 * ref.abs().max(-1, keepdim=True).values + 1e-30
  ratio = ((g - ref).abs() / bar).max().item()
  print(f'{name} ({label}) {math_mode}: loss rows worst |err| / max(1, |exact|) {e_rows:.3e} (bar 1e-6); '
        f'dL/dpred worst |err| / (1e-6 row max + 1e-30) {ratio:.3e}; loss range {rows.min().item():.2f} .. {rows.max().item():.2f}')
  assert e_rows <= 1e-6
  assert torch.all(torch.isfinite(g)) and ratio <= 1.0
  assert amax >= g.abs().max().item()
  if label == 'one component beyond the cap':
    assert torch.all(g[..., M] == 0) and torch.all(g[..., 2 * M] == 0)      # d mu and d log-scale of the capped component
  loss2 = model.loss_and_grads(x.to(dev()))[0]
  assert loss2[0].item() == loss[0].item()
