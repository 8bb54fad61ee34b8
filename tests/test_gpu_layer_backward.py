"""The standalone residual block (WaveNetLayer / wn_layer_fwd / wn_layer_bwd) against tests/layer_reference.py in float64
(DESIGN.md section 29).

Its backward does not use the training step's job table: every weight gradient is its own wn_wgrad_kernel launch followed by
wn_launch_reduce, and it has branches the model never takes -- the time-varying condition (dW_c, db_c, g_cond; g_cond on the
one-row-tile prefetch-ring form of wn_gemm_rows_kernel for D in {32, 64, 128} and Cc <= 32), the two-stage reduce (more than
32 splits), dilations longer than a split, in_channels != channels, and the C-ABI's null-gradient branches.

Bar (as in section 18): max|got - ref| <= 1e-4 max|ref| for every activation and data gradient,
+ 1e-7 for parameter gradients; forward outputs also 1e-4 absolute.  Weights uniform +-0.2 (_layer_pair), inputs randn * 0.7.
The fp64 reference of a case is built once and shared by both math modes.

  A  parity at B = 2: eight cases around the condition, in_channels and stack depth, and the ten LAYER_CASES
  B  many splits: every product on the two-stage reduce (asserted on wn_layer_describe); a determinism check
  C  the C-ABI's null branches, through ctypes on buffers the test owns
  D  three copies of one utterance equal the utterance alone, bit for bit (ragged last tiles)
  E  the autograd surface: interleaved calls, cond.grad, x without requires_grad
"""
import ctypes as C
import functools

import pytest
import torch

import layer_reference as LR
from test_gpu_parity import ATOL_ACT, LAYER_CASES, _layer_pair, dev

pytestmark = pytest.mark.gpu

RTOL = 1e-4               # of the tensor's max
ATOL_PARAM = 1e-7         # parameter gradients, on top


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  """Both contraction modes: 'split' = fp16 hi/lo 3-product MFMA (default), 'fp32' = exact-fp32 MFMA (debug knob 1).  The
  standalone block's backward is exact fp32 in both; the mode changes the forward kernels that fill `saved`."""
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


# id: R, D, S, KS, dilations, Cin, Cc, activation, residual, B, T
A_CASES = {
    'c5_r32':    (32, 32, 64, 2, [8], 32, 5, None, True, 2, 257),
    'c8_r64':    (64, 64, 256, 2, [4], 64, 8, None, True, 2, 300),
    'c36_r128':  (128, 128, 256, 2, [16], 128, 36, None, True, 2, 130),
    'c12_k3':    (64, 64, None, 3, [2], 64, 12, None, False, 2, 97),
    'c7_deep':   (32, 32, 48, 2, [1, 2, 4], 32, 7, 'leaky_relu', True, 2, 90),
    'c3_odd':    (8, 12, 20, 2, [2], 8, 3, None, True, 2, 70),
    'cin16':     (32, 32, 64, 2, [4], 16, 0, None, False, 2, 100),
    'cin1_deep': (16, 24, 40, 2, [2, 1], 1, 0, 'tanh', False, 2, 77),
}
for _i, (_R, _D, _S, _dil, _k, _act, _res, _T) in enumerate(LAYER_CASES):
  A_CASES[f'layer_case{_i}'] = (_R, _D, _S, _k, _dil if isinstance(_dil, list) else [_dil], _R, 0, _act, _res, 2, _T)
assert len(A_CASES) == 18

# every product of these must take the two-stage reduce with this nsplit (wn_layer_describe); the last column: sizes of the
# stage-A groups
B_CASES = {
    'r64_d512':       ((64, 64, 256, 2, [512], 64, 0, None, True, 3, 2900), 36, (16, 16, 4)),
    'r32_k3_d243_c5': ((32, 32, 64, 3, [243], 32, 5, None, True, 3, 2900), 36, (16, 16, 4)),
    'r128_one_utt':   ((128, 128, 256, 2, [16], 128, 0, None, True, 1, 8300), 33, (16, 16, 1)),
}
ALL_CASES = dict(A_CASES, **{k: v[0] for k, v in B_CASES.items()})


def _aligned(*ts):
  for t in ts:
    if t is not None:
      assert t.data_ptr() % 16 == 0 and t.is_contiguous()      # the vector paths are the ones exercised


def _inputs(B, T, cin, Cc, R, S, seed=11):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(B, T, cin, generator=g) * 0.7
  cond = torch.randn(B, T, Cc, generator=g) * 0.7 if Cc else None
  return x, cond, torch.randn(B, T, R, generator=g), torch.randn(B, T, S or R, generator=g)


def _reference(spec, ps, x, cond, gx, gs):
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  f = lambda t: None if t is None else t.double()
  ref = LR.layer_reference(f(x), f(cond), [p.double() for p in ps], dilations=dil, kernel_size=KS, activation=act,
                           residual=res, has_skip=S is not None, g_xout=f(gx), g_skip=f(gs))
  if act in ('relu', 'leaky_relu'):
    # no pre-activation within rounding of the kink: the product's fp32 value (error ~1e-6) lies on the reference's side
    for q in ref['pre']:
      assert q.abs().min().item() >= 1e-5
  return ref


@functools.lru_cache(maxsize=None)
def _case(name):
  """(spec, layer, oracle parameters, inputs, fp64 reference with both gradients): built once, shared by both math modes."""
  spec = ALL_CASES[name]
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  layer, ps, dl = _layer_pair(R, D, S, dil, k=KS, act=act, residual=res, cin=cin, cond_c=Cc)
  assert dl == dil
  inp = _inputs(B, T, cin, Cc, R, S)
  return spec, layer, ps, inp, _reference(spec, ps, *inp)


def describe(layer, B, T):
  """[(product, K, N, splits per utterance, nsplit, reduce form)] of wn_layer_describe."""
  from wavenets_amd import _lib
  buf = C.create_string_buffer(4096)
  _lib.check(_lib.lib().wn_layer_describe(C.byref(layer._desc), B, T, buf, 4096))
  out = []
  for item in buf.value.decode().split(' | '):
    name, *toks = item.split()
    kv = dict(t.split('=') for t in toks)
    out.append((name, int(kv['K']), int(kv['N']), int(kv['splits']), int(kv['nsplit']), kv['reduce']))
  return out


def _split_of(t, T, splits):
  """The time range of wn_wgrad_kernel that row t falls in: (index, first row, end row)."""
  ln = (T + splits - 1) // splits
  ln = (ln + 1) & ~1
  s = t // ln
  return s, s * ln, min(T, s * ln + ln)


class Report:
  """Collects the figure of every compared tensor, prints them, then fails on all that miss the bar at once."""

  def __init__(self, tag, T=None, splits=None):
    self.tag, self.T, self.splits, self.lines, self.bad = tag, T, splits, [], []

  def check(self, name, got, ref, atol=0.0, absolute=None, rows=False):
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    assert torch.isfinite(got).all(), (self.tag, name, 'non-finite')
    scale = ref.abs().max().item()
    err = (got - ref).abs()
    worst = err.max().item()
    idx = tuple(int(i) for i in torch.unravel_index(err.argmax(), err.shape))
    self.lines.append(f'FIG {self.tag} {name} rel={worst / max(scale, 1e-300):.2e} max|ref|={scale:.3e}')
    ok = worst <= RTOL * scale + atol and (absolute is None or worst <= absolute)
    if not ok:
      where = f'worst at {idx}'
      if rows and self.T is not None:
        where = f'worst at (utterance {idx[0]}, t {idx[1]}, channel {idx[2]})'
        if self.splits:
          s, r0, r1 = _split_of(idx[1], self.T, self.splits)
          where += f', in weight-gradient split {s} of utterance {idx[0]} (rows {r0}..{r1 - 1}, {self.splits} an utterance)'
      over = int((err > RTOL * scale + atol).sum())
      self.bad.append(f'{name}: max error {worst:.3e} against a bar of {RTOL * scale + atol:.3e} (max|ref| {scale:.3e}), '
                      f'{where}, {over} elements over the bar')
    return worst / max(scale, 1e-300)

  def finish(self):
    print('\n'.join(self.lines))
    assert not self.bad, f'{self.tag}:\n  ' + '\n  '.join(self.bad)


def _run(layer, x, cond, gx, gs):
  """One forward + backward through the autograd surface.  Returns (x_out, skip, gate, z, g_x, g_cond, flat gradient)."""
  d = dev()
  xd = x.to(d).requires_grad_(True)
  cd = cond.to(d).requires_grad_(True) if cond is not None else None
  gxd = gx.to(d) if gx is not None else None
  gsd = gs.to(d) if gs is not None else None
  _aligned(xd, cd, gxd, gsd, layer.flat_params)
  xo, sk = layer((xd, cd)) if cd is not None else layer(xd)
  saved = xo.grad_fn.saved_tensors[3]                   # [activated stack outputs ... | sigmoid gate | z], rows x D each
  _aligned(xo, sk, saved)
  rows, D = x.shape[0] * x.shape[1], layer.dilation_channels
  nst = layer.depth - 1
  reg = -(-rows * D // 64) * 64                         # every region starts on a multiple of 64 floats
  assert saved.numel() == (nst + 2) * reg
  gate = saved[nst * reg:nst * reg + rows * D].view(x.shape[0], x.shape[1], D)
  z = saved[(nst + 1) * reg:(nst + 1) * reg + rows * D].view(x.shape[0], x.shape[1], D)
  outs = [(o, g) for o, g in ((xo, gxd), (sk, gsd)) if g is not None]
  wrt = [xd] + ([cd] if cd is not None else []) + [layer.flat_params]
  gr = torch.autograd.grad([o for o, _ in outs], wrt, grad_outputs=[g for _, g in outs])
  return xo.detach(), sk.detach(), gate.detach().clone(), z.detach().clone(), gr[0], gr[1] if cd is not None else None, gr[-1]


def _compare(rep, spec, ref, xo, sk, gate, z, g_x, g_cond, g_flat):
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  if xo is not None:
    rep.check('x_out', xo, ref['x_out'], absolute=ATOL_ACT, rows=True)
    rep.check('skip', sk, ref['skip'], absolute=ATOL_ACT, rows=True)
  if gate is not None:
    rep.check('gate', gate, ref['gate'], rows=True)
    rep.check('z', z, ref['z'], rows=True)
  rep.check('g_x', g_x, ref['g_x'], rows=True)
  if Cc:
    rep.check('g_cond', g_cond, ref['g_cond'], rows=True)
  names = LR.param_grad_names(len(dil), S is not None, Cc > 0)
  off = 0
  for n, r in zip(names, ref['param_grads']):
    rep.check(n, g_flat[off:off + r.numel()], r, atol=ATOL_PARAM)
    off += r.numel()
  assert off == g_flat.numel()


def _splits(layer, B, T):
  """Splits per utterance of the gated conv's products (what a data-gradient failure is located in)."""
  return [p for p in describe(layer, B, T) if p[0].startswith(f'dil{layer.depth - 1}.')][0][3]


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize('name', list(A_CASES))
def test_parity_against_the_fp64_reference(name, math_mode):
  spec, layer, ps, (x, cond, gx, gs), ref = _case(name)
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  assert B == 2 and ref['g_x'].shape == (B, T, cin) and ref['g_x'].abs().max() > 0
  got = _run(layer, x, cond, gx, gs)
  rep = Report(f'{name} [{math_mode}]', T, _splits(layer, B, T))
  _compare(rep, spec, ref, *got)
  rep.finish()


# ------------------------------------------------------------------------------------------ B
def _assert_two_stage(name, layer, B, T):
  _, nsplit, groups = B_CASES[name]
  prods = describe(layer, B, T)
  assert sum(groups) == nsplit and all(g <= 16 for g in groups) and len(groups) == -(-nsplit // 16)
  for p in prods:
    assert p[4] == nsplit and p[5] == 'two-stage' and p[3] * B == nsplit, (name, p)
  return prods


@pytest.mark.parametrize('name', list(B_CASES))
def test_many_splits_take_the_two_stage_reduce(name, math_mode):
  spec, layer, ps, (x, cond, gx, gs), ref = _case(name)
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  prods = _assert_two_stage(name, layer, B, T)
  splits = prods[0][3]
  # a dilation longer than a split: whole splits at an utterance's start have no valid shifted row
  ln = _split_of(0, T, splits)[2]
  shift = (KS - 1) * dil[0]
  if name != 'r128_one_utt':
    assert shift > ln and (shift // ln) >= 2
  got = _run(layer, x, cond, gx, gs)
  rep = Report(f'{name} [{math_mode}]', T, splits)
  _compare(rep, spec, ref, *got)
  rep.finish()


def test_two_stage_reduce_is_deterministic():
  """The reduce's comments promise a fixed order of summation: two backward calls give the same bits."""
  spec, layer, ps, (x, cond, gx, gs), ref = _case('r64_d512')
  _assert_two_stage('r64_d512', layer, spec[9], spec[10])
  a = _run(layer, x, cond, gx, gs)
  b = _run(layer, x, cond, gx, gs)
  assert torch.equal(a[6], b[6]) and torch.equal(a[4], b[4])
  assert a[6].abs().max() > 0


# ------------------------------------------------------------------------------------------ C
class CabiLayer:
  """wn_layer_fwd / wn_layer_bwd through ctypes on buffers this object owns."""

  def __init__(self, layer, x, cond):
    from wavenets_amd import _lib
    self.L, self._lib = _lib.lib(), _lib
    self.d, self.flat = layer._desc, layer.flat_params.detach()
    self.B, self.T = x.shape[0], x.shape[1]
    self.x, self.cond = x.to(dev()).contiguous(), cond.to(dev()).contiguous() if cond is not None else None
    n = lambda f: int(f(C.byref(self.d), self.B, self.T))
    self.saved = torch.full((n(self.L.wn_layer_saved_floats),), 7.0, device=dev())
    self.ws = torch.full((n(self.L.wn_layer_workspace_floats),), 7.0, device=dev())
    R, S = layer.channels, layer.skip_channels or layer.channels
    self.x_out = torch.empty(self.B, self.T, R, device=dev())
    self.skip = torch.empty(self.B, self.T, S, device=dev())
    _aligned(self.flat, self.x, self.cond, self.saved, self.ws, self.x_out, self.skip)
    p = _lib.ptr
    _lib.check(self.L.wn_layer_fwd(C.byref(self.d), p(self.flat), p(self.x), p(self.cond), self.B, self.T, p(self.x_out),
                                   p(self.skip), p(self.saved), p(self.ws), _lib.stream_ptr()))

  def bwd(self, gxo, gsk, want_gx=True, want_gcond=True):
    """(g_params, g_x or None, g_cond or None); every output buffer holds 7.0 before the call."""
    p = self._lib.ptr
    gxo = gxo.to(dev()).contiguous() if gxo is not None else None
    gsk = gsk.to(dev()).contiguous() if gsk is not None else None
    g_params = torch.full_like(self.flat, 7.0)
    g_x = torch.full_like(self.x, 7.0) if want_gx else None
    g_cond = torch.full_like(self.cond, 7.0) if (want_gcond and self.cond is not None) else None
    _aligned(gxo, gsk, g_params, g_x, g_cond)
    self._lib.check(self.L.wn_layer_bwd(C.byref(self.d), p(self.flat), p(self.x), p(self.cond), p(self.saved), p(gxo), p(gsk),
                                        self.B, self.T, p(g_x), p(g_cond), p(g_params), p(self.ws), self._lib.stream_ptr()))
    torch.cuda.synchronize()
    return g_params, g_x, g_cond


# id: R, D, S, KS, dilations, Cin, Cc, activation, residual, B, T
C_CASES = {
    'c5_r32_skip': (32, 32, 64, 2, [8], 32, 5, None, True, 2, 257),
    'r64_noskip':  (64, 64, None, 2, [4], 64, 0, None, True, 2, 97),
}


@functools.lru_cache(maxsize=None)
def _cabi_case(name):
  spec = C_CASES[name]
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  layer, ps, dl = _layer_pair(R, D, S, dil, k=KS, act=act, residual=res, cin=cin, cond_c=Cc, seed=3)
  x, cond, gx, gs = _inputs(B, T, cin, Cc, R, S, seed=13)
  return spec, layer, ps, (x, cond, gx, gs), CabiLayer(layer, x, cond)


def _param_slices(spec, ref):
  names = LR.param_grad_names(len(spec[4]), spec[2] is not None, spec[6] > 0)
  out, off = {}, 0
  for n, r in zip(names, ref['param_grads']):
    out[n] = slice(off, off + r.numel())
    off += r.numel()
  return out


@pytest.mark.parametrize('which', ['xout_only', 'skip_only'])
@pytest.mark.parametrize('name', list(C_CASES))
def test_cabi_one_gradient_null(name, which):
  spec, layer, ps, (x, cond, gx, gs), cl = _cabi_case(name)
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  if which == 'xout_only':
    gs = None
  else:
    gx = None
  ref = _reference(spec, ps, x, cond, gx, gs)
  g_params, g_x, g_cond = cl.bwd(gx, gs)
  rep = Report(f'cabi {name} {which}', T, _splits(layer, B, T))
  _compare(rep, spec, ref, None, None, None, None, g_x, g_cond, g_params)
  rep.finish()
  sl = _param_slices(spec, ref)
  if S is not None:
    zero = ('dW_s', 'db_s') if which == 'xout_only' else ('dW_r', 'db_r')
    for n in zero:
      assert g_params[sl[n]].numel() > 0 and not g_params[sl[n]].any(), n        # exactly 0, every element written
  else:
    assert g_params[sl['dW_r']].abs().max() > 0                                    # S == 0: conv1 serves either gradient
  if which == 'skip_only' and res:
    # no residual term: g_x is the conv path alone (the reference's g_x above has none either); adding g_skip would show
    assert (g_x.double().cpu() - ref['g_x']).abs().max() < 1e-3 * gs.abs().max()


@pytest.mark.parametrize('name', list(C_CASES))
def test_cabi_both_gradients_null_writes_zeros_everywhere(name):
  spec, layer, ps, inp, cl = _cabi_case(name)
  g_params, g_x, g_cond = cl.bwd(None, None)
  assert g_params.numel() == layer.flat_params.numel() and not g_params.any()
  assert not g_x.any()
  if spec[6]:
    assert not g_cond.any()


@pytest.mark.parametrize('name', list(C_CASES))
def test_cabi_null_g_x_and_null_g_cond_change_nothing_else(name):
  spec, layer, ps, (x, cond, gx, gs), cl = _cabi_case(name)
  full = cl.bwd(gx, gs)
  assert full[0].abs().max() > 0 and not (full[0] == 7.0).any() and not (full[1] == 7.0).any()
  no_gx = cl.bwd(gx, gs, want_gx=False)
  assert no_gx[1] is None and torch.equal(no_gx[0], full[0])
  if spec[6]:
    assert not (full[2] == 7.0).any() and torch.equal(no_gx[2], full[2])
    no_gc = cl.bwd(gx, gs, want_gcond=False)
    assert no_gc[2] is None and torch.equal(no_gc[0], full[0]) and torch.equal(no_gc[1], full[1])
  again = cl.bwd(gx, gs)
  assert all(torch.equal(a, b) for a, b in zip(again, full) if a is not None)


def test_cabi_s0_both_gradients_sum_in_the_workspace():
  """skip_channels None with both gradients (g_o_tmp): against the reference, and equal to one call given their sum."""
  spec, layer, ps, (x, cond, gx, gs), cl = _cabi_case('r64_noskip')
  ref = _reference(spec, ps, x, cond, gx, gs)
  g_params, g_x, _ = cl.bwd(gx, gs)
  rep = Report('cabi r64_noskip both', spec[10], _splits(layer, spec[9], spec[10]))
  _compare(rep, spec, ref, None, None, None, None, g_x, None, g_params)
  rep.finish()
  summed = cl.bwd(None, (gx.to(dev()) + gs.to(dev())).cpu())
  assert torch.equal(summed[0], g_params)                   # the same g_o bits, by either route; g_x differs by the residual


# ------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize('name', ['c5_r32', 'c8_r64'])
def test_copies_of_one_utterance_equal_the_utterance_alone(name, math_mode):
  """Rows do not see each other: T = 257 and 300 end in ragged 32-row tiles, whose invalid rows the prefetch-ring form of the
  g_cond contraction clamps to row 0 of the utterance and zeroes by a select."""
  spec = A_CASES[name]
  R, D, S, KS, dil, cin, Cc, act, res, B, T = spec
  assert T % 32 != 0 and Cc <= 32 and D in (32, 64, 128)
  layer, ps, dl = _layer_pair(R, D, S, dil, k=KS, act=act, residual=res, cin=cin, cond_c=Cc)
  x, cond, gx, gs = _inputs(1, T, cin, Cc, R, S, seed=17)
  alone = _run(layer, x, cond, gx, gs)
  rep3 = lambda t: t.repeat(3, 1, 1)
  batch = _run(layer, rep3(x), rep3(cond), rep3(gx), rep3(gs))
  for label, i in (('x_out', 0), ('skip', 1), ('g_x', 4), ('g_cond', 5)):
    assert alone[i].abs().max() > 0
    for u in range(3):
      assert torch.equal(batch[i][u], alone[i][0]), (name, math_mode, label, u)


# ------------------------------------------------------------------------------------------ E
def test_autograd_interleaved_calls_share_no_state():
  """Two forwards of one layer at (2, 257) and (3, 300), the second backward first: the gradients of each equal a fresh
  layer's doing that call alone.  The layer's workspace is shared by all its calls and carries nothing between them."""
  mk = lambda: _layer_pair(32, 32, 64, 8, cond_c=5)[0]
  a_in, b_in = _inputs(2, 257, 32, 5, 32, 64, seed=21), _inputs(3, 300, 32, 5, 32, 64, seed=22)

  def fwd(layer, inp):
    xd, cd = inp[0].to(dev()).requires_grad_(True), inp[1].to(dev()).requires_grad_(True)
    xo, sk = layer((xd, cd))
    return (xo, sk), [xd, cd, layer.flat_params], [inp[2].to(dev()), inp[3].to(dev())]

  shared = mk()
  fa, fb = fwd(shared, a_in), fwd(shared, b_in)
  gb = torch.autograd.grad(*fb)
  ga = torch.autograd.grad(*fa)
  alone_a = torch.autograd.grad(*fwd(mk(), a_in))
  alone_b = torch.autograd.grad(*fwd(mk(), b_in))
  for got, ref in ((ga, alone_a), (gb, alone_b)):
    for g, r in zip(got, ref):
      assert r.abs().max() > 0 and torch.equal(g, r)


def test_autograd_cond_grad_and_frozen_input():
  spec, layer0, ps, (x, cond, gx, gs), ref = _case('c5_r32')
  layer = _layer_pair(32, 32, 64, 8, cond_c=5)[0]
  # cond.requires_grad_(): cond.grad is populated, and is the reference's
  xd, cd = x.to(dev()), cond.to(dev()).requires_grad_()
  xo, sk = layer((xd, cd))
  torch.autograd.backward([xo, sk], [gx.to(dev()), gs.to(dev())])
  assert cd.grad is not None and cd.grad.shape == cond.shape
  rep = Report('autograd c5_r32', spec[10])
  rep.check('cond.grad', cd.grad, ref['g_cond'], rows=True)
  # x without requires_grad: the parameters still get their gradient
  assert xd.grad is None and layer.flat_params.grad is not None
  names = LR.param_grad_names(1, True, True)
  off = 0
  for n, r in zip(names, ref['param_grads']):
    rep.check(n, layer.flat_params.grad[off:off + r.numel()], r, atol=ATOL_PARAM)
    off += r.numel()
  rep.finish()
  assert off == layer.flat_params.numel()
