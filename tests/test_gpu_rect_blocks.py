"""Blocks whose gated width D differs from their residual width R, and the square shapes outside R = D in {32, 64, 128} at
kernel size 2: the cases of tests/test_rect_blocks_cpu.py (which pins the kernel family each of them takes) against the fp64
oracle, block by block.

With R != D a transposed or mis-offset piece of a weight image cannot hide: the two-contraction forward's `[f f g g]` image
(K = KS * R steps per 2D columns), the backward's `[W_r | W_s]` / `[W_r | V]` images (second piece at k-step R / 16 of an
image with D rows) and the `g_x` image (KS pieces of 2D columns, R rows) are read here by the resident, streamed and thin
rows kernels, and the generic job table takes rectangular dW_d (R x 2D per tap) and dW_r (D x R) jobs in split precision.
The cases whose split-precision chain drops to the exact-fp32 kernel for one product (32 output columns without a padded
image; an operand width the split-precision images do not take) check that the running max-abs scales still connect.

Bars: DESIGN.md section 5 -- activations 1e-4 absolute, loss 2e-5 * max(1, |loss|), every gradient tensor 1e-4 of its own
scale (+ 1e-7), bit equality where the design claims it.  The leaky_relu kink of the head is treated as in
tests/test_gpu_baseline_nets.py: where the ORACLE's own pre-activation lies within O.KINK_TOL of 0 it takes the side the
product took; such decisions are counted and bounded."""
import pytest
import torch

from test_gpu_parity import ATOL_ACT, O, _inputs, _layer_pair, _rel, dev, make_pair, math_mode   # noqa: F401  (math_mode: fixture)
from test_rect_blocks_cpu import CASES, FWD_TWO, LAYER_SHAPES, SKIP_FOLDED, SPLIT_PATHS

pytestmark = pytest.mark.gpu

ALL_SIZES = ['r64_d128', 'r128_d64', 'r64_k3', 'r32_d64_fold']          # the cases that run at every (B, T)
TWO = [n for n in CASES if SPLIT_PATHS[n][0] == FWD_TWO and 'conditioning' not in CASES[n]]


def _dd(t):
  return t.double() if t is not None else None


def _to_dev(x, cond):
  return (x.to(dev()), cond.to(dev())) if cond is not None else x.to(dev())


_FORWARD = {}


def _oracle_forward(name, wseed, xseed, B, T):
  """Weights, B utterances of T + 1 samples and the oracle's fp64 forward over the first T, once for both math modes."""
  key = (name, wseed, xseed, B, T)
  if key not in _FORWARD:
    kw = CASES[name]
    ocfg = O.OracleConfig(**kw)
    params = O.init_params(ocfg, seed=wseed, bias_range=0.1)
    x, cond = _inputs(kw, B, T + 1, seed=xseed)
    with torch.no_grad():
      out, inter = O.model_forward(x[:, :-1].double(), [p.double() for p in params], ocfg, _dd(cond), return_intermediates=True)
    _FORWARD[key] = (ocfg, params, x, cond, out, inter)
  return _FORWARD[key]


_GRADS = {}


def _oracle_grads(name, wseed, xseed, B, T, head_branch):
  """fp64 loss and gradients: parameters, d loss / d u of every block, d loss / d H[b] of every block input.  Kept per case
  together with the kink decisions it was made with (they are the same in both math modes unless the product itself differs
  inside the undecided band)."""
  key = (name, wseed, xseed, B, T)
  hit = _GRADS.get(key)
  if hit is not None and all(torch.equal(a, b) for a, b in zip(hit[0], head_branch)):
    return hit[1]
  ocfg, params, x, cond, _, _ = _oracle_forward(name, wseed, xseed, B, T)
  ps = [p.double().requires_grad_(True) for p in params]
  pred, inter = O.model_forward(x[:, :-1].double(), ps, ocfg, _dd(cond), return_intermediates=True, head_branch=head_branch)
  loss = O.loss_fn(O.prepare_target(x[:, 1:].double(), ocfg), pred, ocfg).sum() / B
  want = inter['u'] + inter['h'][:-1]                    # (nothing flows into the last block output: skip head)
  gr = torch.autograd.grad(loss, ps + want, allow_unused=True)
  grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(gr[:len(ps)], ps)]
  nb = len(inter['u'])
  res = (loss.detach(), grads, gr[len(ps):len(ps) + nb], gr[len(ps) + nb:], inter['kink_overrides'],
         [a.detach() for a in inter['head_pre']])
  _GRADS[key] = ([b.clone() for b in head_branch], res)
  return res


def _ws(model, what, idx, B, T):
  return model.training_intermediate(what, idx, B, T).cpu().double().reshape(B, T, -1)


def _head_branch(model, n_hidden, B, T):
  """The side of the leaky_relu kink the product took for every head activation."""
  return [_ws(model, 4, i, B, T) >= 0 for i in range(n_hidden)]


def _check_kinks(head_pre, branch, n_kink):
  """Every disagreement between the product's side and the oracle's own sign is one the oracle resolved as a kink, lies inside
  the undecided band, and there are only a handful (a sign bug near zero could otherwise hide behind the mechanism)."""
  n_over, worst = 0, 0.0
  for a, br in zip(head_pre, branch):
    over = (a >= 0) != br
    n_over += int(over.sum())
    if over.any():
      worst = max(worst, a[over].abs().max().item())
  assert n_over == n_kink, (n_over, n_kink)
  assert worst < O.KINK_TOL, worst
  assert n_kink <= 8, n_kink


# ------------------------------------------------------------------------------------------
# (a) forward, block by block; (b) two kernels really ran
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_forward_block_by_block(name, math_mode):
  """B = 3, T = 333: 11 row tiles an utterance, 33 in all -- 5 workgroups of 8 waves with one tile in the last; the last tile
  of every utterance holds 13 rows.  What a training pass keeps (block inputs, gated activations, saved sigmoids, skip sum or
  first head activation) in block order, so that a layout error is named at the first block that shows it; then the
  inference pass."""
  B, T = 3, 333
  ocfg, params, x, cond, ref, inter = _oracle_forward(name, 1, 3, B, T)
  _, _, model = make_pair(seed=1, **dict(CASES[name]))
  model.loss_and_grads(_to_dev(x, cond))
  torch.cuda.synchronize()
  worst = dict(h=0.0, z=0.0, gate=0.0, head=0.0)

  def close(what, idx, want, cls, label):
    e = (_ws(model, what, idx, B, T) - want).abs().max().item()
    worst[cls] = max(worst[cls], e)
    assert e < ATOL_ACT, (name, math_mode, label, e)
  close(0, 0, inter['h'][0], 'h', 'H[0]')
  for b in range(ocfg.blocks):
    close(1, b, inter['z'][b], 'z', f'z[{b}]')
    close(2, b, inter['gate'][b], 'gate', f'sigmoid[{b}]')
    close(0, b + 1, inter['h'][b + 1], 'h', f'H[{b + 1}]')
  try:
    close(3, 0, inter['skip_sum'], 'head', 'skip sum')
    folded = False
  except ValueError:
    folded = True                    # never formed: its consumer, the first head activation, is compared below
  assert folded == (math_mode == 'split' and SPLIT_PATHS[name][1] == SKIP_FOLDED)
  for i, a in enumerate(inter['head_pre']):
    close(4, i, O.activation(a, ocfg.activation), 'head', f'head activation {i}')
  inp = _to_dev(x[:, :-1], cond)
  e_lg = (model.logits(inp).cpu().double() - inter['logits']).abs().max().item()
  assert e_lg < ATOL_ACT, (name, math_mode, 'logits', e_lg)
  out = model(inp)
  assert out.shape == ref.shape
  e_out = (out.cpu().double() - ref).abs().max().item()
  assert e_out < ATOL_ACT, (name, math_mode, 'model(x)', e_out)
  print(f'RECT fwd {name} [{math_mode}]: H {worst["h"]:.2e} z {worst["z"]:.2e} sigmoid {worst["gate"]:.2e} '
        f'skip/head {worst["head"]:.2e} logits {e_lg:.2e} output {e_out:.2e}')


@pytest.mark.parametrize('name', TWO)
def test_two_contraction_forward_is_another_kernel(name):
  """Split-precision and exact-fp32 mode on the same weights: not bit-equal, each within the bar of the other (both are within
  it of the oracle above) -- in the logits and already in the first block's gated activations."""
  B, T = 3, 333
  ocfg, params, x, cond, _, _ = _oracle_forward(name, 1, 3, B, T)
  _, _, model = make_pair(seed=1, **dict(CASES[name]))
  inp = _to_dev(x[:, :-1], cond)
  with model.exact_fp32():
    ref = model.logits(inp).clone()
    model.loss_and_grads(_to_dev(x, cond))
    z_ref = model.training_intermediate(1, 0, B, T).clone()
  out = model.logits(inp)
  model.loss_and_grads(_to_dev(x, cond))
  z = model.training_intermediate(1, 0, B, T)
  assert not torch.equal(out, ref) and not torch.equal(z, z_ref)
  assert (out - ref).abs().max().item() < ATOL_ACT and (z - z_ref).abs().max().item() < ATOL_ACT


# ------------------------------------------------------------------------------------------
# (c), (d) loss and every gradient: parameters, d loss / d u and d loss / d H of every block
# ------------------------------------------------------------------------------------------
GRAD_RUNS = [(n, 2, 150) for n in CASES] + [(n, B, T) for n in ALL_SIZES for B, T in ((3, 97), (1, 7))]


@pytest.mark.parametrize('name,B,T', GRAD_RUNS, ids=[f'{n}-{B}x{T}' for n, B, T in GRAD_RUNS])
def test_loss_and_every_gradient(name, B, T, math_mode):
  """(1, 7): shorter than dilation 8, and few enough tiles for the thin rows kernel in the backward products.  At (2, 150) the
  data gradients at u (a wrong [W_r | W_s] / [W_r | V] image shows here first) and at every block input (a wrong g_x image)
  are compared too; a wrong job of the table then shows in a parameter gradient alone."""
  kw = CASES[name]
  ocfg, params, x, cond, _, _ = _oracle_forward(name, 4, 8, B, T)
  _, _, model = make_pair(seed=4, **dict(kw))
  loss, _, _ = model.loss_and_grads(_to_dev(x, cond))
  torch.cuda.synchronize()
  branch = _head_branch(model, len(ocfg.final_layers_channels), B, T)
  loss_ref, grads_ref, g_u_ref, g_h_ref, n_kink, head_pre = _oracle_grads(name, 4, 8, B, T, branch)
  _check_kinks(head_pre, branch, n_kink)
  assert abs(loss[0].item() - loss_ref.item()) < 2e-5 * max(1.0, abs(loss_ref.item())), (loss[0].item(), loss_ref.item())
  worst = dict(u=0.0, h=0.0, p=('', 0.0))
  if (B, T) == (2, 150):
    for b in reversed(range(ocfg.blocks)):                 # in the order the chain forms them
      for what, cls, ref in ((8, 'u', g_u_ref[b]), (9, 'h', g_h_ref[b])):
        scale = ref.abs().max().item()
        e = (_ws(model, what, b, B, T) - ref).abs().max().item()
        worst[cls] = max(worst[cls], e / scale)
        assert e < 1e-4 * scale + 1e-7, (name, math_mode, f'd loss / d {cls}[{b}]', e, scale)
  names = model.variable_names
  assert len(names) == len(grads_ref)
  if 'conditioning' in kw:
    assert sum('conv_cond' in n for n in names) == 2 * ocfg.blocks and sum(n.startswith('mapping') for n in names) == 4
  for n, g, r in zip(names, model.gradients(), grads_ref):
    scale = max(r.abs().max().item(), 1e-6)
    e = (g.cpu().double() - r).abs().max().item()
    if e / scale > worst['p'][1]:
      worst['p'] = (n, e / scale)
    assert e < 1e-4 * scale + 1e-7, (name, math_mode, n, e, scale)
  print(f'RECT grad {name} {B}x{T} [{math_mode}]: loss {abs(loss[0].item() - loss_ref.item()):.2e} dL/du rel {worst["u"]:.2e} '
        f'dL/dH rel {worst["h"]:.2e} worst parameter gradient {worst["p"][0]} rel {worst["p"][1]:.2e} kinks {n_kink}')


# ------------------------------------------------------------------------------------------
# the running max-abs scales across a product that fell back to the exact-fp32 kernel
# ------------------------------------------------------------------------------------------
SMALL = 4096          # a power of two: scaling by it is exact
SCALE_CASES = ['r64_d32', 'r48_d64', 'r32_d64_sum', 'r32_d64_fold', 'r96', 'r64_d128']


def _small_gradient_errors(name, factor):
  """loss_and_grads of (2, 150) for a global batch `factor` times the local one: every gradient is the one of
  test_loss_and_every_gradient divided by `factor`.  Returns the worst error of d loss / d u, d loss / d H and the parameter
  gradients, each multiplied back by `factor` and relative to its reference tensor's scale (+ 1e-7, as the bar has it)."""
  B, T = 2, 150
  ocfg, params, x, cond, _, _ = _oracle_forward(name, 4, 8, B, T)
  _, _, model = make_pair(seed=4, **dict(CASES[name]))
  loss, _, _ = model.loss_and_grads(_to_dev(x, cond), global_batch=B * factor)
  torch.cuda.synchronize()
  branch = _head_branch(model, len(ocfg.final_layers_channels), B, T)
  loss_ref, grads_ref, g_u_ref, g_h_ref, n_kink, head_pre = _oracle_grads(name, 4, 8, B, T, branch)
  _check_kinks(head_pre, branch, n_kink)
  assert abs(loss[0].item() * factor - loss_ref.item()) < 2e-5 * max(1.0, abs(loss_ref.item()))
  out = {}

  def note(label, got, ref):
    scale = max(ref.abs().max().item(), 1e-6)
    e = (got * factor - ref).abs().max().item() / (1e-4 * scale + 1e-7)
    if e > out.get('worst', ('', 0.0))[1]:
      out['worst'] = (label, e)
  for b in reversed(range(ocfg.blocks)):
    note(f'd loss / d u[{b}]', _ws(model, 8, b, B, T), g_u_ref[b])
    note(f'd loss / d H[{b}]', _ws(model, 9, b, B, T), g_h_ref[b])
  for n, g, r in zip(model.variable_names, model.gradients(), grads_ref):
    note(n, g.cpu().double(), r)
  return out['worst']


@pytest.mark.parametrize('name', SCALE_CASES)
def test_small_gradients_keep_their_precision(name, math_mode):
  """A split-precision product scales its operand by the running max-abs its producer published (an exact power of two), so
  the backward pass is as accurate for gradients of 1e-7 as for gradients of 1e-3 -- provided every producer publishes.  In
  these nets one product of each block's pair runs on the exact-fp32 kernel inside an otherwise split-precision chain (the
  g_u product of 32 gated channels; the g_x product of 32 / 48 / 96 residual channels): what reads its result -- the next
  product, the jobs of the weight-gradient table -- must find a scale all the same.  Gradients of a global batch 4096 times
  the local one, multiplied back, meet the bar of test_loss_and_every_gradient against the same reference.  r64_d128, whose
  products are all split precision, is the control."""
  label, e = _small_gradient_errors(name, SMALL)
  print(f'RECT small {name} [{math_mode}]: worst {label} at {e:.2e} of the bar')
  assert e < 1.0, (name, math_mode, label, e)


# ------------------------------------------------------------------------------------------
# (e) three Adam steps with clipnorm active
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r64_d128', 'r32_d64_fold'])
def test_three_train_steps_match_oracle(name):
  from wavenets_amd import Adam
  kw = CASES[name]
  ocfg, params, model = make_pair(seed=6, **dict(kw))
  model.compile(optimizer=Adam(learning_rate=5e-4, clipnorm=1.0))
  x, _ = _inputs(kw, 2, 129, seed=1)
  p = [q.double() for q in params]
  m = [torch.zeros_like(q) for q in p]
  v = [torch.zeros_like(q) for q in p]
  for step in range(1, 4):
    loss_ref, p, m, v = O.train_step(x.double(), p, m, v, step, ocfg, lr=5e-4, clipnorm=1.0)
    logs = model.train_step(x.to(dev()))
    assert set(logs) == {'loss'}
  for n, got, ref in zip(model.variable_names, model.trainable_variables, p):
    assert (got.cpu().double() - ref).abs().max().item() < 2e-6 + 1e-4 * 5e-4 * 3, n
  assert model.optimizer.iterations == 3


# ------------------------------------------------------------------------------------------
# (f) dropout: the dropped copy is R wide, z is D wide; backward through g_xd -> the dropout kernel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r64_d128', 'r64_d32'])
def test_dropout_training_step(name, math_mode):
  from wavenets_amd import WaveNet
  kw = CASES[name]
  rate, seed = 0.25, 77
  ocfg = O.OracleConfig(**kw)
  params = O.init_params(ocfg, seed=4)
  model = WaveNet(**kw, dropout=rate, device=dev(), seed=seed)
  model.set_weights([p.numpy() for p in params])
  B, T = 2, 140
  x, _ = _inputs(kw, B, T + 1, seed=8)
  pd = [p.double() for p in params]
  for step in (1, 2):                     # the library pre-increments its step counter per call
    loss, _, _ = model.loss_and_grads(x.to(dev()))
    torch.cuda.synchronize()
    branch = _head_branch(model, len(ocfg.final_layers_channels), B, T)
    loss_ref, _, grads_ref, _ = O.loss_and_grads(x.double(), pd, ocfg, dropout=(rate, seed, step), head_branch=branch)
    with torch.no_grad():
      _, inter = O.model_forward(x[:, :-1].double(), pd, ocfg, return_intermediates=True, dropout=(rate, seed, step),
                                 head_branch=branch)
    _check_kinks(inter['head_pre'], branch, inter['kink_overrides'])
    # the dropped copy of every block input: R columns, exact (a mask and one multiplication)
    for b in range(ocfg.blocks):
      assert (_ws(model, 14, b, B, T) - inter['xd'][b]).abs().max().item() < ATOL_ACT, (name, step, b)
    assert abs(loss[0].item() - loss_ref.item()) < 2e-5 * max(1.0, abs(loss_ref.item()))
    for n, g, r in zip(model.variable_names, model.gradients(), grads_ref):
      scale = max(r.abs().max().item(), 1e-6)
      assert (g.cpu().double() - r).abs().max().item() < 1e-4 * scale + 1e-7, (n, step)
  # inference ignores dropout
  ref = O.model_forward(x[:, :-1].double(), pd, ocfg)
  assert (model(x[:, :-1].to(dev())).cpu().double() - ref).abs().max() < ATOL_ACT


# ------------------------------------------------------------------------------------------
# (g) generation: block by block on the ring taps == the sliding window, bit for bit
# ------------------------------------------------------------------------------------------
GEN = ['r64_d128', 'r128_d64', 'r64_k3', 'r32_d64_sum', 'r128_d64_mol']
N_GEN = 40


def _oracle_generation(ocfg, params, w, n):
  """The oracle's sliding window in fp64 and, per utterance (they are independent rows), the number of leading steps at which
  its top-2 margin exceeds the activation tolerance: a step that is not clear ends that utterance's comparison, since its
  later inputs may legitimately differ."""
  pd = [p.double() for p in params]
  xw = w.double().clone()
  ref, clear = [], []
  with torch.no_grad():
    for _ in range(n):
      pred = O.model_forward(xw, pd, ocfg)[:, -1:, :]
      smp = O.sample_waveform_deterministic(pred.float(), ocfg).double()
      top2 = torch.topk(pred, 2, dim=-1).values
      clear.append((top2[..., 0] - top2[..., 1])[:, 0] > 1e-4)
      ref.append(smp)
      xw = torch.cat([xw[:, 1:], smp], dim=1)
  clear = torch.stack(clear, dim=1)                      # (B, n)
  upto = [int((~c).nonzero()[0]) if bool((~c).any()) else n for c in clear]
  return torch.cat(ref, dim=1), upto


@pytest.mark.parametrize('name', GEN)
def test_queued_generation_equals_the_sliding_window(name):
  kw = CASES[name]
  ocfg, params, model = make_pair(seed=7, bias_range=0.3, **dict(kw))
  B = 3
  w = O.synthetic_waveform(B, model.receptive_field, seed=4)
  for ctl in (dict(deterministic=True), dict(deterministic=False, seed=7)):
    naive = model.generate(N_GEN, sample=w.to(dev()), use_queues=False, **ctl)
    queued = model.generate(N_GEN, sample=w.to(dev()), use_queues=True, **ctl)
    assert queued.shape == (B, N_GEN, 1)
    assert torch.equal(queued, naive), (name, ctl, (queued != naive).nonzero()[:4].tolist())
    assert model.generation_guard_trips == 0
    if ctl['deterministic'] and ocfg.sampling_function == 'categorical':
      ref, upto = _oracle_generation(ocfg, params, w, N_GEN)
      assert max(upto) == N_GEN, 'no utterance whose every decision is clear in the oracle: change the seed'
      got = naive.cpu().double()
      for b, n in enumerate(upto):
        assert torch.equal(got[b, :n], ref[b, :n]), (name, b, n)
      print(f'RECT gen {name}: steps clear in the oracle per utterance {upto} of {N_GEN}, all equal')


def test_queued_generation_second_utterance_tile_of_one_row():
  kw = CASES['r64_d128']
  ocfg, params, model = make_pair(seed=7, bias_range=0.3, **dict(kw))
  w = O.synthetic_waveform(33, model.receptive_field, seed=6).to(dev())
  naive = model.generate(N_GEN, sample=w, use_queues=False, deterministic=True)
  queued = model.generate(N_GEN, sample=w, use_queues=True, deterministic=True)
  assert torch.equal(naive, queued)
  few = model.generate(N_GEN, sample=w[:5], use_queues=True, deterministic=True)      # rows are independent
  assert torch.equal(few, queued[:5])


@pytest.mark.parametrize('ctl', [dict(deterministic=True), dict(deterministic=False, seed=7)], ids=['det', 'seed7'])
def test_generation_session_chunks_equal_the_one_shot_call(ctl):
  kw = CASES['r64_d128']
  ocfg, params, model = make_pair(seed=7, bias_range=0.3, **dict(kw))
  w = O.synthetic_waveform(3, model.receptive_field, seed=4).to(dev())
  args = dict(sample=w, use_queues=True, **ctl)
  one = model.generate(N_GEN, **args)
  s = model.generation_session(**args)
  got = torch.cat([s.generate(n) for n in (1, 3, 36)], dim=1)
  assert s.position == N_GEN and torch.equal(got, one)


# ------------------------------------------------------------------------------------------
# (h) standalone WaveNetLayer
# ------------------------------------------------------------------------------------------
LAYER_IDS = [f'{s[0]}_{s[1]}' for s in LAYER_SHAPES]


@pytest.mark.parametrize('R,D,S,dil,k,T', LAYER_SHAPES, ids=LAYER_IDS)
def test_layer_forward(R, D, S, dil, k, T, math_mode):
  layer, ps, dl = _layer_pair(R, D, S, dil, k)
  x = torch.randn(3, T, R, generator=torch.Generator().manual_seed(5)) * 0.7
  xo_ref, sk_ref = O.layer_forward(x.double(), [p.double() for p in ps], dilations=dl, activation_name=None, residual=True,
                                   has_skip=S is not None)
  with torch.no_grad():
    xo, sk = layer(x.to(dev()))
  assert xo.shape == (3, T, R) and sk.shape == (3, T, S or R)
  assert (xo.cpu().double() - xo_ref).abs().max() < ATOL_ACT
  assert (sk.cpu().double() - sk_ref).abs().max() < ATOL_ACT


@pytest.mark.parametrize('R,D,S,dil,k,T', LAYER_SHAPES, ids=LAYER_IDS)
def test_layer_backward(R, D, S, dil, k, T):
  layer, ps, dl = _layer_pair(R, D, S, dil, k)
  g = torch.Generator().manual_seed(11)
  x = torch.randn(2, T, R, generator=g) * 0.7
  gx = torch.randn(2, T, R, generator=g)
  gs = torch.randn(2, T, S or R, generator=g)
  xr = x.double().requires_grad_(True)
  pr = [p.double().requires_grad_(True) for p in ps]
  xo, sk = O.layer_forward(xr, pr, dilations=dl, activation_name=None, residual=True, has_skip=S is not None)
  ref = torch.autograd.grad((xo * gx.double()).sum() + (sk * gs.double()).sum(), [xr] + pr)
  xd = x.to(dev()).requires_grad_(True)
  xo_d, sk_d = layer(xd)
  ((xo_d * gx.to(dev())).sum() + (sk_d * gs.to(dev())).sum()).backward()
  assert _rel(xd.grad, ref[0]) < 2e-5
  got = layer.flat_params.grad.cpu()
  off = 0
  for r in ref[1:]:                                    # tensor by tensor, relative to each tensor's scale
    n = r.numel()
    assert _rel(got[off:off + n], r.reshape(-1)) < 5e-5, (off, tuple(r.shape))
    off += n
  assert off == got.numel()


@pytest.mark.parametrize('R,D,S,dil,k,T', LAYER_SHAPES[:2], ids=LAYER_IDS[:2])
def test_layer_generate_single_step(R, D, S, dil, k, T, math_mode):
  layer, ps, dl = _layer_pair(R, D, S, dil, k=k, seed=2)
  gathered = torch.randn(3, k, R, generator=torch.Generator().manual_seed(11)) * 0.8
  ref_x, ref_s = O.layer_generate(gathered.double(), [p.double() for p in ps], has_skip=True)
  with torch.no_grad():
    gx, gs = layer.generate(gathered.to(dev()))
  assert gx.shape == (3, 1, R) and gs.shape == (3, 1, S)
  assert (gx.cpu().double() - ref_x).abs().max() < ATOL_ACT
  assert (gs.cpu().double() - ref_s).abs().max() < ATOL_ACT
