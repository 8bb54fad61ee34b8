"""Custom losses through WaveNet.differentiable / wn_vjp: the backward pass from a gradient the
caller supplies, against the training step (bit for bit) and against fp64 torch.autograd on the CPU oracle (the project's
gradient bar, err < 1e-4 * max|ref| + 1e-7 per tensor).  Every test runs in both math modes."""
import contextlib
import functools

import pytest
import torch

from oracle import wavenet_oracle as O
from test_gpu_parity import ATOL_ACT, MODEL_CASES, _inputs, dev, make_pair, math_mode  # noqa: F401  (math_mode: fixture)

pytestmark = pytest.mark.gpu

B_, T_ = 2, 150


def _close(what, got, ref):
  """The bar of test_loss_and_gradients_parity, per tensor."""
  scale = max(ref.abs().max().item(), 1e-6)
  err = (got.detach().cpu().double() - ref).abs().max().item()
  print(f'{what}: err {err:.3e} scale {scale:.3e}')
  assert err < 1e-4 * scale + 1e-7, (what, err, scale)


def _n_hidden(kw):
  return len(kw['final_layers_channels'])           # index of the last head conv = of dL/dlogits among the head gradients


def _dlogits(model, kw, B, T):
  return model.training_intermediate(6, _n_hidden(kw), B, T).reshape(B, T, -1)


# ------------------------------------------------------------------------------------------
# 1. bit for bit against the training step
# ------------------------------------------------------------------------------------------
def _step_and_vjp(name, scope):
  """flat_grads of loss_and_grads(want_pred=True) and of differentiable('logits').backward(dL/dlogits of that step): the
  same backward on the same workspace contents.  scope(model): context of the two forward halves."""
  kw = dict(MODEL_CASES[name])
  _, _, model = make_pair(seed=4, **kw)
  x, cond = _inputs(kw, B_, T_ + 1, seed=8)
  xd = x.to(dev())
  cd = cond.to(dev()) if cond is not None else None
  with scope(model):
    loss, _, _ = model.loss_and_grads((xd, cd) if cd is not None else xd, want_pred=True)
  assert loss[2].item() == 0
  want = model.flat_grads.clone()
  g = _dlogits(model, kw, B_, T_).clone()
  assert g.abs().max().item() > 0
  model.flat_grads.zero_()
  with scope(model):
    out = model.differentiable((xd[:, :-1], cd) if cd is not None else xd[:, :-1], training=True, output='logits')
  assert out.grad_fn is not None and out.shape == g.shape
  out.backward(g)
  for n, o, t in zip(model.variable_names, model._offsets, model.gradients()):      # (names the region that differs)
    assert torch.equal(t.reshape(-1), want[o:o + t.numel()]), (n, (t.reshape(-1) - want[o:o + t.numel()]).abs().max().item())
  assert torch.equal(model.flat_grads, want)


@pytest.mark.parametrize('name', ['cat_small_fused', 'cat_r64', 'cat_r128', 'mol', 'cond', 'cat_lpb2_r64'])
def test_backward_from_the_steps_own_gradient_equals_the_step_bit_for_bit(name, math_mode):
  _step_and_vjp(name, lambda model: contextlib.nullcontext())


# ------------------------------------------------------------------------------------------
# 7. guarded path: backward re-enters the math mode of the forward pass
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cat_r64', 'mol'])
def test_backward_outside_exact_fp32_runs_in_the_mode_of_its_forward(name, math_mode):
  _step_and_vjp(name, lambda model: model.exact_fp32())


# ------------------------------------------------------------------------------------------
# 2. custom losses against fp64 autograd on the oracle
# ------------------------------------------------------------------------------------------
MASKED = 37          # frames at the end of utterance 1 that loss (a) masks out


def _loss_expected_sample(out, nxt, bits):
  """(a) on 'probs': squared error between the expected dequantised sample and the next input sample, frame-masked."""
  Bn, Tn, Cn = out.shape
  v = O.dequantize(torch.arange(Cn), bits).to(out.dtype).to(out.device)
  mask = torch.ones(Bn, Tn, dtype=out.dtype, device=out.device)
  mask[1, Tn - MASKED:] = 0
  e = (out * v).sum(-1)
  return (mask * (e - nxt.to(out.dtype).to(out.device)) ** 2).sum() / Bn


def _loss_smoothed_ce(out, nxt, bits):
  """(b) on 'logits': label-smoothed cross entropy (eps = 0.1) through log_softmax, per-utterance weights."""
  Bn = out.shape[0]
  eps = 0.1
  tgt = O.quantize(nxt, bits).to(out.device)
  logp = torch.log_softmax(out, dim=-1)
  nll = -logp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
  per = (1 - eps) * nll + eps * (-logp.mean(-1))
  w = torch.tensor([0.5, 2.0, 1.25][:Bn], dtype=out.dtype, device=out.device)
  return (w[:, None] * per).sum() / Bn


def _loss_mixture(out, nxt, bits):
  """(c) mixture heads: a smooth function of all three parameter groups, tanh(out) against a fixed random tensor."""
  r = torch.randn(out.shape, generator=torch.Generator().manual_seed(21)).to(out.dtype).to(out.device)
  return (torch.tanh(out) * r).sum() / out.shape[0]


LOSSES = {'expected_sample': (_loss_expected_sample, 'probs'), 'smoothed_ce': (_loss_smoothed_ce, 'logits'),
          'mixture': (_loss_mixture, 'probs')}
CAT_CASES = ['cat_small_fused', 'cat_r64', 'cat_r128', 'cat_odd_composed', 'cat_k3', 'cat_lpb2_k3_r32', 'cat_noskip_nores',
             'cond', 'cond_nomap']
LOSS_CASES = [(n, l) for n in CAT_CASES for l in ('expected_sample', 'smoothed_ce')] + [('mol', 'mixture'), ('gauss', 'mixture')]


def _case_data(kw, B, T, seed=8):
  x, cond = _inputs(kw, B, T + 1, seed=seed)
  return x[:, :-1].contiguous(), x[:, 1:, 0].contiguous(), cond


def _oracle_grads(ocfg, params, loss_fn, output, xin, nxt, cond, bits, dropout=None):
  ps = [p.double().clone().requires_grad_(True) for p in params]
  xr = xin.double().clone().requires_grad_(True)
  cr = cond.double().clone().requires_grad_(True) if cond is not None else None
  out = O.model_forward(xr, ps, ocfg, cr, return_logits=(output == 'logits'), dropout=dropout)
  loss = loss_fn(out, nxt, bits)
  leaves = ps + [xr] + ([cr] if cr is not None else [])
  gr = torch.autograd.grad(loss, leaves, allow_unused=True)
  gr = [g if g is not None else torch.zeros_like(l) for g, l in zip(gr, leaves)]
  n = len(ps)
  return loss.item(), gr[:n], gr[n], (gr[n + 1] if cr is not None else None), out.detach()


@functools.lru_cache(maxsize=None)
def _loss_reference(name, loss_name):
  """Computed once per case, shared by both math modes, never modified."""
  kw = dict(MODEL_CASES[name])
  okw = dict(kw)
  ocfg = O.OracleConfig(cond_inputs=okw.pop('cond_inputs', 0), **okw)
  params = O.init_params(ocfg, seed=4)                  # the weights make_pair(seed=4) gives the model
  xin, nxt, cond = _case_data(kw, B_, T_)
  fn, output = LOSSES[loss_name]
  return _oracle_grads(ocfg, params, fn, output, xin, nxt, cond, kw['bits'])


@pytest.mark.parametrize('name,loss_name', LOSS_CASES)
def test_custom_loss_gradients_match_fp64_autograd(name, loss_name, math_mode):
  kw = dict(MODEL_CASES[name])
  _, _, model = make_pair(seed=4, **kw)
  xin, nxt, cond = _case_data(kw, B_, T_)
  fn, output = LOSSES[loss_name]
  loss_ref, gp_ref, gx_ref, gc_ref, _ = _loss_reference(name, loss_name)
  xh = xin.to(dev()).requires_grad_(True)
  ch = cond.to(dev()).requires_grad_(True) if cond is not None else None
  out = model.differentiable((xh, ch) if ch is not None else xh, output=output)
  assert out.grad_fn is not None and out.requires_grad
  loss = fn(out, nxt, kw['bits'])
  print(f'loss {loss.item():.6f} (oracle {loss_ref:.6f})')
  loss.backward()
  for n, g, r in zip(model.variable_names, model.gradients(), gp_ref):
    _close(n, g, r)
  _close('x.grad', xh.grad, gx_ref)
  if cond is not None:
    _close('cond.grad', ch.grad, gc_ref)
  else:
    assert gc_ref is None
  assert model.flat_params.grad is None                 # the caller has not opted in
  if loss_name == 'expected_sample':
    # the masked frames contribute nothing: their rows of dL/dlogits are exactly zero
    dl = _dlogits(model, kw, B_, T_)
    assert torch.count_nonzero(dl[1, T_ - MASKED:]).item() == 0
    assert dl[1, :T_ - MASKED].abs().max().item() > 0 and dl[0, T_ - MASKED:].abs().max().item() > 0


# ------------------------------------------------------------------------------------------
# 3. the softmax vector-Jacobian product at its edges (blocks = 1)
# ------------------------------------------------------------------------------------------
def _one_block(bits):
  from wavenets_amd import WaveNet
  kw = dict(blocks=1, channels=32, skip_channels=32, dilation_bound=2, final_layers_channels=[32], bits=bits)
  model = WaveNet(**kw, device=dev())
  model.set_weights([p.numpy() for p in O.init_params(O.OracleConfig(**kw), seed=6, bias_range=0.5)])
  return kw, model


def _softmax_vjp_reference(q, g):
  q, g = q.double().cpu(), g.double().cpu()
  return q * (g - (g * q).sum(-1, keepdim=True))


@pytest.mark.parametrize('bits', [5, 8, 9])
def test_softmax_vjp_register_form_full_width_and_loop_form(bits, math_mode):
  """32, 256 and 512 classes; reference: fp64 q (g - <g, q>) from the probabilities the library returned; bar
  1e-6 * max|g| (fp32 row arithmetic over at most 512 terms).  Row (0, 0) carries a gradient that is constant over the
  classes: sum_j q_j = 1 leaves |dl| <= 1e-6 |g| there."""
  kw, model = _one_block(bits)
  B, T, C = 3, 150, 1 << bits
  x = O.synthetic_waveform(B, T, seed=12).to(dev())
  q = model.differentiable(x, output='probs')
  assert torch.equal(q.detach(), model(x))              # what call() returns, bit for bit
  g = torch.randn(B, T, C, generator=torch.Generator().manual_seed(bits)) * 3.0
  const = 3.7
  g[0, 0, :] = const
  q.backward(g.to(dev()))
  dl = _dlogits(model, kw, B, T).cpu().double()
  err = (dl - _softmax_vjp_reference(q.detach(), g)).abs().max().item()
  print(f'softmax vjp C = {C}: max err {err:.3e} (bar {1e-6 * g.abs().max().item():.3e}), constant row max |dl| '
        f'{dl[0, 0].abs().max().item():.3e}')
  assert err <= 1e-6 * g.abs().max().item()
  assert dl[0, 0].abs().max().item() <= 1e-6 * const
  # the published max-abs is that of the tensor
  am = model.training_intermediate(10, 0, B, T)[_n_hidden(kw)].item()
  assert am == dl.abs().max().item()


def test_softmax_vjp_rows_beyond_the_launched_waves_equal_their_twins(math_mode):
  """One utterance stacked twice, B * T = 8230 rows: more than the 4 * 2048 waves of the launch, so rows 8192.. are a
  wave's second row while their twins 4077.. of utterance 0 are first rows.  Same logits, same gradient: same bits."""
  kw, model = _one_block(5)
  T, C = 4115, 32
  one = O.synthetic_waveform(1, T, seed=12).to(dev())
  g1 = torch.randn(1, T, C, generator=torch.Generator().manual_seed(3)).to(dev())
  assert 2 * T > 4 * 2048
  q = model.differentiable(torch.cat([one, one], 0), output='probs')
  q.backward(torch.cat([g1, g1], 0))
  dl = _dlogits(model, kw, 2, T)
  assert dl.abs().max().item() > 0
  assert torch.equal(dl[1], dl[0])
  err = (dl.cpu().double() - _softmax_vjp_reference(q.detach(), torch.cat([g1, g1], 0))).abs().max().item()
  assert err <= 1e-6 * g1.abs().max().item()


# ------------------------------------------------------------------------------------------
# 4. the input conv's data gradient at its edges
# ------------------------------------------------------------------------------------------
def _inconv_net(R, KS):
  return dict(blocks=2, kernel_size=KS, channels=R, skip_channels=32, dilation_bound=KS, final_layers_channels=[], bits=5)


@functools.lru_cache(maxsize=None)
def _inconv_reference(R, KS, B, T, only):
  kw = _inconv_net(R, KS)
  ocfg = O.OracleConfig(**kw)
  params = O.init_params(ocfg, seed=9)
  x = O.synthetic_waveform(B, T, seed=5)
  g = torch.randn(B, T, 32, generator=torch.Generator().manual_seed(R + KS))
  if only is not None:
    keep = torch.zeros(B, 1, 1)
    keep[only] = 1
    g = g * keep
  xr = x.double().clone().requires_grad_(True)
  out = O.model_forward(xr, [p.double() for p in params], ocfg, return_logits=True)
  gx, = torch.autograd.grad((out * g.double()).sum(), [xr])
  return kw, params, x, g, gx


@pytest.mark.parametrize('R,KS,B,T', [(32, 3, 2, 1), (32, 3, 2, 2), (12, 2, 3, 50), (32, 3, 3, 50), (64, 2, 3, 50), (128, 3, 3, 50)])
def test_input_gradient_short_utterances_widths_and_no_mixing_of_utterances(R, KS, B, T, math_mode):
  """T = 1, 2 under three taps (every frame lacks taps); widths 12 (composed network), 32, 64, 128; with B = 3 the
  gradient sits in utterance 1 only and must leave g_x of utterances 0 and 2 exactly zero."""
  from wavenets_amd import WaveNet
  only = 1 if B == 3 else None
  kw, params, x, g, gx_ref = _inconv_reference(R, KS, B, T, only)
  model = WaveNet(**kw, device=dev())
  model.set_weights([p.numpy() for p in params])
  xh = x.to(dev()).requires_grad_(True)
  out = model.differentiable(xh, output='logits')
  out.backward(g.to(dev()))
  assert xh.grad.shape == (B, T, 1)
  _close('x.grad', xh.grad, gx_ref)
  if only is not None:
    assert gx_ref[only].abs().max().item() > 0
    assert torch.count_nonzero(xh.grad[0]).item() == 0 and torch.count_nonzero(xh.grad[2]).item() == 0


# ------------------------------------------------------------------------------------------
# 5. dropout
# ------------------------------------------------------------------------------------------
DROP_NET = dict(blocks=2, layers_per_block=2, channels=32, dilation_bound=4, activation='leaky_relu',
                final_layers_channels=[32], num_mixtures=4, sampling_function='gaussian', bits=16)
DROP_RATE, DROP_SEED = 0.1, 77


@functools.lru_cache(maxsize=None)
def _drop_reference(step):
  ocfg = O.OracleConfig(**DROP_NET)
  params = O.init_params(ocfg, seed=4)
  xin, nxt, _ = _case_data(DROP_NET, B_, T_)
  ref = _oracle_grads(ocfg, params, _loss_mixture, 'probs', xin, nxt, None, 16,
                      dropout=(DROP_RATE, DROP_SEED, step) if step else None)
  return params, xin, nxt, ref


def test_dropout_mask_of_the_pass_in_forward_and_backward(math_mode):
  """The reference's default network shape, shrunk (2 x 2 stacked convs, 32 channels, gaussian-4), dropout 0.1:
  training=True draws the masks of training calls 1 and 2 (restated hash, as test_dropout_training_step_parity);
  training=False is the network without dropout."""
  from wavenets_amd import WaveNet
  params, xin, nxt, _ = _drop_reference(0)
  model = WaveNet(**DROP_NET, dropout=DROP_RATE, device=dev(), seed=DROP_SEED)
  model.set_weights([p.numpy() for p in params])
  for step, training in ((1, True), (0, False), (2, True)):
    _, _, _, (loss_ref, gp_ref, gx_ref, _, out_ref) = _drop_reference(step)
    xh = xin.to(dev()).requires_grad_(True)
    out = model.differentiable(xh, training=training)
    assert (out.detach().cpu().double() - out_ref).abs().max().item() < ATOL_ACT      # the forward-parity bar
    loss = _loss_mixture(out, nxt, 16)
    loss.backward()
    for n, g, r in zip(model.variable_names, model.gradients(), gp_ref):
      _close(f'{n} (step {step})', g, r)
    _close(f'x.grad (step {step})', xh.grad, gx_ref)
  assert (_drop_reference(1)[3][4] - _drop_reference(0)[3][4]).abs().max().item() > 1e-4      # the mask does something
  # the training step that follows draws mask 3 on a workspace laid out for dropout
  loss_ref, _, _, _ = O.loss_and_grads(torch.cat([xin, xin[:, :1]], 1).double(), [p.double() for p in params],
                                       O.OracleConfig(**DROP_NET), dropout=(DROP_RATE, DROP_SEED, 3))
  loss, _, _ = model.loss_and_grads(torch.cat([xin, xin[:, :1]], 1).to(dev()))
  assert abs(loss[0].item() - loss_ref.item()) < 2e-5 * max(1.0, abs(loss_ref.item()))


# ------------------------------------------------------------------------------------------
# 6. surface
# ------------------------------------------------------------------------------------------
def _surface_model(**extra):
  from wavenets_amd import WaveNet
  from wavenets_amd.optim import Adam
  kw = dict(MODEL_CASES['cat_small_fused'])
  model = WaveNet(**kw, device=dev())
  model.set_weights([p.numpy() for p in O.init_params(O.OracleConfig(**kw), seed=4)])
  model.compile(optimizer=Adam(learning_rate=1e-3, **extra))
  x = O.synthetic_waveform(B_, T_ + 1, seed=8).to(dev())
  return kw, model, x


def test_surface_errors_name_their_cause(math_mode):
  kw, model, x = _surface_model(use_ema=True)
  with pytest.raises(ValueError, match='output'):
    model.differentiable(x[:, :-1], output='log_probs')
  # a training step between forward and backward
  out = model.differentiable(x[:, :-1], output='logits')
  model.loss_and_grads(x)
  with pytest.raises(RuntimeError, match='workspace'):
    out.sum().backward()
  # another differentiable
  out = model.differentiable(x[:, :-1], output='logits')
  out2 = model.differentiable(x[:, :-1], output='logits')
  with pytest.raises(RuntimeError, match='workspace'):
    out.sum().backward()
  # a second backward on the same graph
  out2.sum().backward(retain_graph=True)
  with pytest.raises(RuntimeError, match='already'):
    out2.sum().backward()
  # a weight change between forward and backward
  out = model.differentiable(x[:, :-1], output='logits')
  model.optimizer.apply_gradients(model)
  with pytest.raises(RuntimeError, match='weights changed'):
    out.sum().backward()
  # second derivatives are refused, not returned without a graph
  xh = x[:, :-1].clone().requires_grad_(True)
  gx, = torch.autograd.grad(model.differentiable(xh, output='logits').sum(), xh, create_graph=True)
  assert gx.shape == xh.shape and not gx.requires_grad
  with pytest.raises(RuntimeError):
    gx.sum().backward()
  # inside averaged_weights()
  model.train_step(x)
  with model.averaged_weights():
    with pytest.raises(RuntimeError, match='averaged_weights'):
      model.differentiable(x[:, :-1])
  # call() is still outside autograd
  p = model(x[:, :-1])
  assert p.requires_grad is False and p.grad_fn is None


def test_optimizer_step_and_parameter_grad_opt_in(math_mode):
  kw, model, x = _surface_model()
  tgt = O.quantize(x[:, 1:, 0].cpu(), kw['bits']).to(dev())

  def step_loss():
    out = model.differentiable(x[:, :-1], output='logits')
    return torch.nn.functional.cross_entropy(out.reshape(-1, out.shape[-1]), tgt.reshape(-1), reduction='sum') / B_
  before = model.flat_params.detach().clone()
  loss0 = step_loss()
  loss0.backward()
  assert model.flat_params.grad is None                 # default: flat_grads only
  assert model.flat_grads.abs().max().item() > 0
  model.optimizer.apply_gradients(model)
  assert not torch.equal(model.flat_params.detach(), before)
  assert step_loss().item() < loss0.item()              # and the step went downhill
  model.flat_params.requires_grad_(True)
  try:
    step_loss().backward()
    assert model.flat_params.grad is not None and torch.equal(model.flat_params.grad, model.flat_grads)
    assert model.flat_params.grad.data_ptr() != model.flat_grads.data_ptr()
  finally:
    model.flat_params.requires_grad_(False)
    model.flat_params.grad = None
