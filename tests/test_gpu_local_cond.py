"""Local conditioning on the device against tests/local_reference.py, the fp64 restatement.

B = 3, T = 192: F = 6 (hop 32: every 32-row tile has a frame of its own), F = 3 (hop 64), F = 2 (hop 96) and F = 1 (the
global model's call).  One network per kernel that adds the bias table to a block's pre-gate:
  r32, r32_1ch   wn_layer_fwd_f16_kernel<1, 1, 2> (FAST == 3 in training passes, the generic form in inference)
  r64_s256       wn_layer_fwd_f16_kernel<2, 2, 2, 3> in the training pass
  r128           wn_layer_fwd_s128_kernel
  r48            the composed path: the rows GEMM's row bias
  lpb2, k3       a stack of two convs in front of the gate; three taps
  mol            a logistic-mixture head
with and without mapping layers, with (B, F) and (B, F, 5) conditions.  Bars: those of tests/test_gpu_parity.py.
"""
import functools
import os

import numpy as np
import pytest
import torch

import local_reference as LR
from oracle import wavenet_oracle as O
from test_gpu_parity import ATOL_ACT, dev, math_mode  # noqa: F401  (math_mode: fixture)

pytestmark = pytest.mark.gpu

B, T = 3, 192
FRAMES = [6, 3, 2, 1]

NETS = {
    'r32': dict(blocks=4, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[32],
                activation='leaky_relu', mapping_layers=[8, 16], mapping_activation='leaky_relu', bits=8, cond_inputs=5),
    'r32_1ch': dict(blocks=3, channels=32, dilation_bound=8, final_layers_channels=[], bits=6, cond_inputs=1),
    'r64_s256': dict(blocks=4, channels=64, skip_channels=256, dilation_bound=8, final_layers_channels=[64],
                     activation='relu', mapping_layers=[16], mapping_activation='tanh', bits=8, cond_inputs=5),
    'r128': dict(blocks=3, channels=128, skip_channels=256, dilation_bound=4, final_layers_channels=[128],
                 activation='leaky_relu', mapping_layers=[32], mapping_activation='relu', bits=8, cond_inputs=1),
    'r48': dict(blocks=3, channels=48, skip_channels=64, dilation_bound=4, final_layers_channels=[32],
                activation='elu', bits=6, cond_inputs=5),
    'lpb2': dict(blocks=3, layers_per_block=2, channels=32, skip_channels=32, dilation_bound=8,
                 final_layers_channels=[32], activation='tanh', mapping_layers=[8], mapping_activation='tanh', bits=6,
                 cond_inputs=5),
    'k3': dict(blocks=4, kernel_size=3, channels=32, skip_channels=32, dilation_bound=9, final_layers_channels=[],
               bits=6, cond_inputs=5),
    'mol': dict(blocks=4, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[32],
                activation='leaky_relu', num_mixtures=10, sampling_function='logistic', bits=16, mapping_layers=[8],
                mapping_activation='sigmoid', cond_inputs=5),
}


def _cfg(name):
  return O.OracleConfig(**NETS[name], conditioning='local')


@functools.lru_cache(maxsize=None)
def _params(name):
  return tuple(p.double() for p in O.init_params(LR.global_cfg(_cfg(name)), seed=4))


def _weights(name, conditioning):
  """The parameter list as the model of that conditioning form takes it (local: mapping kernels (1, cin, w))."""
  names = [n for n, _ in O.param_shapes(LR.global_cfg(_cfg(name)))]
  return [(p.unsqueeze(0) if conditioning == 'local' and n.startswith('mapping') and n.endswith('kernel') else p).float().numpy()
          for n, p in zip(names, _params(name))]


def _model(name, conditioning='local'):
  from wavenets_amd import WaveNet
  kw = dict(NETS[name])
  cin = kw.pop('cond_inputs')
  m = WaveNet(**kw, conditioning=conditioning, device=dev())
  m.build([(1, 8, 1), (1, 2, cin) if conditioning == 'local' else (1, cin)])
  m.set_weights(_weights(name, conditioning))
  return m


@functools.lru_cache(maxsize=None)
def _data(name, F):
  """x (B, T + 1, 1) and the frames in the form the case's condition takes: (B, F) for one channel, else (B, F, 5)."""
  cin = NETS[name]['cond_inputs']
  x = O.synthetic_waveform(B, T + 1, seed=8)
  fr = torch.rand(B, F, cin, generator=torch.Generator().manual_seed(9 + F)) * 2 - 1
  return x, (fr[:, :, 0] if cin == 1 else fr)


@functools.lru_cache(maxsize=None)
def _ref_forward(name, F):
  x, fr = _data(name, F)
  up = LR.upsample(fr.double(), T // F)
  return (LR.local_forward(x[:, :-1].double(), list(_params(name)), _cfg(name), up),
          LR.local_forward(x[:, :-1].double(), list(_params(name)), _cfg(name), up, return_logits=True))


@functools.lru_cache(maxsize=None)
def _ref_grads(name, F):
  x, fr = _data(name, F)
  return LR.local_loss_and_grads(x.double(), list(_params(name)), _cfg(name), fr.double(), T // F)


@functools.lru_cache(maxsize=None)
def _ref_rows(name, F):
  x, fr = _data(name, F)
  with torch.no_grad():
    return LR.local_loss_rows(x.double(), list(_params(name)), _cfg(name), fr.double(), T // F)


def _assert_grads(names, got, ref, what):
  for n, g, r in zip(names, got, ref):
    scale = max(r.abs().max().item(), 1e-6)
    err = (g.detach().cpu().double().reshape(r.shape) - r).abs().max().item()
    assert err < 1e-4 * scale + 1e-7, (what, n, err, scale)


@pytest.mark.parametrize('F', FRAMES)
@pytest.mark.parametrize('name', list(NETS))
def test_forward_and_logits_parity(name, F, math_mode):
  model = _model(name)
  x, fr = _data(name, F)
  ref, ref_logits = _ref_forward(name, F)
  inp = (x[:, :-1].to(dev()), fr.to(dev()))
  out = model(inp)
  assert out.shape == ref.shape
  assert (out.cpu().double() - ref).abs().max() < ATOL_ACT
  assert (model.logits(inp).cpu().double() - ref_logits).abs().max() < ATOL_ACT
  assert f'conditioning=local F={F}' in model.kernel_report()


@pytest.mark.parametrize('F', FRAMES)
@pytest.mark.parametrize('name', list(NETS))
def test_loss_and_every_gradient(name, F, math_mode):
  """The training pass (the FAST == 3 form of the 32- and 64-channel kernel), the frame sums and the conditioning
  backward over B * F rows: conv_cond and the mapping tensors included."""
  model = _model(name)
  x, fr = _data(name, F)
  loss_ref, grads_ref, _ = _ref_grads(name, F)
  loss, _, _ = model.loss_and_grads((x.to(dev()), fr.to(dev())))
  assert loss[2].item() == 0
  assert abs(loss[0].item() - loss_ref.item()) < 2e-5 * max(1.0, abs(loss_ref.item()))
  names = model.variable_names
  assert any('conv_cond' in n for n in names) and (not NETS[name].get('mapping_layers') or any('mapping' in n for n in names))
  _assert_grads(names, model.gradients(), grads_ref, (name, F))
  # a repeat gives the same bits: the frame sums have a fixed order
  first = model.flat_grads.clone()
  model.loss_and_grads((x.to(dev()), fr.to(dev())))
  assert torch.equal(model.flat_grads, first)


@pytest.mark.parametrize('F', FRAMES)
@pytest.mark.parametrize('name', list(NETS))
def test_the_conditions_gradient_through_differentiable(name, F, math_mode):
  """cond.grad has the condition's own shape, (B, F) or (B, F, Cin), and is the restatement's."""
  model = _model(name)
  x, fr = _data(name, F)
  g = torch.randn(B, T, model.spec.out_channels, generator=torch.Generator().manual_seed(3)) * 0.1
  ps = [p.detach().clone().requires_grad_(True) for p in _params(name)]
  frr = fr.double().clone().requires_grad_(True)
  ref_out = LR.local_forward(x[:, :-1].double(), ps, _cfg(name), LR.upsample(frr, T // F), return_logits=True)
  # (with a skip head nothing reads the last block's residual output: its conv1 has no gradient, the library writes zeros)
  ref = torch.autograd.grad((ref_out * g.double()).sum(), ps + [frr], allow_unused=True)
  ref = [r if r is not None else torch.zeros_like(p) for r, p in zip(ref, ps + [frr])]
  cond = fr.to(dev()).requires_grad_(True)
  out = model.differentiable((x[:, :-1].to(dev()), cond), output='logits')
  (out * g.to(dev())).sum().backward()
  assert cond.grad.shape == fr.shape
  _assert_grads(['cond'], [cond.grad], [ref[-1]], (name, F))
  _assert_grads(model.variable_names, model.gradients(), ref[:-1], (name, F))


@pytest.mark.parametrize('name', ['r32', 'r64_s256', 'mol'])
def test_test_step_and_score_with_a_frame_weighted_out(name, math_mode):
  """sample_weight zeroes the whole second frame of every utterance.  A row is a loss: the loss bar, 2e-5 max(1, |row|), per
  row; the per-utterance sums and the step's loss at the same bar."""
  F, hop = 6, T // 6
  model = _model(name)
  x, fr = _data(name, F)
  w = torch.ones(B, T)
  w[:, hop:2 * hop] = 0
  rows_ref = _ref_rows(name, F) * w.double()
  data = (x.to(dev()), fr.to(dev()))
  sc = model.score(data, sample_weight=w.to(dev()), per_sample=True)
  row_err = (sc['rows'].cpu().double() - rows_ref).abs()
  row_bar = 2e-5 * rows_ref.abs().clamp(min=1.0)
  print(f'{name} {math_mode}: rows worst |err| {row_err.max().item():.3e}, worst err / bar {(row_err / row_bar).max().item():.3f}')
  assert bool((row_err <= row_bar).all()), (name, (row_err / row_bar).max().item())
  assert bool((sc['rows'][:, hop:2 * hop] == 0).all())
  nll_ref = rows_ref.sum(1)
  assert bool(((sc['nll'].cpu().double() - nll_ref).abs() < 2e-5 * nll_ref.abs().clamp(min=1.0)).all())
  assert sc['weight'].tolist() == [float(T - hop)] * B
  logs = model.test_step(data, sample_weight=w.to(dev()))
  loss_ref = float(rows_ref.sum()) / B
  assert abs(logs['loss'] - loss_ref) < 2e-5 * max(1.0, abs(loss_ref))


@pytest.mark.parametrize('name', list(NETS))
def test_one_frame_is_the_global_model_bit_for_bit(name, math_mode):
  local, glob = _model(name), _model(name, 'global')
  x, fr = _data(name, 1)
  g_cond = (fr if fr.dim() == 3 else fr[:, :, None])[:, 0, :]
  li, gi = (x[:, :-1].to(dev()), fr.to(dev())), (x[:, :-1].to(dev()), g_cond.to(dev()))
  assert torch.equal(local(li), glob(gi))
  assert torch.equal(local.logits(li), glob.logits(gi))
  ll, _, _ = local.loss_and_grads((x.to(dev()), fr.to(dev())))
  lg, _, _ = glob.loss_and_grads((x.to(dev()), g_cond.to(dev())))
  assert torch.equal(ll, lg)
  assert torch.equal(local.flat_grads, glob.flat_grads)


@pytest.mark.parametrize('name', list(NETS))
def test_equal_frames_are_the_global_model(name, math_mode):
  """F = 6 with the same row in every frame: every tile reads equal bias rows, so the forward pass is the global model's
  bit for bit; the gradients take another summation path (frame sums) and are held to the gradient bar."""
  local, glob = _model(name), _model(name, 'global')
  x, fr1 = _data(name, 1)
  fr = fr1.repeat_interleave(6, dim=1)
  g_cond = (fr1 if fr1.dim() == 3 else fr1[:, :, None])[:, 0, :]
  li, gi = (x[:, :-1].to(dev()), fr.to(dev())), (x[:, :-1].to(dev()), g_cond.to(dev()))
  assert torch.equal(local(li), glob(gi))
  assert torch.equal(local.logits(li), glob.logits(gi))
  ll, _, _ = local.loss_and_grads((x.to(dev()), fr.to(dev())))
  lg, _, _ = glob.loss_and_grads((x.to(dev()), g_cond.to(dev())))
  assert torch.equal(ll[:1], lg[:1])                     # the training pass's forward half, through the loss
  _assert_grads(local.variable_names, local.gradients(), [g.cpu().double() for g in glob.gradients()], name)


def test_a_global_call_behind_a_local_one_sees_no_frames():
  """Frames are armed per call and disarmed afterwards, also when the call raises."""
  model = _model('r32')
  x, fr = _data('r32', 6)
  model((x[:, :-1].to(dev()), fr.to(dev())))
  assert model._frames_armed == 0
  with pytest.raises(ValueError):
    model((x[:, :-2].to(dev()), fr.to(dev())))           # T = 191
  assert model._frames_armed == 0
  out1 = model((x[:, :-1].to(dev()), fr[:, :1].to(dev())))
  assert out1.shape == (B, T, 256)


def test_error_cases():
  model = _model('r32')
  x, _ = _data('r32', 6)
  xin = x[:, :-1].to(dev())
  c = lambda F: torch.zeros(B, F, 5, device=dev())
  with pytest.raises(ValueError, match=r'T = 192.*F = 5'):
    model((xin, c(5)))                                     # T % F
  with pytest.raises(ValueError, match=r'T = 192, F = 4 gives hop = 48'):
    model((xin, c(4)))                                     # hop % 32
  with pytest.raises(ValueError, match=r'T = 192, F = 4 gives hop = 48'):
    model.loss_and_grads((x.to(dev()), c(4)))
  with pytest.raises(ValueError, match='5 channels'):
    model((xin, torch.zeros(B, 6, 4, device=dev())))
  with pytest.raises(ValueError, match='frames'):
    model((xin, torch.zeros(B, 6, 5, 1, device=dev())))


@pytest.mark.parametrize('name', ['r32', 'r64_s256', 'r128', 'r48'])
def test_a_debug_region_behind_the_conditioning_is_that_of_the_pass(name):
  """The workspace regions carved behind the conditioning's move with F.  training_intermediate after a pass with F = 6
  must read dL/du where that pass wrote it: its sum over all rows is the gradient of the block's conv_cond bias."""
  model = _model(name)
  x, fr = _data(name, 6)
  model.loss_and_grads((x.to(dev()), fr.to(dev())))
  grads = dict(zip(model.variable_names, model.gradients()))
  for b in range(NETS[name]['blocks']):
    gu = model.training_intermediate(8, b, B, T).reshape(B * T, -1).double().sum(0).cpu()
    want = grads[f'block{b}/conv_cond/bias'].double().cpu()
    scale = max(want.abs().max().item(), 1e-6)
    assert (gu - want).abs().max().item() < 1e-4 * scale + 1e-7, (name, b)
  assert model._frames_armed == 0


@pytest.mark.parametrize('name', ['r64_s256', 'r128'])
def test_a_held_condition_generates_as_the_global_model(name):
  """One frame, (B, 1, Cin) or (B, 1): generate, a session in chunks and an admission with a (k, 1, Cin) condition are bit
  for bit the global model's with (B, Cin) / (k, Cin), stochastic draws included."""
  local, glob = _model(name), _model(name, 'global')
  _, fr = _data(name, 1)
  held = fr if fr.dim() == 3 else fr[:, :, None]
  rf = local.receptive_field
  w = (torch.rand(B, rf, 1, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev())
  kw = dict(sample=w, use_queues=True, seed=5)
  assert torch.equal(local.generate(12, condition=fr.to(dev()), **kw), glob.generate(12, condition=held[:, 0].to(dev()), **kw))
  skw = dict(sample=w, use_queues=True, seed=[5, 6, 7], stream=[0, 1, 2])
  sl = local.generation_session(condition=held.to(dev()), **skw)
  sg = glob.generation_session(condition=held[:, 0].to(dev()), **skw)
  assert torch.equal(sl.generate(5), sg.generate(5))
  nw = (torch.rand(1, rf, 1, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev())
  nc = torch.rand(1, 1, held.shape[2], generator=torch.Generator().manual_seed(4)).to(dev())
  assert torch.equal(sl.admit([1], nw, condition=nc, seed=[9], stream=[40]), sg.admit([1], nw, condition=nc[:, 0], seed=[9], stream=[40]))
  assert torch.equal(sl.generate(7), sg.generate(7))


@pytest.mark.parametrize('ext', ['npz', 'h5'])
def test_checkpoint_round_trip(ext, tmp_path):
  from wavenets_amd import io
  model = _model('r32')
  path = os.path.join(tmp_path, io.checkpoint_name(3, 0.001, ext))
  io.save_weights(model, path)
  other = _model('r32')
  other.set_weights([np.zeros_like(w) for w in other.get_weights()])
  io.load_weights(other, path)
  assert other.variable_names == model.variable_names
  for n, a, b_ in zip(model.variable_names, model.get_weights(), other.get_weights()):
    assert a.shape == b_.shape and np.array_equal(a, b_), n
  i = model.variable_names.index('mapping0/kernel')
  assert other.get_weights()[i].shape == (1, 5, 8)
  if ext == 'h5':
    assert io.keras_path('mapping1/kernel', local=True) == 'mapping/layers/conv1d_1/vars/0'
    assert io.keras_path('mapping1/kernel') == 'mapping/layers/dense_1/vars/0'
