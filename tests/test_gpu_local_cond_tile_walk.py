"""Local conditioning where a wave of the fused block forward takes several tiles (the pattern of
tests/test_gpu_fwd_tile_walk.py).

5 utterances of T = 27008 = 844 x 32 inputs, hop = 64 (F = 422 random frames an utterance), the 64-channel network with a
mapping stack: one training pass is 4220 tiles on 256 workgroups of 8 waves, so a wave takes two or three tiles and the
bias request it rotates into the next tile (the FAST == 3 form) crosses frames and utterances.  Each utterance alone is 844
tiles, at most one a wave.  H, Z and AG of the batch must be bit for bit those of every utterance alone; and the conv_cond
gradients of the batch -- the frame-sum kernel over 5 x 422 condition rows -- the sum of the single runs' at the gradient bar."""
import pytest
import torch

from test_gpu_fwd_tile_walk import _dev

pytestmark = pytest.mark.gpu

B, T, HOP = 5, 27008, 64
F = T // HOP


def _tensors(model, nblocks, b):
  out = {}
  for what, name, n in ((0, 'H', nblocks + 1), (1, 'Z', nblocks), (2, 'AG', nblocks)):
    for i in range(n):
      out[name, i] = model.training_intermediate(what, i, b, T).reshape(b, T, -1).clone()
  return out


def test_frames_across_the_tiles_of_a_wave():
  from wavenets_amd import WaveNet
  from wavenets_amd.data import synthetic_waveforms
  model = WaveNet(blocks=7, dilation_bound=128, channels=64, skip_channels=256, kernel_size=2, conditioning='local',
                  mapping_layers=[6, 8], mapping_activation='tanh', sampling_function='categorical', bits=8,
                  final_layers_channels=[32], device=_dev())
  model.build([(1, 8, 1), (1, 2, 3)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())
  cond = (torch.rand(B, F, 3, generator=g) * 2 - 1).to(_dev())
  nblocks = len(model.wavenet_blocks)
  cc = [i for i, n in enumerate(model.variable_names) if 'conv_cond' in n or 'mapping' in n]
  assert len(cc) == 2 * nblocks + 4

  loss, _, _ = model.loss_and_grads((x, cond))
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  batch = _tensors(model, nblocks, B)
  batch_grads = [model.gradients()[i].clone() for i in cc]
  assert all(bool(torch.isfinite(v).all()) for v in batch.values())
  assert float(batch['Z', 0].abs().max()) > 0.0

  total = [torch.zeros_like(gr, dtype=torch.float64) for gr in batch_grads]
  for u in range(B):
    loss_u, _, _ = model.loss_and_grads((x[u:u + 1].contiguous(), cond[u:u + 1].contiguous()), global_batch=B, n_replicas=1)
    torch.cuda.synchronize()
    assert float(loss_u[2]) == 0.0, 'range guard tripped'
    alone = _tensors(model, nblocks, 1)
    for key, v in alone.items():
      same = torch.equal(batch[key][u], v[0])
      assert same, (key, u, (batch[key][u] - v[0]).abs().max().item(),
                    (batch[key][u] != v[0]).any(dim=-1).nonzero()[:8].flatten().tolist())
    for t, i in zip(total, cc):
      t += model.gradients()[i].double()
  for i, got, ref in zip(cc, batch_grads, total):
    scale = max(ref.abs().max().item(), 1e-6)
    err = (got.double() - ref).abs().max().item()
    assert err < 1e-4 * scale + 1e-7, (model.variable_names[i], err, scale)
