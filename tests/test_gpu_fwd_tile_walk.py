"""The fused block forward (wn_layer_fwd_f16_kernel) walks the 32-row tiles of a launch with persistent waves, and a
launch of more than 2048 tiles gives a wave a second and a third tile.  What a row gets must not depend on which wave
handled its tile, nor on whether the tile was the wave's first or a later one (wn_common.h: "Results do not depend on
the order of the tiles").

One training pass over 5 utterances of T = 27001 predicted samples is 5 x 844 = 4220 tiles on 256 workgroups of 8 waves:
the XCD-aware branch of wn_tile_walk, 2 or 3 tiles a wave, ragged last tiles (27001 mod 32 = 25) and waves whose next
tile belongs to the next utterance.  Each utterance alone is 844 tiles on 106 workgroups: the other branch of the walk,
at most one tile a wave.  Every tensor the blocks write -- H[b] (the last block's output included), Z, AG -- must be
equal bit for bit between the two."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 5, 27001

CASES = {
    # dilations 1 .. 64: the older tap lies in the same tile, in a neighbour tile or before the utterance's start
    'r64_k2': dict(blocks=7, dilation_bound=128, channels=64, skip_channels=256, kernel_size=2),
    # the same with a per-utterance conditioning bias (the FAST == 3 form of the kernel)
    'r64_k2_global': dict(blocks=7, dilation_bound=128, channels=64, skip_channels=256, kernel_size=2,
                          conditioning='global', mapping_layers=[6, 8]),
    'r32_k2': dict(blocks=4, channels=32, skip_channels=64, kernel_size=2),
    'r32_k3': dict(blocks=4, dilation_bound=81, channels=32, skip_channels=64, kernel_size=3),
}


def _dev():
  return torch.device('cuda', 0)


def _tensors(model, nblocks, b):
  """Clones of everything the block stack left in the training workspace, as (b, T, channels)."""
  out = {}
  for what, name, n in ((0, 'H', nblocks + 1), (1, 'Z', nblocks), (2, 'AG', nblocks)):
    for i in range(n):
      out[name, i] = model.training_intermediate(what, i, b, T).reshape(b, T, -1).clone()
  return out


@pytest.mark.parametrize('case', list(CASES))
def test_rows_do_not_depend_on_the_wave_or_the_position_of_their_tile(case):
  from wavenets_amd import WaveNet
  from wavenets_amd.data import synthetic_waveforms
  kw = dict(CASES[case])
  cond = None
  model = WaveNet(**kw, sampling_function='categorical', bits=8, final_layers_channels=[32], device=_dev())
  if kw.get('conditioning'):
    cond = torch.eye(B, device=_dev())               # a different one-hot condition per utterance
    model.build([(1, 8, 1), (1, B)])
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  x = synthetic_waveforms(B, T + 1, seed=5, device=_dev())
  nblocks = len(model.wavenet_blocks)

  loss, _, _ = model.loss_and_grads((x, cond) if cond is not None else x)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  batch = _tensors(model, nblocks, B)
  assert all(bool(torch.isfinite(v).all()) for v in batch.values())
  assert float(batch['H', nblocks].abs().max()) > 0.0

  for u in range(B):
    xu = x[u:u + 1].contiguous()
    loss_u, _, _ = model.loss_and_grads((xu, cond[u:u + 1]) if cond is not None else xu)
    torch.cuda.synchronize()
    assert float(loss_u[2]) == 0.0, 'range guard tripped'
    alone = _tensors(model, nblocks, 1)
    for key, v in alone.items():
      same = torch.equal(batch[key][u], v[0])
      assert same, (case, key, u, (batch[key][u] - v[0]).abs().max().item(),
                    (batch[key][u] != v[0]).any(dim=-1).nonzero()[:8].flatten().tolist())
