"""wn_bwd_pair_kernel at every position a tile can have in a wave's walk, and at the extremes of its store descriptor.

The kernel's tile body exists in four copies: a wave's only tile, the first of several, a later tile
with a successor, the last tile.  The walk (wn_tile_walk, wn_common.h) picks the copy, so a shape decides which copies run
at all.  tests/test_gpu_bwd_tile_walk.py (5 x 27001: 2 or 3 tiles a wave) stays the yardstick; the shapes here are chosen
per copy, with the `r64_pair` network of that file (7 blocks, dilations 1 .. 64) in split mode:

  B = 1, T = 25      one ragged tile: the only-tile copy alone; every t + d with d >= 32 lies past the utterance's end
  B = 1, T = 95      three tiles, one a wave, a 31-row last tile
  B = 3, T = 22407   2103 tiles (701 an utterance, the last of 7 rows) on 256 workgroups: 55 waves take two tiles (first
                     and last copies), 1993 take one
  B = 3, T = 44001   4128 tiles (1376 an utterance, the last of ONE row: the shortest descriptor there is): 32 waves take
                     three tiles (the middle copy), 2016 take two

The device-free test restates wn_tile_walk and the launcher's grid on the host and asserts these counts, so that a change
of the walk cannot silently empty a copy.

Values: every GH[b] and GU[b] of one training pass over B different utterances against tests/bwd_restatement.py (each
product in float64 from the tensors its own kernel read) at the bar of DESIGN.md sections 5 and 18, max|got - ref| <=
1e-4 max|ref| per tensor.  The tile's rows leave through buffer stores on a descriptor that ends behind the last valid row;
the rows behind a ragged last tile belong to the next utterance, or, behind the last utterance, to the next tensor of the
workspace.  A row that was not dropped therefore overwrites the first rows of another utterance or of another tensor
(written by this launch's other waves or by ANOTHER launch of the chain) with the zeros of masked rows.  What catches it
is that the value checks run over all utterances and over every block's tensors -- GH[b + 1] and GU[b - 1] beside GH[b]
and GU[b] -- not over the ragged utterance alone.

Bitwise: for the two large shapes, three copies of one utterance against that utterance alone (one utterance is 701 or
1376 tiles: at most one tile a wave, and at T = 44001 the other branch of wn_tile_walk), torch.equal on every GH[b] and
GU[b].  Copies, because the operands are scaled by running max-abs over the whole tensor."""
import pytest
import torch

import bwd_restatement as R
from oracle import wavenet_oracle as O
from test_gpu_bwd_tile_walk import CASES, PAIR

gpu = pytest.mark.gpu

KW = CASES['r64_pair'][0]
SHAPES = [(1, 25), (1, 95), (3, 22407), (3, 44001)]
# waves that take 1, 2 and 3 tiles (worked out by hand in the docstring's terms, asserted against the restated walk)
WALK = {(1, 25): (1, 0, 0), (1, 95): (3, 0, 0), (3, 22407): (1993, 55, 0), (3, 44001): (0, 2016, 32),
        (1, 22407): (701, 0, 0), (1, 44001): (1376, 0, 0)}


def tiles_per_wave(b, t):
  """wn_launch_bwd_pair's grid and wn_tile_walk (wn_common.h), restated: how many tiles each wave of the launch takes."""
  ntiles = b * -(-t // 32)
  grid = min(256, -(-ntiles // 8))
  counts = []
  for block in range(grid):
    for wave in range(8):
      if grid % 8 == 0:
        n8 = (ntiles + 7) >> 3
        x = block & 7
        first, end, stride = x * n8 + (block >> 3) * 8 + wave, min((x + 1) * n8, ntiles), (grid >> 3) * 8
      else:
        first, end, stride = block * 8 + wave, ntiles, grid * 8
      counts.append(len(range(first, end, stride)))
  assert sum(counts) == ntiles
  return counts


@pytest.mark.parametrize('shape', sorted(WALK))
def test_how_many_waves_take_one_two_and_three_tiles(shape):
  counts = tiles_per_wave(*shape)
  assert max(counts) <= 3
  assert tuple(counts.count(n) for n in (1, 2, 3)) == WALK[shape]


def test_the_shapes_reach_every_copy_and_the_extremes_of_the_descriptor():
  assert 25 < 32 and 95 == 2 * 32 + 31 and 22407 == 700 * 32 + 7 and 44001 == 1375 * 32 + 1
  assert WALK[1, 25][0] == 1 and WALK[1, 95][0] == 3                    # the only-tile copy alone
  assert WALK[3, 22407][1] > 0 and WALK[3, 22407][2] == 0               # first and last copies, no middle one
  assert WALK[3, 44001][2] > 0                                          # the middle copy
  # the utterance alone: one tile a wave; 172 workgroups are no multiple of 8 (the other branch of the walk), 88 are
  assert -(-1376 // 8) % 8 != 0 and -(-701 // 8) % 8 == 0


def _dev():
  return torch.device('cuda', 0)


def _model():
  from wavenets_amd import WaveNet
  model = WaveNet(**KW, sampling_function='categorical', bits=8, device=_dev())
  g = torch.Generator().manual_seed(11)
  model.flat_params.copy_(((torch.rand(model.flat_params.numel(), generator=g) * 2 - 1) * 0.2).to(_dev()))
  assert PAIR in model.kernel_report(), model.kernel_report()
  return model, O.OracleConfig(**KW)


def _region(model, what, idx, b, t):
  return model.training_intermediate(what, idx, b, t).reshape(b, t, -1)


def _gh_gu(model, n, b, t):
  out = {('GU', i): _region(model, 8, i, b, t).clone() for i in range(n)}
  out.update({('GH', i): _region(model, 9, i, b, t).clone() for i in range(n + 1)})
  return out


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_gh_and_gu_against_the_fp64_restatement(shape):
  from wavenets_amd.data import synthetic_waveforms
  b, t = shape
  model, ocfg = _model()
  n, nf = ocfg.blocks, len(ocfg.final_layers_channels)
  x = synthetic_waveforms(b, t + 1, seed=5, device=_dev())
  loss, _, _ = model.loss_and_grads(x)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  got = {k: v.double() for k, v in _gh_gu(model, n, b, t).items()}
  ws = dict(got)
  for i in range(nf + 1):
    ws['GF', i] = _region(model, 6, i, b, t).double()
  for i in range(n + 1):
    ws['H', i] = _region(model, 0, i, b, t).double()
  for i in range(n):
    ws['Z', i] = _region(model, 1, i, b, t).double()
    ws['AG', i] = _region(model, 2, i, b, t).double()
  for i in range(nf):
    ws['HA', i] = _region(model, 4, i, b, t).double()
  for i in range(n):
    for k in (('GU', i), ('GH', i)):
      assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0.0, (shape, k)
  params = {name: p.double() for name, p in zip(model.variable_names, model.trainable_variables)}
  ref = R.restate(ocfg, params, x[:, :-1].double(), None, ws, True)
  failures = []
  worst = {'GH': 0.0, 'GU': 0.0}
  for k in got:
    if k == ('GH', n):
      continue                                   # zero under a skip head: nothing of the chain's
    r = ref[k]
    g = got[k].reshape(r.shape)
    scale = float(r.abs().max())
    diff = (g - r).abs()
    err = float(diff.max())
    worst[k[0]] = max(worst[k[0]], err / scale if scale > 0 else 0.0)
    if not err <= 1e-4 * scale:
      rows = diff.amax(dim=-1).reshape(-1)
      u, tt = divmod(int(rows.argmax()), t)
      failures.append(f'{k}: max|got - ref| {err:.3e} > {1e-4 * scale:.3e}; worst row: utterance {u}, t {tt} (tile {tt // 32}); '
                      f'rows over the bar: {int((rows > 1e-4 * scale).sum())}')
  print(f'{b} x {t}: worst max|err| / max|ref|  GH {worst["GH"]:.2e}  GU {worst["GU"]:.2e}')
  assert not failures, (shape, failures)


@gpu
@pytest.mark.parametrize('t', [22407, 44001])
def test_three_copies_of_one_utterance_equal_it_alone_bit_for_bit(t):
  from wavenets_amd.data import synthetic_waveforms
  b = 3
  model, ocfg = _model()
  n = ocfg.blocks
  x1 = synthetic_waveforms(1, t + 1, seed=5, device=_dev())
  xb = x1.expand(b, -1, -1).contiguous()
  loss, _, _ = model.loss_and_grads(xb, global_batch=b)
  torch.cuda.synchronize()
  assert float(loss[2]) == 0.0, 'range guard tripped'
  batch = _gh_gu(model, n, b, t)
  for k, v in batch.items():
    assert bool(torch.isfinite(v).all()), k
    if k != ('GH', n):
      assert float(v.abs().max()) > 0.0, k
  loss1, _, _ = model.loss_and_grads(x1, global_batch=b)       # the same 1 / global_batch: the same rows of dL/dlogits
  torch.cuda.synchronize()
  assert float(loss1[2]) == 0.0, 'range guard tripped'
  alone = _gh_gu(model, n, 1, t)

  def rows(a, c):
    return (a != c).any(dim=-1).nonzero()[:8].flatten().tolist()

  for k in batch:
    for u in range(1, b):
      assert torch.equal(batch[k][u], batch[k][0]), (t, k, f'utterance {u} of the batch != utterance 0', rows(batch[k][u], batch[k][0]))
    assert torch.equal(batch[k][0], alone[k][0]), (t, k, 'utterance 0 of the batch != the utterance alone', rows(batch[k][0], alone[k][0]))
