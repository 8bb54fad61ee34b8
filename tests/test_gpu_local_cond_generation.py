"""Local conditioning in queued generation: a frame schedule is the condition table of the session's
workspace rewritten at every frame boundary, between two chunks (wn_generate_set_condition); the step kernels are the
global model's.  A 64-channel network (the chain kernels) and a 128-channel one (the relay), categorical heads of 64
classes, B = 3, F = 3 frames.  The cases and the fp64 side are tests/local_reference.py's."""
import pytest
import torch

import local_reference as LR
from oracle import wavenet_oracle as O
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

B, F = LR.GEN_B, LR.GEN_F


def _model(name, conditioning='local'):
  from wavenets_amd import WaveNet
  kw = dict(LR.GEN_NETS[name])
  cin = kw.pop('cond_inputs')
  m = WaveNet(**kw, conditioning=conditioning, device=dev())
  m.build([(1, 8, 1), (1, 2, cin) if conditioning == 'local' else (1, cin)])
  names = [n for n, _ in O.param_shapes(LR.global_cfg(LR.gen_cfg(name)))]
  m.set_weights([(p.unsqueeze(0) if conditioning == 'local' and n.startswith('mapping') and n.endswith('kernel') else p).float().numpy()
                 for n, p in zip(names, LR.gen_params(name))])
  return m


def _inputs(name, hop):
  w, fr = LR.gen_inputs(name, hop)
  return w.to(dev()), fr.to(dev())


@pytest.mark.parametrize('name', list(LR.GEN_NETS))
def test_equal_frames_are_the_global_generate(name):
  """All frames equal: bit for bit the global model's generate, stochastic draws included."""
  local, glob = _model(name), _model(name, 'global')
  w, fr = _inputs(name, 5)
  same = fr[:, :1].repeat(1, F, 1)
  kw = dict(sample=w, use_queues=True, seed=5)
  got = local.generate(F * 5, condition=same, hop=5, **kw)
  assert got.shape == (B, F * 5, 1)
  assert torch.equal(got, glob.generate(F * 5, condition=same[:, 0], **kw))


@pytest.mark.parametrize('hop', [5, 32])
@pytest.mark.parametrize('name', list(LR.GEN_NETS))
def test_one_call_is_the_sessions_chunks_and_a_global_session_driven_by_hand(name, hop):
  local, glob = _model(name), _model(name, 'global')
  w, fr = _inputs(name, hop)
  total = F * hop
  kw = dict(sample=w, use_queues=True, seed=7)
  one = local.generate(total, condition=fr, hop=hop, **kw)
  assert not torch.equal(one, local.generate(total, condition=fr[:, :1].repeat(1, F, 1), hop=hop, **kw))   # the frames matter
  s = local.generation_session(condition=fr, hop=hop, **kw)
  sizes, left, k = [], total, 0
  while left > 0:                                         # 3, 7, 4, 11, ...: no size divides hop = 5 or 32
    sizes.append(min((3, 7, 4, 11, 2, 13, 6)[k % 7], left))
    left -= sizes[-1]
    k += 1
  pieces = torch.cat([s.generate(n) for n in sizes], 1)
  assert s.position == total and torch.equal(pieces, one), (pieces != one).nonzero()[:4].tolist()
  with pytest.raises(ValueError, match='run past'):
    s.generate(1)
  # the global model, its condition rewritten by hand at every frame boundary
  sg = glob.generation_session(condition=fr[:, 0].contiguous(), **kw)
  hand = []
  for f in range(F):
    if f > 0:
      sg.set_condition(fr[:, f])
    hand.append(sg.generate(hop))
  assert torch.equal(torch.cat(hand, 1), one)


@pytest.mark.parametrize('hop', [5, 32])
@pytest.mark.parametrize('name', list(LR.GEN_NETS))
def test_every_clear_step_is_the_fp64_arg_max(name, hop):
  """deterministic=True: the device's own output, teacher-forced through the restatement with the per-sample condition of
  the rule (frame 0 over the window, frame g // hop at the step that emits sample g).  Wherever the fp64 top-2 margin
  exceeds 1e-4 the emitted class is the fp64 arg max; at most 2 % of the steps may be closer than that (the restatement's
  own rollout is pinned to that in tests/test_local_cond_cpu.py)."""
  local = _model(name)
  w, fr = _inputs(name, hop)
  out = local.generate(F * hop, condition=fr, hop=hop, sample=w, use_queues=True, deterministic=True)
  probs = LR.teacher_forced_probs(name, w.cpu(), out.cpu(), fr.cpu(), hop)
  top = torch.topk(probs, 2, dim=-1).values
  clear = (top[..., 0] - top[..., 1]) > 1e-4
  assert float((~clear).double().mean()) <= 0.02
  want = O.dequantize(probs.argmax(-1), 6).float()
  assert torch.equal(out.cpu()[..., 0][clear], want[clear]), ((out.cpu()[..., 0] != want) & clear).nonzero()[:4].tolist()


@pytest.mark.parametrize('name', list(LR.GEN_NETS))
def test_an_admission_leaves_the_other_rows_alone(name):
  """A held-condition admit into a session on a frame schedule: rows 0 and 2 keep their bits across the later frame
  boundaries; row 1 leaves the schedule and follows set_condition."""
  local = _model(name)
  hop = 5
  w, fr = _inputs(name, hop)
  kw = dict(sample=w, use_queues=True, seed=[5, 6, 7], stream=[0, 1, 2], condition=fr, hop=hop)
  base = local.generation_session(**kw).generate(F * hop)
  s = local.generation_session(**kw)
  a = s.generate(7)
  nw = (torch.rand(1, w.shape[1], 1, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev())
  nc = torch.rand(1, 1, fr.shape[2], generator=torch.Generator().manual_seed(4)).to(dev())
  s.admit([1], nw, condition=nc, seed=[9], stream=[40])
  b = s.generate(4)                                       # crosses the boundary at 10
  s.set_condition(nc[:, 0] * 0.5, slots=[1])
  c = s.generate(F * hop - 11)
  got = torch.cat([a, b, c], 1)
  for r in (0, 2):
    assert torch.equal(got[r], base[r]), r
  assert torch.equal(got[1, :7], base[1, :7]) and not torch.equal(got[1, 7:], base[1, 7:])


def test_error_cases():
  local = _model('r64')
  w, fr = _inputs('r64', 5)
  kw = dict(sample=w, condition=fr)
  with pytest.raises(ValueError, match='hop is required'):
    local.generate(10, use_queues=True, **kw)
  with pytest.raises(ValueError, match='run'):
    local.generate(F * 5 + 1, use_queues=True, hop=5, **kw)
  with pytest.raises(NotImplementedError, match='use_queues=True'):
    local.generate(10, use_queues=False, hop=5, **kw)
  held = local.generate(40, sample=w, condition=fr[:, :1], use_queues=True, deterministic=True)     # one frame, no hop: no end
  assert held.shape == (B, 40, 1)
