"""Every supported activation on the 64- and 128-channel kernels, and the gate and head non-linearities at saturation
(DESIGN.md section 30).

Before this file the GPU suite ran the planes, taps, rows16 and generation kernels of 64- and 128-channel nets with
`leaky_relu` or no activation only; relu, tanh and elu met 12- and 32-channel nets on the composed and fp32 rows kernels,
sigmoid met none, and `mapping_activation` was leaky_relu or None.  The run-time-activation instantiations
wn_gemm_planes16s_kernel<2,4,-1>, <1,8,-1> and <2,2,-1,true>, their backward forms with wn_dact_from_y, the per-layer
activation of wn_gen_head_kernel, the skip_act of the folded skip contraction in the generation chains and the mapping
network's act'(M) had never run under a test.  Every test initialised with Glorot weights, so no non-linearity ever left the
neighbourhood of zero.

  A  a training pass of six nets x {relu, tanh, sigmoid, elu} against the fp64 oracle, both math modes: logits, every block
     input, every head (and inner) activation, the loss, every parameter gradient, at the bars of DESIGN.md section 5
  B  queued generation == sliding window, bit for bit, for every activation on every generation form; the sliding window's
     first samples against the oracle
  C  A on weights that saturate the gate (pre-activations at +-50, +-100, a fifth beyond |u| > 9) and the head, plus dL/du
     and finiteness of everything the pass wrote; B on the saturated tanh nets
  D  the standalone WaveNetLayer at 64 channels with a stack of two convs, for the four activations

Cases, weights, data and the fp64 oracle come from tests/test_activation_cases_cpu.py, which pins on the CPU that the inputs
saturate what this file claims, that the bars are reachable on them and which kernel family every net takes.
"""
import functools

import pytest
import torch

import test_activation_cases_cpu as AC
import test_gpu_head_tile_walk as HW
import test_gpu_layer_backward as LB
from oracle import wavenet_oracle as O
from test_gpu_parity import ATOL_ACT, dev, make_pair

pytestmark = pytest.mark.gpu

B, T = AC.B, AC.T
SENTINEL = 12345.0
KINKED = ('relu', 'leaky_relu')


@pytest.fixture(params=['split', 'fp32'])
def math_mode(request):
  """Both contraction modes (as in tests/test_gpu_parity.py): 'split' = fp16 hi/lo 3-product MFMA, 'fp32' = exact-fp32 MFMA."""
  from wavenets_amd import _lib
  _lib.lib().wn_debug_set(1, 1 if request.param == 'fp32' else 0)
  yield request.param
  _lib.lib().wn_debug_set(1, 0)


def _model(c):
  """The HIP model of a case: make_pair's weights, which are the case's own; the saturated ones are set on top."""
  ocfg, params, model = make_pair(seed=AC.WEIGHT_SEED, bias_range=AC.BIAS_RANGE, **c.kw)
  assert model.variable_names == c.names
  if c.sat:
    model.set_weights([p.numpy() for p in c.params])
  else:
    assert all(torch.equal(a, b) for a, b in zip(params, c.params))
  return model


def _pack(x, cond):
  return (x.to(dev()), cond.to(dev())) if cond is not None else x.to(dev())


class Figures:
  """Collects error / bar of every compared tensor, prints the worst per family, then fails on all that miss at once."""

  def __init__(self, tag):
    self.tag, self.worst, self.bad = tag, {}, []

  def check(self, family, name, got, ref, bar):
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
      self.bad.append(f'{name}: not finite')
      return
    err = (got - ref).abs().max().item()
    if err / bar >= self.worst.get(family, (0.0, ''))[0]:
      self.worst[family] = (err / bar, name)
    if not err <= bar:
      self.bad.append(f'{name}: max|got - ref| {err:.3e} against a bar of {bar:.3e} (max|ref| {ref.abs().max().item():.3e})')

  def finish(self):
    for fam, (r, name) in sorted(self.worst.items()):
      print(f'FIG {self.tag} {fam}: worst err / bar {r:.3f} at {name}')
    assert not self.bad, f'{self.tag}:\n  ' + '\n  '.join(self.bad)


def _training_pass(net, act, sat, math_mode):
  """Tests A and C: one loss_and_grads call against the fp64 oracle.  Returns (model, figures, case, oracle evaluation)."""
  from wavenets_amd import _lib
  c, ev = AC.case(net, act, sat), AC.oracle(net, act, sat)
  ocfg = c.ocfg
  model = _model(c)
  fig = Figures(f'{net} {act} {"saturated " if sat else ""}[{math_mode}]')
  lg = model.logits(_pack(c.x[:, :-1], c.cond))
  assert not model.range_tripped_last_forward()
  fig.check('logits', 'logits', lg, ev.logits, ATOL_ACT)
  # the training pass, with the logits region holding a sentinel: a pass that fused the loss into the last conv leaves it alone
  model._workspace('train', _lib.lib().wn_plan_workspace_floats(model._plan, B, T, 1))        # as loss_and_grads allocates it
  model.training_intermediate(5, 0, B, T).fill_(SENTINEL)
  loss, _, _ = model.loss_and_grads(_pack(c.x, c.cond))
  torch.cuda.synchronize()
  assert loss[2].item() == 0, 'range guard tripped'
  region = model.training_intermediate(5, 0, B, T)
  fused = bool((region == SENTINEL).all())
  assert fused or not bool((region == SENTINEL).any())
  assert fused == (math_mode == 'split' and HW.route(HW._full(c.kw))[-1].startswith('epilogue')), (net, act, math_mode, fused)

  def ws(what, idx, shape):
    return model.training_intermediate(what, idx, B, T).cpu().double().reshape(shape)

  for b, h in enumerate(ev.h):
    fig.check('block inputs', f'H[{b}]', ws(0, b, h.shape), h, ATOL_ACT)
  head = [ws(4, i, a.shape) for i, a in enumerate(ev.head_pre)]
  for i, (ha, ref) in enumerate(zip(head, ev.head_act)):
    fig.check('head activations', f'head activation {i}', ha, ref, ATOL_ACT)
  inner = [[ws(11, b * len(blk) + i, a.shape) for i, a in enumerate(blk)] for b, blk in enumerate(ev.inner_act)]
  for b, blk in enumerate(ev.inner_act):
    for i, ref in enumerate(blk):
      fig.check('inner activations', f'inner activation {b}.{i}', inner[b][i], ref, ATOL_ACT)
  # relu / leaky_relu: the derivative jumps at 0.  Where the ORACLE's own pre-activation lies within KINK_TOL of 0 it takes the
  # side the product took (O.activation_with_branch); every disagreement must lie inside that band and be one the oracle
  # resolved, and there are at most as many as the oracle has elements in the band (capped on the CPU at 5e-4 of them)
  overrides = 0
  if ocfg.activation in KINKED:
    side = (lambda y: y >= 0) if ocfg.activation == 'leaky_relu' else (lambda y: y > 0)
    own = (lambda a: a >= 0) if ocfg.activation == 'leaky_relu' else (lambda a: a > 0)
    head_branch = [side(y) for y in head]
    inner_branch = [[side(y) for y in blk] for blk in inner]
    pairs = list(zip(ev.head_pre, head_branch)) + [(a, br) for pa, pb in zip(ev.inner_pre, inner_branch) for a, br in zip(pa, pb)]
    worst_over = 0.0
    for a, br in pairs:
      over = own(a) != br
      overrides += int(over.sum())
      if over.any():
        worst_over = max(worst_over, a[over].abs().max().item())
    assert worst_over < O.KINK_TOL, (net, act, math_mode, worst_over)
    near, total = AC.near_kink(ev, ocfg.activation)
    assert overrides <= near <= AC.KINK_SHARE * total, (overrides, near, total)
    if overrides:
      ev = AC.evaluate(c, head_branch=head_branch, inner_branch=inner_branch if any(inner_branch) else None)
      assert ev.kink_overrides + sum(k[2] for k in ev.kink_log) == overrides, (ev.kink_overrides, ev.kink_log, overrides)
      assert all(cnt == nov and worst < O.KINK_TOL for cnt, worst, nov in ev.kink_log)
    print(f'FIG {fig.tag} kink decisions taken from the product: {overrides} (oracle elements in the band: {near} of {total})')
  fig.check('loss', 'loss', loss[0], ev.loss, 2e-5 * max(1.0, abs(ev.loss.item())))
  for n, g, r in zip(model.variable_names, model.gradients(), ev.grads):
    fam = 'mapping gradients' if n.startswith('mapping') else 'parameter gradients'
    fig.check(fam, n, g, r, AC.grad_bar(r))
  return model, fig, c, ev


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize('net,act', AC.a_pairs())
def test_training_pass_against_the_fp64_oracle(net, act, math_mode):
  model, fig, c, ev = _training_pass(net, act, False, math_mode)
  fig.finish()


# ------------------------------------------------------------------------------------------ B
# id: net, utterances, 128-channel form
GEN_CASES = {
    'r64_head256_b3': ('r64_head256', 3, None),          # the head's tail inside the head launch
    'r64_head256_b9': ('r64_head256', 9, None),          # past it
    'r128_relay': ('r128', 3, 'relay'),                  # wn_gen_relay128_kernel
    'r128_one_workgroup': ('r128', 3, 'one_workgroup'),  # wn_gen_chain128_kernel (knob 2)
    'r32_f128_b3': ('r32_f128', 3, None),
    'mol_r64_b5': ('mol_r64', 5, None),                  # GEN_HEAD_MIX
    'cond_r64_b3': ('cond_r64', 3, None),
}
N_GEN = 20
# seed of the initial windows: the first of 8, 9, ... at which all six decisions of the fp64 oracle on r64_head256 are clear
# for all four activations (chosen from the oracle alone: the tanh and elu heads are nearly flat at Glorot scale, and at
# most seeds one of their 3 x 6 top-2 margins is under 1e-4, which ends the comparison at that step)
GEN_SEED = 28


def _gen_inputs(c, model, Bg):
  w = O.synthetic_waveform(Bg, model.receptive_field, seed=GEN_SEED)
  cond = None
  if c.cond is not None:
    cond = torch.rand(Bg, c.cond.shape[1], generator=torch.Generator().manual_seed(AC.DATA_SEED))
  return w, cond


def _both_generation_paths(c, model, Bg, form, det):
  from wavenets_amd import _lib
  w, cond = _gen_inputs(c, model, Bg)
  args = dict(sample=w.to(dev()), deterministic=det)
  if cond is not None:
    args['condition'] = cond.to(dev())
  naive = model.generate(N_GEN, use_queues=False, **args)
  _lib.lib().wn_debug_set(2, 1 if form == 'one_workgroup' else 0)
  try:
    queued = model.generate(N_GEN, use_queues=True, **args)
  finally:
    _lib.lib().wn_debug_set(2, 0)
  assert model.generation_guard_trips == 0
  assert naive.shape == (Bg, N_GEN, 1) and bool(torch.isfinite(naive).all()) and float(naive.abs().max()) <= 1.0
  if not det:
    assert len(naive.unique()) > 1                            # (arg-max draws of these near-flat heads may all be one class)
  differ = (naive != queued).reshape(Bg, N_GEN)
  first = int(differ.any(0).float().argmax()) if bool(differ.any()) else -1
  assert torch.equal(naive, queued), (c.net, c.act, Bg, form, det, f'{int(differ.sum())} of {differ.numel()} samples differ, '
                                      f'first at step {first}', (naive - queued).abs().max().item())


@pytest.mark.parametrize('det', [True, False])
@pytest.mark.parametrize('act', AC.ACTS)
@pytest.mark.parametrize('gen_case', list(GEN_CASES))
def test_queued_generation_reproduces_the_sliding_window_bit_for_bit(gen_case, act, det):
  net, Bg, form = GEN_CASES[gen_case]
  c = AC.case(net, act)
  _both_generation_paths(c, _model(c), Bg, form, det)


@functools.lru_cache(maxsize=None)
def _oracle_window(act, n):
  """The oracle's sliding window on r64_head256 in fp64: (samples, is every utterance's decision of step i clear)."""
  c = AC.case('r64_head256', act)
  pd = [p.double() for p in c.params]
  xw = O.synthetic_waveform(3, O.receptive_field(c.ocfg), seed=GEN_SEED).double()
  ref, clear = [], []
  with torch.no_grad():
    for _ in range(n):
      pred = O.model_forward(xw, pd, c.ocfg)[:, -1:, :]
      smp = O.sample_waveform_deterministic(pred.float(), c.ocfg).double()
      top2 = torch.topk(pred, 2, dim=-1).values
      clear.append(bool(((top2[..., 0] - top2[..., 1]) > 1e-4).all()))
      ref.append(smp)
      xw = torch.cat([xw[:, 1:], smp], dim=1)
  return torch.cat(ref, dim=1), clear


@pytest.mark.parametrize('act', AC.ACTS)
def test_sliding_window_matches_the_oracle(act):
  """The first 6 deterministic samples against the oracle's sliding window: exact wherever the oracle's own top-2
  probabilities are more than 1e-4 apart; a step that is not clear ends the comparison (the rule of
  tests/test_gpu_baseline_nets.py)."""
  n = 6
  c = AC.case('r64_head256', act)
  model = _model(c)
  assert model.receptive_field == O.receptive_field(c.ocfg)
  ref, clear = _oracle_window(act, n)
  w, _ = _gen_inputs(c, model, 3)
  out = model.generate(n, sample=w.to(dev()), deterministic=True, use_queues=False).cpu().double()
  assert model.generation_guard_trips == 0
  upto = n if all(clear) else clear.index(False)
  assert upto >= 1, 'not even the first decision of the oracle is clear'
  print(f'r64_head256 {act}: {upto} of {n} steps compared')
  assert torch.equal(out[:, :upto], ref[:, :upto]), (act, upto)


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize('net,act', AC.c_pairs())
def test_saturated_gates_and_heads_against_the_fp64_oracle(net, act, math_mode):
  model, fig, c, ev = _training_pass(net, act, True, math_mode)
  D, N, nf = c.ocfg.D, c.ocfg.blocks, len(c.ocfg.final_layers_channels)

  def region(what, idx):
    return model.training_intermediate(what, idx, B, T)

  # everything the pass wrote is finite (what the comparisons of _training_pass did not already read)
  wrote = [(f'Z[{b}]', region(1, b)) for b in range(N)] + [(f'gate[{b}]', region(2, b)) for b in range(N)]
  wrote += [(f'dL/dH[{b}]', region(9, b)) for b in range(N)] +[(f'dL/da[{i}]', region(6, i)) for i in range(nf + 1)]
  wrote += [('loss rows', region(12, 0)), ('gradients', model.flat_grads)]
  for name, t in wrote:
    assert bool(torch.isfinite(t).all()), (net, act, math_mode, name, 'not finite')
  # dL/du = [dL/du_f | dL/du_g] of every block against the oracle's autograd; the gate channels planted at -100 (sigmoid 4e-44:
  # the g <= 1e-30 branch of wn_gate_bwd, a = z / g undefined) must come out as the zero the oracle has there
  for b, ref in enumerate(ev.g_u):
    got = region(8, b).cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), (net, act, math_mode, f'dL/du[{b}]', 'not finite')
    fig.check('dL/du', f'dL/du[{b}]', got, ref, AC.grad_bar(ref))
    low = ref[..., D:D + 4]
    assert low.abs().max().item() < 1e-20
    assert got[..., D:D + 4].abs().max().item() <= AC.grad_bar(ref), (net, act, math_mode, b)
  fig.finish()


@pytest.mark.parametrize('det', [True, False])
@pytest.mark.parametrize('gen_case', ['r64_head256_b3', 'r128_relay'])
def test_queued_generation_on_the_saturated_tanh_nets(gen_case, det):
  net, Bg, form = GEN_CASES[gen_case]
  c = AC.case(net, 'tanh', True)
  _both_generation_paths(c, _model(c), Bg, form, det)


# ------------------------------------------------------------------------------------------ D
# id: R, D, S, KS, dilations, Cin, Cc, activation, residual, B, T  (the layout of tests/test_gpu_layer_backward.py)
LAYER_CASES = {f'act_{a}_r64_deep': (64, 64, 64, 2, [1, 2], 64, 0, a, True, 2, 97) for a in AC.ACTS}
assert not set(LAYER_CASES) & set(LB.ALL_CASES)
LB.ALL_CASES.update(LAYER_CASES)           # _case looks its name up there; the reference is built once for both math modes


@pytest.mark.parametrize('name', list(LAYER_CASES))
def test_standalone_layer_against_the_fp64_reference(name, math_mode):
  spec, layer, ps, (x, cond, gx, gs), ref = LB._case(name)
  R, D, S, KS, dil, cin, Cc, act, res, Bl, Tl = spec
  assert ref['g_x'].shape == (Bl, Tl, cin) and ref['g_x'].abs().max() > 0 and len(ref['pre']) == 1
  got = LB._run(layer, x, cond, gx, gs)
  rep = LB.Report(f'{name} [{math_mode}]', Tl, LB._splits(layer, Bl, Tl))
  LB._compare(rep, spec, ref, *got)
  rep.finish()
