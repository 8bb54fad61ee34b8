"""The cases of tests/test_gpu_activations.py, and what the fp64 oracle alone says about them.

The GPU file runs every supported activation through the 64- and 128-channel kernels, and drives the gate and the head
non-linearities to saturation.  A green run of it must not be able to mean "nothing was saturated", "every relu kink was
excused" or "the net took another kernel": this file pins, without a device, that

  * every oracle tensor the GPU file compares is finite;
  * the saturated weights (gate scale GS, head scale HS, planted biases) put the stated shares of the oracle's own
    pre-activations beyond |u| > 9, below -70 (the g <= 1e-30 branch of wn_gate_bwd) and below -17 (elu), while the residual
    stream stays far from the range guard and the logits of the unbounded heads below 10;
  * the same oracle evaluated in float32 stays within a QUARTER of every bar (the split contract rounds operands at 2^-22 |v|,
    four times fp32's 2^-24): the bars of DESIGN.md section 5 are reachable on these inputs;
  * relu pre-activations within KINK_TOL of 0 are at most 5e-4 of the elements (the GPU test's overrides are a subset);
  * every net takes, in split mode and whatever its activation, the skip and head paths its row of PATHS names.

The GPU file imports the case construction from here, so both files speak of the same weights and data.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import wavenet_oracle as O

B, T = 2, 197                  # 6 x 32 + 5 and 3 x 64 + 5: ragged last tiles of both tile heights
DATA_SEED, WEIGHT_SEED, BIAS_RANGE = 8, 4, 0.3
ATOL_ACT = 1e-4
ACTS = ('relu', 'tanh', 'sigmoid', 'elu')
SAT_ACTS = ('tanh', 'sigmoid', 'relu', 'elu', None)
SAT_NETS = ('r64_head256', 'r128')
KINK_SHARE = 5e-4

_R64 = dict(blocks=4, channels=64, skip_channels=256, dilation_bound=16, final_layers_channels=[128, 256], bits=8)
NETS = {
    'r64_head256': _R64,
    'r128': dict(blocks=3, channels=128, skip_channels=256, dilation_bound=8, final_layers_channels=[128, 64], bits=8),
    'lpb2_r64': dict(blocks=3, layers_per_block=2, channels=64, skip_channels=64, dilation_bound=8,
                     final_layers_channels=[64], bits=8),
    'r32_f128': dict(blocks=5, channels=32, skip_channels=96, dilation_bound=16, final_layers_channels=[128, 48], bits=8),
    'mol_r64': dict(_R64, num_mixtures=10, sampling_function='logistic', bits=16),
    'cond_r64': dict(_R64, conditioning='global', mapping_layers=[8, 16], cond_inputs=7),
}
# net: (skip token, head tokens, deep16) of wn_debug_fwd_paths in a split-precision training pass that wants the loss
PATHS = {
    'r64_head256': ('folded/planes', ['planes', 'epilogue'], '0'),       # <2,4,act>, <1,8,act>, <1,8,-3>
    'r128': ('folded/planes', ['rows', 'epilogue'], '0'),                # <2,4,act> under 128-channel blocks, rows16 act
    'lpb2_r64': ('sum', ['rows', 'epilogue'], '1'),                      # deep16: the taps form; rows16 act
    'r32_f128': ('sum', ['planes', 'rows', 'epilogue'], '0'),            # 96 -> 128 planes, 128 -> 48 on the fp32 rows kernel
    'mol_r64': ('folded/planes', ['planes', 'rows'], '0'),               # 30-column output conv, wn_mix_loss_kernel
    'cond_r64': ('folded/planes', ['planes', 'epilogue'], '0'),
}
DEEP_FWD = 'per conv of the stack, split precision in training passes'

# Saturation (Test C).  The gate scale multiplies every block*/dil*/kernel, the head scale of hidden layer i every
# final{i}/kernel.  Each value was lowered from 8 until the float32 oracle kept a quarter of every bar, and raised only where a
# share below was missed at 8 (r128's Glorot limit is 0.7 of the 64-channel one: 7.9 % of |u| > 9 at 8, 17 % at 12).  A tanh head
# has one scale per hidden layer: the second layer multiplies the first one's rounding by its own scale again (slope 1 at 0),
# and no single scale gives r64_head256 both 10 % of |pre| > 9 and a quarter of the bar (8: 0.59 of the bar; 6: 0.32; 4: 4.8 %).
# relu / elu heads are unbounded above: their scale is what keeps |logits| < 10.  Measured figures: DESIGN.md section 30.
GS = {'r64_head256': 8.0, 'r128': 12.0}
HS = {('r64_head256', 'tanh'): (8.0, 2.0), ('r128', 'tanh'): (4.0, 4.0)}
for _net in ('r64_head256', 'r128'):
  HS.update({(_net, 'sigmoid'): (8.0, 8.0), (_net, 'relu'): (2.0, 2.0), (_net, 'elu'): (2.0, 2.0)})
GATE_LOW, GATE_HIGH, FILT_HIGH, FILT_LOW, HEAD_PLANT = -100.0, 100.0, 50.0, -50.0, 40.0


def net_kwargs(net, act):
  """Constructor keywords of a (net, activation) pair.  cond_r64: the activation under test is the mapping network's."""
  kw = dict(NETS[net])
  if net == 'cond_r64':
    kw.update(activation='leaky_relu', mapping_activation=act)
  else:
    kw['activation'] = act
  return kw


def saturate(net, act, names, params):
  """The weights of Test C from the unit-scale ones (a new list; `params` is left alone)."""
  kw = NETS[net]
  D, nf = kw['channels'], len(kw['final_layers_channels'])
  out = [p.clone() for p in params]
  for n, p in zip(names, out):
    part = n.split('/')
    if part[0].startswith('block') and part[1].startswith('dil'):
      if part[2] == 'kernel':
        p *= GS[net]
      else:
        assert p.numel() == 2 * D
        p[D:D + 4], p[D + 4:D + 8] = GATE_LOW, GATE_HIGH
        p[8:12], p[12:16] = FILT_HIGH, FILT_LOW
    elif part[0].startswith('final') and int(part[0][5:]) < nf and act is not None:
      if part[1] == 'kernel':
        p *= HS[net, act][int(part[0][5:])]
      else:
        if act in ('tanh', 'sigmoid'):
          p[0:4] = HEAD_PLANT
        p[4:8] = -HEAD_PLANT
  return out


@functools.lru_cache(maxsize=None)
def case(net, act, sat=False):
  """Keywords, oracle configuration, fp32 weights, data and condition of one case; built once."""
  kw = net_kwargs(net, act)
  okw = dict(kw)
  cond_inputs = okw.pop('cond_inputs', 0)
  ocfg = O.OracleConfig(**okw, cond_inputs=cond_inputs)
  names = [n for n, _ in O.param_shapes(ocfg)]
  params = O.init_params(ocfg, seed=WEIGHT_SEED, bias_range=BIAS_RANGE)        # = make_pair(seed=4, bias_range=0.3, ...)
  if sat:
    params = saturate(net, act, names, params)
  x = O.synthetic_waveform(B, T + 1, seed=DATA_SEED)
  cond = torch.rand(B, cond_inputs, generator=torch.Generator().manual_seed(DATA_SEED)) if cond_inputs else None
  return SimpleNamespace(net=net, act=act, sat=sat, kw=kw, ocfg=ocfg, names=names, params=params, x=x, cond=cond)


def evaluate(c, dtype=torch.float64, head_branch=None, inner_branch=None):
  """One oracle training pass in `dtype`: every tensor the GPU file compares, detached.  u = [filter | gate] pre-activations,
  g_u their gradients."""
  ps = [p.to(dtype).requires_grad_(True) for p in c.params]
  cd = c.cond.to(dtype) if c.cond is not None else None
  klog = []
  pred, inter = O.model_forward(c.x[:, :-1].to(dtype), ps, c.ocfg, cd, return_intermediates=True, head_branch=head_branch,
                                inner_branch=inner_branch, kink_log=klog)
  if c.ocfg.num_mixtures is not None:
    # the 16-bit logistic bin mass cancels five digits: a float32 evaluation of the loss formula is good to ~1e-3 only, and
    # the product evaluates the row in double from its fp32 mixture parameters (wn_mix_loss_kernel).  So does the float32 oracle
    pred = pred.double()
  target = O.prepare_target(c.x[:, 1:].to(pred.dtype), c.ocfg)
  loss = O.loss_fn(target, pred, c.ocfg).sum() / B
  gr = torch.autograd.grad(loss, ps + inter['u'], allow_unused=True)
  grads = [g if g is not None else torch.zeros_like(p) for g, p in zip(gr[:len(ps)], ps)]
  det = lambda ts: [t.detach() for t in ts]
  return SimpleNamespace(
      logits=inter['logits'].detach(), h=det(inter['h']), head_pre=det(inter['head_pre']),
      head_act=[O.activation(a.detach(), c.ocfg.activation) for a in inter['head_pre']],
      inner_pre=[det(p) for p in inter['pre']], inner_act=[det(p) for p in inter['p']], u=det(inter['u']),
      loss=loss.detach(), grads=det(grads), g_u=det(gr[len(ps):]), kink_overrides=inter['kink_overrides'], kink_log=klog)


@functools.lru_cache(maxsize=None)
def oracle(net, act, sat=False):
  """The fp64 oracle of a case with every kink on its own side: shared by both math modes of the GPU file."""
  return evaluate(case(net, act, sat))


def compared(ev):
  """[(name, tensor, bar)] of an evaluation `ev` with the bars of DESIGN.md section 5 taken from the fp64 oracle `ev`."""
  out = [('logits', ev.logits, ATOL_ACT)]
  out += [(f'H[{b}]', h, ATOL_ACT) for b, h in enumerate(ev.h)]
  out += [(f'head activation {i}', a, ATOL_ACT) for i, a in enumerate(ev.head_act)]
  out += [(f'inner activation {b}.{i}', a, ATOL_ACT) for b, blk in enumerate(ev.inner_act) for i, a in enumerate(blk)]
  out.append(('loss', ev.loss, 2e-5 * max(1.0, abs(ev.loss.item()))))
  return out


def grad_bar(ref):
  return 1e-4 * ref.abs().max().item() + 1e-7


def near_kink(ev, act):
  """(elements within KINK_TOL of the relu kink, elements) over the head and inner pre-activations of the oracle."""
  pres = list(ev.head_pre) + [p for blk in ev.inner_pre for p in blk]
  return sum(int((p.abs() < O.KINK_TOL).sum()) for p in pres), sum(p.numel() for p in pres)


def a_pairs():
  return [(n, a) for n in NETS for a in ACTS]


def c_pairs():
  return [(n, a) for n in SAT_NETS for a in SAT_ACTS]


ALL = [(n, a, False) for n, a in a_pairs()] + [(n, a, True) for n, a in c_pairs()]
IDS = [f'{n}-{a}-{"saturated" if s else "unit"}' for n, a, s in ALL]


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('net,act,sat', ALL, ids=IDS)
def test_oracle_is_finite_and_float32_keeps_a_quarter_of_every_bar(net, act, sat):
  c, ev = case(net, act, sat), oracle(net, act, sat)
  for name, t, _ in compared(ev):
    assert bool(torch.isfinite(t).all()), (name, 'not finite')
  for n, g in zip(c.names, ev.grads):
    assert bool(torch.isfinite(g).all()), (n, 'gradient not finite')
  assert all(bool(torch.isfinite(g).all()) for g in ev.g_u)
  assert ev.kink_overrides == 0 and ev.loss.item() > 0
  e32 = evaluate(c, torch.float32)
  worst = ('', 0.0)
  for (name, ref, bar), (_, got, _) in zip(compared(ev), compared(e32)):
    r = (got.double() - ref).abs().max().item() / bar
    worst = max(worst, (name, r), key=lambda v: v[1])
    assert r <= 0.25, (net, act, sat, name, r)
  for n, ref, got in zip(c.names, ev.grads, e32.grads):
    r = (got.double() - ref).abs().max().item() / grad_bar(ref)
    worst = max(worst, (n, r), key=lambda v: v[1])
    assert r <= 0.25, (net, act, sat, n, r)
  for b, (ref, got) in enumerate(zip(ev.g_u, e32.g_u)):
    r = (got.double() - ref).abs().max().item() / grad_bar(ref)
    assert r <= 0.25, (net, act, sat, f'dL/du[{b}]', r)
  print(f'{net} {act} {"saturated" if sat else "unit"}: float32 oracle, worst error / bar {worst[1]:.3f} at {worst[0]}')


@pytest.mark.parametrize('net,act', c_pairs())
def test_the_saturated_weights_saturate(net, act):
  c, ev = case(net, act, True), oracle(net, act, True)
  D = c.ocfg.D
  u = torch.stack(ev.u)                                     # (blocks, B, T, 2 D) = [filter | gate]
  gate = u[..., D:]
  big, low = (u.abs() > 9).double().mean().item(), (gate < -70).double().mean().item()
  assert big >= 0.10, (net, act, big)
  assert low >= 0.01, (net, act, low)
  # the planted channels are where the plan says: gate at -100 / +100, filter at +-50, give or take the scaled conv
  assert bool((gate[..., 0:4] < -70).all()) and bool((gate[..., 4:8] > 70).all())
  assert bool((u[..., 8:12] > 20).all()) and bool((u[..., 12:16] < -20).all())
  assert max(h.abs().max().item() for h in ev.h) < 100                        # far from the 65504 guard
  head = torch.cat([p.reshape(-1) for p in ev.head_pre])
  share = None
  if act in ('tanh', 'sigmoid'):
    share = (head.abs() > 9).double().mean().item()
    assert share >= 0.10, (net, act, share)
  elif act == 'elu':
    share = (head < -17).double().mean().item()
    assert share >= 0.01, (net, act, share)
  if act in ('relu', 'elu'):
    assert ev.logits.abs().max().item() < 10, (net, act, ev.logits.abs().max().item())
  # the planted gate channels: the oracle's own dL/du there is what the GPU file expects the product to give as zero
  g_u = torch.stack(ev.g_u)
  assert g_u[..., D:D + 4].abs().max().item() < 1e-20
  print(f'{net} {act}: |u| > 9 share {big:.3f}, gate < -70 share {low:.3f}, head share {share}, '
        f'max|H| {max(h.abs().max().item() for h in ev.h):.2f}, max|logits| {ev.logits.abs().max().item():.2f}')


@pytest.mark.parametrize('net,sat', [(n, False) for n in NETS] + [(n, True) for n in SAT_NETS])
def test_relu_pre_activations_near_the_kink_are_rare(net, sat):
  """(cond_r64: its head is leaky_relu whatever the mapping activation, with the same kink: counted for all four.)"""
  for act in (ACTS if net == 'cond_r64' else ('relu',)):
    near, total = near_kink(oracle(net, act, sat), 'relu')
    assert total > 0 and near <= KINK_SHARE * total, (net, act, sat, near, total)
  print(f'{net} {"saturated" if sat else "unit"}: {near} of {total} relu pre-activations within KINK_TOL of 0')
  assert total > 0 and near <= KINK_SHARE * total, (net, sat, near, total)


def test_the_mapping_network_has_no_pre_activation_near_a_kink():
  """cond_r64 with a relu mapping network: the oracle has no branch override for the mapping layers, so the case is only
  usable if none of its 2 x (8 + 16) pre-activations is near 0."""
  c = case('cond_r64', 'relu')
  off = c.names.index('mapping0/kernel')
  m = c.cond.double()
  for j in range(2):
    pre = m @ c.params[off + 2 * j].double() + c.params[off + 2 * j + 1].double()
    assert pre.abs().min().item() > 10 * O.KINK_TOL, (j, pre.abs().min().item())      # (measured: 4.0e-3)
    m = torch.relu(pre)
  assert float(m.abs().max()) > 0                          # the condition reaches the blocks


@pytest.fixture(scope='module')
def lib():
  import os
  from wavenets_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


@pytest.mark.parametrize('net', list(NETS))
def test_every_net_takes_the_paths_its_row_names_whatever_the_activation(lib, net):
  import test_fwd_paths_cpu as FP
  import test_gpu_head_tile_walk as HW
  assert lib.wn_debug_value(1) == 0
  skip, head, deep = PATHS[net]
  seen = []
  for act in ACTS + ('leaky_relu', None):
    kw = dict(net_kwargs(net, act))
    cond_inputs = kw.pop('cond_inputs', 0)
    got = FP.paths(lib, HW._full(kw), cond_inputs, B, T)
    assert (got['skip'], got['head'], got['deep16']) == (skip, head, deep), (net, act, got)
    assert got['fold'] == ('1' if skip.startswith('folded') else '0')
    assert (got['skip'], got['head']) == FP.reduced(HW.route(HW._full(kw))), (net, act)
    seen.append(got)
  assert all(s == seen[0] for s in seen), net


def test_lpb2_r64_is_planned_on_the_split_precision_stack(lib):
  from wavenets_amd import _lib
  from test_cabi_cpu import _cfg, _plan
  import test_gpu_head_tile_walk as HW
  for act in ACTS:
    p = C.c_void_p(_plan(lib, _cfg(**HW._full(net_kwargs('lpb2_r64', act))), 0))
    assert p.value, lib.wn_last_error_string()
    try:
      buf = C.create_string_buffer(2048)
      assert lib.wn_plan_describe(p, buf, 2048) == _lib.WN_OK
    finally:
      lib.wn_plan_destroy(p)
    assert DEEP_FWD in buf.value.decode(), (act, buf.value.decode())
