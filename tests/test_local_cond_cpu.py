"""Local conditioning without a device: the fp64 restatement against the oracle's global model at
F = 1, the variable table of a local spec, and the host-side checks of wn_plan_set_cond_frames."""
import ctypes as C

import pytest
import torch

import local_reference as LR
from oracle import wavenet_oracle as O
from test_cabi_cpu import _cfg, _plan, lib  # noqa: F401  (lib: fixture)
from wavenets_amd import _lib

CASES = {
    # the two conditioned cases of tests/test_gpu_parity.py
    'cond': dict(blocks=4, channels=32, skip_channels=64, dilation_bound=8, final_layers_channels=[32],
                 activation='leaky_relu', conditioning='global', mapping_layers=[8, 16, 32],
                 mapping_activation='leaky_relu', bits=8, cond_inputs=11),
    'cond_nomap': dict(blocks=3, channels=32, dilation_bound=8, final_layers_channels=[],
                       conditioning='global', bits=6, cond_inputs=4),
}


@pytest.mark.parametrize('name', list(CASES))
def test_one_frame_is_the_oracles_global_model(name):
  """F = 1: the frame repeated over every input is the global model's repeated condition; same operations, fp64."""
  gcfg = O.OracleConfig(**CASES[name])
  lcfg = O.OracleConfig(**dict(CASES[name], conditioning='local'))
  params = [p.double() for p in O.init_params(gcfg, seed=1)]
  B, T = 3, 97
  x = O.synthetic_waveform(B, T, seed=3).double()
  cond = torch.rand(B, gcfg.cond_inputs, generator=torch.Generator().manual_seed(3)).double()
  for logits in (False, True):
    ref = O.model_forward(x, params, gcfg, cond, return_logits=logits)
    got = LR.local_forward(x, params, lcfg, LR.upsample(cond[:, None, :], T), return_logits=logits)
    assert torch.equal(got, ref), (name, logits, float((got - ref).abs().max()))
  with pytest.raises(NotImplementedError):
    O.model_forward(x, params, lcfg, cond)                # the oracle itself keeps refusing 'local'


def test_upsample_is_repeat_interleave():
  f = torch.arange(6.0).reshape(1, 3, 2)
  up = LR.upsample(f, 2)
  assert up.shape == (1, 6, 2) and torch.equal(up[0, :, 0], torch.tensor([0., 0., 2., 2., 4., 4.]))
  assert LR.upsample(torch.arange(3.0).reshape(1, 3), 4).shape == (1, 12, 1)      # (B, F): one channel


def test_frames_reach_only_their_own_inputs_and_later_ones():
  """Changing frame f moves no output before f * hop (the network is causal), and does move outputs inside the frame."""
  lcfg = O.OracleConfig(**dict(CASES['cond_nomap'], conditioning='local'))
  params = [p.double() for p in O.init_params(LR.global_cfg(lcfg), seed=2)]
  B, F, hop = 2, 3, 32
  x = O.synthetic_waveform(B, F * hop, seed=4).double()
  fr = torch.rand(B, F, 4, generator=torch.Generator().manual_seed(5)).double()
  base = LR.local_forward(x, params, lcfg, LR.upsample(fr, hop))
  fr2 = fr.clone()
  fr2[:, 1] += 0.5
  moved = LR.local_forward(x, params, lcfg, LR.upsample(fr2, hop))
  assert torch.equal(moved[:, :hop], base[:, :hop])
  assert not torch.equal(moved[:, hop], base[:, hop])


def test_a_local_spec_has_the_1x1_mapping_kernels():
  s = _cfg(conditioning='local', mapping_layers=[8, 6], mapping_activation='tanh', blocks=3, skip_channels=64)
  shapes = dict(s.param_shapes(5))
  assert shapes['mapping0/kernel'] == (1, 5, 8) and shapes['mapping0/bias'] == (8,)
  assert shapes['mapping1/kernel'] == (1, 8, 6) and shapes['mapping1/bias'] == (6,)
  assert shapes['block0/conv_cond/kernel'] == (1, 6, 64)          # the mapped width feeds every block's conv_cond
  g = _cfg(conditioning='global', mapping_layers=[8, 6], mapping_activation='tanh', blocks=3, skip_channels=64)
  gs = g.param_shapes(5)
  # the same variables at the same places in the creation order; only the mapping kernels carry one more axis
  assert [n for n, _ in s.param_shapes(5)] == [n for n, _ in gs]
  assert [shp for n, shp in s.param_shapes(5) if 'mapping' not in n] == [shp for n, shp in gs if 'mapping' not in n]
  assert dict(gs)['mapping0/kernel'] == (5, 8)


def _conditioned_plan(lib, cond_inputs=5):
  s = _cfg(conditioning='global', mapping_layers=[8], blocks=3, channels=32, skip_channels=64, dilation_bound=8,
           final_layers_channels=[32])
  p = C.c_void_p(_plan(lib, s, cond_inputs))
  assert p.value, lib.wn_last_error_string()
  return p


def test_set_cond_frames_argument_checks(lib):
  assert lib.wn_plan_set_cond_frames(None, 2) == _lib.WN_E_INVALID
  assert b'null plan' in lib.wn_last_error_string()
  p = _conditioned_plan(lib)
  try:
    assert lib.wn_plan_set_cond_frames(p, -1) == _lib.WN_E_INVALID
    assert b'frames must be >= 0' in lib.wn_last_error_string()
    for f in (0, 1, 6, 0):
      assert lib.wn_plan_set_cond_frames(p, f) == _lib.WN_OK
  finally:
    lib.wn_plan_destroy(p)
  u = C.c_void_p(_plan(lib, _cfg(blocks=3, dilation_bound=8)))
  try:
    assert lib.wn_plan_set_cond_frames(u, 1) == _lib.WN_OK
    assert lib.wn_plan_set_cond_frames(u, 2) == _lib.WN_E_INVALID
    assert b'without conditioning' in lib.wn_last_error_string()
  finally:
    lib.wn_plan_destroy(u)


def test_workspace_grows_with_the_frames_and_not_at_one(lib):
  p = _conditioned_plan(lib)
  try:
    B, T = 3, 192
    for training in (0, 1):
      base = lib.wn_plan_workspace_floats(p, B, T, training)
      sizes = []
      for f in (0, 1, 2, 6):
        assert lib.wn_plan_set_cond_frames(p, f) == _lib.WN_OK
        sizes.append(lib.wn_plan_workspace_floats(p, B, T, training))
      assert sizes[0] == base and sizes[1] == base
      assert base < sizes[2] < sizes[3]
      assert lib.wn_plan_set_cond_frames(p, 0) == _lib.WN_OK
      assert lib.wn_plan_workspace_floats(p, B, T, training) == base
      # the forward range-guard slot lies in front of the conditioning's regions: the same float with and without frames
      slot = lib.wn_plan_range_slot(p, B, T, training)
      lib.wn_plan_set_cond_frames(p, 6)
      assert lib.wn_plan_range_slot(p, B, T, training) == slot
      lib.wn_plan_set_cond_frames(p, 0)
  finally:
    lib.wn_plan_destroy(p)


@pytest.mark.parametrize('T,F,text', [(190, 6, b'do not divide'), (192, 4, b'hop = 48'), (96, 2, b'hop = 48')])
def test_frame_geometry_is_refused_before_the_device_is_touched(lib, T, F, text):
  """T % F and hop % 32: WN_E_INVALID with the numbers, from every training-form entry point, with host pointers that
  would fault if anything were launched or read."""
  p = _conditioned_plan(lib)
  one = C.c_void_p(64)                                     # never dereferenced
  try:
    assert lib.wn_plan_set_cond_frames(p, F) == _lib.WN_OK
    B, big = 2, 1 << 40
    calls = {
        'forward': lambda: lib.wn_forward(p, one, one, one, B, T, one, None, one, big, None),
        'forward_training': lambda: lib.wn_forward_training(p, one, one, one, B, T, one, None, one, big, None),
        'train_fwd_bwd': lambda: lib.wn_train_fwd_bwd(p, one, one, one, B, T, B, 1, one, one, None, one, big, None),
        'eval_loss': lambda: lib.wn_eval_loss(p, one, one, one, B, T, B, one, None, one, big, None),
        'score': lambda: lib.wn_score(p, one, one, one, B, T, one, None, None, one, one, big, None),
        'vjp': lambda: lib.wn_vjp(p, one, one, one, B, T, one, 1, one, None, None, one, big, None),
    }
    for who, call in calls.items():
      assert call() == _lib.WN_E_INVALID, who
      msg = lib.wn_last_error_string()
      assert msg.startswith(who.encode() + b':') and text in msg, (who, msg)
      assert f'T = {T}'.encode() in msg and f'F = {F}'.encode() in msg, msg
  finally:
    lib.wn_plan_destroy(p)


def test_generation_entries_refuse_armed_frames(lib):
  p = _conditioned_plan(lib)
  one = C.c_void_p(64)
  try:
    assert lib.wn_plan_set_cond_frames(p, 3) == _lib.WN_OK
    sp = _lib.WnSampling(1.0, 0, 0, 0.0)
    rc = lib.wn_generate_sampled(p, one, one, one, 2, 4, 1, 1, C.byref(sp), one, one, 1 << 40, None)
    assert rc == _lib.WN_E_INVALID and b'3 condition frames are armed' in lib.wn_last_error_string()
  finally:
    lib.wn_plan_destroy(p)


@pytest.mark.parametrize('name', list(LR.GEN_NETS))
@pytest.mark.parametrize('hop', [5, 32])
def test_the_greedy_rollout_is_clear_of_ties(name, hop):
  """The reference-alone condition of the generation test: in the restatement's own greedy rollout the top-2 probability
  margin is at or below 1e-4 at no more than 2 % of the steps, so the device's arg max can be held to the fp64 one."""
  _, margins = LR.greedy_rollout(name, hop)
  close = float((margins <= 1e-4).double().mean())
  assert close <= 0.02, (name, hop, close)


def test_generate_set_condition_argument_checks(lib):
  p = _conditioned_plan(lib)
  one = C.c_void_p(64)
  big = 1 << 40
  try:
    call = lambda pp=p, params=one, cond=one, B=2, queued=1, ws=one, n=big: lib.wn_generate_set_condition(pp, params, cond, B, queued, ws, n, None)
    for kw, text in ((dict(pp=None), b'null plan'), (dict(params=None), b'null params'), (dict(cond=None), b'null cond'),
                     (dict(ws=None), b'null workspace'), (dict(B=0), b'B must be >= 1'), (dict(queued=0), b'queued sequences only'),
                     (dict(n=8), b'workspace too small'), (dict(), b'has not been primed')):
      assert call(**kw) == _lib.WN_E_INVALID, kw
      assert text in lib.wn_last_error_string(), (kw, lib.wn_last_error_string())
    assert lib.wn_plan_set_cond_frames(p, 3) == _lib.WN_OK
    assert call() == _lib.WN_E_INVALID and b'frames are armed' in lib.wn_last_error_string()
  finally:
    lib.wn_plan_destroy(p)
  u = C.c_void_p(_plan(lib, _cfg(blocks=3, dilation_bound=8)))
  try:
    assert lib.wn_generate_set_condition(u, one, one, 2, 1, one, big, None) == _lib.WN_E_INVALID
    assert b'no conditioning' in lib.wn_last_error_string()
  finally:
    lib.wn_plan_destroy(u)
