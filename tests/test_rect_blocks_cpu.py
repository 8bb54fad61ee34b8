"""Networks whose gated width D (dilation_channels) differs from their residual width R (channels), and the square shapes
that miss every shape-specialised kernel: the case table of tests/test_gpu_rect_blocks.py and, for every case, the kernel
families the library decides for it (wn_plan_describe, wn_debug_fwd_paths, on plans made without a device) in both
contraction modes.  The expected strings are literal text, worked out from the width predicates of wn_plan_create; if a
predicate moves, the GPU cases would go on passing while covering another kernel, and this file fails first."""
import ctypes as C

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan
from test_fwd_paths_cpu import paths
import test_layer_describe_cabi_cpu as LD


@pytest.fixture(scope='module')
def lib():
  import os
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


def _net(R, D, S, finals, **kw):
  """Dilations 1, 2, 4, 8, 1: a receptive field of 18 samples."""
  d = dict(blocks=5, channels=R, dilation_channels=D, skip_channels=S, dilation_bound=16, final_layers_channels=finals,
           activation='leaky_relu', bits=8)
  d.update(kw)
  return d


CASES = {
    'r64_d128': _net(64, 128, 256, [128, 256]),
    'r128_d64': _net(128, 64, 256, [128, 256]),
    'r64_k3': _net(64, 64, 256, [128, 256], kernel_size=3, dilation_bound=27),          # dilations 1, 3, 9, 1, 3
    'r32_d64_fold': _net(32, 64, 256, [128, 64]),
    'r32_d64_sum': _net(32, 64, 64, [48]),
    'r64_d32': _net(64, 32, 64, [32]),
    'r96': _net(96, 96, 96, [64]),
    'r48_d64': _net(48, 64, 64, [32]),
    'r64_d128_cond': _net(64, 128, 256, [128, 256], conditioning='global', mapping_layers=[8, 16], cond_inputs=5),
    'r128_d64_mol': _net(128, 64, 256, [128, 256], num_mixtures=10, sampling_function='logistic', bits=16),
    'r64_d32_lpb2': _net(64, 32, 64, [32], layers_per_block=2),                       # dilations 1, 2, 4, 8 twice, then 1, 2
}

# standalone WaveNetLayer shapes of the GPU file: R, D, S, dilation, kernel size, T
LAYER_SHAPES = [
    (64, 128, 256, 4, 2, 130),
    (128, 64, 256, 4, 2, 130),
    (32, 64, 64, 8, 2, 97),
    (64, 32, None, 2, 3, 97),
    (96, 96, 96, 2, 2, 70),
]

# ---- wn_plan_describe, field by field (the text after "<field>: ") ----
SPLIT, EXACT = 'fp16 hi|lo split, 3 products, fp32 accumulate', 'exact fp32 MFMA'
FWD_TWO = 'two split-precision contractions per block (gated conv + gate, 1x1 + residual)'
FWD_COMPOSED = 'composed: rows GEMM -> gate kernel -> rows GEMM'
FWD_FUSED_FP32 = 'fused exact-fp32 block kernel (wn_layer_fwd_kernel)'
FWD_PER_CONV = 'composed per conv (rows GEMM fp32 + fused fp32 kernel for the gated conv where the shape allows)'
SKIP_FOLDED = "folded into the head's first conv (V = W_s W_f0, training / inference / generation)"
SKIP_SUM = "one contraction over all blocks' gated activations, then the head"
BWD_ROWS16 = 'two split-precision rows contractions per block (g_u with the gate derivative, g_x)'
BWD_ROWS32 = 'two exact-fp32 rows contractions per block'
BWD_PER_CONV = 'per-block composed backward, one rows contraction per conv of the stack (layers_per_block > 1)'
WG_GENERIC = 'generic batched job table (wn_wgrad_batched_kernel)'
WG_GENERIC_FP32 = 'generic batched job table in exact fp32, every conv of every stack in one launch (wn_wgrad_batched_kernel)'

# Split mode, from the predicates of wn_plan_create (m16(v): v % 16 == 0; m32(v): v >= 64 and v % 32 == 0):
#  * no case has R = D in {32, 64, 128} at kernel size 2, so none takes the LDS-resident fused kernel; r64_k3 has the shape of
#    the exact-fp32 fused kernel only (the split-precision one is built for kernel size 2);
#  * two contractions: layers_per_block == 1 and D % 64 == 0 and m16(R) and m32(R) -- (64, 128), (128, 64), (64, 64) at k = 3;
#    not (32, 64) or (48, 64) (m32(R) fails), not (64, 32) or (96, 96) (D % 64);
#  * fold: a head with a hidden layer F0 < S, m32(F0), D % 64 == 0, m16(R), m16(S) -- F0 = 128 under S = 256 at D = 128 / 64;
#    not F0 = 48 / 32 (m32(F0)), not D = 32 / 96;
#  * the pair / s128 backward and the per-block weight-gradient kernels want R = D (and kernel size 2): every depth-1 case is
#    on the rows contractions and the generic job table; layers_per_block = 2 at D = 32 has no deep-stack images (R != D),
#    so it keeps the composed kernels and the job table in exact fp32;
#  * head: a conv is on the planes kernel when it has 128 / 256 output columns and an operand of 64 columns or more in
#    multiples of 32 (as the epilogue form when it is the last conv of a 256-class head and the loss is wanted), else rows.
# (describe fields: block forward, skip path, backward data, block weight gradients; fwd_paths: skip, head)
SPLIT_PATHS = {
    'r64_d128': (FWD_TWO, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['planes', 'epilogue']),
    'r128_d64': (FWD_TWO, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['planes', 'epilogue']),
    'r64_k3': (FWD_TWO, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['planes', 'epilogue']),
    'r32_d64_fold': (FWD_COMPOSED, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['rows', 'epilogue']),
    'r32_d64_sum': (FWD_COMPOSED, SKIP_SUM, BWD_ROWS16, WG_GENERIC, 'sum', ['rows', 'epilogue']),
    'r64_d32': (FWD_COMPOSED, SKIP_SUM, BWD_ROWS16, WG_GENERIC, 'sum', ['rows', 'rows']),
    'r96': (FWD_COMPOSED, SKIP_SUM, BWD_ROWS16, WG_GENERIC, 'sum', ['rows', 'epilogue']),
    'r48_d64': (FWD_COMPOSED, SKIP_SUM, BWD_ROWS16, WG_GENERIC, 'sum', ['rows', 'rows']),
    # (the plan holds the two-contraction images; block_forward declines them for a per-utterance condition bias and runs the
    # composed kernels: tests/test_block_paths_cpu.py::test_describe_and_the_launch_disagree_on_the_conditioned_net)
    'r64_d128_cond': (FWD_TWO, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['planes', 'epilogue']),
    'r128_d64_mol': (FWD_TWO, SKIP_FOLDED, BWD_ROWS16, WG_GENERIC, 'folded/planes', ['planes', 'rows']),      # 30 output columns
    'r64_d32_lpb2': (FWD_PER_CONV, SKIP_SUM, BWD_PER_CONV, WG_GENERIC_FP32, 'sum', ['rows', 'rows']),
}
# Exact-fp32 mode: no split-precision image is bound, nothing folds, every head conv is a rows GEMM.
EXACT_FWD = {'r64_k3': FWD_FUSED_FP32, 'r64_d32_lpb2': FWD_PER_CONV}
EXACT_BWD = {'r64_d32_lpb2': BWD_PER_CONV}
EXACT_WG = {'r64_d32_lpb2': WG_GENERIC_FP32}
COND = {'r64_d128_cond': ('small', 'batched')}          # evenly spaced conv_cond tensors, 2D a multiple of 32
SIZES = [(3, 333), (2, 150), (3, 97), (1, 7)]           # the (B, T) of the GPU file


def _kw(name):
  kw = dict(CASES[name])
  return kw, kw.pop('cond_inputs', 0)


def describe(lib, name):
  kw, cond_inputs = _kw(name)
  p = C.c_void_p(_plan(lib, _cfg(**kw), cond_inputs))
  assert p.value, lib.wn_last_error_string()
  try:
    buf = C.create_string_buffer(4096)
    assert lib.wn_plan_describe(p, buf, 4096) == _lib.WN_OK
  finally:
    lib.wn_plan_destroy(p)
  fields = [f.split(': ', 1) for f in buf.value.decode().split(' | ')]
  assert [f[0] for f in fields] == ['math', 'block forward', 'skip path', 'backward data', 'block weight gradients'], buf.value
  return [f[1] for f in fields]


def test_the_case_table_has_what_the_gpu_file_relies_on():
  for name, kw in CASES.items():
    lpb = kw.get('layers_per_block', 1)
    assert kw['blocks'] == 5 and kw['dilation_bound'] == (27 if kw.get('kernel_size') == 3 else 16), name
    s = _cfg(**_kw(name)[0])
    assert len(s.dilations) == 5 * lpb and s.receptive_field < 40, (name, s.dilations, s.receptive_field)
    assert max(s.dilations) == (9 if kw.get('kernel_size') == 3 else 8)          # longer than the 7-step utterances
  assert set(SPLIT_PATHS) == set(CASES)


@pytest.mark.parametrize('name', list(CASES))
def test_split_mode_families(lib, name):
  assert lib.wn_debug_value(1) == 0
  fwd, skip_text, bwd, wg, skip, head = SPLIT_PATHS[name]
  assert describe(lib, name) == [SPLIT, fwd, skip_text, bwd, wg]
  kw, cond_inputs = _kw(name)
  cond, conv_cond = COND.get(name, ('none', 'none'))
  for B, T in SIZES:
    got = paths(lib, kw, cond_inputs, B, T)
    assert (got['skip'], got['head']) == (skip, head), (name, B, T, got)
    assert got['fold'] == ('1' if skip_text == SKIP_FOLDED else '0') == got['first_final']
    assert got['inconv'] == 'elementwise'                             # every R here is a multiple of 4
    assert (got['cond'], got['conv_cond']) == (cond, conv_cond)
    assert got['zfill'] == '0' and got['deep16'] == '0' and got['drop'] == '0'


@pytest.mark.parametrize('name', list(CASES))
def test_exact_fp32_mode_families(lib, name):
  lib.wn_debug_set(1, 1)
  try:
    text = describe(lib, name)
    kw, cond_inputs = _kw(name)
    got = [paths(lib, kw, cond_inputs, B, T) for B, T in SIZES]
  finally:
    lib.wn_debug_set(1, 0)
  assert text == [EXACT, EXACT_FWD.get(name, FWD_COMPOSED), SKIP_SUM, EXACT_BWD.get(name, BWD_ROWS32), EXACT_WG.get(name, WG_GENERIC)]
  cond, conv_cond = COND.get(name, ('none', 'none'))
  for g in got:
    assert g['skip'] == 'sum' and g['fold'] == '0' and g['first_final'] == '0', (name, g)
    assert g['head'] == ['rows'] * (len(kw['final_layers_channels']) + 1), (name, g)
    assert g['inconv'] == 'rows' and (g['cond'], g['conv_cond']) == (cond, conv_cond)


def test_every_family_is_in_the_table():
  """Split mode.  m16 / m32 as in wn_plan_internal.h."""
  def m16(v):
    return v > 0 and v % 16 == 0

  def m32(v):
    return v >= 64 and v % 32 == 0
  rd = {n: (kw['channels'], kw['dilation_channels'], kw.get('kernel_size', 2)) for n, kw in CASES.items()}
  two = [n for n, p in SPLIT_PATHS.items() if p[0] == FWD_TWO]
  composed = [n for n, p in SPLIT_PATHS.items() if p[0] == FWD_COMPOSED]
  assert any(rd[n][0] < rd[n][1] for n in two)
  assert any(rd[n][0] > rd[n][1] for n in two)
  assert any(rd[n] == (64, 64, 3) for n in two)
  assert any(SPLIT_PATHS[n][1] == SKIP_FOLDED and SPLIT_PATHS[n][4].startswith('folded') for n in composed)
  assert any(SPLIT_PATHS[n][1] == SKIP_SUM and SPLIT_PATHS[n][4] == 'sum' for n in composed)
  assert any(p[1] == SKIP_FOLDED and p[2] == BWD_ROWS16 and p[3] == WG_GENERIC for p in SPLIT_PATHS.values())
  narrow = [n for n in CASES if m16(rd[n][0]) and not m32(rd[n][0])]
  assert narrow and any(n in composed for n in narrow), narrow


# ---- the standalone layers: the weight-gradient products of wn_layer_bwd (tests/test_layer_describe_cabi_cpu.py) ----
# B = 2 utterances shorter than 256 rows: one time split an utterance (wn_wgrad_choose_splits caps at ceil(T / 256)), two splits
# in all, reduced in one stage; K x N of every product from the shape: conv1 D x R, conv_skip D x S, each tap R x 2D
def _line(R, D, S, k):
  one = 'splits=1 nsplit=2 reduce=one-stage'
  items = [f'conv1 K={D} N={R} {one}'] + ([f'conv_skip K={D} N={S} {one}'] if S else [])
  return ' | '.join(items + [f'dil0.tap{t} K={R} N={2 * D} {one}' for t in range(k)])


LAYER_LINES = [
    'conv1 K=128 N=64 splits=1 nsplit=2 reduce=one-stage | conv_skip K=128 N=256 splits=1 nsplit=2 reduce=one-stage | '
    'dil0.tap0 K=64 N=256 splits=1 nsplit=2 reduce=one-stage | dil0.tap1 K=64 N=256 splits=1 nsplit=2 reduce=one-stage',
    'conv1 K=64 N=128 splits=1 nsplit=2 reduce=one-stage | conv_skip K=64 N=256 splits=1 nsplit=2 reduce=one-stage | '
    'dil0.tap0 K=128 N=128 splits=1 nsplit=2 reduce=one-stage | dil0.tap1 K=128 N=128 splits=1 nsplit=2 reduce=one-stage',
    'conv1 K=64 N=32 splits=1 nsplit=2 reduce=one-stage | conv_skip K=64 N=64 splits=1 nsplit=2 reduce=one-stage | '
    'dil0.tap0 K=32 N=128 splits=1 nsplit=2 reduce=one-stage | dil0.tap1 K=32 N=128 splits=1 nsplit=2 reduce=one-stage',
    'conv1 K=32 N=64 splits=1 nsplit=2 reduce=one-stage | dil0.tap0 K=64 N=64 splits=1 nsplit=2 reduce=one-stage | '
    'dil0.tap1 K=64 N=64 splits=1 nsplit=2 reduce=one-stage | dil0.tap2 K=64 N=64 splits=1 nsplit=2 reduce=one-stage',
    'conv1 K=96 N=96 splits=1 nsplit=2 reduce=one-stage | conv_skip K=96 N=96 splits=1 nsplit=2 reduce=one-stage | '
    'dil0.tap0 K=96 N=192 splits=1 nsplit=2 reduce=one-stage | dil0.tap1 K=96 N=192 splits=1 nsplit=2 reduce=one-stage',
]


@pytest.mark.parametrize('shape,line', list(zip(LAYER_SHAPES, LAYER_LINES)), ids=[f'{s[0]}_{s[1]}' for s in LAYER_SHAPES])
def test_standalone_layer_products(lib, shape, line):
  R, D, S, dil, k, T = shape
  assert line == _line(R, D, S, k)                       # (the literal and the rule it was written from)
  rc, got = LD.describe(lib, LD.desc(R, D, S, k, [dil]), 2, T)
  assert rc == _lib.WN_OK and got == line
