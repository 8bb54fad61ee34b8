"""The kernels one residual block takes, forward and backward, as the library decides them (wnp::block_fwd_path and
wnp::block_bwd_path through wn_debug_block_paths), on plans made without a device.  The expected tokens are literal text,
worked out from the predicates as they stood in front of the launches of block_forward / block_backward and from what a
model pass binds for block 0 (block_ptrs, deep16_ptrs, FwdCall::blocks, TrainCall::chain_backward): if a predicate moves,
the GPU case tables keyed on these families would go on passing while covering another kernel, and this file fails first."""
import ctypes as C

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan
import test_rect_blocks_cpu as RB

FWD_KEYS = ['inner', 'gate']
BWD_KEYS = ['go', 'gu', 'gu_pad', 'gu_am', 'data', 'gx', 'drop']


@pytest.fixture(scope='module')
def lib():
  import os
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


def block_paths(lib, kw, cond_inputs, B, T, training):
  p = C.c_void_p(_plan(lib, _cfg(**kw), cond_inputs))
  assert p.value, lib.wn_last_error_string()
  try:
    buf = C.create_string_buffer(1024)
    assert lib.wn_debug_block_paths(p, B, T, training, buf, 1024) == _lib.WN_OK
  finally:
    lib.wn_plan_destroy(p)
  text = buf.value.decode()
  assert [t.split('=')[0] for t in text.split()] == FWD_KEYS + (BWD_KEYS if training else []), text
  return text


def exact(lib, fn):
  lib.wn_debug_set(1, 1)
  try:
    return fn()
  finally:
    lib.wn_debug_set(1, 0)


# ---- the eleven rect cases (tests/test_rect_blocks_cpu.py), depth 1 unless noted ----
# forward, split mode:
#  * no case binds F16n (R = D = 128 only) or F16d (R = D in {32, 64} at kernel size 2), so none is s128 / fused16;
#  * F16g (layers_per_block == 1, D % 64 == 0, m16(R), m32(R)): (64, 128), (128, 64), (64, 64) at k = 3 -> two contractions,
#    unless a conditioning bias is bound (r64_d128_cond: `!k.cb` fails, k.fused is false -> composed);
#  * the others have no image and no fused shape -> composed; r64_d32_lpb2 runs its inner conv on the fp32 rows GEMM (no
#    deep-stack images: R != D).
# forward, exact fp32 (knob 1): every split form declines; r64_k3 has the fused shape (64, 64, 3) -> fused32, the rest composed.
# backward, split mode (the per-block chain: no case has the pair / s128 shape, so g_x is formed here):
#  * folded nets hand g_fold with G16uf instead of g_skip -> gu=fold over (gxout, gfold);
#  * unfolded: G16u (m32(D), m16(R), m16(S)) -> image over (gxout, gskip); D = 32 has none -> fp32 (no slots);
#  * g_x: G16x (m32(R), m16(2D)) -> g16x; R = 32 / 48 have none -> exact fp32 publishing g_x's max-abs.
# backward, exact fp32: nothing folds, so the folded nets take their [W_r | W_s] image; block_backward has no knob-1 term
# of its own (Gemm::run sends an image-carrying contraction to the fp32 kernel), so the rest reads as in split mode.
def _t(gate, gu, gx, inner='none', data='none', pad=0):
  am = {'fold': 'gxout,gfold', 'image': 'gxout,gskip', 'pad': 'gxout,gskip', 'fp32': 'none,none'}[gu]
  return f'inner={inner} gate={gate}', f'go=xout gu={gu} gu_pad={pad} gu_am={am} data={data} gx={gx} drop=0'


SPLIT = {
    'r64_d128': _t('two', 'fold', 'g16x'),
    'r128_d64': _t('two', 'fold', 'g16x'),
    'r64_k3': _t('two', 'fold', 'g16x'),
    'r32_d64_fold': _t('composed', 'fold', 'fp32+absmax'),
    'r32_d64_sum': _t('composed', 'image', 'fp32+absmax'),
    'r64_d32': _t('composed', 'fp32', 'g16x'),
    'r96': _t('composed', 'image', 'g16x'),
    'r48_d64': _t('composed', 'image', 'fp32+absmax'),
    'r64_d128_cond': _t('composed', 'fold', 'g16x'),
    'r128_d64_mol': _t('two', 'fold', 'g16x'),
    'r64_d32_lpb2': _t('composed', 'fp32', 'fp32+absmax', inner='rows32', data='rows32'),
}
EXACT = {
    'r64_d128': _t('composed', 'image', 'g16x'),
    'r128_d64': _t('composed', 'image', 'g16x'),
    'r64_k3': _t('fused32', 'image', 'g16x'),
    'r32_d64_fold': _t('composed', 'image', 'fp32+absmax'),
    'r32_d64_sum': SPLIT['r32_d64_sum'],
    'r64_d32': SPLIT['r64_d32'],
    'r96': SPLIT['r96'],
    'r48_d64': SPLIT['r48_d64'],
    'r64_d128_cond': _t('composed', 'image', 'g16x'),
    'r128_d64_mol': _t('composed', 'image', 'g16x'),
    'r64_d32_lpb2': SPLIT['r64_d32_lpb2'],
}

# ---- one net each for the families the rect table does not reach ----
NETS = {
    'f16': RB._net(64, 64, 256, [128, 256]),
    's128': RB._net(128, 128, 256, [128, 256]),
    'deep64': RB._net(64, 64, 256, [128, 256], layers_per_block=3),
    'deep32': RB._net(32, 32, 64, [32], layers_per_block=2),
}
# f16 / s128 fold and have the pair / s128 backward shape (R = D, kernel size 2, F0 = 128): the chain forms g_x of block 0 in
# its pair launch (gx=none); in exact fp32 nothing folds, the chain is per block and both have the fused fp32 shape.
# deep64 / deep32 in a split-precision training pass bind the deep-stack images: 64- and 32-wide inner convs on the planes
# kernel both ways (taps * (plane_k / 16) >= 3), the [W_r | W_s] image padded to two row tiles, g_x on conv 0's image (at 32
# channels padded to two row tiles: the rows kernel with an image); F16d / F16r come from deep16_ptrs -> fused16.  Outside
# training passes and in exact fp32 nothing is bound: fp32 rows GEMMs and the fused fp32 kernel.
NET_SPLIT = {
    'f16': _t('fused16', 'fold', 'none'),
    's128': _t('s128', 'fold', 'none'),
    'deep64': _t('fused16', 'pad', 'deep', inner='planes,planes', data='planes,planes', pad=1),
    'deep32': _t('fused16', 'pad', 'deep', inner='planes', data='planes', pad=1),
}
NET_EXACT = {
    'f16': _t('fused32', 'image', 'g16x'),
    's128': _t('fused32', 'image', 'g16x'),
    'deep64': _t('fused32', 'fp32', 'fp32+absmax', inner='rows32,rows32', data='rows32,rows32'),
    'deep32': _t('fused32', 'fp32', 'fp32+absmax', inner='rows32', data='rows32'),
}
NET_EVAL = {'f16': 'inner=none gate=fused16', 's128': 'inner=none gate=s128',
            'deep64': 'inner=rows32,rows32 gate=fused32', 'deep32': 'inner=rows32 gate=fused32'}


def _both(lib, kw, cond_inputs, B, T):
  return block_paths(lib, kw, cond_inputs, B, T, 0), block_paths(lib, kw, cond_inputs, B, T, 1)


@pytest.mark.parametrize('name', list(RB.CASES))
def test_rect_cases_split_mode(lib, name):
  assert lib.wn_debug_value(1) == 0
  kw, cond_inputs = RB._kw(name)
  fwd, bwd = SPLIT[name]
  for B, T in RB.SIZES:
    assert _both(lib, kw, cond_inputs, B, T) == (fwd, fwd + ' ' + bwd), (name, B, T)


@pytest.mark.parametrize('name', list(RB.CASES))
def test_rect_cases_exact_fp32_mode(lib, name):
  kw, cond_inputs = RB._kw(name)
  fwd, bwd = EXACT[name]
  for B, T in RB.SIZES:
    assert exact(lib, lambda: _both(lib, kw, cond_inputs, B, T)) == (fwd, fwd + ' ' + bwd), (name, B, T)


def test_the_tables_cover_the_rect_cases():
  assert set(SPLIT) == set(EXACT) == set(RB.CASES) and len(RB.CASES) == 11


@pytest.mark.parametrize('name', list(NETS))
def test_the_other_families(lib, name):
  kw = NETS[name]
  fwd, bwd = NET_SPLIT[name]
  assert _both(lib, kw, 0, 2, 150) == (NET_EVAL[name], fwd + ' ' + bwd)
  fwd, bwd = NET_EXACT[name]
  assert exact(lib, lambda: _both(lib, kw, 0, 2, 150)) == (fwd, fwd + ' ' + bwd)


def test_every_family_is_reached():
  texts = [' '.join(t) for tab in (SPLIT, EXACT, NET_SPLIT, NET_EXACT) for t in tab.values()]
  for token in ('gate=s128', 'gate=two', 'gate=fused16', 'gate=fused32', 'gate=composed', 'inner=planes', 'inner=rows32',
                'gu=fold', 'gu=pad', 'gu=image', 'gu=fp32', 'data=planes', 'data=rows32', 'gx=none', 'gx=g16x', 'gx=deep',
                'gx=fp32+absmax'):
    assert any(token in t for t in texts), token


def test_describe_and_the_launch_disagree_on_the_conditioned_net(lib):
  """wn_plan_describe restates the dispatch at plan level: it sees the two-contraction images of r64_d128_cond, not that
  block_forward declines them for a bound conditioning bias (follow-ups)."""
  assert RB.describe(lib, 'r64_d128_cond')[1] == RB.FWD_TWO == RB.describe(lib, 'r64_d128')[1]
  kw, cond_inputs = RB._kw('r64_d128_cond')
  assert cond_inputs > 0
  assert block_paths(lib, kw, cond_inputs, 2, 150, 0) == 'inner=none gate=composed'
  kw, cond_inputs = RB._kw('r64_d128')
  assert block_paths(lib, kw, cond_inputs, 2, 150, 0) == 'inner=none gate=two'


def test_the_streamed_forward_across_its_32_bit_row_limit(lib):
  """wn_layer_fwd_s128 indexes activations with 32-bit byte offsets: B * T * R * 4 < 2^32, R = 128.  Beyond it the two
  split-precision contractions take over (their image is bound beside the streamed kernel's).  No memory is allocated."""
  kw = NETS['s128']
  assert block_paths(lib, kw, 0, 1, 2 ** 23 - 1, 0) == 'inner=none gate=s128'
  assert block_paths(lib, kw, 0, 1, 2 ** 23, 0) == 'inner=none gate=two'
  assert block_paths(lib, kw, 0, 8, 2 ** 20, 0) == 'inner=none gate=two'                       # B * T, not T
  assert block_paths(lib, kw, 0, 8, 2 ** 20 - 1, 0) == 'inner=none gate=s128'
  # training passes: the same limit; the s128 pair chain has given way to the per-block one long before (rows * 2D * 4 < 2^32)
  below, at = block_paths(lib, kw, 0, 1, 2 ** 23 - 1, 1), block_paths(lib, kw, 0, 1, 2 ** 23, 1)
  assert below == 'inner=none gate=s128 ' + _t('', 'fold', 'g16x')[1]
  assert at == 'inner=none gate=two ' + _t('', 'fold', 'g16x')[1]


def test_the_planes_form_of_the_inner_convs_across_its_row_limit(lib):
  """Planes::takes lists the operand width: rows * w * 4 < 2^32.  deep32: forward operand 32 wide, backward operand 2D = 64
  wide; beyond the limit the rows kernel runs on the same (padded) images."""
  kw = NETS['deep32']
  fwd, bwd = NET_SPLIT['deep32']
  assert block_paths(lib, kw, 0, 1, 2 ** 24 - 1, 1) == fwd + ' ' + bwd
  assert block_paths(lib, kw, 0, 1, 2 ** 24, 1) == fwd + ' ' + bwd.replace('data=planes', 'data=rows16')
  assert block_paths(lib, kw, 0, 1, 2 ** 25 - 1, 1) == fwd + ' ' + bwd.replace('data=planes', 'data=rows16')
  assert block_paths(lib, kw, 0, 2, 2 ** 24, 1) == fwd.replace('planes', 'rows16') + ' ' + bwd.replace('data=planes', 'data=rows16')


def test_argument_errors_follow_wn_debug_fwd_paths(lib):
  """Null plan, null buffer, len < 1: WN_E_INVALID.  A buffer too short gets the text truncated and terminated inside it
  and WN_OK, as wn_debug_fwd_paths does it."""
  kw, _ = RB._kw('r64_d128')
  p = C.c_void_p(_plan(lib, _cfg(**kw), 0))
  assert p.value
  try:
    buf = C.create_string_buffer(1024)
    assert lib.wn_debug_block_paths(None, 1, 1, 0, buf, 1024) == _lib.WN_E_INVALID == lib.wn_debug_fwd_paths(None, 1, 1, 0, 0, buf, 1024)
    assert lib.wn_debug_block_paths(p, 1, 1, 0, None, 1024) == _lib.WN_E_INVALID == lib.wn_debug_fwd_paths(p, 1, 1, 0, 0, None, 1024)
    assert lib.wn_debug_block_paths(p, 1, 1, 0, buf, 0) == _lib.WN_E_INVALID == lib.wn_debug_fwd_paths(p, 1, 1, 0, 0, buf, 0)
    assert lib.wn_debug_block_paths(p, 0, 1, 0, buf, 1024) == _lib.WN_E_INVALID == lib.wn_debug_fwd_paths(p, 0, 1, 0, 0, buf, 1024)
    assert lib.wn_debug_block_paths(p, 1, 0, 0, buf, 1024) == _lib.WN_E_INVALID == lib.wn_debug_fwd_paths(p, 1, 0, 0, 0, buf, 1024)
    for fn, args in ((lib.wn_debug_block_paths, (p, 2, 150, 1)), (lib.wn_debug_fwd_paths, (p, 2, 150, 1, 1))):
      assert fn(*args, buf, 1024) == _lib.WN_OK
      line = buf.value
      need = len(line) + 1
      short = C.create_string_buffer(b'\x7f' * need, need + 1)
      assert fn(*args, short, need - 1) == _lib.WN_OK                 # one byte short
      assert short.raw[:need - 2] == line[:need - 2] and short.raw[need - 2] == 0
      assert short.raw[need - 1] == 0x7f                              # nothing written past len
  finally:
    lib.wn_plan_destroy(p)
