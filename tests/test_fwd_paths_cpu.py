"""The kernel paths of a forward pass as the library decides them (wnp::fwd_paths through wn_debug_fwd_paths), on plans made
without a device, against the Python restatement the GPU tests select their cases with: route() of
tests/test_gpu_head_tile_walk.py.  If the C++ moves and route() does not, the case tables of that file and of
tests/test_gpu_sample_weight.py would go on passing while their tests cover another kernel; here the two are compared."""
import ctypes as C

import pytest

from wavenets_amd import _lib
from test_cabi_cpu import _cfg, _plan
import test_gpu_head_tile_walk as HW
import test_gpu_sample_weight as SW


@pytest.fixture(scope='module')
def lib():
  import os
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


def _cases():
  """(id, constructor keywords, cond_inputs, B, T): every entry of the two case tables at its file's batch."""
  out = []
  for case, kw in HW.CASES.items():
    kw = HW._full(kw)
    out.append(('head_tile_walk/' + case, kw, HW.B if kw.get('conditioning') else 0, HW.B, HW.T))
  for case in SW.NETS:
    kw = dict(SW._kw(case))
    cond_inputs = kw.pop('cond_inputs', 0)
    out.append(('sample_weight/' + case, HW._full(kw), cond_inputs, SW.B, SW.T))
  return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def paths(lib, kw, cond_inputs, B, T, training=1, loss=1):
  p = C.c_void_p(_plan(lib, _cfg(**kw), cond_inputs))
  assert p.value, lib.wn_last_error_string()
  try:
    buf = C.create_string_buffer(1024)
    assert lib.wn_debug_fwd_paths(p, B, T, training, loss, buf, 1024) == _lib.WN_OK
  finally:
    lib.wn_plan_destroy(p)
  tokens = dict(t.split('=') for t in buf.value.decode().split())
  assert list(tokens) == ['cond', 'conv_cond', 'inconv', 'zfill', 'fold', 'prep', 'drop', 'deep16', 'skip', 'first_final', 'hc0',
                          'head'], buf.value
  tokens['head'] = tokens['head'].split(',')
  return tokens


def reduced(route):
  """route() in the vocabulary of wn_debug_fwd_paths: (skip token, head tokens).  The trailing name of a standalone loss
  kernel is not part of the forward pass."""
  skip, head = 'none', []
  for i, r in enumerate(route):
    if r.startswith('fold planes16s'):
      assert i == 0
      skip = 'folded/planes'
    elif r.startswith('fold rows'):
      assert i == 0
      skip = 'folded/rows'
    elif r.startswith('skip '):
      assert i == 0
      skip = 'sum'
    elif r.startswith('planes16s<'):
      head.append('planes')
    elif r.startswith('epilogue'):
      head.append('epilogue')
    elif r.startswith('rows'):
      head.append('rows')
    else:
      assert i == len(route) - 1 and r.startswith('wn_') and r.endswith('_kernel'), route
  return skip, head


def test_the_vocabulary_reduction_on_the_recorded_routes():
  assert reduced(HW.ROUTES['r64_head256']) == ('folded/planes', ['planes', 'epilogue'])
  assert reduced(HW.ROUTES['r64_wide_unfolded']) == ('sum', ['planes', 'rows', 'epilogue'])
  assert reduced(HW.ROUTES['r32_odd_widths']) == ('sum', ['rows', 'rows', 'rows'])
  assert reduced(HW.ROUTES['r32_noskip']) == ('none', ['rows', 'epilogue'])
  assert reduced(['fold rows16<4> x 1 column blocks', 'wn_mix_loss_kernel']) == ('folded/rows', [])
  assert len(CASES) == len(HW.CASES) + len(SW.NETS)


@pytest.mark.parametrize('case,kw,cond_inputs,B,T', CASES, ids=IDS)
def test_split_mode_paths_are_the_ones_route_states(lib, case, kw, cond_inputs, B, T):
  """A training pass that wants the loss epilogue: what route() describes."""
  assert lib.wn_debug_value(1) == 0
  got = paths(lib, kw, cond_inputs, B, T)
  skip, head = reduced(HW.route({k: v for k, v in kw.items()}))
  assert (got['skip'], got['head']) == (skip, head), (case, got)
  assert got['fold'] == ('1' if skip.startswith('folded') else '0')
  assert got['first_final'] == got['fold'] and got['drop'] == '0'
  assert (got['cond'] == 'none') == (cond_inputs == 0) == (got['conv_cond'] == 'none')
  assert got['inconv'] == ('elementwise' if kw['channels'] % 4 == 0 else 'rows')
  # the 32-bit row limits are not reached at the batches of the two files: a small call decides the same
  assert paths(lib, kw, cond_inputs, 1, 1024) == got, case


@pytest.mark.parametrize('case,kw,cond_inputs,B,T', CASES, ids=IDS)
def test_exact_fp32_mode_takes_no_split_precision_path(lib, case, kw, cond_inputs, B, T):
  lib.wn_debug_set(1, 1)
  try:
    got = paths(lib, kw, cond_inputs, B, T)
  finally:
    lib.wn_debug_set(1, 0)
  assert got['fold'] == '0' and not got['skip'].startswith('folded'), (case, got)
  assert 'planes' not in got['head'] and 'epilogue' not in got['head'], (case, got)
  assert got['inconv'] == 'rows' and got['deep16'] == '0' and got['prep'] in ('none', 'inline'), (case, got)
  assert got['skip'] == ('sum' if kw.get('use_skip', True) else 'none')


def test_the_loss_epilogue_only_where_the_caller_wants_it(lib):
  kw, B, T = HW._full(SW._kw('cat_r64')), SW.B, SW.T
  train = paths(lib, kw, 0, B, T, training=1, loss=1)
  assert train['head'] == ['planes', 'epilogue']
  none = paths(lib, kw, 0, B, T, training=1, loss=0)
  assert none['head'] == ['planes', 'planes']                      # want_pred: the logits are written
  assert {k: v for k, v in none.items() if k != 'head'} == {k: v for k, v in train.items() if k != 'head'}
  assert paths(lib, kw, 0, B, T, training=0, loss=0)['head'] == ['planes', 'planes']          # logits, call, test_step
  assert paths(lib, kw, 0, B, T, training=0, loss=2)['head'] == ['planes', 'epilogue']        # score
  # a head the epilogue does not fit keeps its kernels whatever the caller wants
  small = HW._full(SW._kw('cat_small_fused'))
  assert paths(lib, small, 0, B, T, loss=1) == paths(lib, small, 0, B, T, loss=0)
  buf = C.create_string_buffer(64)
  assert lib.wn_debug_fwd_paths(None, 1, 1, 0, 0, buf, 64) == _lib.WN_E_INVALID


def test_deep_stacks_bind_their_split_images_in_training_passes_only(lib):
  kw = HW._full(SW._kw('cat_lpb2_r64'))
  assert paths(lib, kw, 0, SW.B, SW.T, training=1)['deep16'] == '1'
  assert paths(lib, kw, 0, SW.B, SW.T, training=0, loss=0)['deep16'] == '0'


def test_the_paths_depend_on_the_call_across_each_32_bit_row_limit(lib):
  """The planes kernel indexes rows with 32-bit byte offsets; every site keeps the terms it had.
  r64_head256: Z planes of 64 columns -> 128 (folded), 128 -> 256 (planes), 256 -> 256 (epilogue).  Pairs of calls that differ
  in B * T alone."""
  kw = HW._full(HW.CASES['r64_head256'])

  def at(T, B=1):
    got = paths(lib, kw, 0, B, T)
    return got['skip'], got['head']
  small = at(1024)
  assert small == ('folded/planes', ['planes', 'epilogue'])
  assert at(2 ** 23 + 1) == ('folded/rows', ['rows', 'rows']) != small
  # each term on its own: rows * width * 4 < 2^32
  assert at(2 ** 22 - 1) == small
  assert at(2 ** 22) == ('folded/planes', ['planes', 'rows'])            # the last conv's 256-wide operand
  assert at(2 ** 23 - 1) == ('folded/planes', ['planes', 'rows'])
  assert at(2 ** 23) == ('folded/rows', ['rows', 'rows'])                # the 128-wide operand; the fold's 128-wide OUTPUT
  assert at(2 ** 21, B=2) == at(2 ** 22) and at(2 ** 20, B=8) == at(2 ** 23)                   # B * T, not T
  # everything but the planes sites is the same on both sides of every limit
  a, b = paths(lib, kw, 0, 1, 1024), paths(lib, kw, 0, 1, 2 ** 23 + 1)
  assert {k: v for k, v in a.items() if k not in ('skip', 'head')} == {k: v for k, v in b.items() if k not in ('skip', 'head')}
  # a net without a planes site does not depend on the call
  small_net = HW._full(SW._kw('cat_small_fused'))
  assert paths(lib, small_net, 0, 1, 1024) == paths(lib, small_net, 0, 1, 2 ** 23 + 1)
