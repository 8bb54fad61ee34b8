"""wn_layer_describe through the C-ABI, without a device: the weight-gradient products of wn_layer_bwd, their time split and
the form of their reduce, as the launch path's own functions decide them.  tests/test_gpu_layer_backward.py asserts on this
line that its many-split cases reach the two-stage reduce; here the line itself is checked against shapes worked out by hand
from wn_wgrad_choose_splits (a 64 x 128 tile per job, 1024 waves wanted, at least 256 rows a split) and the reduce's
threshold (two stages above 32 splits)."""
import ctypes as C

import pytest

from wavenets_amd import _lib


@pytest.fixture(scope='module')
def lib():
  import os
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


def desc(R, D, S, KS, dil, cin=None, Cc=0, act=None, residual=True):
  d = _lib.WnLayerDesc()
  d.kernel_size, d.channels, d.dilation_channels, d.skip_channels = KS, R, D, S or 0
  d.depth = len(dil)
  for i, r in enumerate(dil[:16]):
    d.dilations[i] = r
  d.activation, d.residual, d.cond_channels = _lib.ACTIVATIONS[act], int(residual), Cc
  d.in_channels = R if cin is None else cin
  return d


def describe(lib, d, B, T, n=4096):
  buf = C.create_string_buffer(n)
  rc = lib.wn_layer_describe(C.byref(d), B, T, buf, n)
  return rc, buf.value.decode()


def parse(line):
  """[(name, {K, N, splits, nsplit}, reduce)] of a describe line."""
  out = []
  for item in line.split(' | '):
    name, *toks = item.split()
    kv = dict(t.split('=') for t in toks)
    assert list(kv) == ['K', 'N', 'splits', 'nsplit', 'reduce'], item
    out.append((name, {k: int(kv[k]) for k in ('K', 'N', 'splits', 'nsplit')}, kv['reduce']))
  return out


def test_many_splits_by_hand(lib):
  """64 / 64 / 256, B = 3, T = 2900: every product is one or two 64 x 128 jobs, so 512 to 1024 splits are wanted and the cap
  ceil(2900 / 256) = 12 per utterance decides: nsplit = 36 > 32, two stages."""
  rc, line = describe(lib, desc(64, 64, 256, 2, [512]), 3, 2900)
  assert rc == _lib.WN_OK
  two = 'splits=12 nsplit=36 reduce=two-stage'
  assert line == (f'conv1 K=64 N=64 {two} | conv_skip K=64 N=256 {two} | dil0.tap0 K=64 N=128 {two} | '
                  f'dil0.tap1 K=64 N=128 {two}')


def test_small_composed_layer_by_hand(lib):
  """16 / 24 / 40 with a stack of two, one input channel and a five-channel condition at T = 77: one split an utterance."""
  rc, line = describe(lib, desc(16, 24, 40, 2, [2, 1], cin=1, Cc=5, act='tanh', residual=False), 2, 77)
  assert rc == _lib.WN_OK
  one = 'splits=1 nsplit=2 reduce=one-stage'
  assert line == (f'conv1 K=24 N=16 {one} | conv_skip K=24 N=40 {one} | conv_cond K=5 N=48 {one} | '
                  f'dil1.tap0 K=24 N=48 {one} | dil1.tap1 K=24 N=48 {one} | dil0.tap0 K=1 N=24 {one} | dil0.tap1 K=1 N=24 {one}')


def test_wanted_waves_decide_below_the_row_cap(lib):
  """128 / 128 / 256, B = 16, T = 16000 (cap 63): conv1 is 2 jobs -> 512 wanted -> 32 an utterance; conv_skip and the gated conv
  are 4 jobs -> 256 wanted -> 16 an utterance.  Three taps, no condition."""
  rc, line = describe(lib, desc(128, 128, 256, 3, [4]), 16, 16000)
  assert rc == _lib.WN_OK
  got = parse(line)
  assert [g[0] for g in got] == ['conv1', 'conv_skip', 'dil0.tap0', 'dil0.tap1', 'dil0.tap2']
  assert got[0][1:] == (dict(K=128, N=128, splits=32, nsplit=512), 'two-stage')
  for g in got[1:]:
    assert g[1:] == (dict(K=128, N=256, splits=16, nsplit=256), 'two-stage')


def test_the_reduce_threshold_is_the_launch_paths(lib):
  """One utterance: the cap ceil(T / 256) is nsplit.  32 splits reduce in one stage, 33 in two."""
  d = desc(128, 128, 256, 2, [16])
  for T, n, form in ((8192, 32, 'one-stage'), (8193, 33, 'two-stage'), (8300, 33, 'two-stage')):
    rc, line = describe(lib, d, 1, T)
    assert rc == _lib.WN_OK
    for name, kv, red in parse(line):
      assert (kv['splits'], kv['nsplit'], red) == (n, n, form), (T, name)


def test_bad_descriptor_and_short_buffer(lib):
  good = desc(32, 32, 64, 2, [8], Cc=5)
  rc, line = describe(lib, good, 2, 257)
  assert rc == _lib.WN_OK and line.startswith('conv1 K=32 N=32 splits=2 nsplit=4 reduce=one-stage | ')
  for bad in (desc(32, 32, 64, 4, [8]), desc(32, 32, 64, 1, [8]), desc(32, 32, 64, 2, []), desc(32, 32, 64, 2, [1] * 17),
              desc(0, 0, 64, 2, [8])):
    buf = C.create_string_buffer(b'x' * 63, 64)
    assert lib.wn_layer_describe(C.byref(bad), 2, 257, buf, 64) == _lib.WN_E_INVALID
    assert buf.value == b''
    assert b'bad descriptor' in lib.wn_last_error_string()
  buf = C.create_string_buffer(4096)
  assert lib.wn_layer_describe(None, 2, 257, buf, 4096) == _lib.WN_E_INVALID
  assert lib.wn_layer_describe(C.byref(good), 0, 257, buf, 4096) == _lib.WN_E_INVALID
  assert lib.wn_layer_describe(C.byref(good), 2, 0, buf, 4096) == _lib.WN_E_INVALID
  assert lib.wn_layer_describe(C.byref(good), 2, 257, None, 4096) == _lib.WN_E_INVALID
  assert lib.wn_layer_describe(C.byref(good), 2, 257, buf, 0) == _lib.WN_E_INVALID
  # a buffer one byte short: WN_E_INVALID naming the bytes needed, the text truncated and terminated inside the buffer
  need = len(line) + 1
  short = C.create_string_buffer(b'\x7f' * need, need + 1)
  assert lib.wn_layer_describe(C.byref(good), 2, 257, short, need - 1) == _lib.WN_E_INVALID
  assert str(need).encode() in lib.wn_last_error_string()
  assert short.raw[:need - 2] == line.encode()[:need - 2] and short.raw[need - 2] == 0
  assert short.raw[need - 1] == 0x7f                             # nothing written past len
  exact = C.create_string_buffer(need)
  assert lib.wn_layer_describe(C.byref(good), 2, 257, exact, need) == _lib.WN_OK and exact.value.decode() == line
