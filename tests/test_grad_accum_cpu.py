"""CPU-only checks of Adam(gradient_accumulation_steps=k): the keyword and its errors, the export, signature and header text
of wn_grad_accumulate, every WN_E_INVALID of it (checked before the device is touched: the pointers handed over here would
fault if read), the known answers of tests/accum_reference.py (the restatement the GPU tests compare with bit for bit), and
the two checkpoint keys through io.save_weights / load_weights on plain arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import accum_reference as AC
from wavenets_amd import _lib


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_lib.LIB_PATH):
    _lib.build_library()
  return _lib.lib()


# ------------------------------------------------------------------------------------------
# Python surface
# ------------------------------------------------------------------------------------------
def test_keyword_defaults_and_acceptance():
  from wavenets_amd import Adam
  opt = Adam(clipnorm=1.0)
  assert opt.gradient_accumulation_steps is None and opt.accumulated == 0 and opt.accum is None and opt.updates_next()
  for k in (2, 3, 7, 64):
    opt = Adam(clipnorm=1.0, gradient_accumulation_steps=k)
    assert opt.gradient_accumulation_steps == k and opt.accumulated == 0 and opt.iterations == 0 and opt.accum is None
    assert not opt.updates_next()
  # every other keyword goes with it
  Adam(global_clipnorm=1.0, weight_decay=0.1, amsgrad=True, use_ema=True, ema_overwrite_frequency=1, gradient_accumulation_steps=2)
  Adam(clipvalue=0.5, gradient_accumulation_steps=2, clip_before_reduce=False)


@pytest.mark.parametrize('bad', [1, 0, -1, -2, True, False, 2.0, 3.5, '2', [2], (2,), float('nan'), float('inf')])
def test_keyword_rejects_everything_but_none_and_an_int_of_two_or_more(bad):
  from wavenets_amd import Adam
  with pytest.raises(ValueError, match='gradient_accumulation_steps'):
    Adam(gradient_accumulation_steps=bad)


def test_keyword_with_clip_before_reduce_names_both():
  from wavenets_amd import Adam
  for kw in (dict(clipnorm=1.0), dict(global_clipnorm=1.0), dict(clipvalue=1.0), dict()):
    with pytest.raises(ValueError) as e:
      Adam(gradient_accumulation_steps=2, clip_before_reduce=True, **kw)
    assert 'gradient_accumulation_steps' in str(e.value) and 'clip_before_reduce' in str(e.value)


def test_undo_restores_the_pair_and_is_the_old_decrement_without_the_keyword():
  from wavenets_amd import Adam
  opt = Adam()
  opt.iterations, opt._before = 5, (4, 0)             # what apply_gradients leaves behind without the keyword
  opt.undo_last_apply()
  assert (opt.iterations, opt.accumulated) == (4, 0)
  opt = Adam(gradient_accumulation_steps=3)
  opt.iterations, opt.accumulated, opt._before = 2, 0, (1, 2)      # after the final micro-step of a cycle
  opt.undo_last_apply()
  assert (opt.iterations, opt.accumulated) == (1, 2) and opt.updates_next()
  opt.iterations, opt.accumulated, opt._before = 1, 2, (1, 1)      # after a storing one
  opt.undo_last_apply()
  assert (opt.iterations, opt.accumulated) == (1, 1) and not opt.updates_next()


def test_driver_default_holds_the_key():
  import importlib
  train = importlib.import_module('train')
  assert train.config['gradient_accumulation_steps'] is None


# ------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared(lib):
  P = C.c_void_p
  assert _lib._SIGS['wn_grad_accumulate'] == (C.c_int, [P, P, C.c_int64, C.c_int32, C.c_int32, P, P])
  assert 'wn_grad_accumulate' in _lib.EXPORTS and lib.wn_grad_accumulate.restype is C.c_int
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  with open(os.path.join(root, 'include', 'wn_hip.h')) as f:
    text = f.read()
  assert ('int wn_grad_accumulate(float* acc, float* grads, int64_t n, int32_t mode, int32_t steps, const float* skip_flag, '
          'void* stream);') in text
  for name in ('WN_ACCUM_FIRST', 'WN_ACCUM_ADD', 'WN_ACCUM_FINISH', 'WN_ACCUM_ONE_PASS'):
    assert int(re.search(rf'#define {name} (\d+)', text).group(1)) == getattr(_lib, name)
  assert (AC.FIRST, AC.ADD, AC.FINISH) == (_lib.WN_ACCUM_FIRST, _lib.WN_ACCUM_ADD, _lib.WN_ACCUM_FINISH)
  # the semantics are restated where the issue asks for them
  for words in ('acc = g ', 'acc = acc + g', 'g = (g + acc) / (float)steps', 'OVERWRITES', 'skip_flag != 0', 'counts updates'):
    assert words in text, words
  with open(os.path.join(root, 'wavenets_amd', 'csrc', 'wn_kernels.h')) as f:
    assert 'int wn_launch_grad_accumulate(float* acc, float* g, int64_t n, int mode, float steps' in f.read()
  import wavenets_amd.optim as optim
  for words in ('gradient_accumulation_steps=k', '(g_k + acc) / k', 'UPDATES', 'accumulated', 'overwrites'):
    assert words in optim.__doc__, words


BAD = 0x10           # an address in the zero page: reading or writing it faults


def _invalid(lib, rc, word):
  assert rc == _lib.WN_E_INVALID
  msg = lib.wn_last_error_string().decode()
  assert 'grad_accumulate' in msg and word in msg, msg


def test_null_buffers_are_invalid(lib):
  for mode in (AC.FIRST, AC.ADD, AC.FINISH):
    _invalid(lib, lib.wn_grad_accumulate(None, BAD, 8, mode, 2, None, None), 'acc is NULL')
    _invalid(lib, lib.wn_grad_accumulate(BAD, None, 8, mode, 2, None, None), 'grads is NULL')
    _invalid(lib, lib.wn_grad_accumulate(None, None, 8, mode, 2, BAD, None), 'acc is NULL')


@pytest.mark.parametrize('n', [-1, -4, -2 ** 31, -2 ** 40])
def test_negative_count_is_invalid(lib, n):
  _invalid(lib, lib.wn_grad_accumulate(BAD, BAD, n, AC.ADD, 2, BAD, None), 'n must be >= 0')


@pytest.mark.parametrize('mode', [-1, 3, 4, 7, 256, -2 ** 31])
def test_unknown_mode_is_invalid(lib, mode):
  _invalid(lib, lib.wn_grad_accumulate(BAD, BAD, 8, mode, 2, BAD, None), 'mode')


@pytest.mark.parametrize('steps', [1, 0, -1, -2 ** 31])
def test_finish_with_fewer_than_two_steps_is_invalid(lib, steps):
  _invalid(lib, lib.wn_grad_accumulate(BAD, BAD, 8, AC.FINISH, steps, BAD, None), 'steps must be >= 2')


def test_empty_buffers_are_ok_without_a_launch(lib):
  """n == 0 returns before the launch, in every mode, whatever steps says in the storing modes: nothing here could run a
  kernel (the test machine may have no device at all) and the pointers are never read."""
  for mode, steps in ((AC.FIRST, 0), (AC.ADD, -5), (AC.FINISH, 2), (AC.FINISH, 7)):
    assert lib.wn_grad_accumulate(BAD, BAD, 0, mode, steps, BAD, None) == _lib.WN_OK


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def f32(*v):
  return np.array(v, dtype=np.float32)


def test_reference_three_modes_by_hand():
  g1, g2, g3 = f32(1.0, -2.0, 0.5), f32(0.25, 2.0, 0.5), f32(1.75, 3.0, 0.5)
  acc, g = AC.accumulate(f32(9.0, 9.0, np.nan), g1, AC.FIRST)          # an overwrite: the stale NaN is gone
  assert acc.tolist() == [1.0, -2.0, 0.5] and g.tolist() == g1.tolist()
  acc, g = AC.accumulate(acc, g2, AC.ADD)
  assert acc.tolist() == [1.25, 0.0, 1.0] and g.tolist() == g2.tolist()
  acc2, g = AC.accumulate(acc, g3, AC.FINISH, 3)
  assert acc2.tolist() == acc.tolist()                                 # FINISH leaves the accumulator alone
  assert g.tolist() == [1.0, 1.0, 0.5]
  assert AC.cycle_mean([g1, g2, g3]).tolist() == [1.0, 1.0, 0.5]
  assert AC.mean64([g1, g2, g3]).tolist() == [1.0, 1.0, 0.5]
  assert acc.dtype == g.dtype == np.float32 and AC.mean64([g1, g2]).dtype == np.float64


def test_reference_rounds_once_per_operation_in_fp32():
  """(1 + 2^-24) is a tie that fp32 rounds to 1; fp64 keeps it.  1/3 and 1/7 are inexact: the quotient is the fp32
  division, not the fp64 one rounded and not a product with a rounded reciprocal."""
  one, tiny = f32(1.0), f32(2.0 ** -24)
  assert AC.cycle_mean([one, tiny])[0] == np.float32(0.5)              # (tiny + 1) -> 1, / 2
  assert AC.mean64([one, tiny])[0] == (1.0 + 2.0 ** -24) / 2.0
  # the order is (g_k + acc): acc = 1 + tiny -> 1, then + tiny -> 1 again; fp64 sees both
  assert AC.cycle_mean([one, tiny, tiny])[0] == np.float32(1.0) / np.float32(3.0)
  assert AC.mean64([one, tiny, tiny])[0] == (1.0 + 2.0 ** -23) / 3.0
  for k in (3, 7):
    x = f32(5.0)
    got = AC.accumulate(f32(0.0), x, AC.FINISH, k)[1][0]
    assert got == np.float32(5.0) / np.float32(k)
    assert float(got) == float(np.float32(5.0 / k))                    # one division of two floats: double rounding is exact
  # a product with the rounded reciprocal is another float: 5 / 3 and 3 / 7 tell the two apart
  for x, k in ((5.0, 3), (3.0, 7)):
    assert np.float32(x) * (np.float32(1.0) / np.float32(k)) != np.float32(x) / np.float32(k)
    assert AC.accumulate(f32(0.0), f32(x), AC.FINISH, k)[1][0] == np.float32(x) / np.float32(k)


def test_reference_specials():
  inf, nan = np.inf, np.nan
  g1 = f32(0.0, -0.0, inf, inf, nan, 1.0, -0.0)
  g2 = f32(-0.0, -0.0, 1.0, -inf, 1.0, nan, 0.0)
  m = AC.cycle_mean([g1, g2])
  assert m[0] == 0.0 and not np.signbit(m[0])                          # -0 + 0 = +0
  assert m[1] == 0.0 and np.signbit(m[1])                              # -0 + -0 = -0, / 2 keeps the sign
  assert m[2] == inf and np.isnan(m[3]) and np.isnan(m[4]) and np.isnan(m[5])
  assert m[6] == 0.0 and not np.signbit(m[6])
  assert AC.same_bits(m, m.copy()) and AC.same_bits(f32(nan), f32(-nan))
  assert not AC.same_bits(f32(0.0), f32(-0.0)) and not AC.same_bits(f32(1.0, 2.0), f32(1.0))
  assert not AC.same_bits(f32(nan, 1.0), f32(1.0, nan))


# ------------------------------------------------------------------------------------------
# checkpoints, on plain arrays
# ------------------------------------------------------------------------------------------
class _Model:
  """What io.save_weights / load_weights touch of a model, on the host."""

  def __init__(self, seed):
    rng = np.random.RandomState(seed)
    self.variable_names = ['causal/kernel', 'causal/bias']
    self.w = [rng.randn(2, 1, 4).astype(np.float32), rng.randn(4).astype(np.float32)]
    self.flat_params = torch.nn.Parameter(torch.from_numpy(np.concatenate([w.reshape(-1) for w in self.w])))

  def get_weights(self):
    return [w.copy() for w in self.w]

  def set_weights(self, ws):
    self.w = [np.array(w) for w in ws]


def _saved(tmp_path, name, k, held, seed=0):
  from wavenets_amd import Adam, io
  model = _Model(seed)
  opt = Adam(gradient_accumulation_steps=k)
  opt.build(model)
  gen = torch.Generator().manual_seed(seed)
  assert opt.accum is not None and opt.accum.shape == opt.m.shape and opt.accum.dtype == torch.float32
  opt.accum.copy_(torch.randn(opt.accum.shape, generator=gen))
  opt.m.copy_(torch.randn(opt.m.shape, generator=gen))
  opt.iterations, opt.accumulated = 4, held
  path = str(tmp_path / name)
  io.save_weights(model, path, opt)
  return model, opt, path


def test_checkpoint_round_trip_of_the_accumulator(tmp_path):
  from wavenets_amd import Adam, io
  model, opt, path = _saved(tmp_path, 'a.weights.npz', 3, 2)
  with np.load(path) as d:
    assert np.array_equal(d['adam_accum'], opt.accum.numpy()) and d['adam_accum'].dtype == np.float32
    assert int(d['adam_accumulated']) == 2 and int(d['adam_iterations']) == 4
  back = Adam(gradient_accumulation_steps=3)
  io.load_weights(_Model(1), path, back)
  assert (back.iterations, back.accumulated) == (4, 2)
  assert torch.equal(back.accum, opt.accum) and torch.equal(back.m, opt.m)
  # a wider cycle takes it too: 2 micro-steps held of 5
  wider = Adam(gradient_accumulation_steps=5)
  io.load_weights(_Model(1), path, wider)
  assert wider.accumulated == 2 and torch.equal(wider.accum, opt.accum)


def test_checkpoint_without_the_keys_loads_as_a_fresh_cycle(tmp_path):
  from wavenets_amd import Adam, io
  model = _Model(0)
  plain = Adam()
  plain.build(model)
  assert plain.accum is None                                           # allocated only with the keyword
  plain.iterations = 6
  path = str(tmp_path / 'b.weights.npz')
  io.save_weights(model, path, plain)
  with np.load(path) as d:
    assert 'adam_accum' not in d and 'adam_accumulated' not in d
  opt = Adam(gradient_accumulation_steps=2)
  opt.accumulated = 1                                                  # whatever it held before the load
  io.load_weights(_Model(1), path, opt)
  assert (opt.iterations, opt.accumulated) == (6, 0) and opt.accum is not None


def test_stored_accumulator_is_ignored_without_the_keyword(tmp_path):
  from wavenets_amd import Adam, io
  model, opt, path = _saved(tmp_path, 'c.weights.npz', 2, 1)
  plain = Adam()
  io.load_weights(_Model(1), path, plain)
  assert plain.accum is None and plain.accumulated == 0 and plain.iterations == 4 and torch.equal(plain.m, opt.m)


@pytest.mark.parametrize('k,held', [(2, 2), (2, 3), (3, 3), (3, 6)])
def test_stored_count_of_a_whole_cycle_or_more_is_an_error(tmp_path, k, held):
  from wavenets_amd import Adam, io
  model, opt, path = _saved(tmp_path, 'd.weights.npz', 7, held)
  with pytest.raises(ValueError, match='adam_accumulated'):
    io.load_weights(_Model(1), path, Adam(gradient_accumulation_steps=k))
