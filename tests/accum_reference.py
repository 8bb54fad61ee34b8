"""Gradient accumulation restated on the host (not a test module): what ``wn_grad_accumulate`` and
``Adam(gradient_accumulation_steps=k)`` compute, in the order include/wn_hip.h fixes, and the fp64 mean beside it.

fp32, one correctly rounded operation per element, nothing fused:
    acc = g_1;   acc = acc + g_j  (j = 2 .. k-1);   mean = (g_k + acc) / (float)k
numpy's float32 add and divide are IEEE operations, so the restatement is exact and a device result can be compared with it
bit for bit (NaN payloads aside: the tests compare a NaN as a NaN)."""
import numpy as np

FIRST, ADD, FINISH = 0, 1, 2          # WN_ACCUM_* of include/wn_hip.h


def _f32(x):
  x = np.asarray(x)
  assert x.dtype == np.float32, x.dtype
  return x


def accumulate(acc, g, mode, steps=None):
  """One call of wn_grad_accumulate: returns the new (acc, g) as fresh fp32 arrays; ``acc`` may be None in FIRST."""
  g = _f32(g)
  with np.errstate(all='ignore'):
    if mode == FIRST:
      return g.copy(), g.copy()
    acc = _f32(acc)
    if mode == ADD:
      return (acc + g).astype(np.float32), g.copy()
    if mode == FINISH:
      assert isinstance(steps, int) and steps >= 2
      return acc.copy(), ((g + acc) / np.float32(steps)).astype(np.float32)
  raise ValueError(mode)


def cycle_mean(grads):
  """The mean that reaches Adam after a cycle of ``len(grads)`` micro-steps, fp32 in the device's order."""
  k = len(grads)
  assert k >= 2
  acc, _ = accumulate(None, grads[0], FIRST)
  for g in grads[1:-1]:
    acc, _ = accumulate(acc, g, ADD)
  return accumulate(acc, grads[-1], FINISH, k)[1]


def mean64(grads):
  """The same mean in fp64 (sum in list order, one division)."""
  total = np.zeros(np.asarray(grads[0]).shape, dtype=np.float64)
  with np.errstate(all='ignore'):
    for g in grads:
      total = total + np.asarray(g, dtype=np.float64)
    return total / float(len(grads))


def same_bits(a, b):
  """Equal bit for bit, except that any NaN equals any NaN."""
  a, b = _f32(a), _f32(b)
  if a.shape != b.shape:
    return False
  na, nb = np.isnan(a), np.isnan(b)
  return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
