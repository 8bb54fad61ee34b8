"""One step of Adam with the Keras keywords, restated in numpy fp64 (Keras 3 base_optimizer.py / adam.py), for the tests of
global_clipnorm, clipvalue, weight_decay and amsgrad.  Not a test module: tests/test_adam_options_cpu.py holds its known
answers, tests/test_gpu_adam_options.py compares the kernels with it.

Everything the kernel is handed as fp32 enters here as that fp32 value, widened: the state, the gradient, lr, the betas,
epsilon, the clip value, the decay, and alpha (formed on the host in double and handed over as a float).  From there on
every operation is fp64, so the result is the exact value of the specified expressions up to ~1e-16 relative.

  g'    = g * c / max(||g_t||, c)                per tensor                       (clipnorm)
        = g * (c / max(N, c) + (N - N))          N the norm of the whole gradient (global_clipnorm; N - N poisons with NaN)
        = g < -c ? -c : (g > c ? c : g)          NaN stays NaN                    (clipvalue)
  p0    = p - (p * wd) * lr                      on tensors that decay            (weight_decay)
  m     = m + (g' - m) * (1 - beta_1)
  v     = v + (g' g' - v) * (1 - beta_2)
  vhat  = max(vhat, v)                                                            (amsgrad)
  p     = p0 - alpha * m / (sqrt(v or vhat) + eps),   alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t)
  ema   = p at t == 1, else ema + (p - ema) * (1 - momentum);  p = ema when the step overwrites           (use_ema)
"""
import math

import numpy as np

U = 2.0 ** -24                        # unit roundoff of fp32


def f32(x):
  """The fp32 value the kernel is handed, as a double."""
  return float(np.float32(x))


def alpha_of(lr, beta_1, beta_2, t):
  lr, b1, b2 = f32(lr), f32(beta_1), f32(beta_2)
  return f32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def clip_factors(g, tensors, clipnorm=None, global_clipnorm=None):
  """Per tensor of ``tensors`` [(offset, length)]: the factor its gradient is multiplied with."""
  g = np.asarray(g, dtype=np.float64)
  n2 = [float(np.sum(g[o:o + n] ** 2)) for o, n in tensors]
  if clipnorm:
    c = f32(clipnorm)
    return [c / max(math.sqrt(s), c) for s in n2]
  if global_clipnorm:
    c = f32(global_clipnorm)
    with np.errstate(invalid='ignore'):
      N = float(np.sqrt(np.float64(sum(n2))))
    if not math.isfinite(N):
      return [float('nan')] * len(tensors)
    return [c / max(N, c)] * len(tensors)
  return [1.0] * len(tensors)


def clip(g, tensors, clipnorm=None, global_clipnorm=None, clipvalue=None):
  """The clipped gradient g' (fp64) of a flat fp32 gradient."""
  g = np.asarray(g, dtype=np.float64)
  if clipvalue:
    c = f32(clipvalue)
    return np.where(g < -c, -c, np.where(g > c, c, g))      # a NaN compares false twice and stays
  out = g.copy()
  for (o, n), s in zip(tensors, clip_factors(g, tensors, clipnorm, global_clipnorm)):
    if s != 1.0:
      with np.errstate(invalid='ignore'):
        out[o:o + n] = g[o:o + n] * s
  return out


def adam_step(p, m, v, vhat, g, t, tensors, *, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None,
              global_clipnorm=None, clipvalue=None, weight_decay=None, decays=None, amsgrad=False, ema=None,
              ema_momentum=0.99, ema_overwrite=False):
  """One step.  p, m, v, g (and vhat, ema where used): flat arrays holding fp32 values; tensors: [(offset, length)];
  decays: per tensor, None = all.  Returns a dict of fp64 arrays p, m, v, vhat, ema, g (the clipped gradient), p_step (the p
  of the update, before an overwrite by the average) and the float alpha."""
  p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
  b1, b2, eps, lr32 = f32(beta_1), f32(beta_2), f32(epsilon), f32(lr)
  alpha = alpha_of(lr, beta_1, beta_2, t)
  gc = clip(g, tensors, clipnorm, global_clipnorm, clipvalue)
  p0 = p.copy()
  if weight_decay:
    wd = f32(weight_decay)
    for i, (o, n) in enumerate(tensors):
      if decays is None or decays[i]:
        p0[o:o + n] = p[o:o + n] - (p[o:o + n] * wd) * lr32
  with np.errstate(invalid='ignore'):
    m1 = m + (gc - m) * (1.0 - b1)
    v1 = v + (gc * gc - v) * (1.0 - b2)
    vh1 = None
    den = v1
    if amsgrad:
      vh = np.asarray(vhat, dtype=np.float64)
      vh1 = np.where(v1 > vh, v1, vh)                        # fmaxf: a NaN v leaves vhat
      den = vh1
    p1 = p0 - alpha * m1 / (np.sqrt(den) + eps)
  out = {'p': p1, 'p_step': p1, 'm': m1, 'v': v1, 'vhat': vh1, 'g': gc, 'alpha': alpha, 'eps': eps, 'ema': None}
  if ema is not None:
    a = np.asarray(ema, dtype=np.float64)
    a1 = p1.copy() if t == 1 else a + (p1 - a) * (1.0 - f32(ema_momentum))
    out['ema'] = a1
    if ema_overwrite:
      out['p'] = a1.copy()
  return out


def bars(ref):
  """The elementwise error bars of the issue against a restated step ``ref``: m, v (vhat takes v's), p."""
  g, m, v = np.abs(ref['g']), np.abs(ref['m']), np.abs(ref['v'])
  den = ref['vhat'] if ref['vhat'] is not None else ref['v']
  with np.errstate(divide='ignore', invalid='ignore'):       # (the denominator the step divided by: vhat under amsgrad)
    upd = np.where(m > 0, ref['alpha'] * m / (np.sqrt(den) + ref['eps']), 0.0)
  return {'m': 8 * U * (m + g), 'v': 12 * U * (v + g * g), 'p': 4 * U * np.abs(ref['p_step']) + 24 * U * upd}
