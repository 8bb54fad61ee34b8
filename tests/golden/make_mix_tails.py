#!/usr/bin/env python3
"""Generates tests/golden/mix_tails.npz: mixture-loss rows at the floor of the log-scales, at the cap of the Gaussian
argument and in both far tails, with the loss and its gradient evaluated in 50-digit arithmetic (mpmath) from the fp32
inputs.  The fp64 oracle cannot be the reference there: loss_logistic as the source writes it loses the bin mass of a
target above a sharp component's mean.  Data only (inputs + expected outputs).

  python tests/golden/make_mix_tails.py          # rewrites tests/golden/mix_tails.npz, byte for byte

Groups are keyed '<kind>_M<M>_b<bits>' (kind: logistic | gaussian; the Gaussian loss has no bits, its groups say b16):
  <key>_pred  (n, 3M) float32   [weights | means | log-scales]
  <key>_y     (n,)    float32
  <key>_loss  (n,)    float64   exact loss, +inf where the exact likelihood is below 1e-320
  <key>_grad  (n, 3M) float64   exact dL/dpred (NaN on the +inf rows)
  <key>_exp10 (n,)    int64     floor(log10(exact likelihood))
  <key>_tail  (n,)    int8      logistic only, what sigmoid(a) - sigmoid(b) in double does to the row:
                                0 "no tail": every component that matters (share > 1e-9) has b <= 12
                                1 "upper tail": components with b > 37 (both sigmoids round to 1) hold > half of it
                                2 in between (asserted neither way)
Rows whose likelihood lies in 1e-320 .. 1e-280 (denormal results on either side) are not generated.
"""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
PI_REF = mp.mpf('3.14159265359')                  # the source's own constant (oracle: _PI_REF)
F32 = np.float32
M7 = F32(-7.0)
LS_ALL = [F32(-9.0), M7, np.nextafter(M7, F32(-8)), np.nextafter(M7, F32(0)), F32(-3.0), F32(0.0), F32(3.0)]
D_ALL = [0.0] + [s * d for d in (1e-6, 0.01, 0.02, 0.03, 0.1, 0.5) for s in (1, -1)]
D_FEW = [0.0, 0.03, -0.03, 0.1, -0.1]


def sig(x):
  return 1 / (1 + mp.exp(-x))


def exact_row(kind, M, bits, pred, y):
  """(loss, grad[3M], exp10, tail) of one row in mp arithmetic; the formulas are those of oracle.loss_logistic /
  loss_gaussian (clamp at -7 with the gradient passing at equality, cap at 1e8 likewise)."""
  p = [mp.mpf(float(v)) for v in pred]
  yy = mp.mpf(float(y))
  wm = max(p[:M])
  e = [mp.exp(v - wm) for v in p[:M]]
  z = sum(e)
  w = [v / z for v in e]
  h = mp.mpf(1) / 2 / (1 << bits)
  comp, dmu, dls, bs = [], [], [], []
  for k in range(M):
    mu, lsr = p[M + k], p[2 * M + k]
    ls = max(lsr, mp.mpf(-7))
    lm = 1 if lsr >= -7 else 0
    if kind == 'logistic':
      inv = mp.exp(-ls)
      a, b = (yy - mu + h) * inv, (yy - mu - h) * inv
      sa, sb = sig(a), sig(b)
      da, db = sa * sig(-a), sb * sig(-b)
      comp.append(sa * sig(-b) * -mp.expm1(b - a))           # = sa - sb, with nothing cancelling in either tail
      dmu.append(-inv * (da - db))
      dls.append(-lm * (a * da - b * db))
      bs.append(b)
    else:
      sc = mp.exp(ls)
      xr = (yy - mu) / sc
      xm = 1 if xr <= mp.mpf(10) ** 8 else 0
      xx = xr if xm else mp.mpf(10) ** 8
      pdf = mp.exp(-xx * xx / 2) / (sc * mp.sqrt(2 * PI_REF))
      comp.append(pdf)
      dmu.append(pdf * xx / sc * xm)
      dls.append(lm * pdf * (xx * xx * xm - 1))
      bs.append(mp.mpf(0))
  lik = sum(wk * ck for wk, ck in zip(w, comp))
  exp10 = int(mp.floor(mp.log10(lik)))
  tail = 0
  if kind == 'logistic':
    share = [wk * ck / lik for wk, ck in zip(w, comp)]
    if sum(s for s, b in zip(share, bs) if b > 37) > mp.mpf(1) / 2:
      tail = 1
    elif any(s > mp.mpf(10) ** -9 and b > 12 for s, b in zip(share, bs)):
      tail = 2
  if exp10 < -320:
    return np.inf, np.full(3 * M, np.nan), exp10, tail
  g = [-(wk * ck - wk * lik) / lik for wk, ck in zip(w, comp)]
  g += [-wk * d / lik for wk, d in zip(w, dmu)]
  g += [-wk * d / lik for wk, d in zip(w, dls)]
  return float(-mp.log(lik)), np.array([float(v) for v in g]), exp10, tail


def rows():
  """(kind, M, bits, pred fp32[3M], y fp32) of every row."""
  out = []

  def add(kind, bits, w, mu, ls, y):
    M = len(w)
    out.append((kind, M, bits, np.concatenate([np.asarray(w, F32), np.asarray(mu, F32), np.asarray(ls, F32)]), F32(y)))

  heads = [('logistic', 8), ('logistic', 16), ('gaussian', 16)]
  # M = 1: the whole table; a target 0.9 off a floor-sharp logistic component underflows for real
  for kind, bits in heads:
    for ls in LS_ALL:
      for d in D_ALL:
        add(kind, bits, [0.0], [0.0], [ls], d)
    for d in D_ALL:
      add(kind, bits, [0.3], [0.25], [M7], F32(0.25) + F32(d))
    if kind == 'logistic':
      for ls in LS_ALL[:2]:
        for d in (0.9, -0.9):
          add(kind, bits, [0.0], [0.0], [ls], d)
  # M = 2: the target next to component 1, component 0 half a unit below it (its far upper tail at the floor)
  for kind, bits in heads[1:]:
    for ls in ([M7, M7], [LS_ALL[3], LS_ALL[2]], [F32(-9), F32(0)], [F32(-3), F32(-3)]):
      for w in ([0.0, 0.0], [40.0, 0.0]):
        for d in D_FEW + [0.5, -0.5]:
          add(kind, bits, w, [-0.25, 0.25], ls, F32(0.25) + F32(d))
  # M = 10: one broad component among sharp ones (the sharp ones masked), and all sharp; the raised weight is not the
  # nearest component's
  mu10 = np.linspace(-0.9, 0.9, 10).astype(F32)
  for kind, bits in heads[1:]:
    for sharp in (F32(-9), M7):
      for broad in (True, False):
        ls = np.full(10, sharp, F32)
        if broad:
          ls[3] = 0.0
        for hot in (None, 7):
          w = np.linspace(-0.2, 0.2, 10).astype(F32)
          if hot is not None:
            w[hot] += 40.0
          for d in D_FEW:
            add(kind, bits, w, mu10, ls, mu10[5] + F32(d))
  for d in D_FEW:
    ls = np.full(10, M7, F32)
    add('logistic', 8, np.zeros(10, F32), mu10, ls, mu10[5] + F32(d))
  # M = 32: the full size of the kernel's arrays
  mu32 = np.linspace(-0.93, 0.93, 32).astype(F32)
  for kind, bits in heads[1:]:
    for hot in (None, 20):
      w = np.linspace(-0.3, 0.3, 32).astype(F32)
      if hot is not None:
        w[hot] += 40.0
      ls = np.where(np.arange(32) % 5 == 0, F32(-9), M7).astype(F32)
      ls[31] = -3.0
      for d in (0.0, 0.03, -0.03):
        add(kind, bits, w, mu32, ls, mu32[16] + F32(d))
  # Gaussian cap: (y - mu) / sigma > 1e8 on one component (mu = -2e5 at the floor): that component's gradients are 0
  for d in (0.0, 0.01, -0.01, 0.02):
    add('gaussian', 16, [0.0, 0.1], [-2e5, 0.1], [M7, F32(-3)], F32(0.1) + F32(d))
    add('gaussian', 16, [40.0, 0.1], [-2e5, 0.1], [F32(-9), F32(-3)], F32(0.1) + F32(d))
  # M = 8, the Gaussian head of the parity suite: broad and floor-sharp components, one beyond the cap
  mu8 = np.linspace(-0.875, 0.875, 8).astype(F32)
  ls8 = np.array([-9, -3, -2.5, -7, -3, -1, -3, -2.5], F32)
  w8 = np.linspace(0.3, -0.3, 8).astype(F32)
  for d in D_FEW:
    add('gaussian', 16, w8, mu8, ls8, mu8[3] + F32(d))
  mu8c = mu8.copy()
  mu8c[0] = -2e5
  for d in D_FEW:
    add('gaussian', 16, w8, mu8c, ls8, mu8[3] + F32(d))
  return out


def main():
  groups = {}
  dropped = 0
  for kind, M, bits, pred, y in rows():
    loss, grad, exp10, tail = exact_row(kind, M, bits, pred, y)
    if -320 <= exp10 <= -280:
      dropped += 1
      continue
    g = groups.setdefault(f'{kind}_M{M}_b{bits}', dict(pred=[], y=[], loss=[], grad=[], exp10=[], tail=[]))
    g['pred'].append(pred); g['y'].append(y); g['loss'].append(loss); g['grad'].append(grad)
    g['exp10'].append(exp10); g['tail'].append(tail)
  out = {}
  n = 0
  for key in sorted(groups):
    g = groups[key]
    n += len(g['y'])
    out[f'{key}_pred'] = np.stack(g['pred']).astype(np.float32)
    out[f'{key}_y'] = np.asarray(g['y'], np.float32)
    out[f'{key}_loss'] = np.asarray(g['loss'], np.float64)
    out[f'{key}_grad'] = np.stack(g['grad']).astype(np.float64)
    out[f'{key}_exp10'] = np.asarray(g['exp10'], np.int64)
    if key.startswith('logistic'):
      out[f'{key}_tail'] = np.asarray(g['tail'], np.int8)
  path = os.path.join(HERE, 'mix_tails.npz')
  np.savez_compressed(path, **out)
  print(f'{n} rows in {len(groups)} groups ({dropped} rows in the denormal band not generated), '
        f'{os.path.getsize(path)} bytes')


if __name__ == '__main__':
  main()
