#!/usr/bin/env python3
"""Generates tests/golden/adam_bits.json: what the optimizer entry points of the C ABI computed BEFORE the three Adam
kernels became one, as sha256 digests of the raw fp32 bytes -- one per tensor of the plan's table
(its first 8 hex digits: it locates a difference, the array's digest detects it) and one per whole array.  Digests only; the inputs' digests are stored too, so that a drift of the inputs is told apart
from a change of the kernels.

  WN_HIP_LIB=<libwn_hip.so of the parent commit> python tests/golden/make_adam_bits.py        # on the MI355X, once

The file is written by the parent's library and is NOT regenerated afterwards: tests/test_gpu_adam_bits.py runs
``record()`` below on the library under test and compares.  A mismatch is a change of a result bit, not a reason to
record again.

Network: the `small` one of tests/test_gpu_adam_options.py (its 40 x 256 output kernel wraps the grid-stride loop, its
biases are short tensors at offsets that are no multiple of a wave).  Inputs: np.random.RandomState (a frozen stream).
Every Adam case runs consecutive steps (t = 1, 2, 3) from the same fixed state on the gradient of ``inputs`` scaled by
STEP_SCALE[t - 1]; p, m, v (vhat, ema where the case has them) are recorded after every step.  The comments at the ext
cases name the instantiation of the recording library's kernel; together the cases reach all eight of wn_adam_kernel.  The clips run in place on the
unscaled gradient; the clipped gradient and scratch[:num_tensors] (preset to -1) are recorded.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):          # tests/ and the repository root
  if _d not in sys.path:
    sys.path.insert(0, _d)
PATH = os.path.join(HERE, 'adam_bits.json')
HEADER = ('recorded on an MI355X by the library of the parent commit (19b1c1d), where the Adam step had three kernels, before '
          'wn_optim.hip; not regenerated afterwards (tests/golden/make_adam_bits.py)')
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.999, 1e-7
STEP_SCALE = (1.0, 0.5, 0.75)
NONE, NORM, GLOBAL, VALUE = 0, 1, 2, 4                    # WN_CLIP_*
PREFIX = 8                                                # hex digits kept of a tensor's digest
GLOBAL_C = 20.0                                           # the whole gradient's norm is about 108, 54 at the smallest scale

CASES = {
    'guarded_clipnorm': dict(entry='guarded', clipnorm=1.0),
    'guarded_no_clip': dict(entry='guarded', clipnorm=0.0),
    'guarded_skip_at_step_2': dict(entry='guarded', clipnorm=1.0, skip_at=2),
    'unguarded': dict(entry='plain', clipnorm=1.0, steps=1),
    'ema': dict(entry='ema', clipnorm=1.0, ema=True, momentum=0.99, overwrite_at=2, ema_nan=True),
    'ext_value_decay_table': dict(entry='ext', clip=(VALUE, 0.5), wd=0.1, flags=True),                     # <false, false>
    'ext_amsgrad': dict(entry='ext', clip=(NORM, 1.0), amsgrad=True),                                      # <false, true>
    'ext_amsgrad_decay': dict(entry='ext', clip=(NORM, 1.0), amsgrad=True, wd=0.1),
    'ext_amsgrad_ema': dict(entry='ext', clip=(NORM, 1.0), amsgrad=True, ema=True, momentum=0.9, overwrite_at=2),
    'ext_ema_global': dict(entry='ext', clip=(GLOBAL, GLOBAL_C), ema=True, momentum=0.9, overwrite_at=2),  # <true, false>
    'ext_all': dict(entry='ext', clip=(GLOBAL, GLOBAL_C), wd=0.1, amsgrad=True, ema=True, momentum=0.9, overwrite_at=2),
}
CLIPS = {'clip_gradients': (None, 1.0), 'clip_ext_norm': (NORM, 1.0), 'clip_ext_global': (GLOBAL, GLOBAL_C),
         'clip_ext_value': (VALUE, 0.1)}


def _rand(rs, n, lo, hi):
  """fp32 values of magnitude in [lo, hi] and random sign."""
  mag = lo + (hi - lo) * rs.random_sample(n)
  return (mag * np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)).astype(np.float32)


def make_inputs(tensors, names):
  n = sum(ln for _, ln in tensors)
  rs = np.random.RandomState(20240607)
  x = {'p': _rand(rs, n, 0.05, 0.2), 'm': _rand(rs, n, 0.01, 0.05), 'v': np.abs(_rand(rs, n, 1e-3, 1e-2)),
       'vhat': np.abs(_rand(rs, n, 1e-3, 1e-2)), 'ema': _rand(rs, n, 0.05, 0.2)}
  # the construction of _heavy_gradient (tests/test_gpu_adam_options.py): the longest tensor carries almost all of the norm
  g = _rand(rs, n, 0.05, 0.15)
  big = max(range(len(tensors)), key=lambda i: tensors[i][1])
  o, ln = tensors[big]
  g[o:o + ln] = _rand(rs, ln, 0.5, 1.5)
  x['g'] = g
  x['decay_flags'] = np.array([0 if nm.endswith('bias') else 1 for nm in names], dtype=np.int32)
  x['table'] = np.array(tensors, dtype=np.int64)
  # clipnorm = 1.0 must act on the largest tensor and leave the short ones alone, at every step's scale
  for f in STEP_SCALE:
    norms = [float(np.sqrt(np.sum((g[o:o + ln].astype(np.float64) * f) ** 2))) for o, ln in tensors]
    short = [nr for nr, (_, ln) in zip(norms, tensors) if ln < 64]
    assert norms[big] > 2.0 and short and max(short) < 0.9, (f, norms[big], short)
  N = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
  assert min(STEP_SCALE) * N > 1.5 * GLOBAL_C, N
  assert 0 < x['decay_flags'].sum() < len(names)
  return x


def _sha(a):
  return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(a, tensors):
  """The array's sha256, and one string of the tensors' digests, PREFIX hex digits each: the first is the check, the second
  only says where a difference begins."""
  return {'all': _sha(a), 'tensors': ''.join(_sha(a[o:o + ln])[:PREFIX] for o, ln in tensors)}


def record(model):
  """Every case on the library that wavenets_amd._lib has loaded: {'inputs': ..., 'cases': ...} of digests."""
  import torch
  from wavenets_amd import _lib
  L, dev = _lib.lib(), model.flat_params.device
  tensors = [(int(o), int(np.prod(s))) for o, s in zip(model._offsets, model._shapes)]
  nt = len(tensors)
  x = make_inputs(tensors, model.variable_names)
  assert x['p'].size == model.flat_params.numel()
  up = lambda a: torch.from_numpy(a).to(dev)
  flags = up(x['decay_flags'])
  out = {'inputs': {k: _sha(v) for k, v in x.items()}, 'cases': {}}

  for name, c in CASES.items():
    st = {k: up(x[k].copy()) for k in ('p', 'm', 'v')}
    st['vhat'] = up(x['vhat'].copy()) if c.get('amsgrad') else None
    st['ema'] = up(x['ema'].copy()) if c.get('ema') else None
    if c.get('ema_nan'):
      st['ema'][tensors[2][0] + 1] = float('nan')         # step 1 copies p: the NaN must not survive
    scratch = torch.zeros(nt + 8, dtype=torch.float32, device=dev)
    steps = []
    for t in range(1, c.get('steps', 3) + 1):
      g = up(x['g'] * np.float32(STEP_SCALE[t - 1]))
      skip = torch.full((1,), 1.0 if c.get('skip_at') == t else 0.0, dtype=torch.float32, device=dev)
      over = 1 if c.get('overwrite_at') == t else 0
      head = (model._plan, _lib.ptr(st['p']), _lib.ptr(g), _lib.ptr(st['m']), _lib.ptr(st['v']))
      if c['entry'] == 'guarded':
        rc = L.wn_adam_step_guarded(*head, t, LR, BETA1, BETA2, EPS, c['clipnorm'], _lib.ptr(scratch), _lib.ptr(skip), _lib.stream_ptr())
      elif c['entry'] == 'plain':
        rc = L.wn_adam_step(*head, t, LR, BETA1, BETA2, EPS, c['clipnorm'], _lib.ptr(scratch), _lib.stream_ptr())
      elif c['entry'] == 'ema':
        rc = L.wn_adam_step_ema(*head, _lib.ptr(st['ema']), t, LR, BETA1, BETA2, EPS, c['clipnorm'], c['momentum'], over,
                                _lib.ptr(scratch), _lib.ptr(skip), _lib.stream_ptr())
      else:
        o = _lib.WnAdamOptions()
        o.lr, o.beta1, o.beta2, o.eps = LR, BETA1, BETA2, EPS
        o.clip_mode, o.clip = c['clip']
        o.weight_decay, o.amsgrad = c.get('wd', 0.0), int(bool(c.get('amsgrad')))
        o.decay_flags = flags.data_ptr() if c.get('flags') else None
        o.ema_momentum, o.ema_overwrite = (c['momentum'], over) if c.get('ema') else (0.0, 0)
        rc = L.wn_adam_step_ext(*head, _lib.ptr(st['vhat']), _lib.ptr(st['ema']), t, C.byref(o), _lib.ptr(scratch), _lib.ptr(skip),
                                _lib.stream_ptr())
      _lib.check(rc)
      torch.cuda.synchronize()
      steps.append({k: digests(a.cpu().numpy(), tensors) for k, a in st.items() if a is not None})
    if c.get('skip_at'):
      assert steps[c['skip_at'] - 1] == steps[c['skip_at'] - 2] != steps[c['skip_at']], name
    if c.get('ema_nan'):
      assert not torch.isnan(st['ema']).any()
    out['cases'][name] = steps

  for name, (mode, c) in CLIPS.items():
    g = up(x['g'].copy())
    scratch = torch.full((nt + 8,), -1.0, dtype=torch.float32, device=dev)
    if mode is None:
      rc = L.wn_clip_gradients(model._plan, _lib.ptr(g), c, _lib.ptr(scratch), _lib.stream_ptr())
    else:
      rc = L.wn_clip_gradients_ext(model._plan, _lib.ptr(g), mode, c, _lib.ptr(scratch), _lib.stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert not np.array_equal(got, x['g']), name          # the clip acts
    out['cases'][name] = [{'g': digests(got, tensors), 'scratch': {'all': _sha(scratch.cpu().numpy()[:nt]), 'tensors': ''}}]
  return out


def write(out):
  """One line per recorded array."""
  j = lambda v: json.dumps(v, sort_keys=True)
  cases = [f'  {j(name)}: [\n' + ',\n'.join('   {' + ',\n    '.join(f'{j(k)}: {j(d)}' for k, d in sorted(step.items())) + '}' for step in steps) + ']'
           for name, steps in sorted(out['cases'].items())]
  with open(PATH, 'w') as f:
    f.write('{\n' + ''.join(f' {j(k)}: {j(out[k])},\n' for k in ('header', 'inputs', 'variable_names'))
            + ' "cases": {\n' + ',\n'.join(cases) + '}}\n')


def small_model():
  import torch
  from test_gpu_adam_options import KW, SEED
  from wavenets_amd import WaveNet
  m = WaveNet(**KW, device=torch.device('cuda', 0), seed=SEED)
  m.build((1, 8, 1))
  return m


def main():
  from wavenets_amd import _lib
  m = small_model()
  out = {'header': HEADER, 'variable_names': list(m.variable_names)}
  out.update(record(m))
  write(out)
  print(f'{len(out["cases"])} cases, {len(m.variable_names)} tensors, {os.path.getsize(PATH)} bytes, library {_lib.LIB_PATH}')


if __name__ == '__main__':
  main()
