#!/usr/bin/env python3
"""Generates tests/golden/python_surface.json: the Python surface of the package as it stood BEFORE wavenets_amd/model.py
was split by concern.  Host only: the package is imported, nothing is built or run.

  python tests/golden/make_python_surface.py        # on the parent commit, once

Recorded: for WaveNet, GenerationSession and MeanSquaredError every public attribute that a class of the package defines
(the mixins and bases of the package included, torch.nn.Module's own not), and the private helpers of WaveNet that tests
and tools call (EXTRA) -- per attribute its kind (function, static, property, or value for a plain class attribute),
``str(inspect.signature(...))`` and the sha256 of its docstring; ``wavenets_amd.__all__``; and the classes of the package
that ``wavenets_amd.model`` holds, which is what ``from wavenets_amd.model import ...`` can name.

The file is NOT regenerated afterwards: tests/test_python_surface_cpu.py runs ``record()`` below on the working tree and
compares for equality.  A mismatch is a changed signature, a changed docstring or a lost name, not a reason to record again.
"""
import hashlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, 'python_surface.json')
HEADER = ('recorded on the parent commit (55c6c64), where wavenets_amd/model.py held seven classes; not regenerated '
          'afterwards (tests/golden/make_python_surface.py)')
EXTRA = {'WaveNet': ('_sampling', '_sampling_rows', '_generation_args', '_local_frames', '_world', '_rank')}


def _doc(obj):
  doc = getattr(obj, '__doc__', None)
  return None if doc is None else hashlib.sha256(doc.encode()).hexdigest()


def _describe(raw):
  if isinstance(raw, staticmethod):
    fn = raw.__func__
    return {'kind': 'static', 'signature': str(inspect.signature(fn)), 'doc': _doc(fn)}
  if isinstance(raw, property):
    return {'kind': 'property', 'signature': str(inspect.signature(raw.fget)), 'doc': _doc(raw.fget)}
  if inspect.isfunction(raw):
    return {'kind': 'function', 'signature': str(inspect.signature(raw)), 'doc': _doc(raw)}
  return {'kind': 'value', 'signature': repr(raw), 'doc': None}


def _surface(cls):
  """Name -> description, over the classes of the package in cls's MRO (the first that defines a name wins, as lookup does)."""
  out = {}
  for base in cls.__mro__:
    if not base.__module__.startswith('wavenets_amd'):
      continue
    for name, raw in vars(base).items():
      if name in out or (name.startswith('_') and name != '__init__' and name not in EXTRA.get(cls.__name__, ())):
        continue
      out[name] = _describe(raw)
  return dict(sorted(out.items()))


def record():
  import wavenets_amd
  from wavenets_amd import model
  classes = {c.__name__: _surface(c) for c in (wavenets_amd.WaveNet, wavenets_amd.GenerationSession,
                                               wavenets_amd.MeanSquaredError)}
  for cls, names in EXTRA.items():
    missing = [n for n in names if n not in classes[cls]]
    assert not missing, (cls, missing)
  importable = sorted(n for n, v in vars(model).items()
                      if inspect.isclass(v) and v.__module__.startswith('wavenets_amd'))
  return {'classes': classes, '__all__': list(wavenets_amd.__all__), 'model_classes': importable}


if __name__ == '__main__':
  with open(PATH, 'w') as f:
    json.dump({'header': HEADER, **record()}, f, indent=1, sort_keys=True)
    f.write('\n')
  print(PATH)
