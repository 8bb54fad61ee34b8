"""The Python surface against tests/golden/python_surface.json: the public attributes of WaveNet,
GenerationSession and MeanSquaredError with their kinds, signatures and docstring digests, ``wavenets_amd.__all__`` and
the classes ``wavenets_amd.model`` holds.  tests/golden/make_python_surface.py wrote the file once on the commit before
model.py was split by concern; its ``record()`` runs here on the working tree.  Host only."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def surfaces():
  spec = importlib.util.spec_from_file_location('make_python_surface', os.path.join(GOLDEN, 'make_python_surface.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  with open(os.path.join(GOLDEN, 'python_surface.json')) as f:
    want = json.load(f)
  want.pop('header')
  return want, mod.record()


@pytest.mark.parametrize('cls', ['WaveNet', 'GenerationSession', 'MeanSquaredError'])
def test_every_attribute_keeps_kind_signature_and_docstring(surfaces, cls):
  want, got = surfaces
  assert sorted(got['classes'][cls]) == sorted(want['classes'][cls])
  for name, rec in want['classes'][cls].items():
    assert got['classes'][cls][name] == rec, (cls, name)


def test_the_package_and_the_model_module_export_what_they_did(surfaces):
  want, got = surfaces
  assert got['__all__'] == want['__all__']
  assert got['model_classes'] == want['model_classes']
  assert got == want
