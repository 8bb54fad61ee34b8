"""Every optimizer entry point of the C ABI against tests/golden/adam_bits.json, bit for bit.

The file holds sha256 digests of what the library computed when the Adam step still had three kernels, one per family of
entry points; tests/golden/make_adam_bits.py wrote it once on the MI355X with that library and its ``record()`` is run here
on the library under test.  The bit-for-bit tests between the entry points
(tests/test_gpu_adam_options.py, tests/test_gpu_ema.py) compare a kernel with itself since the three became one; this one
compares it with the record.  A mismatch is a changed result bit: the file is not to be recorded again."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _maker():
  spec = importlib.util.spec_from_file_location('make_adam_bits', os.path.join(GOLDEN, 'make_adam_bits.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_every_entry_point_matches_the_recording():
  M = _maker()
  with open(M.PATH) as f:
    want = json.load(f)
  assert 'not regenerated' in want['header']
  model = M.small_model()
  names = list(model.variable_names)
  assert names == want['variable_names'], 'inputs differ from the recording (the network has other tensors)'
  got = M.record(model)
  bad = [k for k in want['inputs'] if got['inputs'].get(k) != want['inputs'][k]]
  assert not bad and set(got['inputs']) == set(want['inputs']), f'inputs differ from the recording: {bad}'
  assert set(got['cases']) == set(want['cases']) == set(M.CASES) | set(M.CLIPS)
  for case, steps in want['cases'].items():
    assert len(got['cases'][case]) == len(steps), case
    for t, (w, g) in enumerate(zip(steps, got['cases'][case]), 1):
      assert set(w) == set(g), (case, t)
      for array in sorted(w):
        if g[array] == w[array]:
          continue
        cut = lambda s: [s[i:i + M.PREFIX] for i in range(0, len(s), M.PREFIX)]       # one prefix per tensor
        where = [names[i] for i, (a, b) in enumerate(zip(cut(g[array]['tensors']), cut(w[array]['tensors']))) if a != b]
        pytest.fail(f'{case}, step {t}, {array}: bits differ from the recording, first in tensor '
                    f'{where[0] if where else "(whole array only)"} ({len(where)} of {len(names)} tensors differ)')
