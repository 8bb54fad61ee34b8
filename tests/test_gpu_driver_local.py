"""train.py with conditioning: local (the pattern of tests/test_gpu_driver.py): condition_hop, the
synthetic per-frame condition (mean absolute amplitude of the uncompanded waveform, the reference's (n, F) form), training,
a checkpoint whose mapping kernel is the 1x1 Conv1D's rank 3, resume, and the final generation on the frames and the hop."""
import os
import re

import numpy as np
import pytest

from test_gpu_driver import BASE, _run

pytestmark = pytest.mark.gpu


def test_train_driver_with_local_conditioning(tmp_path):
  cfg = dict(BASE, recording_length=384, condition_hop=32, conditioning='local', mapping_layers=[4, 8],
             mapping_activation='leaky_relu')
  out, losses, run_dir = _run(tmp_path, cfg, 3)
  assert len(losses) == 3 and losses[-1] < losses[0] and all(np.isfinite(losses))
  ckpts = sorted(f for f in os.listdir(run_dir) if f.endswith('.weights.npz'))
  assert ckpts
  with np.load(run_dir / ckpts[-1]) as d:
    names = [str(n) for n in d['names']]
    assert d[f'w{names.index("mapping0/kernel"):03d}'].shape == (1, 1, 4)       # (B, F): one channel -> mapping [4, 8]
    assert 'block0/conv_cond/kernel' in names
  gen = np.load(run_dir / 'samples' / 'samples.npy')
  assert gen.shape == (4, 24, 1) and np.isfinite(gen).all() and np.abs(gen).max() <= 1.0
  assert 'Speed of generation was' in out
  out2, losses2, _ = _run(tmp_path, cfg, 5)
  m = re.search(r'resuming from .*weights-e(\d+)-lr', out2)
  assert m and 1 <= len(losses2) <= 5 - int(m.group(1)) and losses2[0] < losses[0]
