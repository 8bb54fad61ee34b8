"""train.py's end-of-run generation under the sampling controls (keys preview_temperature, preview_top_k, preview_seed),
after the pattern of test_gpu_driver.py: the seed selects the take, and a run that resumes from the checkpoint with no
epochs left regenerates exactly what the training run wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(lr=0.002, recording_length=400, batch_size=4, apply_mulaw=True, dataset='synthetic', kernel_size=2, channels=32,
            blocks=4, layers_per_block=1, activation='leaky_relu', dropout=0.1, dilation_bound=16, num_mixtures=None,
            sampling_function='categorical', bits=8, skip_channels=64, final_layers_channels=[32], synthetic_utterances=8,
            preview_length=48, preview_temperature=0.8, preview_top_k=32)


def _run(tmp_path, cfg, epochs):
  cfg = dict(cfg, results_dir=str(tmp_path / 'results'))
  path = tmp_path / 'run.yaml'
  path.write_text(yaml.safe_dump(cfg))
  res = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--configfile', str(path), '--epochs', str(epochs)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
  assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
  return res.stdout, np.load(tmp_path / 'results' / 'run' / 'samples' / 'samples.npy')


def test_train_driver_preview_sampling_controls(tmp_path):
  # one epoch: its checkpoint (the first loss is always the best so far) holds the weights the preview was drawn from
  out, first = _run(tmp_path, dict(BASE, preview_seed=7), 1)
  assert 'Epoch 1/1' in out and 'Speed of generation was' in out
  assert first.shape == (4, 48, 1) and np.isfinite(first).all() and np.abs(first).max() <= 1.0
  out, second = _run(tmp_path, dict(BASE, preview_seed=8), 1)
  assert 'resuming from' in out and 'Epoch ' not in out            # no epochs left: generation only
  assert second.shape == first.shape and not np.array_equal(second, first)
  out, third = _run(tmp_path, dict(BASE, preview_seed=7), 1)
  assert 'resuming from' in out and 'Epoch ' not in out
  assert np.array_equal(third, first)
  # the controls reach the draw: the same seed without them is another take
  out, plain = _run(tmp_path, dict(BASE, preview_seed=7, preview_temperature=1.0, preview_top_k=0), 1)
  assert not np.array_equal(plain, first)
