"""train.py's end-of-run generation under top_p (YAML key top_p, default 1.0), after the pattern of
test_gpu_driver_preview.py: the key reaches the draw, and with a mixture head it is rejected with a message that names
it, before any training."""
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
            preview_length=48, preview_seed=7)


def _train(tmp_path, cfg, epochs):
  cfg = dict(cfg, results_dir=str(tmp_path / 'results'))
  path = tmp_path / 'run.yaml'
  path.write_text(yaml.safe_dump(cfg))
  return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--configfile', str(path), '--epochs', str(epochs)],
                        capture_output=True, text=True, cwd=ROOT, timeout=600)


def _samples(tmp_path, cfg, epochs=1):
  res = _train(tmp_path, cfg, epochs)
  assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
  return res.stdout, np.load(tmp_path / 'results' / 'run' / 'samples' / 'samples.npy')


def test_train_driver_preview_top_p(tmp_path):
  out, first = _samples(tmp_path, dict(BASE, top_p=0.9))
  assert 'Epoch 1/1' in out and 'Speed of generation was' in out
  assert first.shape == (4, 48, 1) and np.isfinite(first).all() and np.abs(first).max() <= 1.0
  # resumed with no epochs left: the same weights, the same seed
  out, again = _samples(tmp_path, dict(BASE, top_p=0.9))
  assert 'resuming from' in out and 'Epoch ' not in out
  assert np.array_equal(again, first)
  # top_p reaches the draw: without the key (1.0, off) the same seed is another take, and 1.0 is the key left out
  out, plain = _samples(tmp_path, dict(BASE))
  assert not np.array_equal(plain, first)
  out, one = _samples(tmp_path, dict(BASE, top_p=1.0))
  assert np.array_equal(one, plain)


def test_train_driver_rejects_top_p_with_a_mixture_head(tmp_path):
  cfg = dict(BASE, num_mixtures=4, sampling_function='logistic', bits=16, top_p=0.9)
  res = _train(tmp_path, cfg, 1)
  assert res.returncode != 0
  assert 'top_p' in res.stderr and 'categorical' in res.stderr
  assert 'Epoch ' not in res.stdout                                   # rejected before any training
  res = _train(tmp_path, dict(BASE, top_p=1.5), 1)
  assert res.returncode != 0 and 'top_p' in res.stderr and 'Epoch ' not in res.stdout
