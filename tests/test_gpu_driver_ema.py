"""train.py with use_ema and validation_utterances (tests/test_gpu_driver.py's tiny config): the checkpoint carries the
average, the epoch lines carry val_loss, averaged.weights.h5 is written once at the end and is no resume candidate, a second
invocation resumes; with the four keys absent the driver prints and writes what it did before."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = dict(lr=0.002, recording_length=400, batch_size=4, apply_mulaw=True, dataset='synthetic', kernel_size=2, channels=32,
            blocks=4, layers_per_block=1, activation='leaky_relu', dropout=0.1, dilation_bound=16, num_mixtures=None,
            sampling_function='categorical', bits=8, skip_channels=64, final_layers_channels=[32], synthetic_utterances=8,
            preview_length=24)
MODEL = dict(kernel_size=2, channels=32, blocks=4, layers_per_block=1, activation='leaky_relu', dropout=0.1, dilation_bound=16,
             sampling_function='categorical', bits=8, skip_channels=64, final_layers_channels=[32])


def _run(tmp_path, cfg, epochs):
  cfg = dict(cfg, results_dir=str(tmp_path / 'results'))
  path = tmp_path / 'run.yaml'
  path.write_text(yaml.safe_dump(cfg))
  res = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--configfile', str(path), '--epochs', str(epochs)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
  assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
  return res.stdout, tmp_path / 'results' / 'run'


def test_driver_with_use_ema_and_validation(tmp_path):
  from wavenets_amd import WaveNet, io
  cfg = dict(BASE, use_ema=True, ema_momentum=0.9, validation_utterances=4)
  out, run_dir = _run(tmp_path, cfg, 2)
  # 8 utterances of 4 frames each; the last 4 utterances' 16 frames are held out
  assert '16 frames of 401 samples' in out
  lines = [l for l in out.splitlines() if l.startswith('Epoch ')]
  assert len(lines) == 2
  vals = [float(re.search(r' - val_loss: ([0-9.eE+-]+)', l).group(1)) for l in lines]
  assert all(np.isfinite(vals)) and all(v > 0 for v in vals)
  assert all(re.search(r'- loss: [0-9.eE+-]+ .* - val_loss: .* - lr: ', l) for l in lines)
  ckpts = sorted(f for f in os.listdir(run_dir) if f.endswith('.weights.npz'))
  assert ckpts
  with np.load(run_dir / ckpts[-1]) as d:
    assert 'adam_ema' in d and d['adam_ema'].shape == d['adam_m'].shape
    ema = d['adam_ema'].copy()
    raw = np.concatenate([d[f'w{i:03d}'].reshape(-1) for i in range(len(d['names']))])
    assert not np.array_equal(ema, raw)
  assert 'Speed of generation was' in out and (run_dir / 'samples' / 'samples.npy').exists()
  # the averaged exchange file loads into a model of the same spec; it is no resume candidate
  assert (run_dir / 'averaged.weights.h5').exists()
  model = WaveNet(**MODEL, device=torch.device('cuda', 0))
  model.build((1, 8, 1))
  io.load_weights(model, str(run_dir / 'averaged.weights.h5'))
  got = model.flat_params.data.cpu().numpy()
  assert got.shape == ema.shape and np.isfinite(got).all()
  if re.search(r'weights-e0002', ckpts[-1]):         # the last epoch was the best one: the file holds that checkpoint's average
    assert np.array_equal(got.view(np.int32), ema.view(np.int32))
  assert io.find_resume(str(run_dir))[0].endswith(ckpts[-1])
  # a second invocation resumes and continues
  out2, _ = _run(tmp_path, cfg, 4)
  m = re.search(r'resuming from .*weights-e(\d+)-lr', out2)
  assert m and int(m.group(1)) == int(re.search(r'weights-e(\d+)', ckpts[-1]).group(1))
  lines2 = [l for l in out2.splitlines() if l.startswith('Epoch ')]
  assert 1 <= len(lines2) <= 4 - int(m.group(1)) and all('val_loss' in l for l in lines2)


def test_driver_without_the_keys_is_unchanged(tmp_path):
  out, run_dir = _run(tmp_path, dict(BASE), 2)
  assert '32 frames of 401 samples' in out
  lines = [l for l in out.splitlines() if l.startswith('Epoch ')]
  assert len(lines) == 2 and not any('val_loss' in l for l in lines)
  assert not (run_dir / 'averaged.weights.h5').exists()
  ckpts = sorted(f for f in os.listdir(run_dir) if f.endswith('.weights.npz'))
  with np.load(run_dir / ckpts[-1]) as d:
    assert 'adam_ema' not in d and 'adam_m' in d
