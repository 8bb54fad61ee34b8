"""train.py with gradient_accumulation_steps (tests/test_gpu_driver.py's tiny config): the weights move every second batch,
the checkpoint carries the cycle under way (adam_accum, adam_accumulated) beside the count of updates, a second invocation
resumes from it; together with clip_before_reduce the driver stops with the constructor's error."""
import os
import re
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
            preview_length=0)
STEPS = 3          # batches per epoch: odd, so a cycle of 2 straddles every epoch end


def _run(tmp_path, cfg, epochs):
  cfg = dict(cfg, results_dir=str(tmp_path / 'results'))
  path = tmp_path / 'run.yaml'
  path.write_text(yaml.safe_dump(cfg))
  return subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--configfile', str(path), '--epochs', str(epochs)],
                        capture_output=True, text=True, cwd=ROOT, timeout=600), tmp_path / 'results' / 'run'


def _checkpoints(run_dir):
  return sorted(f for f in os.listdir(run_dir) if f.endswith('.weights.npz'))


def test_driver_accumulates_checkpoints_the_cycle_and_resumes(tmp_path):
  cfg = dict(BASE, gradient_accumulation_steps=2, steps_per_epoch=STEPS)
  res, run_dir = _run(tmp_path, cfg, 1)
  assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
  assert len([l for l in res.stdout.splitlines() if l.startswith('Epoch ')]) == 1
  ckpts = _checkpoints(run_dir)
  assert len(ckpts) == 1 and 'weights-e0001' in ckpts[0]
  with np.load(run_dir / ckpts[0]) as d:
    # three batches: one update, one micro-step held
    assert int(d['adam_iterations']) == 1 and int(d['adam_accumulated']) == 1
    assert d['adam_accum'].shape == d['adam_m'].shape and d['adam_accum'].dtype == np.float32
    assert np.isfinite(d['adam_accum']).all() and d['adam_accum'].any()
  # a second invocation resumes in mid-cycle and continues: every checkpoint it writes has 3 * epoch batches behind it
  res2, _ = _run(tmp_path, cfg, 3)
  assert res2.returncode == 0, res2.stdout[-3000:] + res2.stderr[-3000:]
  assert re.search(r'resuming from .*weights-e0001-lr', res2.stdout)
  lines = [l for l in res2.stdout.splitlines() if l.startswith('Epoch ')]
  assert 1 <= len(lines) <= 2 and all(np.isfinite(float(re.search(r'- loss: ([0-9.eE+-]+)', l).group(1))) for l in lines)
  for name in _checkpoints(run_dir):
    epoch = int(re.search(r'weights-e(\d+)', name).group(1))
    with np.load(run_dir / name) as d:
      assert 2 * int(d['adam_iterations']) + int(d['adam_accumulated']) == STEPS * epoch, name


def test_driver_with_clip_before_reduce_is_the_constructors_error(tmp_path):
  res, _ = _run(tmp_path, dict(BASE, gradient_accumulation_steps=2, clip_before_reduce=True, steps_per_epoch=STEPS), 1)
  assert res.returncode != 0
  assert 'ValueError' in res.stderr and 'gradient_accumulation_steps' in res.stderr and 'clip_before_reduce' in res.stderr
