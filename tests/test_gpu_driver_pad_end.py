"""train.py with pad_end (tests/test_gpu_driver_ema.py's tiny config on recordings whose length is no multiple of
recording_length): every recording keeps its tail as one more, zero-padded frame that trains and validates under a
sample_weight of 0 on the padding; with the key absent the same recordings give the frames they gave before."""
import re

import numpy as np
import pytest

from test_gpu_driver_ema import BASE, _run

pytestmark = pytest.mark.gpu
L, N, TAIL = 400, 8, 57


def _recordings(tmp_path):
  from wavenets_amd.data import synthetic_waveforms
  path = tmp_path / 'recordings.npy'
  np.save(path, synthetic_waveforms(N, 4 * L + 1 + TAIL, seed=1234)[:, :, 0].numpy())       # already companded, in [-1, 1]
  return str(path)


def test_driver_with_pad_end_trains_on_the_tails(tmp_path):
  cfg = dict(BASE, dataset=_recordings(tmp_path), apply_mulaw=False, validation_utterances=2)
  # without the key the driver frames with data.preprocess_waveform (tests/test_gpu_driver_ema.py runs that path): the
  # tails are dropped
  from wavenets_amd import data
  import torch
  raw = torch.from_numpy(np.load(cfg['dataset']))
  plain = sum(data.preprocess_waveform(w, L, False).shape[0] for w in raw[:N - 2])
  assert plain == (N - 2) * 4
  out, _ = _run(tmp_path, dict(cfg, pad_end=True), 2)
  assert f'{plain + (N - 2)} frames of {L + 1} samples' in out              # one more frame per recording
  lines = [l for l in out.splitlines() if l.startswith('Epoch ')]
  assert len(lines) == 2
  for l in lines:
    loss = float(re.search(r' - loss: ([0-9.eE+-]+)', l).group(1))
    val = float(re.search(r' - val_loss: ([0-9.eE+-]+)', l).group(1))
    mse = float(re.search(r' - mean_squared_error: ([0-9.eE+-]+)', l).group(1))
    assert np.isfinite([loss, val, mse]).all() and loss > 0 and val > 0
  assert 'Speed of generation was' in out
