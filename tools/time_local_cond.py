"""Local conditioning against global conditioning at the configs[4] shape: ms per training step of
the globally conditioned network, of the same network with conditioning='local' at hop = 320 (F = 50) and hop = 32
(F = 500), and the frame-sum kernel's own time and GB/s (device time from torch.profiler).

  python tools/time_local_cond.py [--steps 50] [--warmup 10] [--global-only] [--generation [--hop 256]]

--generation times the queued generation step instead: 2048 samples at B = 8, three alternating runs of the global
network, the local one on a frame schedule of --hop samples a frame (every row crosses its boundaries at the same steps),
and the local one with unaligned rows: row j admitted by admit_own_clock hop / 8 * j samples into
a frame, with frames of its own, so the eight rows cross their boundaries at eight different steps.

--global-only times the global network alone: the form a library built before local conditioning can run (WN_HIP_LIB)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wavenets_amd import WaveNet, Adam
from wavenets_amd.data import synthetic_waveforms

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--global-only', action='store_true')
ap.add_argument('--generation', action='store_true')
ap.add_argument('--hop', type=int, default=256)
args = ap.parse_args()

dev = torch.device('cuda', 0)
NET = dict(blocks=30, channels=64, skip_channels=256, dilation_bound=1024, final_layers_channels=[128, 256],
           activation='leaky_relu', bits=8, mapping_layers=[8, 16, 32], mapping_activation='leaky_relu')
B, T, CIN = 8, 16000, 110
x = synthetic_waveforms(B, T + 1, seed=5, device=dev)
g = torch.Generator().manual_seed(1)


def step_ms(model, data):
  for _ in range(args.warmup):
    model.train_step(data)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    model.train_step(data)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / args.steps * 1e3


def build(conditioning):
  m = WaveNet(**NET, conditioning=conditioning, device=dev)
  m.compile(optimizer=Adam(learning_rate=5e-4, clipnorm=1.0))
  return m


if args.generation:
  n, hop = 2048, args.hop
  gl, lo = build('global'), build('local')
  held = torch.rand(B, CIN, generator=g).to(dev)
  frames = torch.rand(B, -(-n // hop), CIN, generator=g).to(dev)
  w = x[:, :gl.receptive_field].contiguous()
  shift = max(1, hop // 8)
  lead = hop + B * shift                               # samples the session makes before the timed ones
  long_frames = torch.rand(B, -(-(lead + n) // hop) + 1, CIN, generator=g).to(dev)
  own = -(-(n + B * shift) // hop) + 1                 # frames a request brings: its timed samples and its lead inside the session

  def unaligned():
    """A session whose row j was admitted j * shift samples into a frame of the session; returns its timed n samples' time."""
    s = lo.generation_session(sample=w, condition=long_frames, hop=hop, use_queues=True, stream=list(range(B)))
    s.generate(hop)
    for j in range(B):
      s.generate(shift)
      s.admit_own_clock(j, w[j:j + 1], condition=long_frames[j:j + 1, :own], stream=[100 + j])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.generate(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6

  def us_per_step(fn):
    fn()                                               # (builds the model, primes the caches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6
  for run in range(3):
    a = us_per_step(lambda: gl.generate(n, sample=w, condition=held, use_queues=True, seed=1))
    b = us_per_step(lambda: lo.generate(n, sample=w, condition=frames, hop=hop, use_queues=True, seed=1))
    if run == 0:
      unaligned()                                      # (warms the admission's scratch and tables)
    c = unaligned()
    print(f'generation run {run + 1}: global {a:.1f} us/step, local hop={hop} {b:.1f} us/step, '
          f'local hop={hop} unaligned rows {c:.1f} us/step', flush=True)
  sys.exit(0)

spk = torch.nn.functional.one_hot(torch.randint(0, CIN, (B,), generator=g), CIN).float().to(dev)
print(f'global: {step_ms(build("global"), (x, spk)):.3f} ms/step', flush=True)
if args.global_only:
  sys.exit(0)

for hop in (320, 32):
  F = T // hop
  frames = torch.rand(B, F, CIN, generator=g).to(dev)
  m = build('local')
  print(f'local hop={hop} F={F}: {step_ms(m, (x, frames)):.3f} ms/step', flush=True)
  # the frame-sum kernel alone: device time of its launches in a few profiled steps
  try:
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
      for _ in range(5):
        m.train_step((x, frames))
      torch.cuda.synchronize()
    ev = [e for e in prof.key_averages() if 'wn_cond_frame_sum' in e.key]
    if ev:
      us = sum(e.device_time_total for e in ev) / sum(e.count for e in ev)
      gb = NET['blocks'] * B * T * 2 * NET['channels'] * 4 / 1e9
      print(f'  wn_cond_frame_sum_kernel: {us:.1f} us a launch, {gb:.2f} GB read -> {gb / (us * 1e-6):.0f} GB/s', flush=True)
    else:
      print('  wn_cond_frame_sum_kernel: not seen by the profiler', flush=True)
  except Exception as exc:                       # the profiler is optional: the step times above stand without it
    print(f'  wn_cond_frame_sum_kernel: profiler unavailable ({type(exc).__name__})', flush=True)
  del m
  torch.cuda.empty_cache()
