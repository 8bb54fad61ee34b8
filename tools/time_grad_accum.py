"""What Adam(gradient_accumulation_steps=k) costs per micro-step: BASELINE configs[1] (8 x 16000), one process and no process
group.  Two optimizers on ONE model, alternated in one process, so parameters and data are shared: `reference` is
Adam(clipnorm=1.0), `accumulate` is Adam(clipnorm=1.0, gradient_accumulation_steps=k).  A block of the latter is a whole number
of cycles: k - 1 storing micro-steps (one 5 MB read and write instead of the sumsq and Adam launches) and one that forms the
mean and updates.  Also timed: the three modes of wn_grad_accumulate alone on buffers of the network's size.

  python tools/time_grad_accum.py [--k 4] [--steps 40] [--runs 3]
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--k', type=int, default=4)
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--runs', type=int, default=3)
args = ap.parse_args()
assert args.steps % args.k == 0, 'a block is a whole number of cycles'

import torch
import bench
from wavenets_amd import WaveNet, Adam, MeanSquaredError, _lib
from wavenets_amd.data import synthetic_waveforms

dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
m = WaveNet(**bench.CFG2, device=dev, seed=0)
OPTS = {'reference': Adam(learning_rate=5e-4, clipnorm=1.0),
        'accumulate': Adam(learning_rate=5e-4, clipnorm=1.0, gradient_accumulation_steps=args.k)}
m.compile(optimizer=OPTS['reference'], metrics=[MeanSquaredError()])
x = synthetic_waveforms(8, 16001, seed=99, device=dev)


def block(name, n):
  m.optimizer = OPTS[name]
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    m.train_step(x)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


def kernel_alone(mode, n_calls=200):
  n = m.flat_params.numel()
  acc, g = torch.ones(n, device=dev), torch.ones(n, device=dev)      # FINISH converges to 1 / (k - 1): nothing denormal
  L = _lib.lib()
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  for i in range(n_calls + 20):
    if i == 20:
      start.record()
    _lib.check(L.wn_grad_accumulate(_lib.ptr(acc), _lib.ptr(g), n, mode, args.k, None, _lib.stream_ptr()))
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / n_calls * 1e3


for name in OPTS:
  block(name, 12)
ms = {name: [] for name in OPTS}
for _ in range(args.runs):
  for name in OPTS:
    ms[name].append(block(name, args.steps))
ref = statistics.median(ms['reference'])
for name, v in ms.items():
  print(f'{name}: ' + ' '.join(f'{t:.3f}' for t in v) + f' ms/micro-step ({args.steps} per run), median '
        f'{statistics.median(v):.3f}, spread {max(v) - min(v):.3f}, vs reference {(statistics.median(v) - ref) * 1e3:+.1f} us')
for label, mode in (('FIRST', _lib.WN_ACCUM_FIRST), ('ADD', _lib.WN_ACCUM_ADD), ('FINISH', _lib.WN_ACCUM_FINISH)):
  print(f'wn_grad_accumulate {label}: {kernel_alone(mode):.1f} us per launch, back to back')
acc = OPTS['accumulate']
print(f'{m.flat_params.numel()} parameters; k = {args.k}; guard trips {m.train_guard_trips}; updates: reference '
      f'{OPTS["reference"].iterations}, accumulate {acc.iterations} (+{acc.accumulated} held); library {_lib.LIB_PATH}')
