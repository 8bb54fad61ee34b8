"""What Adam(use_ema=True) costs per step: BASELINE configs[1] (8 x 16000), one process and no process group, with the flag
off and on, alternated in one process.  Toggling the flag on one optimizer keeps parameters, moments and data the same for
both settings (the average observes: it never feeds back into the step).

  python tools/time_ema.py [--steps 40] [--runs 3]                step time, flag off / on alternated, `runs` blocks each
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_ema.py --profile
                                                                  a few steps of each: wn_adam_kernel<false,false,false> / <true,false,false>
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from wavenets_amd import WaveNet, Adam, MeanSquaredError
from wavenets_amd.data import synthetic_waveforms

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--profile', action='store_true')
args = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
m = WaveNet(**bench.CFG2, device=dev, seed=0)
opt = Adam(learning_rate=5e-4, clipnorm=1.0, use_ema=True)
m.compile(optimizer=opt, metrics=[MeanSquaredError()])
x = synthetic_waveforms(8, 16001, seed=99, device=dev)


def block(flag, n):
  opt.use_ema = flag                                      # the buffer stays allocated; off: the launch of the default path
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    m.train_step(x)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


if args.profile:
  block(False, 12)
  block(True, 12)
else:
  for flag in (False, True):                              # both shapes of the step warmed up
    block(flag, 10)
  ms = {False: [], True: []}
  for _ in range(args.runs):
    for flag in (False, True):
      ms[flag].append(block(flag, args.steps))
  for flag in (False, True):
    print(f'use_ema={flag}: ' + ' '.join(f'{v:.3f}' for v in ms[flag]) +
          f' ms/step ({args.steps} steps per run), median {statistics.median(ms[flag]):.3f}, '
          f'spread {max(ms[flag]) - min(ms[flag]):.3f}')
  print(f'difference of the medians: {(statistics.median(ms[True]) - statistics.median(ms[False])) * 1e3:+.1f} us; '
        f'{m.flat_params.numel()} parameters; guard trips {m.train_guard_trips}')
