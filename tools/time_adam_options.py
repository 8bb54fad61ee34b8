"""What Adam's keywords global_clipnorm, clipvalue, weight_decay and amsgrad cost per step: BASELINE configs[1] (8 x 16000),
one process and no process group.  The variants are set on ONE optimizer and alternated in one process, so parameters,
moments and data are shared; `reference` is Adam(clipnorm=1.0), the launch of the default path.

  python tools/time_adam_options.py [--steps 40] [--runs 3]      every variant, alternated, `runs` blocks each
  python tools/time_adam_options.py --default-only [--parent-lib]
                                                                  the default step alone: run it with WN_HIP_LIB pointing
                                                                  at the parent's library (--parent-lib: that library has
                                                                  no wn_adam_step_ext to bind) and without, alternating
                                                                  processes in one session on one box
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_adam_options.py --profile
                                                                  a few steps of each: the instantiations of wn_adam_kernel
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--profile', action='store_true')
ap.add_argument('--default-only', action='store_true')
ap.add_argument('--parent-lib', action='store_true')
args = ap.parse_args()

from wavenets_amd import _lib
if args.parent_lib:
  for name in ('wn_adam_step_ext', 'wn_clip_gradients_ext'):
    _lib._SIGS.pop(name)
import torch
import bench
from wavenets_amd import WaveNet, Adam, MeanSquaredError
from wavenets_amd.data import synthetic_waveforms

dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
m = WaveNet(**bench.CFG2, device=dev, seed=0)
opt = Adam(learning_rate=5e-4, clipnorm=1.0)
m.compile(optimizer=opt, metrics=[MeanSquaredError()])
x = synthetic_waveforms(8, 16001, seed=99, device=dev)

OFF = dict(clipnorm=None, global_clipnorm=None, clipvalue=None, weight_decay=None, amsgrad=False, use_ema=False)
VARIANTS = {
    'reference': dict(clipnorm=1.0),
    'global_clipnorm': dict(global_clipnorm=1.0),
    'clipvalue': dict(clipvalue=0.01),
    'weight_decay': dict(clipnorm=1.0, weight_decay=1e-4),
    'amsgrad': dict(clipnorm=1.0, amsgrad=True),
    'all': dict(global_clipnorm=1.0, weight_decay=1e-4, amsgrad=True, use_ema=True),
}
if args.default_only:
  VARIANTS = {'reference': VARIANTS['reference']}


def block(name, n):
  for k, v in {**OFF, **VARIANTS[name]}.items():          # buffers stay allocated once built; off: the launch of the default path
    setattr(opt, k, v)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    m.train_step(x)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


if args.profile:
  for name in VARIANTS:
    block(name, 12)
else:
  for name in VARIANTS:                                   # every shape of the step warmed up
    block(name, 10)
  ms = {name: [] for name in VARIANTS}
  for _ in range(args.runs):
    for name in VARIANTS:
      ms[name].append(block(name, args.steps))
  ref = statistics.median(ms['reference'])
  for name, v in ms.items():
    print(f'{name}: ' + ' '.join(f'{t:.3f}' for t in v) + f' ms/step ({args.steps} steps per run), median '
          f'{statistics.median(v):.3f}, spread {max(v) - min(v):.3f}, vs reference {(statistics.median(v) - ref) * 1e3:+.1f} us')
  print(f'{m.flat_params.numel()} parameters; guard trips {m.train_guard_trips}; steps through wn_adam_step_ext {opt.ext_steps}; '
        f'library {_lib.LIB_PATH}')
