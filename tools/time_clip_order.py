"""What Adam(clip_before_reduce=True) costs per step: BASELINE configs[1] (8 x 16000) under a world-size-1 RCCL process
group -- the data-parallel step path, one collective per step -- with the flag off and on, alternated in one process.

  python tools/time_clip_order.py [--steps 40] [--runs 3]         step time, flag off / on alternated, `runs` blocks each
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_clip_order.py --profile
                                                                  a few flag-on steps: wn_clip_kernel's own time
"""
import argparse, os, socket, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
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
sk = socket.socket()
sk.bind(('127.0.0.1', 0))
port = sk.getsockname()[1]
sk.close()
dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=0, world_size=1, device_id=dev)
m = WaveNet(**bench.CFG2, device=dev, seed=0)
opt = Adam(learning_rate=5e-4, clipnorm=1.0)
m.compile(optimizer=opt, metrics=[MeanSquaredError()])
x = synthetic_waveforms(8, 16001, seed=99, device=dev)


def block(flag, n):
  opt.clip_before_reduce = flag
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    m.train_step(x)
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


if args.profile:
  block(True, 12)
else:
  for flag in (False, True):                              # both shapes of the step warmed up
    block(flag, 10)
  ms = {False: [], True: []}
  for _ in range(args.runs):
    for flag in (False, True):
      ms[flag].append(block(flag, args.steps))
  for flag in (False, True):
    print(f'clip_before_reduce={flag}: ' + ' '.join(f'{v:.3f}' for v in ms[flag]) +
          f' ms/step ({args.steps} steps per run), median {statistics.median(ms[flag]):.3f}')
  print(f'difference of the medians: {(statistics.median(ms[True]) - statistics.median(ms[False])) * 1e3:+.1f} us; '
        f'guard trips {m.train_guard_trips}')
  nt = len(m.variable_names)
  block(True, 1)
  print(f'{int((opt._scratch[:nt] > 1.0).sum())} of {nt} tensors exceed clipnorm 1.0 in the last step (rescaled in place)')
dist.destroy_process_group()
