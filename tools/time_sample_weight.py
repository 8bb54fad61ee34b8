"""What sample_weight costs per step: at the BASELINE configs[1] shape (8 x 16000, 256 classes), in
one process, host clocks around `steps` steps after `warmup`, `runs` windows each, alternated:

  train_step(x, sample_weight=w)     w = length_weights of lengths between 8000 and 16000
  train_step(x)
  the custom-loss route of section 20: differentiable('logits', training=True) + masked cross_entropy + backward +
  optimizer.apply_gradients (configs[1] only: it is the route sample_weight replaces)

and the first two at configs[3] (mixture of logistics), one window each.

  python tools/time_sample_weight.py [--steps 20] [--warmup 5] [--runs 3]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_sample_weight.py --profile     a few weighted and unweighted steps
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from wavenets_amd import WaveNet, Adam, MeanSquaredError
from wavenets_amd.data import synthetic_waveforms, length_weights

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--profile', action='store_true')
args = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
B, T = 8, 16000
x = synthetic_waveforms(B, T + 1, seed=99, device=dev)
lengths = torch.randint(8000, 16001, (B,), generator=torch.Generator().manual_seed(3))
w = length_weights(lengths, T, device=dev)


def window(fn, n):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


def measure(name, kw, runs, custom):
  m = WaveNet(**kw, device=dev, seed=0)
  m.compile(optimizer=Adam(learning_rate=5e-4, clipnorm=1.0), metrics=[MeanSquaredError()])
  target = m.prepare_target(x[:, 1:, 0]).long() if custom else None

  def custom_step():
    logits = m.differentiable(x[:, :-1, :], training=True, output='logits')
    per = torch.nn.functional.cross_entropy(logits.reshape(B * T, -1), target.reshape(-1), reduction='none')
    ((per * w.reshape(-1)).sum() / B).backward()
    m.optimizer.apply_gradients(m)
  steps = {'train_step(x, sample_weight=w)': lambda: m.train_step(x, sample_weight=w), 'train_step(x)': lambda: m.train_step(x)}
  if custom:
    steps["differentiable('logits') + masked cross_entropy"] = custom_step
  if args.profile:
    for fn in steps.values():
      window(fn, 6)
    return
  for fn in steps.values():
    window(fn, args.warmup)
  ms = {k: [] for k in steps}
  for _ in range(runs):
    for k, fn in steps.items():
      ms[k].append(window(fn, args.steps))
  for k, v in ms.items():
    print(f'{name} {k}: ' + ' '.join(f'{t:.3f}' for t in v) + f' ms/step ({args.steps} steps per window), median '
          f'{statistics.median(v):.3f}, spread {max(v) - min(v):.3f}', flush=True)
  print(f'{name}: sum w / (B T) = {float(w.mean()):.3f}; guard trips {m.train_guard_trips}', flush=True)
  del m
  torch.cuda.empty_cache()


measure('configs[1]', bench.CFG2, args.runs, True)
measure('configs[3]', bench.OTHER_CONFIGS['configs[3]'][0], 1, False)
