"""Admission into a running batch on BASELINE configs[1] weights, B = 8, queued.
default: 20 admissions of k = 1 and of k = 4 into a running session, by host clock around the 20 calls ending in a
  synchronise, against the alternative without admission: beginning the session of 8 rows again (reset, then its first
  chunk of length 1); the three forms alternate, three runs each; ms per call.
--steps: us per step over 2000 steps of a session (the step path of a continuation), three runs.  WN_TREE names another
  checkout of the project to import instead of this one (A/B against the parent commit, one process per run).
--origin none|zeros|mixed (with --steps): the session without an origin array, with one of zeros
  (own_clock=True at start = 0), or with mixed origins (rows 0 .. 3 admitted by admit_own_clock before the clock starts).
--cfg3: BASELINE configs[3] weights (128 residual channels, MoL-10) instead of configs[1].
--own-clock (without --steps): the admissions by admit_own_clock."""
import os, sys, time
ROOT = os.environ.get('WN_TREE') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wavenets_amd import WaveNet
import bench

B, REPS = 8, 20
dev = torch.device('cuda', 0)
origin = sys.argv[sys.argv.index('--origin') + 1] if '--origin' in sys.argv else 'none'
own = '--own-clock' in sys.argv
cfg3 = '--cfg3' in sys.argv
m = WaveNet(**(bench.OTHER_CONFIGS['configs[3]'][0] if cfg3 else bench.CFG2), device=dev)
rf = m.receptive_field
gen = torch.Generator().manual_seed(0)
w = (torch.rand(B, rf, 1, generator=gen) * 2 - 1).to(dev)
args = dict(sample=w, use_queues=True, stream=list(range(B)), temperature=[1.0, 0.7] * (B // 2))


def clock(fn, per):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / per


if '--steps' in sys.argv:
  N = 2000
  s = m.generation_session(**args, **(dict(own_clock=True) if origin == 'zeros' else {}))
  s.generate(1)
  if origin == 'mixed':
    s.admit_own_clock([0, 1, 2, 3], (torch.rand(4, rf, 1, generator=gen) * 2 - 1).to(dev), stream=[100, 101, 102, 103],
                      temperature=0.8)
  s.generate(200)                                         # warm-up of the step path
  runs = [clock(lambda: s.generate(N), N) * 1e6 for _ in range(3)]
  print(f'{os.path.basename(ROOT)}{" cfg3" if cfg3 else ""} origin={origin}: B={B} {N} steps, us/step ' + ' '.join(f'{v:.2f}' for v in runs) +
        f' (median {sorted(runs)[1]:.2f})', flush=True)
  sys.exit(0)

s = m.generation_session(**args)
s.generate(1)
s.generate(16)
again = m.generation_session(**args)
new = {k: (torch.rand(k, rf, 1, generator=gen) * 2 - 1).to(dev) for k in (1, 4)}


def admit(k):
  for i in range(REPS):
    (s.admit_own_clock if own else s.admit)(list(range(k)), new[k], stream=[100 + i * k + j for j in range(k)], temperature=0.8)


def begin_again():
  for _ in range(REPS):
    again.reset()
    again.generate(1)


forms = [('admit, k = 1', lambda: admit(1)), ('admit, k = 4', lambda: admit(4)), ('begin the 8 rows again', begin_again)]
for _, fn in forms:
  fn()                                                    # warm-up: scratch workspaces, tables
runs = {name: [] for name, _ in forms}
for _ in range(3):
  for name, fn in forms:
    runs[name].append(clock(fn, REPS) * 1e3)
for name, _ in forms:
  print(f'{name}{", own_clock" if own else ""}: B={B}, ms per call ' + ' '.join(f'{v:.3f}' for v in runs[name]) + f' (median {sorted(runs[name])[1]:.3f})',
        flush=True)
assert not s.exact and m.generation_guard_trips == 0
