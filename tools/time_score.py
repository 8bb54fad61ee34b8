"""What a scoring pass costs against the evaluation pass: wn_score and wn_eval_loss at the C-ABI, at the
BASELINE configs[1] shape (8 x 16000, 256 classes: the loss rows come from the last conv's evaluation epilogue, no logits are
written) and at configs[3] (mixture of logistics: the standalone loss kernel either way).  Host clocks around `steps` calls
ending in a device synchronise, after `warmup` calls, `runs` windows each, alternated in one process.

  python tools/time_score.py [--steps 20] [--warmup 5] [--runs 3] [--only score|eval]

--only eval touches nothing but wn_eval_loss, so the same file also times a build of the library that has no wn_score (another
checkout's, started from that checkout as a process of its own).
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from wavenets_amd import WaveNet, _lib
from wavenets_amd.data import synthetic_waveforms

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--only', choices=['score', 'eval'], default=None)
args = ap.parse_args()

dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
B, T = 8, 16000
x = synthetic_waveforms(B, T + 1, seed=99, device=dev)


def window(fn, n):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / n * 1e3


def measure(name, kw):
  m = WaveNet(**kw, device=dev, seed=0)
  m.build(tuple(x.shape))
  L = _lib.lib()
  ws = m._workspace('fwd', L.wn_plan_workspace_floats(m._plan, B, T, 0))
  out = torch.zeros(2 * B + 4, dtype=torch.float32, device=dev)
  nll, weight, flag, loss = out[:B], out[B:2 * B], out[2 * B:2 * B + 1], out[2 * B + 1:]
  s = _lib.stream_ptr()
  calls = {}
  if args.only != 'eval':
    calls['wn_score'] = lambda: _lib.check(L.wn_score(m._plan, _lib.ptr(m.flat_params), _lib.ptr(x), None, B, T, _lib.ptr(nll),
                                                      _lib.ptr(weight), None, _lib.ptr(flag), _lib.ptr(ws), ws.numel(), s))
  if args.only != 'score':
    calls['wn_eval_loss'] = lambda: _lib.check(L.wn_eval_loss(m._plan, _lib.ptr(m.flat_params), _lib.ptr(x), None, B, T, B,
                                                              _lib.ptr(loss), None, _lib.ptr(ws), ws.numel(), s))
  for fn in calls.values():
    window(fn, args.warmup)
  ms = {k: [] for k in calls}
  for _ in range(args.runs):
    for k, fn in calls.items():
      ms[k].append(window(fn, args.steps))
  for k, v in ms.items():
    print(f'{name} {k}: ' + ' '.join(f'{t:.3f}' for t in v) + f' ms/call ({args.steps} calls per window), median '
          f'{statistics.median(v):.3f}, spread {max(v) - min(v):.3f}', flush=True)
  vals = out.tolist()
  print(f'{name}: range flags {vals[2 * B]} / {vals[2 * B + 3]}; sum nll / B {sum(vals[:B]) / B if args.only != "eval" else None}, '
        f'eval loss {vals[2 * B + 1] if args.only != "score" else None}', flush=True)
  del m
  torch.cuda.empty_cache()


measure('configs[1]', bench.CFG2)
measure('configs[3]', bench.OTHER_CONFIGS['configs[3]'][0])
