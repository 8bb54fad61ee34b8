"""Generation speed (the reference prints 'Speed of generation was ... samples/s', train.py:253-261):
naive sliding window vs queued ring buffers on BASELINE configs[1] weights, batch B.
--temperature T / --top-k K / --top-p P anywhere on the command line: the sampling controls of the stochastic leg.
--chunked: instead of the legs, 4000 queued stochastic samples as one call and as generation sessions at chunk sizes
16, 256 and 4000, alternating, three runs each, in us per step."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
controls = {}
for flag, key, conv in (('--temperature', 'temperature', float), ('--top-k', 'top_k', int), ('--top-p', 'top_p', float)):
  if flag in sys.argv:
    i = sys.argv.index(flag)
    controls[key] = conv(sys.argv[i + 1])
    del sys.argv[i:i + 2]
chunked = '--chunked' in sys.argv
if chunked:
  sys.argv.remove('--chunked')
import torch
from wavenets_amd import WaveNet
import bench

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
dev = torch.device('cuda', 0)
# second argument 'cfg3': BASELINE configs[3] weights (128 residual channels, MoL-10) instead of configs[1]
kw = bench.OTHER_CONFIGS['configs[3]'][0] if len(sys.argv) > 2 and sys.argv[2] == 'cfg3' else bench.CFG2
m = WaveNet(**kw, device=dev)
# further arguments: KEY VAL pairs of debug knobs (wavenets_amd/csrc/wn_error.cpp)
from wavenets_amd import _lib
for k_, v_ in zip(sys.argv[3::2], sys.argv[4::2]):
  _lib.lib().wn_debug_set(int(k_), int(v_))
w = (torch.rand(B, m.receptive_field, 1, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
if chunked:
  # --chunked: queued stochastic generation of N samples as one generate call and as generation sessions at three chunk
  # sizes; the forms alternate, three runs each; us per step (priming pass included in every form)
  N = 4000
  args = dict(sample=w, use_queues=True, deterministic=False, **controls)

  def session(chunk):
    return torch.cat(list(m.generate_stream(N, chunk, **args)), dim=1)
  forms = [('one-shot generate', lambda: m.generate(N, **args))] + \
          [(f'session, chunk {c}', (lambda c=c: session(c))) for c in (16, 256, 4000)]
  ref = forms[0][1]()
  for name, fn in forms:
    assert torch.equal(fn(), ref), name                       # (and the warm-up of the form)
  runs = {name: [] for name, _ in forms}
  for _ in range(3):
    for name, fn in forms:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      runs[name].append((time.perf_counter() - t0) / N * 1e6)
  for name, _ in forms:
    print(f'{name}: B={B} {N} samples/utterance, us/step ' + ' '.join(f'{v:.2f}' for v in runs[name]) +
          f' (median {sorted(runs[name])[1]:.2f})')
  sys.exit(0)
legs = [('naive', False, 20, True), ('queued', True, 400, True), ('queued, stochastic draws', True, 400, False)]
if controls:
  legs = [(f'queued, stochastic draws, {controls}', True, 400, False)]
for name, queued, n, det in legs:
  kw_ = {} if det else controls
  m.generate(3, sample=w, use_queues=queued, deterministic=det, **kw_)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  out = m.generate(n, sample=w, use_queues=queued, deterministic=det, **kw_)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  print(f'{name}: B={B} {n} samples/utterance in {dt:.3f} s -> {n / dt:.1f} samples/s per utterance, '
        f'{B * n / dt:.1f} samples/s aggregate, {dt / n * 1e3:.3f} ms/step')
