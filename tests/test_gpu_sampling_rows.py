"""Sampling controls per utterance (semantics in include/wn_hip.h, struct wn_sampling_row) on the
GPU.  The Philox counter is (row, step) and the key is the seed, so row b of a call with per-row controls must be bit for
bit row b of the scalar call at the same B with row b's controls: every comparison here is torch.equal against the
scalar path, which test_gpu_sampling_controls.py and test_gpu_top_p.py hold against the oracle."""
import ctypes as C
import functools

import pytest
import torch

from test_gpu_parity import MODEL_CASES, O, dev, make_pair

pytestmark = pytest.mark.gpu

SA, SB, SC = 0x5EED1234ABCD, 0x0402, 0xFEDCBA9876543210        # three Philox keys, bits in both halves
OFF = 1.0
# (T, top_k, top_p, seed) of the five utterances: off | T | top_k | T, top_k and top_p | T and top_p
ROWS = [(1.0, 0, OFF, SA), (0.7, 0, OFF, SB), (1.0, 20, OFF, SA), (0.7, 20, 0.9, SC), (1.3, 0, 0.5, SB)]
# the same without top_p anywhere: no row sends the step to the sampler launch, so B <= 8 draws in the head launch (tail 2)
ROWS_NO_P = [(T, k, OFF, s) for T, k, p, s in ROWS]


def _kw(rows):
  T, k, p, s = zip(*rows)
  return dict(temperature=list(T), top_k=list(k), top_p=list(p), seed=list(s))


def _on(row):
  return row[0] != 1.0 or row[1] > 0 or row[2] < 1.0


@functools.lru_cache(maxsize=None)
def _net(name):
  if name == 'r128':       # the network of test_gpu_sampling_controls.py's 128-channel chain test
    kw = dict(blocks=5, channels=128, skip_channels=256, dilation_bound=16, final_layers_channels=[128, 64],
              activation='leaky_relu', bits=8, use_skip=True)
    return kw, make_pair(seed=17, bias_range=0.3, **kw)[2]
  if name.startswith('mix_'):   # the head-in-one-launch networks of test_queued_equals_sliding_window_mixture_head_in_one_launch
    channels, sampler, mix, finals = {'mix_64': (64, 'logistic', 10, [128, 256]), 'mix_32': (32, 'gaussian', 8, [64, 64]),
                                      'mix_128': (128, 'logistic', 5, [128, 128])}[name]
    kw = dict(blocks=6, channels=channels, skip_channels=256, dilation_bound=32, final_layers_channels=finals,
              activation='leaky_relu', num_mixtures=mix, sampling_function=sampler, bits=16)
    return kw, make_pair(seed=23, bias_range=0.3, **kw)[2]
  kw = dict(MODEL_CASES[name])
  return kw, make_pair(seed=11, bias_range=0.3, **kw)[2]


def _window(model, B, seed=12):
  return O.synthetic_waveform(B, model.receptive_field, seed=seed).to(dev())


def _check_rows(model, n, rows, queued, nonvacuous=True, **common):
  """The per-row call against one scalar call per distinct row of controls; returns the per-row result."""
  got = model.generate(n, use_queues=queued, **_kw(rows), **common)
  assert got.shape == (len(rows), n, 1)
  scalar, plain = {}, {}
  for b, row in enumerate(rows):
    T, k, p, s = row
    if row not in scalar:
      scalar[row] = model.generate(n, use_queues=queued, temperature=T, top_k=k, top_p=p, seed=s, **common)
    assert torch.equal(got[b], scalar[row][b]), (b, row, (got[b] - scalar[row][b]).abs().max())
    if nonvacuous and _on(row):
      if s not in plain:
        plain[s] = model.generate(n, use_queues=queued, seed=s, **common)
      assert not torch.equal(got[b], plain[s][b]), (b, row)
  return got


# ------------------------------------------------------------------------------------------
# 1. the row oracle, categorical heads
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [ROWS, ROWS_NO_P, ROWS[:3]], ids=['top_p_rows', 'top_p_off', 'three_rows'])
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'cat_small_fused', 'cat_lpb3'])
def test_row_oracle_categorical(name, queued, rows):
  """B = 5 enters the second 4-row block of the sampler kernels; without a top_p row cat_r64 draws in the head launch."""
  kw, model = _net(name)
  _check_rows(model, 14, rows, queued, sample=_window(model, len(rows)))


@pytest.mark.parametrize('queued', [True, False])
def test_row_oracle_without_a_sample_draws_each_rows_window_from_its_seed(queued):
  kw, model = _net('cat_r64')
  _check_rows(model, 14, ROWS, queued, batch_size=5)


# ------------------------------------------------------------------------------------------
# 2. the 128-channel chain, both forms
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['relay', 'one_workgroup'])
def test_row_oracle_128_channel_chain(form):
  from wavenets_amd import _lib
  kw, model = _net('r128')
  w = _window(model, 5, seed=3)
  _lib.lib().wn_debug_set(2, 1 if form == 'one_workgroup' else 0)
  try:
    queued = _check_rows(model, 24, ROWS, True, sample=w)
  finally:
    _lib.lib().wn_debug_set(2, 0)
  assert torch.equal(queued, model.generate(24, sample=w, use_queues=False, **_kw(ROWS)))


# ------------------------------------------------------------------------------------------
# 3. mixture heads
# ------------------------------------------------------------------------------------------
MIX_ROWS = [(T, 0, OFF, s) for T, s in zip([0.5, 1.0, 1.3, 1.0, 0.5], [SA, SB, SC, SA, SB])]


@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['mix_64', 'mix_32', 'mix_128', 'mol'])
def test_row_oracle_mixture_heads(name, queued):
  """Head, exact-fp32 last layer and mixture draw in one launch (tail 4), and 'mol' with its sampler in a launch of its own."""
  kw, model = _net(name)
  w = _window(model, 5, seed=6)
  _check_rows(model, 20, MIX_ROWS, queued, sample=w)
  with pytest.raises(ValueError, match='row 2.*top_k'):
    model.generate(4, sample=w, use_queues=queued, temperature=[0.5, 1.0, 1.3, 1.0, 0.5], top_k=[0, 0, 3, 0, 0])


# ------------------------------------------------------------------------------------------
# 4. where the index can go wrong
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
def test_row_oracle_sampler_launch_behind_the_head_at_9_utterances(queued):
  kw, model = _net('cat_r64')
  rows = [(1.0, 0, OFF, SA)] * 9
  rows[2], rows[7], rows[8] = (0.7, 0, OFF, SB), (1.0, 20, OFF, SC), (1.3, 5, OFF, SB)
  _check_rows(model, 14, rows, queued, sample=_window(model, 9))


@pytest.mark.parametrize('name', ['cat_r64', 'mix_64', 'r128'])
def test_row_oracle_second_workgroup_at_33_utterances(name):
  """Row 32 is the first row of the second 32-utterance workgroup of the chain and of the head launch: it must read
  record 32, not record 0."""
  kw, model = _net(name)
  cat = model.sampling_function == 'categorical'
  rows = [(1.0, 0, OFF, SA)] * 33
  rows[0], rows[31], rows[32] = (0.7, 0, OFF, SB), (1.3, 20 if cat else 0, OFF, SC), (0.5, 0, 0.8 if cat else OFF, SA)
  _check_rows(model, 14, rows, True, sample=_window(model, 33))


# ------------------------------------------------------------------------------------------
# 5. a uniform table through the C-ABI is the scalar entry
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [1, 0])
@pytest.mark.parametrize('ctl', [(1.0, 0, OFF, SA), (0.7, 20, OFF, SB), (0.7, 20, 0.9, SC)], ids=['off', 'on', 'top_p'])
@pytest.mark.parametrize('name', ['cat_r64', 'mix_64'])
def test_uniform_table_through_the_cabi_equals_the_scalar_entry(name, ctl, queued):
  from wavenets_amd import _lib
  from wavenets_amd.model import _RowControls
  kw, model = _net(name)
  T, k, p, s = ctl
  if model.sampling_function != 'categorical':
    k, p = 0, OFF
  B, n = 5, 14
  w = _window(model, B)
  want = model.generate(n, sample=w, use_queues=bool(queued), temperature=T, top_k=k, top_p=p, seed=s)
  L = _lib.lib()
  entry = model._sampling(T, k, s, 2 ** model.bits, p)
  ctrl = _RowControls([entry] * B, None, _lib.HEADS[model.sampling_function], 2 ** model.bits)
  assert [r.stream for r in ctrl.host] == list(range(B))
  table = ctrl.device_table(dev())
  ws = torch.zeros(int(L.wn_generate_workspace_floats(model._plan, B, queued)), dtype=torch.float32, device=dev())
  out = torch.empty(B, n, 1, dtype=torch.float32, device=dev())
  _lib.check(L.wn_generate_rows_chunk(model._plan, _lib.ptr(model.flat_params), _lib.ptr(w), None, B, 0, n, 0, queued,
                                      _lib.ptr(table), ctrl.flags, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
  torch.cuda.synchronize()
  slot = L.wn_generate_guard_slot(model._plan, B, queued)
  assert float(ws[slot]) < L.wn_range_limit()
  assert torch.equal(out, want), (out - want).abs().max()


# ------------------------------------------------------------------------------------------
# 6. sessions
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name,rows', [('cat_r64', ROWS), ('cat_r64', ROWS_NO_P), ('mix_32', MIX_ROWS)],
                         ids=['cat_top_p', 'cat_head_tail', 'mix'])
def test_session_chunks_and_stream_equal_the_one_call(name, rows, queued):
  kw, model = _net(name)
  w = _window(model, 5)
  one = model.generate(14, sample=w, use_queues=queued, **_kw(rows))
  session = model.generation_session(sample=w, use_queues=queued, **_kw(rows))
  pieces = [session.generate(n) for n in (1, 1, 5, 7)]
  assert torch.equal(torch.cat(pieces, 1), one)
  streamed = list(model.generate_stream(14, 4, sample=w, use_queues=queued, **_kw(rows)))
  assert [t.shape[1] for t in streamed] == [4, 4, 4, 2]
  assert torch.equal(torch.cat(streamed, 1), one)


# ------------------------------------------------------------------------------------------
# 7. exact_fp32()
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name,rows', [('cat_r64', ROWS), ('mix_64', MIX_ROWS)], ids=['cat', 'mix'])
def test_row_oracle_in_exact_fp32(name, rows, queued):
  kw, model = _net(name)
  with model.exact_fp32():
    _check_rows(model, 14, rows, queued, sample=_window(model, 5))


# ------------------------------------------------------------------------------------------
# 8. top_k = 1 on one row is that row's arg max
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('queued', [True, False])
def test_top_k_1_on_one_row_is_the_deterministic_row(queued):
  kw, model = _net('cat_r64')
  w = _window(model, 5)
  det = model.generate(40, sample=w, use_queues=queued, deterministic=True)
  got = model.generate(40, sample=w, use_queues=queued, top_k=[0, 0, 1, 0, 0], temperature=[1.0, 0.7, 0.6, 1.0, 1.3],
                       seed=[SA, SB, SC, SA, SB])
  assert torch.equal(got[2], det[2])
  for b in (0, 1, 3, 4):
    assert not torch.equal(got[b], det[b]), b


# ------------------------------------------------------------------------------------------
# 9. / 10. streams: a request keeps its draws whichever slot it lands in, and whatever the batch around it
# ------------------------------------------------------------------------------------------
PERM = [3, 0, 4, 1, 2]


def _stream_batch(name, queued):
  from test_gpu_parity import _inputs
  kw, model = _net(name)
  w = _window(model, 5)
  cond = None
  if kw.get('conditioning') is not None:
    cond = _inputs(kw, 5, 4)[1].to(dev())
  rows = ROWS if name != 'cond' else ROWS_NO_P
  out = model.generate(16, sample=w, condition=cond, use_queues=queued, stream=[0, 1, 2, 3, 4], **_kw(rows))
  return model, w, cond, rows, out


@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'cond'])
def test_streams_follow_the_request_through_a_permutation(name, queued):
  model, w, cond, rows, out = _stream_batch(name, queued)
  # stream = 0 .. B - 1 is stream=None
  assert torch.equal(out, model.generate(16, sample=w, condition=cond, use_queues=queued, **_kw(rows)))
  idx = torch.tensor(PERM, device=w.device)
  permuted = model.generate(16, sample=w[idx].contiguous(), condition=None if cond is None else cond[idx].contiguous(),
                            use_queues=queued, stream=PERM, **_kw([rows[j] for j in PERM]))
  assert torch.equal(permuted, out[idx])
  # duplicates: two slots with the same request make the same audio
  twice = model.generate(16, sample=w[[1, 1, 2]].contiguous(), condition=None if cond is None else cond[[1, 1, 2]].contiguous(),
                         use_queues=queued, stream=[1, 1, 2], **_kw([rows[1], rows[1], rows[2]]))
  assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], out[1]) and torch.equal(twice[2], out[2])


@pytest.mark.parametrize('queued', [True, False])
@pytest.mark.parametrize('name', ['cat_r64', 'cond'])
def test_a_request_alone_draws_what_it_draws_in_the_batch(name, queued):
  """B = 1 with stream = [j] against row j of the batch of five: the row arithmetic of every kernel on the way does not
  depend on B."""
  model, w, cond, rows, out = _stream_batch(name, queued)
  for j in range(5):
    alone = model.generate(16, sample=w[j:j + 1].contiguous(), condition=None if cond is None else cond[j:j + 1].contiguous(),
                           use_queues=queued, stream=[j], **_kw([rows[j]]))
    assert torch.equal(alone[0], out[j]), (j, (alone[0] - out[j]).abs().max())
