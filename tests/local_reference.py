"""fp64 restatement of WaveNet.call with conditioning='local' (src/model.py:216-220), built from the oracle's public
functions only: causal_conv1d, conv1x1, activation, layer_forward(..., cond=(B, T, Cc)), loss_fn, prepare_target,
init_params.  The oracle's own model_forward keeps raising for 'local'.

The reference maps the condition with 1x1 convolutions at the frame rate and repeats the result `hop` times.  A 1x1
convolution acts on every time step alone, so mapping the repeated condition gives the same tensor: the restatement takes
the condition per SAMPLE, (B, T, Cin) = upsample(frames, hop), maps it there and hands every block its (B, T, Cc) rows.

Parameters are the list of the GLOBAL configuration of the same network (oracle.param_shapes has no mapping tensors for
'local'): the Dense kernels (cin, w) are the 1x1 kernels (1, cin, w) without the leading axis.
"""
from dataclasses import replace

import torch

from oracle import wavenet_oracle as O


def global_cfg(cfg):
  """The configuration whose parameter list a local network shares."""
  return replace(cfg, conditioning='global')


def upsample(frames, hop):
  """(B, F[, Cin]) -> (B, F * hop, Cin): tf.repeat(condition, hop, axis=1)."""
  if frames.dim() == 2:
    frames = frames.unsqueeze(-1)                # the reference's expand_dims (src/model.py:133)
  return torch.repeat_interleave(frames, hop, dim=1)


def mapped(cond_up, params, cfg):
  """The mapping stack on per-sample rows (B, T, Cin) -> (B, T, Cc)."""
  g = global_cfg(cfg)
  npb = O._params_per_block(g)
  off = 2 + g.blocks * npb + 2 * (len(g.final_layers_channels) + 1)
  m = cond_up
  for j in range(len(O.mapping_widths(g))):
    m = O.activation(O.conv1x1(m, params[off + 2 * j].unsqueeze(0), params[off + 2 * j + 1]), g.mapping_activation)
  return m


def local_forward(x, params, cfg, cond_up, return_logits=False):
  """x (B, T, 1), cond_up (B, T, Cin): probabilities (categorical) or mixture parameters, as O.model_forward."""
  g = global_cfg(cfg)
  dil = O.dilation_schedule(g)
  c = mapped(cond_up, params, cfg)
  h = O.causal_conv1d(x, params[0], params[1], 1)
  npb, lpb = O._params_per_block(g), g.layers_per_block
  pos, skips = 2, []
  for b in range(g.blocks):
    lp = params[pos:pos + npb]
    pos += npb
    h, sk = O.layer_forward(h, lp, dilations=dil[b * lpb:(b + 1) * lpb], activation_name=g.activation,
                            residual=g.use_residual, has_skip=g.skip_channels is not None, cond=c)
    skips.append(sk)
  if g.use_skip:
    h = skips[0]
    for sk in skips[1:]:
      h = h + sk
  for i in range(len(g.final_layers_channels)):
    h = O.activation(O.conv1x1(h, params[pos], params[pos + 1]), g.activation)
    pos += 2
  logits = O.conv1x1(h, params[pos], params[pos + 1])
  if g.num_mixtures is None and not return_logits:
    return torch.softmax(logits, dim=-1)
  return logits


def local_loss_rows(x_full, params, cfg, frames, hop):
  """Per-row losses (B, T) of the training-form call: inputs x[:, :-1], targets prepare_target(x[:, 1:])."""
  g = global_cfg(cfg)
  pred = local_forward(x_full[:, :-1, :], params, cfg, upsample(frames, hop))
  return O.loss_fn(O.prepare_target(x_full[:, 1:, :], g), pred, g)


def local_loss_and_grads(x_full, params, cfg, frames, hop, global_batch=None):
  """loss = sum l / global_batch; gradients of every parameter and of the frames (autograd).
  Returns (loss, parameter gradients, gradient at the frames in their own shape)."""
  ps = [p.detach().clone().requires_grad_(True) for p in params]
  fr = frames.detach().clone().requires_grad_(True)
  per = local_loss_rows(x_full, ps, cfg, fr, hop)
  loss = per.sum() / (x_full.shape[0] if global_batch is None else global_batch)
  grads = torch.autograd.grad(loss, ps + [fr], allow_unused=True)
  grads = [gr if gr is not None else torch.zeros_like(p) for gr, p in zip(grads, ps + [fr])]
  return loss.detach(), grads[:-1], grads[-1]


# ---- generation (tests/test_gpu_local_cond_generation.py; the reference-alone pin in tests/test_local_cond_cpu.py) ----
GEN_B, GEN_F = 3, 3
GEN_NETS = {
    'r64': dict(blocks=3, channels=64, skip_channels=64, dilation_bound=4, final_layers_channels=[64], activation='relu',
                mapping_layers=[8], mapping_activation='tanh', bits=6, cond_inputs=3),
    'r128': dict(blocks=3, channels=128, skip_channels=128, dilation_bound=4, final_layers_channels=[128],
                 activation='leaky_relu', bits=6, cond_inputs=3),
}
GEN_SEED = {'r64': 13, 'r128': 4}         # parameter seeds for which the greedy rollout below is clear of ties


def gen_cfg(name):
  return O.OracleConfig(**GEN_NETS[name], conditioning='local')


def gen_params(name):
  return [p.double() for p in O.init_params(global_cfg(gen_cfg(name)), seed=GEN_SEED[name])]


def gen_inputs(name, hop):
  """The prompt window (B, RF, 1) and the frames (B, F, Cin)."""
  rf = O.receptive_field(global_cfg(gen_cfg(name)))
  g = torch.Generator().manual_seed(21)
  window = torch.rand(GEN_B, rf, 1, generator=g) * 2 - 1
  frames = torch.rand(GEN_B, GEN_F, GEN_NETS[name]['cond_inputs'], generator=g) * 2 - 1
  return window, frames


def gen_condition(frames, rf, steps, hop):
  """The per-sample condition of a generated sequence's inputs x = [window, y_0 .. y_{steps-2}]: the priming pass over
  the window (inputs 0 .. rf - 1, the last of which emits y_0) holds frame 0; the step that emits y_g, g >= 1, reads the
  input at rf - 1 + g with frame g // hop."""
  idx = [0] * (rf - 1) + [g // hop for g in range(steps)]
  return frames[:, idx, :]


def teacher_forced_probs(name, window, samples, frames, hop):
  """fp64 probabilities (B, steps, classes) of every generated sample given the sequence that was generated."""
  rf, steps = window.shape[1], samples.shape[1]
  seq = torch.cat([window, samples], 1).double()
  probs = local_forward(seq[:, :-1], gen_params(name), gen_cfg(name), gen_condition(frames.double(), rf, steps, hop))
  return probs[:, rf - 1:]


def greedy_rollout(name, hop):
  """The restatement's own arg-max sequence of F * hop samples and the top-2 probability margin of every step."""
  window, frames = gen_inputs(name, hop)
  cfg, params = gen_cfg(name), gen_params(name)
  rf, steps = window.shape[1], GEN_F * hop
  seq, margins = window.double(), []
  with torch.no_grad():
    for g in range(steps):
      cond = gen_condition(frames.double(), rf, g + 1, hop)
      p = local_forward(seq, params, cfg, cond)[:, -1]
      top = torch.topk(p, 2, dim=-1).values
      margins.append(top[:, 0] - top[:, 1])
      nxt = O.sample_waveform_deterministic(p[:, None, :], global_cfg(cfg)).double()
      seq = torch.cat([seq, nxt.reshape(GEN_B, 1, 1)], 1)
  return seq[:, rf:], torch.stack(margins, 1)
