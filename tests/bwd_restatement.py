"""What every kernel of the block stack's forward, of the head's forward and the loss, and of the backward phase of one
training pass should have produced FROM ITS OWN INPUTS, in float64.

Not a conftest and not a test: a plain helper (tests/test_bwd_restatement_cpu.py pins it against fp64 autograd of the
oracle, tests/test_gpu_bwd_tile_walk.py, tests/test_gpu_deep_tile_walk.py and tests/test_gpu_head_tile_walk.py compare
the HIP kernels with it).  It is plain torch float64 on whatever device its inputs live on and never calls into libwn_hip.

A product is restated from the tensors its kernel read, not from other restated values: `GH[b]` from the stored `GU[b]`
and `GH[b+1]`, `GU[b]` from the stored `GH[b+1]`, `AG[b]`, `Z[b]` and so on.  An error in one kernel therefore shows in
that kernel's tensor alone, at the size of the error, and a chain of 7 blocks does not blur it.

Scope: any `layers_per_block`, with or without dropout, time-invariant (global) conditioning; `restate` is the backward
phase (DESIGN.md sections 18, 19), `restate_forward` the block stack's forward, the input conv and the skip sum (section
19), `restate_head` the head's forward, the loss rows, the loss and GF[nf] = d loss / d logits (section 24).  `restate`
itself still takes HA and GF[nf] as given: they are outputs of `restate_head`, each from the tensors its own kernel read.

Notation: block b has the convs i = 0..L-1 (L = layers_per_block) with dilations d_i = dilation_schedule[b L + i].  Conv 0
reads X_0 = XD[b] under dropout and H[b] otherwise, conv i > 0 reads X_i = P[b][i-1]; the output gradient of the last conv
is G_{L-1} = GU[b], that of an inner conv G_i = GP[b][i], taken at its PRE-activation output.

Workspace tensors (`ws`, keyed as below, each `(B, T, channels)`; regions of WaveNet.training_intermediate):

  ('H', b)  b = 0..N    region 0   block inputs; H[N] is the last block's output
  ('Z', b)  b = 0..N-1  region 1   gated activation tanh * sigmoid (leading dimension Dp >= D: the first D columns count)
  ('AG', b)             region 2   saved sigmoid gate
  ('HA', i) i = 0..nf-1 region 4   head activations (post-activation output of final conv i)
  ('GF', i) i = 0..nf   region 6   d loss / d (output of final conv i, pre-activation); GF[nf] = d loss / d logits is the
                                   loss epilogue's: `restate` takes it as given, `restate_head` restates it
  'logits'              region 5   the head's output, where the pass wrote it (not under the fused loss epilogue)
  ('GU', b)             region 8   d loss / d u of block b, [filter half | gate half]
  ('GH', b) b = 0..N    region 9   d loss / d H[b]
  'skipsum', 'g_skipsum' regions 3, 7   unfolded passes with use_skip only
  ('P', b, i)  i = 0..L-2  region 11  activated output of inner conv i of block b
  ('GP', b, i) i = 0..L-2  region 13  d loss / d (pre-activation output of inner conv i of block b)
  ('XD', b)                region 14  dropped copy of H[b] (dropout passes only)
"""
import functools

import numpy as np
import torch

from oracle import wavenet_oracle as O


def _shift_back(x, s):
  """y[:, t] = x[:, t - s] (zero before the utterance's start)."""
  if s == 0:
    return x
  y = torch.zeros_like(x)
  if s < x.shape[1]:
    y[:, s:] = x[:, :x.shape[1] - s]
  return y


def _shift_fwd(x, s):
  """y[:, t] = x[:, t + s]: zero where the index reaches T, never crossing into the next utterance."""
  if s == 0:
    return x
  y = torch.zeros_like(x)
  if s < x.shape[1]:
    y[:, :x.shape[1] - s] = x[:, s:]
  return y


def _rows(x):
  return x.reshape(-1, x.shape[-1])


def _outer(a, b):
  """a^T b over every row of every utterance."""
  return _rows(a).T @ _rows(b)


def dact_from_output(y, name):
  """Derivative of a head activation through its OUTPUT (wn_dact_from_y in wn_common.h)."""
  if name is None or name == 'linear':
    return torch.ones_like(y)
  if name == 'relu':
    return (y > 0).to(y.dtype)
  if name == 'leaky_relu':
    return torch.where(y >= 0, torch.ones_like(y), torch.full_like(y, O.LEAKY_SLOPE))
  if name == 'tanh':
    return 1 - y * y
  if name == 'sigmoid':
    return y * (1 - y)
  if name == 'elu':
    return torch.where(y > 0, torch.ones_like(y), y + 1)
  raise NotImplementedError(name)


def gate_bwd(g_z, ag, z):
  """wn_gate_bwd (wn_common.h) in fp64 from the saved sigmoid g and z = tanh * g: a = z / g is the tanh;
  d/du_f = g_z g (1 - a^2), d/du_g = g_z a g (1 - g) = g_z z (1 - g).  (g underflowed: both vanish.)"""
  a = torch.where(ag > 1e-30, z / ag.clamp_min(1e-30), torch.zeros_like(z))
  return torch.cat([g_z * ag * (1 - a * a), g_z * z * (1 - ag)], dim=-1)


@functools.lru_cache(maxsize=8)
def _keep_cpu(n, key, rate):
  return O.dropout_keep_mask(n, key, rate)


def drop_scale(rate):
  """s = 1 / (1 - rate) as wn_launch_dropout forms it: in float32."""
  return float(np.float32(1) / (np.float32(1) - np.float32(rate)))


def keep_mask(like, b, dropout):
  """keep_b of block b over the elements of `like` (B, T, R) in their workspace order; dropout = (rate, seed, step)."""
  rate, seed, step = dropout
  return _keep_cpu(like.numel(), O.dropout_key(seed, b, step), rate).view(like.shape).to(like.device)


def _conv(x, w, bias, d):
  """Causal dilated conv: sum_j shift_back(x, (KS - 1 - j) d) W[j] + bias."""
  KS = w.shape[0]
  return sum(_shift_back(x, (KS - 1 - j) * d) @ w[j] for j in range(KS)) + bias


def _mapped(cfg, P, cond):
  m = cond
  for j in range(len(O.mapping_widths(cfg))):
    m = O.activation(m @ P[f'mapping{j}/kernel'] + P[f'mapping{j}/bias'], cfg.mapping_activation)
  return m


def restate_forward(cfg, params, x_in, cond, ws, folded, dropout=None):
  """The block stack's forward, the input conv and the skip sum; arguments as for `restate`.  ws needs H, Z, P and, under
  dropout, XD.

  Returns {key: float64 tensor}: ('H', b) for b = 0..N, ('XD', b) under dropout, ('P', b, i), ('AG', b), ('Z', b) and
  'skipsum' (unfolded passes with use_skip).

  XD[b] = where(keep_b, H[b] s, 0): the kernel does ONE fp32 multiply.  For float32-valued H the float64 product H s is
  exact (24 + 24 significant bits), so rounding the returned tensor to float32 once IS that multiply and the comparison with
  the kernel's XD is bitwise; for float64 H (the CPU pin) it is the oracle's own expression."""
  N, L, D = cfg.blocks, cfg.layers_per_block, cfg.D
  dil = O.dilation_schedule(cfg)
  P = params
  drop = dropout is not None and dropout[0] > 0
  out = {('H', 0): _conv(x_in, P['causal/kernel'], P['causal/bias'], 1)}
  crow = None
  if cfg.conditioning == 'global':
    crow = _mapped(cfg, P, cond)[:, None, :]         # (B, 1, Cc): the same row for every t of an utterance
  for b in range(N):
    x = ws['H', b]
    if drop:
      out['XD', b] = torch.where(keep_mask(x, b, dropout), x * drop_scale(dropout[0]), torch.zeros_like(x))
      x = ws['XD', b]
    for i in range(L - 1):
      out['P', b, i] = O.activation(_conv(x, P[f'block{b}/dil{i}/kernel'], P[f'block{b}/dil{i}/bias'], dil[b * L + i]),
                                    cfg.activation)
      x = ws['P', b, i]
    u = _conv(x, P[f'block{b}/dil{L - 1}/kernel'], P[f'block{b}/dil{L - 1}/bias'], dil[b * L + L - 1])
    if crow is not None:
      u = u + crow @ P[f'block{b}/conv_cond/kernel'][0] + P[f'block{b}/conv_cond/bias']
    ag = torch.sigmoid(u[..., D:])
    out['AG', b] = ag
    out['Z', b] = torch.tanh(u[..., :D]) * ag
    h = ws['Z', b][..., :D] @ P[f'block{b}/conv1/kernel'][0] + P[f'block{b}/conv1/bias']
    out['H', b + 1] = h + ws['H', b] if cfg.use_residual else h          # the residual is the UNDROPPED block input
  if cfg.use_skip and not folded:
    conv = 'conv_skip' if cfg.skip_channels is not None else 'conv1'     # (no skip convs: the pre-residual 1x1 output)
    out['skipsum'] = sum(ws['Z', b][..., :D] @ P[f'block{b}/{conv}/kernel'][0] + P[f'block{b}/{conv}/bias']
                         for b in range(N))
  return out


def _loss_rows(cfg, target, pred):
  """Per-row loss of a (rows, Cout) head output in fp64: the categorical reference is Keras's (clip to [1e-7, 1 - 1e-7] and
  renormalise) on the soft-max, the logistic one the form that is exact in both tails."""
  if cfg.sampling_function == 'categorical':
    return O.loss_categorical(target, torch.softmax(pred, dim=-1))
  if cfg.sampling_function == 'logistic':
    return O.loss_logistic_exact(target, pred, cfg.num_mixtures, cfg.bits)
  if cfg.sampling_function == 'gaussian':
    return O.loss_gaussian(target, pred, cfg.num_mixtures)
  raise NotImplementedError(cfg.sampling_function)


def restate_head(cfg, params, ws, folded, y_true, global_batch, row_chunk=16384):
  """The head's forward and the loss of one training pass; cfg, params, ws, folded as for `restate`.  y_true: (B, T, 1) raw
  next samples (x[:, 1:]).  global_batch: the divisor of the step's loss (compute_average_loss).

  ws needs Z (folded passes), 'skipsum' (unfolded passes with use_skip) or ('H', N) (use_skip False), every ('HA', i) and,
  where the pass wrote a logits tensor (region 5: standalone loss kernels, exact-fp32 mode, mixture and 512-class heads),
  'logits'.  Without 'logits' in ws -- the loss was the epilogue of the head's last conv -- the loss is restated from the
  stored HA[nf-1] through the last conv.

  Returns {key: float64 tensor}:
    ('HA', 0)    folded: act(sum_b Z_b (W_s(b) W_f0) + b_f0 + (sum_b b_s(b)) W_f0), V(b) = W_s(b) W_f0 formed here in fp64;
                 unfolded: act(head_in W_f0 + b_f0), head_in the stored skip sum, or H[N] when use_skip is False
    ('HA', i)    from the stored HA[i-1]
    'logits'     from the stored HA[nf-1] (from head_in when there is no hidden layer)
    'loss_rows'  (B, T), from the stored logits where the pass wrote them, else from 'logits' above
    ('GF', nf)   d (sum of the rows / global_batch) / d logits by fp64 autograd, in chunks of row_chunk rows
    'loss'       sum of the rows / global_batch
    'target_prob'  categorical heads: the soft-max probability of each row's target (B, T), the quantity that Keras clips"""
  N, D = cfg.blocks, cfg.D
  nf = len(cfg.final_layers_channels)
  P = params
  if folded and not (cfg.use_skip and cfg.skip_channels is not None and nf >= 1):
    raise ValueError('only a skip head with skip_channels and a hidden head layer can fold')
  conv = lambda x, i: x @ P[f'final{i}/kernel'][0] + P[f'final{i}/bias']
  out = {}
  head_in = None
  if folded:
    w_f0 = P['final0/kernel'][0]                   # (S, F0)
    b_s = sum(P[f'block{b}/conv_skip/bias'] for b in range(N))
    pre = sum(ws['Z', b][..., :D] @ (P[f'block{b}/conv_skip/kernel'][0] @ w_f0) for b in range(N))
    out['HA', 0] = O.activation(pre + P['final0/bias'] + b_s @ w_f0, cfg.activation)
  else:
    head_in = ws['skipsum'] if cfg.use_skip else ws['H', N]
    if nf:
      out['HA', 0] = O.activation(conv(head_in, 0), cfg.activation)
  for i in range(1, nf):
    out['HA', i] = O.activation(conv(ws['HA', i - 1], i), cfg.activation)
  out['logits'] = conv(ws['HA', nf - 1] if nf else head_in, nf)

  src = ws['logits'] if 'logits' in ws else out['logits']
  B, T, Cout = src.shape
  flat = src.detach().reshape(B * T, Cout)
  target = O.prepare_target(y_true.detach().cpu(), cfg).to(flat.device)
  categorical = cfg.sampling_function == 'categorical'
  target = target.reshape(B * T) if categorical else target.reshape(B * T, 1).to(flat.dtype)
  rows, grad, tprob = [], [], []
  for r0 in range(0, B * T, row_chunk):
    with torch.enable_grad():
      lg = flat[r0:r0 + row_chunk].clone().requires_grad_(True)
      lr = _loss_rows(cfg, target[r0:r0 + row_chunk], lg)
      g, = torch.autograd.grad(lr.sum() / global_batch, lg)
    rows.append(lr.detach())
    grad.append(g)
    if categorical:
      q = torch.softmax(lg.detach(), dim=-1)
      tprob.append(torch.gather(q, -1, target[r0:r0 + row_chunk].unsqueeze(-1))[:, 0])
  out['loss_rows'] = torch.cat(rows).reshape(B, T)
  out['GF', nf] = torch.cat(grad).reshape(B, T, Cout)
  out['loss'] = out['loss_rows'].sum() / global_batch
  if categorical:
    out['target_prob'] = torch.cat(tprob).reshape(B, T)
  return out


def restate(cfg, params, x_in, cond, ws, folded, dropout=None):
  """cfg: O.OracleConfig.  params: {variable name: float64 tensor}.  x_in: (B, T, 1) raw input samples (the model's
  inputs, x[:, :-1]).  cond: (B, cond_inputs) or None.  ws: the workspace tensors of the module docstring, float64.
  folded: the pass contracted the skip path into the head's first conv (split-precision passes with a hidden head layer
  and skip_channels): no skip sum and no gradient of it exist, the blocks read GF[0] = dL/da through V(b) = W_s(b) W_f0.

  dropout: (rate, seed, step) of the pass, or None; with a rate above 0 ws holds ('XD', b).

  Returns {key: float64 tensor}: ('GH', b), ('GU', b), ('GP', b, i), ('GF', i) for i < nf, 'g_skipsum' (unfolded skip
  heads) and ('param', name) for every trainable variable."""
  N, KS, D, L = cfg.blocks, cfg.kernel_size, cfg.D, cfg.layers_per_block
  drop = dropout is not None and dropout[0] > 0
  S = cfg.skip_channels
  nf = len(cfg.final_layers_channels)
  dil = O.dilation_schedule(cfg)
  P = params
  if folded and not (cfg.use_skip and S is not None and nf >= 1):
    raise ValueError('only a skip head with skip_channels and a hidden head layer can fold')
  out = {}
  GH = lambda b: ws['GH', b]
  GU = lambda b: ws['GU', b]
  Z = lambda b: ws['Z', b][..., :D]

  # ---- head data gradients: GF[i-1] = (GF[i] W_i^T) * act'(HA[i-1]); below final0 no activation ----
  for i in range(nf, 0, -1):
    out['GF', i - 1] = (ws['GF', i] @ P[f'final{i}/kernel'][0].T) * dact_from_output(ws['HA', i - 1], cfg.activation)
  g_skip = None                                    # d loss / d (head input) as the kernels read it
  if not folded:
    head_in_grad = ws['GF', 0] @ P['final0/kernel'][0].T
    if cfg.use_skip:
      out['g_skipsum'] = head_in_grad
      g_skip = ws['g_skipsum']
    else:
      out['GH', N] = head_in_grad                  # the head reads the last block's output
  if cfg.use_skip:
    out['GH', N] = torch.zeros_like(ws['H', N])    # nothing flows into the last block's output

  # ---- blocks ----
  if folded:
    w_f0 = P['final0/kernel'][0]                   # (S, F0)
    g_a = ws['GF', 0]
    g_skip_fold = g_a @ w_f0.T                     # d loss / d skip sum, formed here only for dW_s / db_s
    skipsum = sum(Z(b) @ P[f'block{b}/conv_skip/kernel'][0] + P[f'block{b}/conv_skip/bias'] for b in range(N))
  for b in range(N):
    w_r = P[f'block{b}/conv1/kernel'][0]           # (D, R)
    # g_o: gradient at the 1x1 conv's output (before the residual add)
    g_o = GH(b + 1)
    if S is None and cfg.use_skip:
      g_o = g_o + g_skip                           # the skip output IS the pre-residual 1x1 output
    g_z = g_o @ w_r.T
    if S is not None and cfg.use_skip:
      w_s = P[f'block{b}/conv_skip/kernel'][0]     # (D, S)
      if folded:
        g_z = g_z + g_a @ (w_s @ w_f0).T           # V(b) = W_s(b) W_f0 in fp64
      else:
        g_z = g_z + g_skip @ w_s.T
    out['GU', b] = gate_bwd(g_z, ws['AG', b], Z(b))
    # the stack, last conv first: reversed dilated conv of the STORED output gradient G_i of conv i (G_{L-1} = GU[b],
    # G_i = GP[b][i]); below an inner conv the derivative of its activation, through the STORED activated output
    for i in range(L - 1, -1, -1):
      d = dil[b * L + i]
      w_d = P[f'block{b}/dil{i}/kernel']           # (KS, cin, cout)
      g_i = GU(b) if i == L - 1 else ws['GP', b, i]
      g_x = sum(_shift_fwd(g_i, (KS - 1 - j) * d) @ w_d[j].T for j in range(KS))
      if i > 0:
        out['GP', b, i - 1] = g_x * dact_from_output(ws['P', b, i - 1], cfg.activation)
      else:
        if drop:                                   # the mask of the forward; the residual term below is unmasked
          g_x = torch.where(keep_mask(g_x, b, dropout), g_x * drop_scale(dropout[0]), torch.zeros_like(g_x))
        if cfg.use_residual:
          g_x = g_x + GH(b + 1)
        out['GH', b] = g_x
      # parameter gradients of conv i from the input it read
      x_i = ws['P', b, i - 1] if i > 0 else (ws['XD', b] if drop else ws['H', b])
      out['param', f'block{b}/dil{i}/kernel'] = torch.stack(
          [_outer(_shift_back(x_i, (KS - 1 - j) * d), g_i) for j in range(KS)])
      out['param', f'block{b}/dil{i}/bias'] = _rows(g_i).sum(0)
    out['param', f'block{b}/conv1/kernel'] = _outer(Z(b), g_o)[None]
    out['param', f'block{b}/conv1/bias'] = _rows(g_o).sum(0)
    if S is not None:
      if cfg.use_skip:
        gs = g_skip_fold if folded else g_skip
        out['param', f'block{b}/conv_skip/kernel'] = _outer(Z(b), gs)[None]
        out['param', f'block{b}/conv_skip/bias'] = _rows(gs).sum(0)
      else:                                        # unused skip convs
        out['param', f'block{b}/conv_skip/kernel'] = torch.zeros_like(P[f'block{b}/conv_skip/kernel'])
        out['param', f'block{b}/conv_skip/bias'] = torch.zeros_like(P[f'block{b}/conv_skip/bias'])

  # ---- head parameters: dW_f(i) = (input of final conv i)^T GF[i] ----
  for i in range(nf + 1):
    if i > 0:
      a_in = ws['HA', i - 1]
    elif folded:
      a_in = skipsum                               # re-formed in fp64 from Z: the pass never wrote it
    else:
      a_in = ws['skipsum'] if cfg.use_skip else ws['H', N]
    out['param', f'final{i}/kernel'] = _outer(a_in, ws['GF', i])[None]
    out['param', f'final{i}/bias'] = _rows(ws['GF', i]).sum(0)

  # ---- input conv (1 -> R channels, dilation 1) from the raw samples and GH[0] ----
  out['param', 'causal/kernel'] = torch.stack([_outer(_shift_back(x_in, KS - 1 - j), GH(0)) for j in range(KS)])
  out['param', 'causal/bias'] = _rows(GH(0)).sum(0)

  # ---- global conditioning: u += m W_c + b_c, the same row for every t of an utterance ----
  if cfg.conditioning == 'global':
    widths = O.mapping_widths(cfg)
    mp = []
    for j in range(len(widths)):
      mp += [P[f'mapping{j}/kernel'].detach().clone().requires_grad_(True),
             P[f'mapping{j}/bias'].detach().clone().requires_grad_(True)]
    with torch.enable_grad():
      m = cond
      for j in range(len(widths)):
        m = O.activation(m @ mp[2 * j] + mp[2 * j + 1], cfg.mapping_activation)
    g_m = torch.zeros_like(m.detach())
    for b in range(N):
      su = GU(b).sum(1)                            # (B, 2D): per-utterance sum over t
      w_c = P[f'block{b}/conv_cond/kernel'][0]     # (Cc, 2D)
      out['param', f'block{b}/conv_cond/kernel'] = (m.detach().T @ su)[None]
      out['param', f'block{b}/conv_cond/bias'] = su.sum(0)
      g_m = g_m + su @ w_c.T
    if mp:
      gm = torch.autograd.grad(m, mp, grad_outputs=g_m)     # the small mapping net by fp64 autograd under g_m
      for j in range(len(widths)):
        out['param', f'mapping{j}/kernel'], out['param', f'mapping{j}/bias'] = gm[2 * j], gm[2 * j + 1]
  return out


def param_names(restated):
  return [k[1] for k in restated if isinstance(k, tuple) and k[0] == 'param']
