"""What every kernel of the backward phase of one training pass should have produced FROM ITS OWN INPUTS, in float64.

Not a conftest and not a test: a plain helper (tests/test_bwd_restatement_cpu.py pins it against fp64 autograd of the
oracle, tests/test_gpu_bwd_tile_walk.py compares the HIP kernels with it).  It is plain torch float64 on whatever
device its inputs live on and never calls into libwn_hip.

A product is restated from the tensors its kernel read, not from other restated values: `GH[b]` from the stored `GU[b]`
and `GH[b+1]`, `GU[b]` from the stored `GH[b+1]`, `AG[b]`, `Z[b]` and so on.  An error in one kernel therefore shows in
that kernel's tensor alone, at the size of the error, and a chain of 7 blocks does not blur it.

Scope: `layers_per_block == 1`, no dropout.

Workspace tensors (`ws`, keyed as below, each `(B, T, channels)`; regions of WaveNet.training_intermediate):

  ('H', b)  b = 0..N    region 0   block inputs; H[N] is the last block's output
  ('Z', b)  b = 0..N-1  region 1   gated activation tanh * sigmoid (leading dimension Dp >= D: the first D columns count)
  ('AG', b)             region 2   saved sigmoid gate
  ('HA', i) i = 0..nf-1 region 4   head activations (post-activation output of final conv i)
  ('GF', i) i = 0..nf   region 6   d loss / d (output of final conv i, pre-activation); GF[nf] = d loss / d logits is the
                                   loss epilogue's and is taken as given
  ('GU', b)             region 8   d loss / d u of block b, [filter half | gate half]
  ('GH', b) b = 0..N    region 9   d loss / d H[b]
  'skipsum', 'g_skipsum' regions 3, 7   unfolded passes with use_skip only
"""
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


def restate(cfg, params, x_in, cond, ws, folded):
  """cfg: O.OracleConfig.  params: {variable name: float64 tensor}.  x_in: (B, T, 1) raw input samples (the model's
  inputs, x[:, :-1]).  cond: (B, cond_inputs) or None.  ws: the workspace tensors of the module docstring, float64.
  folded: the pass contracted the skip path into the head's first conv (split-precision passes with a hidden head layer
  and skip_channels): no skip sum and no gradient of it exist, the blocks read GF[0] = dL/da through V(b) = W_s(b) W_f0.

  Returns {key: float64 tensor}: ('GH', b), ('GU', b), ('GF', i) for i < nf, 'g_skipsum' (unfolded skip heads) and
  ('param', name) for every trainable variable."""
  if cfg.layers_per_block != 1:
    raise NotImplementedError('layers_per_block > 1: the inner gradients have no workspace region')
  N, KS, D = cfg.blocks, cfg.kernel_size, cfg.D
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
    d = dil[b]
    w_d = P[f'block{b}/dil0/kernel']               # (KS, R, 2D)
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
    # reversed dilated conv of the STORED g_u
    g_x = sum(_shift_fwd(GU(b), (KS - 1 - j) * d) @ w_d[j].T for j in range(KS))
    if cfg.use_residual:
      g_x = g_x + GH(b + 1)
    out['GH', b] = g_x
    # parameter gradients of the block
    out['param', f'block{b}/dil0/kernel'] = torch.stack(
        [_outer(_shift_back(ws['H', b], (KS - 1 - j) * d), GU(b)) for j in range(KS)])
    out['param', f'block{b}/dil0/bias'] = _rows(GU(b)).sum(0)
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
