"""One standalone residual block (WaveNetLayer.call, src/layers.py:178-224) and its backward, written out in float64.

Not a conftest and not a test: a plain helper in the style of tests/bwd_restatement.py.  tests/test_layer_reference_cpu.py
pins it against fp64 autograd of O.layer_forward, tests/test_gpu_layer_backward.py compares wn_layer_fwd / wn_layer_bwd
with it.  Explicit time shifts and matmuls only: no conv1d, no autograd, no call into libwn_hip.

Notation: the stack has the convs i = 0..L-1 with dilations d_i, taps j = 0..KS-1; conv i < L-1 has D outputs and the
activation behind it, conv L-1 is the gated one with 2 D outputs.  W_d[i] (KS, cin_i, cout_i), W_r (1, D, R), W_s (1, D, S),
W_c (1, Cc, 2 D).

  forward   pre_i = sum_j x_i[t - (KS-1-j) d_i] W_d[i][j] + b_d[i]     x_0 = x, x_i = p_{i-1} = act(pre_{i-1})
            u = pre_{L-1} + cond W_c + b_c                              (the condition enters the gated conv only)
            gate = sigmoid(u[D:]), a = tanh(u[:D]), z = a gate
            o = z W_r + b_r;  skip = z W_s + b_s, or o itself without skip_channels;  x_out = o + x when residual
  backward  objective = <g_xout, x_out> + <g_skip, skip>; a gradient that is None does not enter it
            g_o = g_xout, without skip_channels g_xout + g_skip (whichever exist)
            g_z = g_o W_r^T + g_skip W_s^T
            g_u = [g_z gate (1 - a^2) | g_z a gate (1 - gate)]
            dW_r = z^T g_o, db_r = sum g_o;  dW_s = z^T g_skip, db_s = sum g_skip;  zeros where the gradient is None
            dW_c = cond^T g_u, db_c = sum g_u, g_cond = g_u W_c^T
            G_{L-1} = g_u;  dW_d[i][j] = sum_t x_i[t - (KS-1-j) d_i]^T G_i[t], db_d[i] = sum G_i
            g_{x_i}[t] = sum_j G_i[t + (KS-1-j) d_i] W_d[i][j]^T  (zero where the index reaches T, never into the next
            utterance);  G_{i-1} = g_{x_i} act'(pre_{i-1});  g_x = g_{x_0} + g_xout when residual
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


def _act(pre, name, branch_pos):
  """(act(pre), act'(pre)).  branch_pos (bool, or None): the side of a relu / leaky_relu kink the implementation under test
  took; it decides ONLY where |pre| < O.KINK_TOL (O.activation_with_branch), every other element takes its own sign."""
  one = torch.ones_like(pre)
  if name is None or name == 'linear':
    return pre, one
  if name in ('relu', 'leaky_relu'):
    pos = (pre >= 0) if name == 'leaky_relu' else (pre > 0)
    if branch_pos is not None:
      pos = torch.where(pre.abs() < O.KINK_TOL, branch_pos.to(torch.bool), pos)
    slope = O.LEAKY_SLOPE if name == 'leaky_relu' else 0.0
    return torch.where(pos, pre, pre * slope), torch.where(pos, one, one * slope)
  if name == 'tanh':
    y = torch.tanh(pre)
    return y, 1 - y * y
  if name == 'sigmoid':
    y = torch.sigmoid(pre)
    return y, y * (1 - y)
  if name == 'elu':
    e = torch.expm1(pre)
    return torch.where(pre > 0, pre, e), torch.where(pre > 0, one, e + 1)
  raise NotImplementedError(name)


def layer_reference(x, cond, params, *, dilations, kernel_size, activation, residual, has_skip, g_xout, g_skip,
                    inner_branch=None):
  """x (B, T, Cin); cond (B, T, Cc) or None; params in the order of O.layer_forward: the stack's kernels and biases, conv1,
  [conv_skip], [conv_cond].  g_xout (B, T, R) and g_skip (B, T, S or R): either may be None.  inner_branch: per non-gated
  conv a bool tensor, see _act.  Everything is computed in the dtype of x (float64 in every test).

  Returns a dict: 'x_out', 'skip', 'g_x', 'g_cond' (None without a condition), 'dW_d' and 'db_d' (lists over the stack),
  'dW_r', 'db_r', 'dW_s', 'db_s' (None without skip_channels), 'dW_c', 'db_c' (None without a condition), the
  intermediates 'u', 'gate', 'z', 'g_u', 'pre' and 'p' (lists over the non-gated convs), and 'param_grads': the parameter
  gradients in the order of params."""
  KS, L = kernel_size, len(dilations)
  p = list(params)
  Wd, bd = [p[2 * i] for i in range(L)], [p[2 * i + 1] for i in range(L)]
  assert all(w.shape[0] == KS for w in Wd)
  Wr, br = p[2 * L][0], p[2 * L + 1]
  nxt = 2 * L + 2
  Ws = bs = Wc = bc = None
  if has_skip:
    Ws, bs = p[nxt][0], p[nxt + 1]
    nxt += 2
  if cond is not None:
    Wc, bc = p[nxt][0], p[nxt + 1]
    nxt += 2
  assert nxt == len(p)
  D = Wr.shape[0]

  def conv(h, i):
    return sum(_shift_back(h, (KS - 1 - j) * dilations[i]) @ Wd[i][j] for j in range(KS)) + bd[i]

  # ---- forward ----
  xin, pre, dact = [x], [], []
  for i in range(L - 1):
    q = conv(xin[i], i)
    y, dy = _act(q, activation, inner_branch[i] if inner_branch is not None else None)
    pre.append(q)
    dact.append(dy)
    xin.append(y)
  u = conv(xin[L - 1], L - 1)
  if cond is not None:
    u = u + cond @ Wc + bc
  gate = torch.sigmoid(u[..., D:])
  a = torch.tanh(u[..., :D])
  z = a * gate
  o = z @ Wr + br
  skip = z @ Ws + bs if has_skip else o
  x_out = o + x if residual else o

  # ---- backward ----
  g_o = g_xout
  if not has_skip and g_skip is not None:
    g_o = g_skip if g_xout is None else g_xout + g_skip
  g_z = torch.zeros_like(z)
  if g_o is not None:
    g_z = g_z + g_o @ Wr.T
  if has_skip and g_skip is not None:
    g_z = g_z + g_skip @ Ws.T
  g_u = torch.cat([g_z * gate * (1 - a * a), g_z * a * gate * (1 - gate)], dim=-1)
  out = dict(x_out=x_out, skip=skip, u=u, gate=gate, z=z, g_u=g_u, pre=pre, p=xin[1:])
  out['dW_r'] = _outer(z, g_o)[None] if g_o is not None else torch.zeros_like(p[2 * L])
  out['db_r'] = _rows(g_o).sum(0) if g_o is not None else torch.zeros_like(br)
  out['dW_s'] = out['db_s'] = out['dW_c'] = out['db_c'] = out['g_cond'] = None
  if has_skip:
    out['dW_s'] = _outer(z, g_skip)[None] if g_skip is not None else torch.zeros_like(Ws)[None]
    out['db_s'] = _rows(g_skip).sum(0) if g_skip is not None else torch.zeros_like(bs)
  if cond is not None:
    out['dW_c'] = _outer(cond, g_u)[None]
    out['db_c'] = _rows(g_u).sum(0)
    out['g_cond'] = g_u @ Wc.T
  dW_d, db_d = [None] * L, [None] * L
  G = g_u
  for i in range(L - 1, -1, -1):
    d = dilations[i]
    dW_d[i] = torch.stack([_outer(_shift_back(xin[i], (KS - 1 - j) * d), G) for j in range(KS)])
    db_d[i] = _rows(G).sum(0)
    g_in = sum(_shift_fwd(G, (KS - 1 - j) * d) @ Wd[i][j].T for j in range(KS))
    if i > 0:
      G = g_in * dact[i - 1]
    else:
      out['g_x'] = g_in + g_xout if (residual and g_xout is not None) else g_in
  out['dW_d'], out['db_d'] = dW_d, db_d
  pg = []
  for i in range(L):
    pg += [dW_d[i], db_d[i]]
  pg += [out['dW_r'], out['db_r']]
  if has_skip:
    pg += [out['dW_s'], out['db_s']]
  if cond is not None:
    pg += [out['dW_c'], out['db_c']]
  out['param_grads'] = pg
  return out


def param_grad_names(depth, has_skip, has_cond):
  """Names of 'param_grads', in order."""
  n = []
  for i in range(depth):
    n += [f'dW_d[{i}]', f'db_d[{i}]']
  n += ['dW_r', 'db_r']
  if has_skip:
    n += ['dW_s', 'db_s']
  if has_cond:
    n += ['dW_c', 'db_c']
  return n
