"""WaveNet.differentiable: the network as one torch.autograd node."""
from __future__ import annotations

import torch

from . import _guard, _lib


class _NetFn(torch.autograd.Function):
  """WaveNet.differentiable: wn_forward_training on the model's training workspace, wn_vjp from the gradient autograd
  hands back.  Inputs (x, cond, flat_params) and a zero-size anchor that keeps the node alive."""

  @staticmethod
  def forward(ctx, x, cond, flat_params, anchor, model, drop, want_probs):
    L = _lib.lib()
    B, T = x.shape[0], x.shape[1]
    x, cond = x.detach(), (cond.detach() if cond is not None else None)
    # the workspace layout depends on the dropout rate in force: kept_pass sets it first (off unless this pass draws a mask)
    if drop:
      model._arm_dropout()
    state = (model.dropout if drop else 0.0, model._drop_armed_step if drop else 0)
    frames = cond.shape[1] if (cond is not None and cond.dim() == 3) else 0     # local conditioning, F > 1
    mode = L.wn_debug_value(1)
    with _guard.kept_pass(model, frames, drop_state=state):
      ws = model._workspace('train', L.wn_plan_workspace_floats(model._plan, B, T, 1))
      model._train_gen += 1
      model._last_train_frames = frames if frames > 1 else 0
      out = torch.empty(B, T, model.spec.out_channels, dtype=torch.float32, device=model._device)

      def run():
        _lib.check(L.wn_forward_training(model._plan, _lib.ptr(flat_params), _lib.ptr(x), _lib.ptr(cond), B, T,
                                         _lib.ptr(out) if want_probs else None, None if want_probs else _lib.ptr(out),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))

      def tripped():
        slot = L.wn_plan_range_slot(model._plan, B, T, 1)
        return model._guard_over(ws[slot:slot + 1].clone(), drop)
      if _guard.guarded(model, run, tripped, skip=not model.range_check or mode == 1):
        mode = 1
    ctx.model, ctx.mode, ctx.drop_state, ctx.stamp, ctx.done = model, mode, state, model._train_gen, False
    ctx.want_probs, ctx.frames = want_probs, frames
    ctx.save_for_backward(x, cond)
    return out

  @staticmethod
  @torch.autograd.function.once_differentiable          # second derivatives are refused, not returned without a graph
  def backward(ctx, g):
    model = ctx.model
    if ctx.done:
      raise RuntimeError('differentiable: this graph has already been run backward (one pass of activations is kept: '
                         'retain_graph re-runs are not supported; call differentiable again)')
    if model._train_gen != ctx.stamp:
      raise RuntimeError('differentiable: another pass used the training workspace between forward and backward '
                         '(loss_and_grads / train_step, call(training=True) or another differentiable), or the '
                         'weights changed (optimizer step, set_weights): the saved activations are gone or stale; '
                         'one graph is alive at a time')
    model._not_averaged('backward of differentiable')
    ctx.done = True
    x, cond = ctx.saved_tensors
    flat_params = model.flat_params                # (read in place: the optimizer writes it through the library)
    L = _lib.lib()
    B, T = x.shape[0], x.shape[1]
    g = g.to(torch.float32).contiguous()
    need_x, need_c, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
    g_x = torch.empty_like(x) if need_x else None
    g_c = torch.empty_like(cond) if (need_c and cond is not None) else None
    ws = model._ws['train']
    # the math mode and the mask of the pass that was kept, whatever the calling thread's are now
    with _guard.kept_pass(model, ctx.frames, mode=ctx.mode, drop_state=ctx.drop_state):
      _lib.check(L.wn_vjp(model._plan, _lib.ptr(flat_params), _lib.ptr(x), _lib.ptr(cond), B, T, _lib.ptr(g),
                          0 if ctx.want_probs else 1, _lib.ptr(model.flat_grads), _lib.ptr(g_x), _lib.ptr(g_c),
                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    return g_x, g_c, (model.flat_grads.clone() if need_p else None), None, None, None, None
