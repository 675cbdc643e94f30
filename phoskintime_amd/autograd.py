"""``torch.autograd`` access to the per-protein solves: ``solve_flat`` is differentiable in ``theta``.

Forward is the throughput path (``batch.solve_ode_batch``: every model size); backward is ONE launch of the sensitivity kernels' VJP
flavour (``batch.solve_ode_vjp_batch``, linear mode with ``w = grad_output``): the vector-Jacobian product is formed in the kernels'
output stage and d flat / d theta never exists in memory.  The two integrations are separate: the gradient is the exact derivative of
the sensitivity kernel's discrete solution, which agrees with the forward pass's ``flat`` within the solver tolerances."""
from __future__ import annotations

import torch

from . import batch

_VJP_OPTS = ("rtol", "atol", "h0", "max_steps", "clip_nonneg", "normalize", "device")


class _SolveFlat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, model, init_cond, num_psites, t, opts):
        ctx.save_for_backward(theta)
        ctx.call = (model, init_cond, num_psites, t, opts)
        flat = batch.solve_ode_batch(model, theta.detach(), init_cond, num_psites, t, want_sol=False, want_flat=True, **opts).flat
        return flat if theta.dim() == 2 else flat[0]

    @staticmethod
    def backward(ctx, grad_flat):
        (theta,) = ctx.saved_tensors
        model, init_cond, num_psites, t, opts = ctx.call
        # the sensitivity kernels integrate with the default method only: an explicit other choice has no backward pass
        # (`kernel` only picks among the forward pass's kernel families)
        other = sorted(k for k, v in opts.items() if k not in _VJP_OPTS + ("kernel",) and v is not None and (k, v) not in (("method", "lrp12"), ("method", 5)))
        if other:
            raise batch.PhoskinError(f"solve_flat: no backward pass with the solver options {other} (the sensitivity kernels take {_VJP_OPTS[:-1]})")
        g = grad_flat if theta.dim() == 2 else grad_flat.unsqueeze(0)
        res = batch.solve_ode_vjp_batch(model, theta.detach(), init_cond, num_psites, t, g.contiguous(), **{k: v for k, v in opts.items() if k in _VJP_OPTS})
        grad = res.grad if theta.dim() == 2 else res.grad[0]
        return grad.to(dtype=theta.dtype), None, None, None, None, None


def solve_flat(model, theta: torch.Tensor, init_cond, num_psites: int, t, **opts) -> torch.Tensor:
    """``flat`` of ``batch.solve_ode_batch`` ([B, F], or [F] for a single parameter vector) as a differentiable function of ``theta``
    (a float64 GPU tensor).  ``opts`` are ``solve_ode_batch``'s solver options.  The backward pass raises ``PhoskinError`` where no
    sensitivity kernel exists (``batch.sens_available``) or the options name another method; no gradient flows to the other arguments."""
    return _SolveFlat.apply(theta, model, init_cond, num_psites, t, dict(opts))
