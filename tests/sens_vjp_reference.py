"""Reference for the VJP flavour of the sensitivity kernels (pk_solve_protein_sens_vjp_batch), shared by tests/test_sens_vjp_cpu.py and
tests/test_gpu_sens_vjp.py (not a test module).

With v [F] = flat and d [F, C] = dflat as oracle.protein_models.flat_and_jacobian post-processes them (the flat layout: no slot for the mRNA
row at the first five output times; value clipped at 0, derivative row zero where the clip is active; both scaled by 1 / y0 under
`normalize`; zero derivative rows at t0, the initial values being data), w [F] the weights and target [F] or None:

    linear mode         c = w                            value = sum_f w_f v_f             grad_p = sum_f c_f d_fp
    least-squares mode  r = w (v - target),  c = w r     value = 1/2 sum_f r_f^2           grad_p = sum_f c_f d_fp

`bounds` propagates limits eps_v [F] / eps_d [F, C] on v / d through both to first order:
    linear          bound_value = sum |w| eps_v                 bound_grad_p = sum |w| eps_d
    least squares   bound_value = sum |w r| eps_v               bound_grad_p = sum |c| eps_d + sum w^2 |d| eps_v
The entries at t0 carry no error (`t0_entries`)."""
import numpy as np

from oracle import protein_models as pm


def t0_entries(n, T):
    """Flat indices of the entries at output time 0: P(t0) and the sites at t0 (the mRNA row has a slot from the sixth time on)."""
    T5 = max(T - 5, 0)
    return np.array([T5] + [T5 + T + j * T for j in range(n)])


def cotangent(v, w, target=None):
    """c [F] and the terms [F] whose sum is value (twice value in least-squares mode), formed as the kernels form them."""
    if target is None:
        return w, w * v
    r = w * (v - target)
    return w * r, r * r


def vjp(v, d, w, target=None):
    """(value, grad [C], sum |value terms|, sum |grad terms| [C]) in numpy; the two sums of magnitudes are what a rounding bound scales with."""
    c, terms = cotangent(v, w, target)
    scale = 1.0 if target is None else 0.5
    return scale * terms.sum(), (c[:, None] * d).sum(axis=0), scale * np.abs(terms).sum(), np.abs(c[:, None] * d).sum(axis=0)


def flat_reference(model, sol, dsol, y0, n, **post):
    """(v [F], d [F, C]) of an exact solution and its exact derivative (pm.sens_exact_lti), post-processed as the library does."""
    return pm.flat_and_jacobian(pm.MODEL_IDS[model] if isinstance(model, str) else model, sol, dsol, y0, n, **post)


def bounds(v, d, w, target, eps_v, eps_d, n, T):
    """(bound_value, bound_grad [C]): eps_v [F] / eps_d [F, C] propagated to first order; nothing from the entries at t0."""
    ev = np.array(eps_v, dtype=float); ed = np.array(eps_d, dtype=float)
    ev[t0_entries(n, T)] = 0.0; ed[t0_entries(n, T)] = 0.0
    c, _ = cotangent(v, w, target)
    if target is None:
        return float((np.abs(w) * ev).sum()), (np.abs(w)[:, None] * ed).sum(axis=0)
    return float((np.abs(c) * ev).sum()), (np.abs(c)[:, None] * ed).sum(axis=0) + ((w * w * ev)[:, None] * np.abs(d)).sum(axis=0)
