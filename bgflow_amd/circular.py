"""Smooth (C^2) bijections of the unit circle: a mixture of wrapped bump-function CDFs with a zero-probability floor
(bgflow/nn/flow/circular.py).  ``CircularTransformSimple`` is the unconditioned flow, ``ConditionalCircularTransformSimple`` the
coupling transformer; both call ``circular_bump_transform``.

Per element (row b, column j) and component k, from the raw conditioner outputs mu_raw, log_sigma, log_weight [B, K, D] (stored
[B, K D], k major) and log_eps [B, D]:

    mu = 0.5 sin(mu_raw) + 0.5      sigma = 1 + exp(log_sigma)      w = softmax_k(log_weight)      eps = sigmoid(log_eps)
    u  = y - mu;   hi = mu > 0.5;   wrapped = u < -0.5 if hi else u > 0.5
    s  = u if not wrapped else (u + 1 if hi else u - 1)              signed distance on the circle
    off = not wrapped if hi else wrapped                             (y >= mu - 0.5 if hi else y > mu + 0.5, decided ONCE, from u)
    s0 = 1 - mu if hi else -mu                                       s at y = 0
    bump(z): z <- clamp(z, 0, 1); a = z^3; b = (1 - z)^3; cdf = a / (a + b); pdf = 3 z^2 (1 - z)^2 / (a + b)^2
    c, p = bump(sigma s + 0.5);   c0 = bump(sigma s0 + 0.5)
    F = sum_k w (c - c0 + off)      f = sum_k w sigma p
    out = F (1 - eps) + y eps       dlogp = sum_j log(f (1 - eps) + eps)

The inverse solves out(x) = y by 25 halvings of [0, 1], returns the midpoint and dlogp = -sum_j log(..) at that x; it is
differentiable through the implicit-function theorem.  DESIGN.md "Circular bump mixture" lists where this deviates from the reference
(saturation clamp, the seam tie, the fixed trip count, the gradient at y == mu, ValueError instead of assert).

The general path is these formulas in torch ops: any device, dtype and layout, differentiable to any order in both directions.  A
contiguous 2-d f32 HIP input with at most ``CIRCULAR_MAX_COMPONENTS`` components runs on csrc/bgk_circular.hip instead: one launch
forward, one launch inverse (the bisection in registers and LDS), one launch backward for either direction.  ``FUSED`` selects,
per operation, whether the kernel is used where it applies.
"""
import numpy as np
import torch

from .flow import Flow

__all__ = ["circular_bump_transform", "CircularTransformSimple", "ConditionalCircularTransformSimple"]

CIRCULAR_MAX_COMPONENTS = 32       # BGK_CIRCULAR_MAX_COMPONENTS: the inverse keeps (mu, sigma, weight) [K][lane] in LDS
CIRCULAR_MAX_WIDTH = 2048          # BGK_CIRCULAR_MAX_WIDTH: one row of per-element log-densities fits the LDS tile
N_HALVINGS = 25

# the kernel path per operation where it applies (False: the torch formulas).  "backward" covers the backward of both directions.
# Defaults follow the measurement of tools/circular_time.py (DESIGN.md "Circular bump mixture"): the kernel wherever it was faster at
# every measured shape.
FUSED = {"forward": True, "inverse": True, "backward": True}


# ---- the general path ---------------------------------------------------------------------------------------------------------------

def _bump(z):
    """(cdf, pdf) of the bump distribution on [0, 1], z clamped into it first"""
    z = z.clamp(0.0, 1.0)
    zc = 1.0 - z
    r = 1.0 / (z ** 3 + zc ** 3)
    return z ** 3 * r, 3.0 * (z * zc * r) ** 2


def _elementwise(y, mu_raw, log_sigma, log_weight, log_eps):
    """out [B, D] and the per-element log-density log(f (1 - eps) + eps) [B, D]; parameters [B or 1, K, D] / [B or 1, D]"""
    mu = 0.5 * torch.sin(mu_raw) + 0.5
    sigma = 1.0 + torch.exp(log_sigma)
    w = torch.softmax(log_weight, dim=1)
    eps = torch.sigmoid(log_eps)
    ome = torch.sigmoid(-log_eps)
    yk = y.unsqueeze(1)
    u = yk - mu
    hi = mu > 0.5
    wrapped = torch.where(hi, u < -0.5, u > 0.5)
    s = torch.where(wrapped, torch.where(hi, u + 1.0, u - 1.0), u)
    off = (wrapped != hi).to(y.dtype)
    s0 = torch.where(hi, 1.0 - mu, -mu)
    c, p = _bump(sigma * s + 0.5)
    c0, _ = _bump(sigma * s0 + 0.5)
    F = (w * ((c - c0) + off)).sum(1)
    f = (w * (sigma * p)).sum(1)
    return F * ome + y * eps, torch.log(f * ome + eps)


def _bisect(t, params):
    """x with out(x) = t: N_HALVINGS halvings of [0, 1], the midpoint of the last bracket"""
    lo, hi = torch.zeros_like(t), torch.ones_like(t)
    for _ in range(N_HALVINGS):
        mid = 0.5 * (lo + hi)
        above = _elementwise(mid, *params)[0] > t
        hi = torch.where(above, mid, hi)
        lo = torch.where(above, lo, mid)
    return 0.5 * (lo + hi)


class _InverseTorchFn(torch.autograd.Function):
    """x(y, parameters) of the general path.  The backward is the implicit-function theorem at x, written in differentiable torch ops
    on the saved OUTPUT, so it can itself be differentiated.  ``x0``: an x already known (the kernel's), else the bisection runs."""

    @staticmethod
    def forward(ctx, x0, y, *params):
        with torch.no_grad():
            x = _bisect(y, params) if x0 is None else x0.detach().clone()
        ctx.save_for_backward(x, *params)
        return x

    @staticmethod
    def backward(ctx, g_x):
        x, *params = ctx.saved_tensors
        higher = torch.is_grad_enabled()
        with torch.enable_grad():
            # the PARTIAL derivatives at fixed x: taken with respect to aliases of the parameters, so that the engine does not walk
            # from the saved output x back through this very node to them; x keeps its graph for a recorded (higher-order) backward
            x = x if higher else x.detach()
            ps = [p.view_as(p) if p.requires_grad else p.detach().requires_grad_(True) for p in params]
            out, logf = _elementwise(x, *ps)
            v = g_x * torch.exp(-logf)                         # g_y = g_x / f_tot
            need = [i for i in range(4) if ctx.needs_input_grad[2 + i]]
            gs = torch.autograd.grad(out, [ps[i] for i in need], grad_outputs=-v, create_graph=higher, allow_unused=True) if need else ()
        grads = [None] * 4
        for i, g in zip(need, gs):
            grads[i] = g
        return (None, v if ctx.needs_input_grad[1] else None, *grads)


def _transform_torch(y, params, inverse, x0=None):
    if not inverse:
        out, logf = _elementwise(y, *params)
        return out, logf.sum(-1, keepdim=True)
    if x0 is None and ((y > 1 + 1e-6).any() or (y < -1e-6).any()):
        raise ValueError(f"the inverse of the circular bump transform operates on [0,1] but input was {y}")
    x = _InverseTorchFn.apply(None if x0 is None else x0.detach(), y, *params)
    return x, -_elementwise(x, *params)[1].sum(-1, keepdim=True)


# ---- the kernel path ----------------------------------------------------------------------------------------------------------------

_BAD = {}        # device -> int32 [1]: inverse targets outside [-1e-6, 1 + 1e-6] seen by the kernel since the last poll


def _bad_counter(device):
    key = str(device)
    if key not in _BAD:
        _BAD[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _BAD[key]


def check_unit_interval():
    """poll (host sync) and reset the counters of out-of-range inverse targets; ValueError if any kernel launch since the last poll saw
    one -- the ``_RangeChecked`` convention of modulo.py (the reference asserts; the torch path raises at once)"""
    total = 0
    for c in _BAD.values():
        total += int(c.item())
        c.zero_()
    if total:
        raise ValueError(f"the inverse of the circular bump transform operates on [0,1] but {total} input elements were outside "
                         "[-1e-6, 1 + 1e-6]")
    return total


def _operands(params, K, D):
    """the four parameters as contiguous rows ([Bp, K D] x 3, [Bp, D]) with the row pitch of the first three and of log_eps (0: one
    row for the whole batch); the first three share one pitch, so a mix of shared and per-row ones is expanded"""
    rows = max(p.shape[0] for p in params[:3])
    kd = [p.detach().reshape(p.shape[0], K * D) for p in params[:3]]
    kd = [(p.expand(rows, K * D) if p.shape[0] != rows else p).contiguous() for p in kd]
    le = params[3].detach().reshape(params[3].shape[0], D).contiguous()
    return kd, (0 if rows == 1 else K * D), le, (0 if le.shape[0] == 1 else D)


def _launch(y, params, K, inverse):
    from . import _lib
    B, D = y.shape
    (mr, ls, lw), pp, le, pe = _operands(params, K, D)
    out = torch.empty_like(y)
    dlogp = torch.empty(B, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        st = _lib.lib().bgk_circular_bump_transform(_lib.ptr(y), _lib.ptr(mr), _lib.ptr(ls), _lib.ptr(lw), pp, _lib.ptr(le), pe, B, K, D,
                                                    int(bool(inverse)), _lib.ptr(out), _lib.ptr(dlogp),
                                                    _lib.ptr(_bad_counter(y.device)) if inverse else None, _lib.stream_ptr(y.device))
    _lib.check(st, "bgk_circular_bump_transform")
    return out, dlogp[:, None]


def _launch_backward(point, params, K, inverse, g_out, g_dlogp):
    """(g_y, g_mu_raw, g_log_sigma, g_log_weight [B, K D], g_log_eps [B, D]) at ``point``: the forward's input, or the inverse's x"""
    from . import _lib
    B, D = point.shape
    dev = point.device
    (mr, ls, lw), pp, le, pe = _operands(params, K, D)
    go = torch.zeros_like(point) if g_out is None else g_out.to(torch.float32).contiguous()
    gl = torch.zeros(B, dtype=torch.float32, device=dev) if g_dlogp is None else g_dlogp.reshape(-1).to(torch.float32).contiguous()
    gy = torch.empty_like(point)
    gk = [torch.empty((B, K * D), dtype=torch.float32, device=dev) for _ in range(3)]
    ge = torch.empty((B, D), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_circular_bump_backward(_lib.ptr(point), _lib.ptr(mr), _lib.ptr(ls), _lib.ptr(lw), pp, _lib.ptr(le), pe, B, K, D,
                                                   int(bool(inverse)), _lib.ptr(go), _lib.ptr(gl), _lib.ptr(gy), _lib.ptr(gk[0]),
                                                   _lib.ptr(gk[1]), _lib.ptr(gk[2]), _lib.ptr(ge), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_circular_bump_backward")
    return (gy, *gk, ge)


class _CircularBumpFn(torch.autograd.Function):
    """(out, dlogp [B, 1]) of one direction on bgk_circular_bump_transform; the backward of either direction is one launch of
    bgk_circular_bump_backward.  The kernel has no second derivatives: a backward that is itself recorded (``create_graph=True``)
    runs the torch formulas from the saved inputs instead."""

    @staticmethod
    def forward(ctx, K, inverse, y, *params):
        out, dlogp = _launch(y, params, K, inverse)
        ctx.save_for_backward(y, out, *params)
        ctx.cfg = (K, inverse)
        return out, dlogp

    @staticmethod
    def backward(ctx, g_out, g_dlogp):
        K, inverse = ctx.cfg
        y, out, *params = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        if torch.is_grad_enabled() or not FUSED["backward"]:
            with torch.enable_grad():
                # (the saved OUTPUT enters only as a detached value: with its graph the engine would walk from it back into this node)
                ins = [t if t.requires_grad else t.detach().requires_grad_(True) for t in (y, *params)]
                o, dl = _transform_torch(ins[0], _shaped(ins[1:], K, y.shape[1]), inverse, x0=out.detach() if inverse else None)
                want = [i for i in range(5) if need[i]]
                gs = torch.autograd.grad((o, dl), [ins[i] for i in want], grad_outputs=(g_out, g_dlogp),
                                         create_graph=torch.is_grad_enabled(), allow_unused=True)
            grads = [None] * 5
            for i, g in zip(want, gs):
                grads[i] = g
            return (None, None, *grads)
        gs = _launch_backward(out if inverse else y, params, K, inverse, g_out, g_dlogp)
        grads = [gs[0] if need[0] else None]
        for i, p in enumerate(params):
            g = None
            if need[1 + i]:
                g = gs[1 + i]
                g = (g.sum(0, keepdim=True) if p.shape[0] == 1 and g.shape[0] != 1 else g).reshape(p.shape)
            grads.append(g)
        return (None, None, *grads)


def _shaped(params, K, D):
    mr, ls, lw, le = params
    return [p.reshape(p.shape[0], K, D) for p in (mr, ls, lw)] + [le.reshape(le.shape[0], D)]


def _kernel_takes(y, params, K, inverse):
    if not FUSED["inverse" if inverse else "forward"]:
        return False
    if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.is_contiguous() and y.shape[0] > 0):
        return False
    if not (1 <= K <= CIRCULAR_MAX_COMPONENTS and 1 <= y.shape[1] <= CIRCULAR_MAX_WIDTH):
        return False
    return all(p.device == y.device and p.dtype == torch.float32 for p in params)


def circular_bump_transform(y, mu_raw, log_sigma, log_weight, log_eps, inverse=False):
    """The circular bump-mixture bijection of y [..., D] in [0, 1] (module docstring) or, with ``inverse=True``, its inverse:
    ``(out [..., D], dlogp [..., 1])``.  ``mu_raw``, ``log_sigma``, ``log_weight``: [B, K D] (k major) or [B, K, D]; ``log_eps``:
    [B, D]; B the number of rows of y, or 1 (the parameters are shared by all rows)."""
    D = y.shape[-1]
    y2 = y.reshape(-1, D)
    n = mu_raw.numel() // mu_raw.shape[0]
    if n % D != 0 or n == 0:
        raise ValueError(f"circular_bump_transform: {n} parameters per row are no multiple of the width {D}")
    K = n // D
    params = (mu_raw, log_sigma, log_weight, log_eps)
    for p, width in zip(params, (K * D, K * D, K * D, D)):
        if p.shape[0] not in (1, y2.shape[0]) or p.numel() != p.shape[0] * width:
            raise ValueError(f"circular_bump_transform: a parameter of shape {tuple(p.shape)} does not fit input {tuple(y.shape)} "
                             f"with {K} components")
    if _kernel_takes(y2, params, K, inverse):
        if torch.is_grad_enabled() and any(t.requires_grad for t in (y2, *params)):
            out, dlogp = _CircularBumpFn.apply(K, bool(inverse), y2, *params)
        else:
            out, dlogp = _launch(y2, params, K, inverse)
    else:
        out, dlogp = _transform_torch(y2, _shaped(params, K, D), inverse)
    if y.dim() == 2:
        return out, dlogp
    return out.reshape(y.shape), dlogp.reshape(*y.shape[:-1], 1)


# ---- the flows ----------------------------------------------------------------------------------------------------------------------

class _CircularBump(Flow):
    check_unit_interval = staticmethod(check_unit_interval)

    def _forward(self, x, y, *args, **kwargs):
        return circular_bump_transform(y, *self._raw(x, y))

    def _inverse(self, x, y, *args, **kwargs):
        return circular_bump_transform(y, *self._raw(x, y), inverse=True)


class CircularTransformSimple(_CircularBump):
    """Simple circular flow based on a mixture of bump function distributions (circular.py:129-169).  The transformation of ``y`` is
    NOT conditioned on ``x``.  Parameters ``_mu``, ``_log_sigma``, ``_log_weight`` [1, n_bases, n_dim] and ``_log_eps`` [1, n_dim],
    initialised as in the reference."""

    def __init__(self, n_bases=10, n_dim=1):
        super().__init__()
        self._mu = torch.nn.Parameter(torch.Tensor(1, n_bases, n_dim).uniform_(0, 2 * np.pi))
        self._log_sigma = torch.nn.Parameter(torch.Tensor(1, n_bases, n_dim).normal_())
        self._log_weight = torch.nn.Parameter(torch.Tensor(1, n_bases, n_dim).normal_())
        self._log_eps = torch.nn.Parameter(torch.Tensor(1, n_dim).normal_())

    def _raw(self, x, y):
        return self._mu, self._log_sigma, self._log_weight, self._log_eps


class ConditionalCircularTransformSimple(_CircularBump):
    """Circular flow based on a mixture of bump functions, ``y`` transformed conditioned on ``x`` (circular.py:172-221): the four nets
    map x to mu [B, K D], log_sigma [B, K D], log_weight [B, K D] (k major) and log_eps [B, D].  It is the ``transformer`` of a
    ``CouplingFlow`` as it stands."""

    def __init__(self, mu, log_sigma, log_weight, log_eps):
        super().__init__()
        self._mu = mu
        self._log_sigma = log_sigma
        self._log_weight = log_weight
        self._log_eps = log_eps

    def _raw(self, x, y):
        n, D = x.shape[0], y.shape[-1]
        mu, log_sigma, log_weight = (net(x).view(n, -1, D) for net in (self._mu, self._log_sigma, self._log_weight))
        assert all(p.shape[1] == mu.shape[1] for p in [log_sigma, log_weight])
        return mu, log_sigma, log_weight, self._log_eps(x).view(n, D)
