"""Robust reverse-KL training: clipped energies and gradient clipping.

``linlogcut`` and ``ClipGradient`` (bgflow/utils/train.py:60-118), ``LinLogCutEnergy`` and ``GradientClippedEnergy``
(bgflow/distribution/energy/clipped.py:8-38) with the reference's constructor signatures, attribute names and buffers.

On CPU tensors and in f64 all four are the reference's torch operations.  On f32 HIP tensors:
  * a chain of at most one ``LinLogCutEnergy`` and at most one ``GradientClippedEnergy`` (either order) around a distribution that
    describes itself by kernel fields runs as ONE launch (bgk_energy_fields_cut) and ONE backward launch that applies the cut's
    derivative and the group clip before the gradient is stored (distributions._kernel_plan); ``kl_loss_sums`` works on such a chain;
  * around any other delegate ``GradientClippedEnergy`` registers the reference's tensor hooks, which run bgk_clip_gradient, and
    ``LinLogCutEnergy`` cuts the delegate's [B, 1] result with bgk_linlogcut.

Not provided: a tensor-valued ``clip`` (one threshold per group) and groups that straddle rows (``norm_dim`` must be -1 or divide
the row width); both raise ``ValueError``.  Where the fused chain differs from the hook: the hook clips the gradient a tensor
receives from ALL its consumers, the fused backward clips the energy's contribution -- the same thing whenever the energy is the
tensor's only consumer (the KL loss).
"""
from functools import partial

import torch
from torch.autograd.function import once_differentiable

from .distributions import Energy, kernel_energy
from .utils import unpack_tensor_tuple

__all__ = ["linlogcut", "ClipGradient", "LinLogCutEnergy", "GradientClippedEnergy"]


def _kernel_tensor(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() > 0


class _LinLogCutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vals, high, max_val):
        from . import _lib
        v = vals.contiguous()
        out = torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.check(_lib.lib().bgk_linlogcut(_lib.ptr(v), None, v.numel(), high, max_val, _lib.ptr(out), _lib.stream_ptr(v.device)),
                       "bgk_linlogcut")
        ctx.save_for_backward(v)
        ctx.cfg = (high, max_val)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import _lib
        (v,) = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        out = torch.empty_like(v)
        with torch.cuda.device(v.device):
            _lib.check(_lib.lib().bgk_linlogcut(_lib.ptr(v), _lib.ptr(g), v.numel(), *ctx.cfg, _lib.ptr(out), _lib.stream_ptr(v.device)),
                       "bgk_linlogcut")
        return out, None, None


def linlogcut(vals, high_val=1e3, max_val=1e9):
    """``where(v >= high, high + log(1 + v - high), v)``, then ``clamp(max=max_val)`` (train.py:60-62)"""
    if _kernel_tensor(vals) and isinstance(high_val, (int, float)) and isinstance(max_val, (int, float)):
        return _LinLogCutFn.apply(vals, float(high_val), float(max_val))
    cut = torch.where(vals >= high_val, high_val + torch.log(1 + vals - high_val), vals)
    return cut.clamp(min=None, max=max_val)


def _host_scalar(clip):
    """the threshold as a host float, or None for a tensor-valued one (not provided)"""
    if torch.is_tensor(clip):
        return float(clip) if clip.numel() == 1 else None
    return float(clip)


def clip_launch(g, clip, norm_dim, out=None):
    """bgk_clip_gradient on a [B, D] f32 HIP tensor (``out`` may be ``g``)"""
    from . import _lib
    g2, ldg = _lib.rowmajor(g)
    if out is None:
        out = torch.empty(g2.shape, dtype=torch.float32, device=g2.device)
    o2, ldo = _lib.rowmajor(out)
    assert o2 is out or o2.data_ptr() == out.data_ptr(), "clip_launch: the output must be row-major"
    B, D = g2.shape
    nblk = 1024
    ws = torch.empty(nblk + 1, dtype=torch.float64, device=g2.device) if norm_dim == -1 else None
    with torch.cuda.device(g2.device):
        st = _lib.lib().bgk_clip_gradient(_lib.ptr(g2), ldg, B, D, float(clip), int(norm_dim), _lib.ptr(out), ldo, _lib.ptr(ws), nblk,
                                          _lib.stream_ptr(g2.device))
    _lib.check(st, "bgk_clip_gradient")
    return out


class ClipGradient(torch.nn.Module):
    """Clips the gradients of its inputs in the backward pass (train.py:82-118).

    clip: the max norm (a scalar); norm_dim: the number of consecutive elements a norm is formed over -- 1 clips by value, 3 by
    atom, -1 the norm of the whole tensor (batch included)."""

    def __init__(self, clip, norm_dim=1):
        super().__init__()
        self.register_buffer("clip", torch.as_tensor(clip))
        self.norm_dim = norm_dim
        self._refresh_host()

    def _refresh_host(self):
        # host copy of the scalar threshold: taken here, not per launch (a device-to-host read per backward would sync the step)
        self._clip_host = _host_scalar(self.clip)

    def _apply(self, fn, *args, **kwargs):
        res = super()._apply(fn, *args, **kwargs)
        self._refresh_host()
        return res

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._refresh_host()

    def forward(self, *xs):
        clip = self.clip if self._clip_host is None else self._clip_host
        for x in xs:
            if x.requires_grad:
                x.register_hook(partial(ClipGradient.clip_tensor, clip=clip, last_dim=self.norm_dim))
        return unpack_tensor_tuple(xs)

    @staticmethod
    def clip_tensor(tensor, clip, last_dim):
        """NaN -> 0, then every group of ``last_dim`` consecutive elements (-1: the whole tensor) is scaled by min(clip / |group|, 1)"""
        scalar = _host_scalar(clip)
        if scalar is None:
            raise ValueError("ClipGradient: a tensor-valued clip (one threshold per group) is not provided; clip must be a scalar")
        width = tensor.shape[-1] if tensor.dim() > 0 else 1
        if not isinstance(last_dim, int) or not (last_dim == -1 or (last_dim >= 1 and width % last_dim == 0)):
            raise ValueError(f"ClipGradient: norm_dim must be -1 or divide the row width ({width}); got {last_dim} "
                             "(groups that straddle rows are not provided)")
        if _kernel_tensor(tensor) and tensor.dim() >= 1 and not (torch.is_grad_enabled() and tensor.requires_grad):
            return clip_launch(tensor.reshape(-1, width), scalar, last_dim).reshape(tensor.shape)
        original_shape = tensor.shape
        shape = (-1,) if last_dim == -1 else (-1, last_dim)
        out = torch.nan_to_num(tensor, nan=0.0).flatten().reshape(*shape)
        norm = torch.linalg.norm(out.detach(), dim=-1, keepdim=True)
        clip_t = clip if torch.is_tensor(clip) and clip.device == tensor.device else torch.tensor(scalar, dtype=torch.float32, device=tensor.device)
        factor = (clip_t.view(-1) / norm.view(-1)).view(-1)
        factor = torch.minimum(factor, torch.ones_like(factor))
        out = out.view(*shape) * factor.view(-1, 1)
        return out.reshape(original_shape)


class LinLogCutEnergy(Energy):
    """Cut off energy at singularities (clipped.py:8-27): energies beyond ``high_energy`` are replaced by
    ``high_energy + log(1 + energy - high_energy)``, the result is bounded by ``max_energy``.  The delegate is evaluated at T = 1 and
    the CUT energy is divided by the temperature (energy/base.py:124-146): ``energy(x, T) = linlogcut(delegate.energy(x)) / T``."""

    def __init__(self, energy, high_energy=1e3, max_energy=1e9):
        super().__init__(energy.event_shapes)
        self.delegate = energy
        self.high_energy = high_energy
        self.max_energy = max_energy

    def energy(self, *xs, temperature=1.0, **kwargs):
        fast = kernel_energy(self, xs, temperature) if not kwargs else None
        if fast is not None:
            return fast
        return super().energy(*xs, temperature=temperature, **kwargs)

    def _energy(self, *xs, **kwargs):
        u = self.delegate.energy(*xs, **kwargs)
        return linlogcut(u, high_val=self.high_energy, max_val=self.max_energy)


class GradientClippedEnergy(Energy):
    """An Energy with clipped gradients (clipped.py:30-38); see ``ClipGradient``."""

    def __init__(self, energy, gradient_clipping):
        super().__init__(energy.event_shapes)
        self.delegate = energy
        self.clipping = gradient_clipping

    def energy(self, *xs, temperature=1.0, **kwargs):
        fast = kernel_energy(self, xs, temperature) if not kwargs else None
        if fast is not None:
            return fast
        return super().energy(*xs, temperature=temperature, **kwargs)

    def _energy(self, *xs, **kwargs):
        return self.delegate.energy(*((self.clipping(x) for x in xs)), **kwargs)
