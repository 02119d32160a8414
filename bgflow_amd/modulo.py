"""Constraint layers of the builder on one column-map kernel (csrc/bgk_colmap.hip): CircularShiftFlow, IncreaseMultiplicityFlow
(bgflow/nn/flow/modulo.py), TorchTransform (nn/flow/torchtransform.py) and the fused ``SetConstantFlow -> WrapFlow(index
MergeFlow)`` pair that ``BoltzmannGeneratorBuilder.add_merge_constraints`` appends (factory/generator_builder.py:461-498).

Each of them maps one [B, n] field column by column: an output column is an elementwise function of at most one input column, or
a constant.  On a contiguous f32 HIP matrix inside the kernel's envelope that is ONE launch of ``bgk_colmap`` driven by a small
table, forward, inverse and -- with the transposed table -- backward.  On anything else (CPU, f64, non-contiguous rows, a field
wider than COLMAP_MAX_WIDTH, parameters of another shape) the flows run the reference's torch expressions unchanged.
"""
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .distributions import COLMAP_MAX_WIDTH, _FusedSampling
from .flow import ACC_KW, Flow, MergeFlow, SetConstantFlow, SplitFlow, WrapFlow

__all__ = ["CircularShiftFlow", "IncreaseMultiplicityFlow", "TorchTransform"]

COPY, CONST, AFFINE_FWD, AFFINE_INV, SHIFT, MULT_INV, MULT_FWD = range(7)    # kinds of bgk_colmap (include/bgflow_amd.h)
_ENTRY = np.dtype([("kind", "<i4"), ("src", "<i4"), ("p0", "<f4"), ("p1", "<f4")])


class ColumnTable:
    """n_out entries (kind, src, p0, p1) describing how a [B, n_in] field becomes a [B, n_out] one, the constant log|det J| of
    that map, the device copies of the table (one per device, made on first use) and the table of the map's backward."""

    def __init__(self, n_in, entries, logdet=0.0):
        self.n_in, self.n_out, self.logdet = int(n_in), len(entries), float(logdet)
        tab = np.zeros(self.n_out, dtype=_ENTRY)
        for j, (kind, src, p0, p1) in enumerate(entries):
            if kind != CONST and not 0 <= int(src) < self.n_in:
                raise ValueError(f"column table: source column {src} outside [0, {self.n_in})")
            tab[j] = (kind, src, p0, p1)
        self.host = tab
        self.checks_range = bool(np.isin(tab["kind"], (SHIFT, MULT_INV, MULT_FWD)).any())
        self.draws = bool((tab["kind"] == MULT_FWD).any())
        self._device, self._backward = {}, None

    def on(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.host.view(np.int32).reshape(self.n_out, 4).copy()).to(device)
        return self._device[key]

    def backward(self):
        """table of g_in [B, n_in] from g_out [B, n_out]: g_in[:, i] = coef_i * g_out[:, j] for the output column j that reads input
        column i (a copy, one multiplication or one division); an input column nothing reads gets zero.  The modulo kinds have
        derivative 1 (shift), m (multiplicity inverse), 1 / m (forward) almost everywhere."""
        if self._backward is None:
            entries = [(CONST, 0, 0.0, 0.0)] * self.n_in
            seen = set()
            for j, (kind, src, p0, p1) in enumerate(self.host.tolist()):
                if kind == CONST:
                    continue
                if src in seen:
                    raise NotImplementedError("column table: an input column read by two output columns has no one-column backward")
                seen.add(src)
                entries[src] = {COPY: (COPY, j, 0.0, 0.0), SHIFT: (COPY, j, 0.0, 0.0),
                                AFFINE_FWD: (AFFINE_FWD, j, 0.0, p1), AFFINE_INV: (AFFINE_INV, j, 0.0, p1),
                                MULT_INV: (AFFINE_FWD, j, 0.0, p0), MULT_FWD: (AFFINE_INV, j, 0.0, p0)}[kind]
            self._backward = ColumnTable(self.n_out, entries)
        return self._backward


def kernel_ok(x, n_in):
    """the envelope of bgk_colmap: a non-empty contiguous [B, n_in] f32 HIP matrix with n_in <= COLMAP_MAX_WIDTH"""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous()
            and x.shape[0] > 0 and x.shape[1] == n_in and 1 <= n_in <= COLMAP_MAX_WIDTH)


def colmap_launch(x, table, dlogp=None, accumulate=False, sign=1.0, u=None, seed=0, offset=0, row0=0, bad=None):
    """one launch of bgk_colmap: the mapped [B, n_out] field; ``dlogp`` [B] receives (accumulate: is increased by) sign * logdet"""
    from . import _lib
    assert table.n_out <= COLMAP_MAX_WIDTH
    out = torch.empty((x.shape[0], table.n_out), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = _lib.lib().bgk_colmap(_lib.ptr(x), table.n_in, _lib.ptr(out), table.n_out, _lib.ptr(table.on(x.device)), _lib.ptr(u),
                                   int(seed) & (2 ** 64 - 1), int(offset) & 0xffffffff, int(row0), x.shape[0],
                                   _lib.ptr(dlogp), int(bool(accumulate)), float(sign) * table.logdet, _lib.ptr(bad),
                                   _lib.stream_ptr(x.device))
    _lib.check(st, "bgk_colmap")
    return out


class _ColMapFn(torch.autograd.Function):
    """y, dlogp [B, 1] of one column map under autograd; the backward is the same kernel with the transposed table.  The log-det is
    a constant: it carries no gradient.  ``once_differentiable``: a second derivative raises instead of silently dropping terms."""

    @staticmethod
    def forward(ctx, x, table, sign, launch_kw):
        dlogp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        y = colmap_launch(x, table, dlogp=dlogp, sign=sign, **launch_kw)
        ctx.table = table
        dlogp = dlogp[:, None]
        ctx.mark_non_differentiable(dlogp)
        return y, dlogp

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, _g_dlogp):
        return colmap_launch(g_y.to(torch.float32).contiguous(), ctx.table.backward()), None, None, None


def run_table(x, table, kwargs, sign=1.0, **launch_kw):
    """(y, dlogp) of a column map on the kernel: dlogp is the accumulator of the enclosing SequentialFlow pass when it travels in
    ``kwargs`` (a zero log-det touches its buffer only as the first writer), else a [B, 1] tensor the kernel wrote"""
    acc = kwargs.get(ACC_KW)
    if torch.is_grad_enabled() and x.requires_grad:
        y, dlogp = _ColMapFn.apply(x, table, sign, launch_kw)
        if acc is not None:
            acc.add(dlogp)
            return y, acc
        return y, dlogp
    if acc is not None:
        buf, started = acc.peek()
        if started and table.logdet == 0.0:
            return colmap_launch(x, table, **launch_kw), acc
        y = colmap_launch(x, table, dlogp=buf, accumulate=started, sign=sign, **launch_kw)
        acc.commit()
        return y, acc
    dlogp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    y = colmap_launch(x, table, dlogp=dlogp, sign=sign, **launch_kw)
    return y, dlogp[:, None]


def _assert_in_unit_interval(x):
    if (x > 1 + 1e-6).any() or (x < - 1e-6).any():
        raise ValueError(f'IncreaseMultiplicityFlow operates on [0,1] but input was {x}')


def _column_values(t, n):
    """a per-column or scalar parameter as n f32 values on the host, or None when it is neither (the torch form handles it).
    Integer tensors are what torch promotes to f32 next to an f32 input under the default dtype."""
    if not torch.is_tensor(t):
        if isinstance(t, (int, float)) and not isinstance(t, bool):
            return torch.full((n,), float(t), dtype=torch.float32).numpy() if abs(float(t)) < 3e38 else None
        return None
    if t.dtype != torch.float32 and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool
                                     or torch.get_default_dtype() != torch.float32):
        return None
    if t.requires_grad or t.dim() > 1 or (t.dim() == 1 and t.shape[0] not in (1, n)):
        return None
    return torch.broadcast_to(t.detach().to(device="cpu", dtype=torch.float32), (n,)).numpy()


class _RangeChecked(Flow):
    """the unit-interval check of modulo.py:42-44 on the kernel path: the kernel counts offending elements into a device counter
    (an atomic add, as the coordinate transforms count their clamp events) and ``check_unit_interval()`` polls it -- one host sync
    when the caller asks, not one per call -- and raises the reference's ValueError.  ``SYNC_RANGE_CHECK = True`` reads the counter
    after every launch instead, so that the call itself raises as on the CPU."""
    SYNC_RANGE_CHECK = False
    _bgk_acc = True

    def _bad_counter(self, device):
        counters = self.__dict__.setdefault("_bad", {})
        key = str(device)
        if key not in counters:
            counters[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return counters[key]

    def check_unit_interval(self):
        """poll (host sync) and reset the counters of out-of-range inputs; ValueError if any launch since the last poll saw one"""
        total = 0
        for c in self.__dict__.get("_bad", {}).values():
            total += int(c.item())
            c.zero_()
        if total:
            raise ValueError(f"{type(self).__name__} operates on [0,1] but {total} input elements were outside [-1e-6, 1 + 1e-6]")
        return total

    def _table(self, n, inverse):
        """the cached ColumnTable of one direction for an n-wide field, or None outside the kernel's parameter envelope"""
        buf = self._parameter()
        key = (n, bool(inverse), id(buf), buf._version, torch.get_default_dtype())
        cache = self.__dict__.setdefault("_tables", {})
        if cache.get("key") != key[2:]:
            cache.clear()
            cache["key"] = key[2:]
        if key[:2] not in cache:
            values = _column_values(buf, n)
            cache[key[:2]] = None if values is None else self._make_table(n, values, inverse)
        return cache[key[:2]]

    def _on_kernel(self, x, inverse, kwargs, **launch_kw):
        table = self._table(x.shape[1], inverse) if kernel_ok(x, x.shape[-1]) else None
        if table is None:
            return None
        res = run_table(x, table, kwargs, bad=self._bad_counter(x.device), **launch_kw)
        if self.SYNC_RANGE_CHECK:
            self.check_unit_interval()
        return res


class CircularShiftFlow(_RangeChecked):
    """A flow that shifts the position of torsional degrees of freedom: y = (x + shift) mod 1 on [0, 1] (modulo.py:47-76)."""

    def __init__(self, shift):
        super().__init__()
        self.register_buffer("_shift", torch.as_tensor(shift))

    def _parameter(self):
        return self._shift

    def _make_table(self, n, shift, inverse):
        return ColumnTable(n, [(SHIFT, j, -s if inverse else s, 0.0) for j, s in enumerate(shift.tolist())])

    def _forward(self, x, **kwargs):
        res = self._on_kernel(x, False, kwargs)
        if res is not None:
            return res
        _assert_in_unit_interval(x)
        y = (x + self._shift) % 1
        dlogp = torch.zeros_like(x[..., [0]])
        return y, dlogp

    def _inverse(self, x, **kwargs):
        res = self._on_kernel(x, True, kwargs)
        if res is not None:
            return res
        _assert_in_unit_interval(x)
        y = (x - self._shift) % 1
        dlogp = torch.zeros_like(x[..., [0]])
        return y, dlogp


def _randint(high):
    with torch.no_grad():
        return torch.floor(torch.rand(high.shape, device=high.device) * high)


class IncreaseMultiplicityFlow(_RangeChecked, _FusedSampling):
    """A flow that increases the multiplicity of torsional degrees of freedom (modulo.py:7-35): forward places x in [0, 1] on one of
    m sheaves drawn uniformly, y = (x + sheaf) / m; the inverse folds them back, x = (y mod 1 / m) m.

    On the kernel the sheaf is floor(u m) with u the Philox4x32-10 uniform of (seed, stream, call, global row, column) -- key and
    call counter as the fused priors keep them (``set_philox_stream``, ``_philox_state`` in the state_dict); a shard of a batch
    passes ``row0=<its first global row>`` to draw what the whole batch would.  ``sheaf_uniforms=<[B, n] tensor>`` supplies u
    instead.  On CPU tensors the sheaves come from ``torch.rand`` exactly as in the reference."""

    def __init__(self, multiplicities):
        super().__init__()
        self.register_buffer("_multiplicities", torch.as_tensor(multiplicities))

    def _parameter(self):
        return self._multiplicities

    def _make_table(self, n, m, inverse):
        if not (np.all(m >= 1) and np.all(m == np.floor(m)) and np.all(m < 2 ** 20)):
            return None
        if not inverse:
            return ColumnTable(n, [(MULT_FWD, j, v, 0.0) for j, v in enumerate(m.tolist())])
        period = (1 / torch.from_numpy(m.copy())).numpy()           # 1 / m rounded to f32 as torch rounds it
        return ColumnTable(n, [(MULT_INV, j, v, p) for j, (v, p) in enumerate(zip(m.tolist(), period.tolist()))])

    def _forward(self, x, row0=0, sheaf_uniforms=None, **kwargs):
        if kernel_ok(x, x.shape[-1]) and self._table(x.shape[1], False) is not None:
            if sheaf_uniforms is not None:
                u = sheaf_uniforms.detach().to(device=x.device, dtype=torch.float32).contiguous()
                assert u.shape == x.shape, "sheaf_uniforms must have the shape of the input"
                return self._on_kernel(x, False, kwargs, u=u)
            from . import dp
            st = self._philox_ids()
            seed = (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (st[0] + 1)) & (2 ** 64 - 1)
            offset, st[1] = st[1], st[1] + 1
            return self._on_kernel(x, False, kwargs, seed=seed, offset=offset, row0=row0)
        _assert_in_unit_interval(x)
        multiplicities = torch.ones_like(x) * self._multiplicities
        if sheaf_uniforms is not None:
            sheaves = torch.floor(sheaf_uniforms.detach().to(x) * multiplicities)
        else:
            sheaves = _randint(multiplicities)
        y = (x + sheaves) / self._multiplicities
        dlogp = torch.zeros_like(x[..., [0]])
        return y, dlogp

    def _inverse(self, x, **kwargs):
        res = self._on_kernel(x, True, kwargs)
        if res is not None:
            return res
        _assert_in_unit_interval(x)
        y = (x % (1 / self._multiplicities)) * self._multiplicities
        dlogp = torch.zeros_like(x[..., [0]])
        return y, dlogp


class TorchTransform(Flow):
    """Wrap a torch.distributions.Transform as a Flow instance (torchtransform.py:7-33).  ``reinterpreted_batch_ndims`` > 0 wraps
    the transform in a torch.distributions.IndependentTransform.

    An ``AffineTransform`` with scalar or per-column ``loc`` / ``scale`` reinterpreted over the last axis (what
    ``add_constrain_chirality`` builds) runs on the column-map kernel; its log|det J| = sum_j ln|scale_j| is a constant, summed in
    f64 on the host.  Every other transform runs through torch."""
    _bgk_acc = True

    def __init__(self, transform, reinterpreted_batch_ndims=0):
        super().__init__()
        self._affine = transform if (type(transform) is torch.distributions.AffineTransform and reinterpreted_batch_ndims == 1
                                     and transform.event_dim == 0) else None
        if reinterpreted_batch_ndims > 0:
            transform = torch.distributions.IndependentTransform(transform, reinterpreted_batch_ndims)
        self._delegate_transform = transform

    def _table(self, n, inverse):
        t = self._affine
        if t is None:
            return None
        key = tuple((id(p), p._version) if torch.is_tensor(p) else p for p in (t.loc, t.scale)) + (torch.get_default_dtype(),)
        cache = self.__dict__.setdefault("_tables", {})
        if cache.get("key") != key:
            cache.clear()
            cache["key"] = key
        if (n, inverse) not in cache:
            loc, scale = _column_values(t.loc, n), _column_values(t.scale, n)
            table = None
            if loc is not None and scale is not None and np.all(scale != 0) and np.isfinite(scale).all() and np.isfinite(loc).all():
                logdet = math.fsum(math.log(abs(s)) for s in scale.astype(np.float64).tolist())
                kind = AFFINE_INV if inverse else AFFINE_FWD
                table = ColumnTable(n, [(kind, j, l, s) for j, (l, s) in enumerate(zip(loc.tolist(), scale.tolist()))], logdet=logdet)
            cache[(n, inverse)] = table
        return cache[(n, inverse)]

    def _forward(self, x, **kwargs):
        table = self._table(x.shape[1], False) if kernel_ok(x, x.shape[-1]) else None
        if table is not None:
            return run_table(x, table, kwargs)
        y = self._delegate_transform(x)
        dlogp = self._delegate_transform.log_abs_det_jacobian(x, y)
        return y, dlogp[..., None]

    def _inverse(self, y, **kwargs):
        table = self._table(y.shape[1], True) if kernel_ok(y, y.shape[-1]) else None
        if table is not None:
            return run_table(y, table, kwargs, sign=-1.0)
        x = self._delegate_transform.inv(y)
        dlogp = - self._delegate_transform.log_abs_det_jacobian(x, y)
        return x, dlogp[..., None]


# ---- SetConstantFlow -> WrapFlow(index MergeFlow): the pair add_merge_constraints appends, as one launch --------------------------

def constant_merge_pair(first, second, inverse):
    """(set_constant, wrap) if the two blocks, in execution order, are the pair ``SetConstantFlow(one 1-d constant) ->
    WrapFlow(MergeFlow(field indices, constant indices))`` merging the inserted slot into one field (generator_builder.py:491-498),
    else None"""
    const, wrap = (second, first) if inverse else (first, second)
    if not (type(const) is SetConstantFlow and type(wrap) is WrapFlow):
        return None
    merge = wrap._flow
    split = getattr(merge, "_delegate", None)
    if not (type(merge) is MergeFlow and type(split) is SplitFlow and split._indices is not None and len(split._indices) == 2
            and split._split_dim == -1 and len(const.indices) == 1 and const.n_event_dims0 == 1):
        return None
    values = const.values
    slots, out = [int(i) for i in wrap._indices], [int(i) for i in wrap._out_indices]
    k = int(const.indices[0])
    if not (len(values) == 1 and values[0].dim() == 1 and len(slots) == 2 and len(out) == 1 and slots[1] == k and slots[0] != k
            and len(split._indices[1]) == values[0].shape[0]):
        return None
    # the merged tensor must land where the tuple plumbing of the two blocks puts it: the field's slot once the constant's is gone
    if out[0] != slots[0] - (1 if k < slots[0] else 0):
        return None
    return const, wrap


class FusedConstantMerge:
    """callable standing in for ``SetConstantFlow -> WrapFlow(MergeFlow(index lists))`` (forward: constants scattered into the
    field, COPY + CONST table; inverse: the unconstrained columns gathered, COPY table) -- one launch, no [B, c] tensor of repeated
    constants.  Falls back to the two blocks when the field is outside the kernel's envelope."""
    _bgk_acc = True

    def __init__(self, const, wrap):
        self._const, self._wrap = const, wrap

    def _blocks_path(self, xs, inverse, kwargs):
        from .flow import _acc_kwargs
        acc = kwargs.get(ACC_KW)
        total = None
        for block in ((self._wrap, self._const) if inverse else (self._const, self._wrap)):
            *xs, dd = block(*xs, inverse=inverse, **_acc_kwargs(block, kwargs))
            if acc is not None:
                acc.add(dd)
            else:
                total = dd if total is None else total + dd
        return (*xs, acc if acc is not None else total)

    def _table(self, inverse):
        split, value = self._wrap._flow._delegate, self._const.values[0]
        free, fixed = (np.asarray(ix, dtype=np.int64) for ix in split._indices)
        key = (bool(inverse), id(value), value._version)
        cache = self.__dict__.setdefault("_tables", {})
        if key not in cache:
            cache.clear()
            n = len(free) + len(fixed)
            split._check_cover(n, "split" if inverse else "merge")
            table = None
            if inverse:
                table = ColumnTable(n, [(COPY, int(j), 0.0, 0.0) for j in free])
            elif value.dtype == torch.float32 and not value.requires_grad:
                entries = [None] * n
                for i, j in enumerate(free):
                    entries[int(j)] = (COPY, i, 0.0, 0.0)
                for v, j in zip(value.detach().cpu().numpy().tolist(), fixed):
                    entries[int(j)] = (CONST, 0, v, 0.0)
                table = ColumnTable(len(free), entries)
            cache[key] = table
        return cache[key]

    def __call__(self, *xs, inverse=False, **kwargs):
        slot = int(self._wrap._out_indices[0]) if inverse else int(self._wrap._indices[0])
        if not inverse:
            slot -= 1 if int(self._const.indices[0]) < slot else 0      # the constant is not in the tuple yet
        # keyword arguments reach neither block's arithmetic (both ignore them), so they do not keep the pair off the kernel
        x = xs[slot] if 0 <= slot < len(xs) else None
        table = self._table(inverse) if torch.is_tensor(x) and x.dim() == 2 else None
        if table is None or not kernel_ok(x, table.n_in) or table.n_out > COLMAP_MAX_WIDTH or table.n_out < 1:
            return self._blocks_path(xs, inverse, kwargs)
        y, dlogp = run_table(x, table, kwargs)
        return (*xs[:slot], y, *xs[slot + 1:], dlogp)
