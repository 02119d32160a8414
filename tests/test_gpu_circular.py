"""GPU (-m gpu): ``bgflow_amd.circular`` on csrc/bgk_circular.hip against the reference's f64 run (tests/golden/circular.npz, written by
tests/golden/make_circular_goldens.py), against the f64 torch path that tests/test_host_circular.py pins to that fixture, and bitwise
against itself.  Inputs, special rows and row groups: tests/circular_common.py.

Parity bound, the project's bound for every kernel: |v - v64| / (1 + |v64|) <= 4 err_v32 + 1e-6 with err_v32 the error of the
reference's own f32 run of that quantity -- on the NARROW row for that row, on the BULK rows for every other group (the
UNYARDSTICKED rows, where the reference's f32 run is NaN or wrong, and the TIES rows, whose gradients of y and mu_raw are compared
with central differences).  All 100 rows of every case are compared.  Every test first asserts that its case takes the kernel."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
import circular_common as cc
from bgflow_amd import circular
from bgflow_amd.circular import circular_bump_transform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(golden):
    return golden("circular")


@pytest.fixture(scope="module")
def on_dev(hip_lib, dev):
    @functools.lru_cache(maxsize=None)
    def case(K, D, well=False):
        """(mu_raw, log_sigma, log_weight, log_eps, y, a, c, t) of the case on the device, f32"""
        return tuple(cc.tensors(cc.inputs(K, D, well=well), torch.float32, dev))

    return case


def kernel(y, *params, inverse=False):
    """the transform, asserted to run on the kernel"""
    D = y.shape[-1]
    K = params[0].numel() // params[0].shape[0] // D
    assert circular._kernel_takes(y, params, K, inverse), "the case must take the kernel path"
    out = circular_bump_transform(y, *params, inverse=inverse)
    if out[0].requires_grad:
        assert type(out[0].grad_fn).__name__ == "_CircularBumpFnBackward"
    return out


@pytest.mark.parametrize("K,D", cc.ENVELOPE)
def test_forward_parity(G, on_dev, dev, K, D):
    """out, dlogp and the five gradients of sum a out + sum c dlogp on every row"""
    res = cc.evaluate(kernel, cc.inputs(K, D), torch.float32, dev)
    cc.assert_within(cc.group_errors(res, G, cc.key(K, D)), G, cc.key(K, D), what="kernel ")


@pytest.mark.parametrize("K,D", cc.ENVELOPE)
def test_inverse_bracket_and_dlogp(G, on_dev, K, D):
    """with h = 2^-23 and tol = 4 x (the reference's f32 absolute error of out on BULK and NARROW) + 1e-6:
    out64(x - h) - tol <= t <= out64(x + h) + tol on every row, out64 the f64 torch path at clamp(x -+ h, 0, 1) -- the statement of
    an inverse for a monotone map that may be nearly flat or nearly a step; and dlogp = -(the kernel forward's dlogp at the same x)
    within 1e-6 (1 + |dlogp|)"""
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    x, dlogp = kernel(t, mr, ls, lw, le, inverse=True)
    circular.check_unit_interval()
    assert x.shape == t.shape and dlogp.shape == (cc.B, 1)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
    h, tol = 2.0 ** -23, 4.0 * float(G[cc.key(K, D) + "abserr_out32"]) + 1e-6
    p64 = [v.double().cpu() for v in (mr, ls, lw, le)]
    x64, t64 = x.double().cpu(), t.double().cpu()
    below = circular_bump_transform((x64 - h).clamp(0.0, 1.0), *p64)[0]
    above = circular_bump_transform((x64 + h).clamp(0.0, 1.0), *p64)[0]
    worst = max(float((below - t64).max()), float((t64 - above).max()))
    print(f"({K}, {D}): worst bracket violation {worst:.3g}, tolerance {tol:.3g}")
    assert (below - tol <= t64).all() and (t64 <= above + tol).all()
    fwd = kernel(x, mr, ls, lw, le)[1]
    err = float(((dlogp + fwd).abs() / (1.0 + dlogp.abs())).max())
    print(f"({K}, {D}): inverse dlogp against the forward's at x: {err:.3g}")
    assert err <= 1e-6


def test_inverse_gradients(G, on_dev):
    """the well-conditioned (4, 3) case: the kernel's inverse backward against the implicit-function gradients formed here from the f64
    torch-path FORWARD at the kernel's own x.  Bound: 4 x (the reference's f32 error of that gradient on this case) / (the smallest
    density of the case) + 1e-6, relative to 1 + |v64|: dividing by the density is the only amplification the formula adds."""
    K, D = cc.WELL
    k = cc.key(K, D, well=True)
    mr, ls, lw, le, y, a, c, t = on_dev(K, D, well=True)
    leaves = [v.detach().clone().requires_grad_(True) for v in (t, mr, ls, lw, le)]
    x, dlogp = kernel(*leaves, inverse=True)
    got = torch.autograd.grad((a * x).sum() + (c * dlogp[:, 0]).sum(), leaves)
    # f64: x(t, theta) solves out(x, theta) = t; dx/dt = 1 / f_tot, dx/dtheta = -(d out / d theta) / f_tot; dlogp = -sum_j L(x, theta)
    a64, c64 = a.double().cpu(), c.double().cpu()
    x64 = x.detach().double().cpu().requires_grad_(True)
    p64 = [v.detach().double().cpu().requires_grad_(True) for v in (mr, ls, lw, le)]
    out64, logf = circular._elementwise(x64, *circular._shaped(p64, K, D))
    ftot = logf.exp()
    dL_dx, = torch.autograd.grad(logf.sum(), x64, retain_graph=True)
    Gx = a64 - c64[:, None] * dL_dx
    want = [Gx / ftot]
    direct = torch.autograd.grad(logf, p64, grad_outputs=-c64[:, None].expand_as(logf), retain_graph=True)
    implicit = torch.autograd.grad(out64, p64, grad_outputs=-(Gx / ftot).detach())
    want += [d + i for d, i in zip(direct, implicit)]
    density = float(G[k + "min_density"])
    for name, g, w in zip(("g_y", "g_mu", "g_ls", "g_lw", "g_le"), got, want):
        err = cc.rel_err(g.cpu().numpy(), w.detach().numpy())
        bound = 4.0 * float(G[f"{k}err_{name}32_bulk"]) / density + 1e-6
        print(f"inverse {name}: error {err:.3g}, bound {bound:.3g}")
        assert np.isfinite(err) and err <= bound, (name, err, bound)


def test_rows_do_not_depend_on_the_batch(on_dev):
    """a batch of 100 against the same rows in batches of 7: bitwise equal, forward, inverse and both backwards"""
    K, D = 8, 5
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)

    def run(rows, inverse):
        leaves = [v[rows].detach().clone().requires_grad_(True) for v in ((t if inverse else y), mr, ls, lw, le)]
        out, dlogp = kernel(*leaves, inverse=inverse)
        grads = torch.autograd.grad((a[rows] * out).sum() + (c[rows] * dlogp[:, 0]).sum(), leaves)
        return (out.detach(), dlogp.detach(), *grads)

    for inverse in (False, True):
        whole = run(slice(0, cc.B), inverse)
        for r0 in range(0, cc.B, 7):
            part = run(slice(r0, min(r0 + 7, cc.B)), inverse)
            for w, p in zip(whole, part):
                assert torch.equal(w[r0:r0 + 7], p), (inverse, r0)


def test_several_tiles(on_dev, dev):
    """1000 rows of the (8, 5) case (the 100 rows tiled ten times): tiles of 409 rows, so three workgroups and a partial last tile;
    every copy of a row equals the row of the single-tile run bit for bit"""
    K, D = 8, 5
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    rep = lambda v: v.repeat(10, *([1] * (v.dim() - 1))).contiguous()
    for inverse in (False, True):
        src = t if inverse else y
        small = kernel(src, mr, ls, lw, le, inverse=inverse)
        big = kernel(rep(src), rep(mr), rep(ls), rep(lw), rep(le), inverse=inverse)
        assert big[0].shape == (1000, D) and big[1].shape == (1000, 1)
        assert torch.equal(big[0], rep(small[0])) and torch.equal(big[1], rep(small[1]))
        leaves = [rep(v).requires_grad_(True) for v in (src, mr, ls, lw, le)]
        o, dl = kernel(*leaves, inverse=inverse)
        gb = torch.autograd.grad((rep(a) * o).sum() + (rep(c) * dl[:, 0]).sum(), leaves)
        leaves = [v.detach().clone().requires_grad_(True) for v in (src, mr, ls, lw, le)]
        o, dl = kernel(*leaves, inverse=inverse)
        gs = torch.autograd.grad((a * o).sum() + (c * dl[:, 0]).sum(), leaves)
        for b, s in zip(gb, gs):
            assert torch.equal(b, rep(s))


def test_parameter_layouts(G, on_dev, dev):
    """strided parameters are re-laid and give the kernel's result bit for bit; a strided input takes the torch path and stays within
    the parity bound; shared parameters (pitch 0: the unconditioned class) equal expanded ones bit for bit, their gradients the batch sum"""
    K, D = 8, 5
    k = cc.key(K, D)
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    base = kernel(y, mr, ls, lw, le)
    wide = torch.zeros(cc.B, 2 * K * D, device=dev)
    wide[:, ::2] = mr
    strided = kernel(y, wide[:, ::2], ls, lw, le)
    assert not wide[:, ::2].is_contiguous() and torch.equal(strided[0], base[0]) and torch.equal(strided[1], base[1])
    ywide = torch.zeros(cc.B, 2 * D, device=dev)
    ywide[:, ::2] = y
    assert not circular._kernel_takes(ywide[:, ::2], (mr, ls, lw, le), K, False)
    out, dlogp = circular_bump_transform(ywide[:, ::2], mr, ls, lw, le)
    res = (out.cpu().numpy(), dlogp[:, 0].cpu().numpy())
    cc.assert_within(cc.group_errors(res, G, k, names=("out", "dlogp")), G, k, what="strided input ")
    # pitch 0
    torch.manual_seed(3)
    flow = bg.CircularTransformSimple(n_bases=K, n_dim=D).to(dev)
    shared = [p.detach() for p in (flow._mu, flow._log_sigma, flow._log_weight, flow._log_eps)]
    expanded = [p.expand(cc.B, *p.shape[1:]).contiguous() for p in shared]
    for inverse in (False, True):
        src = t if inverse else y
        one = flow(None, src, inverse=inverse)
        assert type(one[0].grad_fn).__name__ == "_CircularBumpFnBackward"
        full = kernel(src, *expanded, inverse=inverse)
        assert torch.equal(one[0], full[0]) and torch.equal(one[1], full[1])
        g_one = torch.autograd.grad((a * one[0]).sum() + (c * one[1][:, 0]).sum(), list(flow.parameters()))
        leaves = [p.clone().requires_grad_(True) for p in expanded]
        o, dl = kernel(src, *leaves, inverse=inverse)
        g_full = torch.autograd.grad((a * o).sum() + (c * dl[:, 0]).sum(), leaves)
        for g1, gf, p in zip(g_one, g_full, flow.parameters()):
            assert g1.shape == p.shape and torch.equal(g1, gf.sum(0, keepdim=True).reshape(p.shape))


def test_fallbacks(G, on_dev, dev, monkeypatch):
    """K = 33, an f64 input and create_graph=True take the torch path"""
    K, D = 33, 2
    k = cc.key(K, D)
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    assert not circular._kernel_takes(y, (mr, ls, lw, le), K, False)
    res = cc.evaluate(circular_bump_transform, cc.inputs(K, D), torch.float32, dev, grads=False)
    cc.assert_within(cc.group_errors(res, G, k, names=("out", "dlogp")), G, k, what="K = 33 ")
    K, D = 3, 2
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    d64 = [v.double() for v in (y, mr, ls, lw, le)]
    assert not circular._kernel_takes(d64[0], d64[1:], K, False)
    res = cc.evaluate(circular_bump_transform, cc.inputs(K, D), torch.float64, dev)
    cc.assert_exact(cc.group_errors(res, G, cc.key(K, D)), what="f64 on the device ")
    # create_graph: the forward runs on the kernel, the recorded backward on the torch formulas from the saved inputs (the inverse's at
    # the kernel's x): the backward kernel is never launched, the gradient carries a graph and second derivatives come out finite.
    # The recorded first-order gradient and the backward kernel's are both within the parity bound of the f64 value, so they differ
    # by at most twice that bound (the reference's recorded f32 error of g_y on this case; for the inverse divided by the smallest
    # density, as in test_inverse_gradients).  The values of the torch path's second derivatives are gradgradcheck'ed on the host.
    K, D = cc.WELL
    k = cc.key(K, D, well=True)
    mr, ls, lw, le, y, a, c, t = on_dev(K, D, well=True)

    def refuse(*args, **kwargs):
        raise AssertionError("the backward kernel ran under create_graph=True")

    for inverse in (False, True):
        src = (t if inverse else y).detach().clone().requires_grad_(True)
        params = [v.detach().clone().requires_grad_(True) for v in (mr, ls, lw, le)]
        out, dlogp = kernel(src, *params, inverse=inverse)
        scalar = (a * out).sum() + (c * dlogp[:, 0]).sum()
        plain, = torch.autograd.grad(scalar, src, retain_graph=True)
        monkeypatch.setattr(circular, "_launch_backward", refuse)
        g, = torch.autograd.grad(scalar, src, create_graph=True)
        assert g.requires_grad
        second = torch.autograd.grad(g.sum(), [src] + params)
        monkeypatch.undo()
        assert all(torch.isfinite(v).all() for v in second)
        err = cc.rel_err(g.detach().cpu().numpy(), plain.cpu().numpy())
        bound = 2.0 * (4.0 * float(G[k + "err_g_y32_bulk"]) / (float(G[k + "min_density"]) if inverse else 1.0) + 1e-6)
        print(f"create_graph g_y against the backward kernel's (inverse = {inverse}): difference {err:.3g}, bound {bound:.3g}")
        assert err <= bound


def test_range_counter(on_dev):
    """one target of 1.1 makes check_unit_interval() raise; a clean call does not"""
    K, D = 3, 2
    mr, ls, lw, le, y, a, c, t = on_dev(K, D)
    circular.check_unit_interval()
    kernel(t, mr, ls, lw, le, inverse=True)
    assert circular.check_unit_interval() == 0
    bad = t.clone()
    bad[17, 1] = 1.1
    kernel(bad, mr, ls, lw, le, inverse=True)
    with pytest.raises(ValueError):
        circular.check_unit_interval()
    assert circular.check_unit_interval() == 0          # the poll reset the counter
    flow = bg.CircularTransformSimple(n_bases=K, n_dim=D).to(t.device)
    with torch.no_grad():
        flow(None, bad, inverse=True)
    with pytest.raises(ValueError):
        flow.check_unit_interval()
