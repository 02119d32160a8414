"""Host (CPU): the torch path of ``bgflow_amd.circular`` against the reference's f64 and f32 runs (tests/golden/circular.npz, written
by tests/golden/make_circular_goldens.py; inputs, special rows and row groups: tests/circular_common.py).

f64: 1e-12 relative to 1 + |v64| on every row, except the gradients of y and mu_raw on the TIES rows, where the reference's autograd
is an artefact of abs'(0) = 0: those are compared with the recorded central differences within 1e-7.  f32: the project's bound,
4 x (the reference's own f32 error of the quantity: on the NARROW row for that row, on the BULK rows for every other group) + 1e-6."""
import functools

import numpy as np
import pytest
import torch

import bgflow_amd as bg
import circular_common as cc
from bgflow_amd import circular
from bgflow_amd.circular import circular_bump_transform


@pytest.fixture(scope="module")
def G(golden):
    return golden("circular")


@functools.lru_cache(maxsize=None)
def cpu_run(K, D, dtype, grads=True):
    return cc.evaluate(circular_bump_transform, cc.inputs(K, D), dtype, grads=grads)


def test_inputs_are_the_fixtures(G):
    for K, D in cc.CASES:
        np.testing.assert_array_equal(cc.checksum(cc.inputs(K, D)), G[cc.key(K, D) + "check"])
        np.testing.assert_array_equal(cc.inputs(K, D)["t"], G[cc.key(K, D) + "t"])
    np.testing.assert_array_equal(cc.checksum(cc.inputs(*cc.WELL, well=True)), G[cc.key(*cc.WELL, well=True) + "check"])
    assert len(cc.BULK) + len(cc.NARROW) + len(cc.TIES) + len(cc.UNYARDSTICKED) == cc.B


@pytest.mark.parametrize("K,D", cc.ENVELOPE)
def test_f64_matches_the_reference(G, K, D):
    cc.assert_exact(cc.group_errors(cpu_run(K, D, torch.float64), G, cc.key(K, D)))


@pytest.mark.parametrize("K,D", cc.ENVELOPE)
def test_f32_within_the_references_own_error(G, K, D):
    res = cpu_run(K, D, torch.float32)
    assert all(v.dtype == np.float32 for v in res)
    cc.assert_within(cc.group_errors(res, G, cc.key(K, D)), G, cc.key(K, D))


def test_case_outside_the_envelope_runs(G):
    K, D = 33, 2
    k = cc.key(K, D)
    cc.assert_exact(cc.group_errors(cpu_run(K, D, torch.float64, grads=False), G, k, names=("out", "dlogp")))
    cc.assert_within(cc.group_errors(cpu_run(K, D, torch.float32, grads=False), G, k, names=("out", "dlogp")), G, k)


def test_saturation_is_finite_in_f32():
    """rows 3 and 4 (log_sigma = 40), where the reference's f32 run is NaN: every value and gradient is finite"""
    for K, D in cc.ENVELOPE:
        for v in cpu_run(K, D, torch.float32):
            assert np.isfinite(v[[3, 4]]).all()


def test_seam_tie_is_monotone_in_f32():
    """row 5 (f32 mu == 1.0, y = 0.5 = mu - 0.5 exactly): out(0.5 - 2^-24) <= out(0.5) <= out(0.5 + 2^-24), and out(0.5) = 0.5"""
    for K, D in cc.ENVELOPE:
        inp = cc.inputs(K, D)
        mr, ls, lw, le, y, *_ = cc.tensors(inp, torch.float32, rows=[5])
        assert float((0.5 * torch.sin(mr) + 0.5).min()) == 1.0
        outs = [circular_bump_transform(y + d, mr, ls, lw, le)[0] for d in (-2.0 ** -24, 0.0, 2.0 ** -24)]
        assert (y - 2.0 ** -24 < y).all() and (y + 2.0 ** -24 > y).all()
        assert (outs[0] <= outs[1]).all() and (outs[1] <= outs[2]).all()
        assert float((outs[1] - 0.5).abs().max()) <= 1e-6


@pytest.mark.parametrize("K,D", cc.ENVELOPE)
def test_inverse_round_trip_f64(K, D):
    """x = inverse(forward(y)): |x - y| <= 2^-24 on every row (25 halvings leave a bracket of 2^-25), dlogp the negative of the
    forward's at x"""
    mr, ls, lw, le, y, *_ = cc.tensors(cc.inputs(K, D), torch.float64)
    out, _ = circular_bump_transform(y, mr, ls, lw, le)
    x, dlogp = circular_bump_transform(out, mr, ls, lw, le, inverse=True)
    assert x.shape == y.shape and dlogp.shape == (cc.B, 1)
    err = float((x - y).abs().max())
    print(f"({K}, {D}): |x - y| {err:.3g}")
    assert err <= 2.0 ** -24
    torch.testing.assert_close(dlogp, -circular_bump_transform(x, mr, ls, lw, le)[1], rtol=0, atol=1e-12)


def well_inputs(n=6):
    K, D = cc.WELL
    mr, ls, lw, le, y, a, c, t = cc.tensors(cc.inputs(K, D, well=True), torch.float64, rows=list(range(n)))
    return K, D, mr, ls, lw, le, y, t


def test_inverse_gradcheck(monkeypatch):
    """gradcheck's central differences (step 1e-6) need x far better resolved than the 2^-26 of 25 halvings, which alone would put
    2^-26 / 1e-6 = 1.5e-2 of noise on every numerical derivative: the bisection runs 52 halvings here (f64 resolves them); the
    backward under test does not depend on the trip count.  gradcheck's default tolerances."""
    monkeypatch.setattr(circular, "N_HALVINGS", 52)
    K, D, mr, ls, lw, le, y, t = well_inputs()
    leaves = [v.clone().requires_grad_(True) for v in (t, mr, ls, lw, le)]
    assert torch.autograd.gradcheck(lambda *v: circular_bump_transform(*v, inverse=True), leaves, eps=1e-6, atol=1e-5, rtol=1e-3)


def test_inverse_second_order(monkeypatch):
    """the inverse's backward is written in differentiable torch ops at the returned x: its own derivatives check out too"""
    monkeypatch.setattr(circular, "N_HALVINGS", 52)
    K, D, mr, ls, lw, le, y, t = well_inputs(2)
    leaves = [v.clone().requires_grad_(True) for v in (t, mr, ls, lw, le)]
    assert torch.autograd.gradgradcheck(lambda *v: circular_bump_transform(*v, inverse=True), leaves, eps=1e-6, atol=1e-5, rtol=1e-3)


def test_forward_gradcheck_and_second_order():
    K, D, mr, ls, lw, le, y, t = well_inputs(3)
    leaves = [v.clone().requires_grad_(True) for v in (y, mr, ls, lw, le)]
    assert torch.autograd.gradcheck(lambda *v: circular_bump_transform(*v), leaves, eps=1e-6, atol=1e-5, rtol=1e-3)
    assert torch.autograd.gradgradcheck(lambda *v: circular_bump_transform(*v), leaves, eps=1e-6, atol=1e-5, rtol=1e-3)


def test_inverse_out_of_range_raises():
    K, D, mr, ls, lw, le, y, t = well_inputs()
    bad = t.clone()
    bad[2, 1] = 1.1
    with pytest.raises(ValueError):
        circular_bump_transform(bad, mr, ls, lw, le, inverse=True)
    circular_bump_transform(t, mr, ls, lw, le, inverse=True)


def test_shared_parameters_broadcast():
    K, D, mr, ls, lw, le, y, t = well_inputs()
    one = [v[:1] for v in (mr, ls, lw, le)]
    full = [v.expand(y.shape[0], -1) for v in one]
    for inverse in (False, True):
        a = circular_bump_transform(y, *one, inverse=inverse)
        b = circular_bump_transform(y, *full, inverse=inverse)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        circular_bump_transform(y, mr[:2], ls[:2], lw[:2], le[:2])


def test_unconditioned_class_state_dict_and_init():
    torch.manual_seed(0)
    flow = bg.CircularTransformSimple(n_bases=7, n_dim=3)
    sd = flow.state_dict()
    assert list(sd) == ["_mu", "_log_sigma", "_log_weight", "_log_eps"]
    assert [tuple(v.shape) for v in sd.values()] == [(1, 7, 3), (1, 7, 3), (1, 7, 3), (1, 3)]
    assert 0.0 <= float(sd["_mu"].min()) and float(sd["_mu"].max()) <= 2 * np.pi
    other = bg.CircularTransformSimple(n_bases=7, n_dim=3)
    other.load_state_dict(sd)
    y = torch.rand(11, 3)
    a, b = flow(None, y), other(None, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape == (11, 1)
    x, dl = flow(None, a[0], inverse=True)
    assert float((x - y).detach().abs().max()) < 1e-5 and float((dl + a[1]).detach().abs().max()) < 1e-4
    loss = (flow(None, y)[1].sum() + flow(None, y, inverse=True)[1].sum())
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.shape == p.shape for p in flow.parameters())
    from bgflow_amd.nn.flow.circular import CircularTransformSimple as compat
    assert compat is bg.CircularTransformSimple


def test_conditional_class_in_a_coupling_flow():
    torch.manual_seed(1)
    K, D, n_cond = 5, 3, 4
    nets = [torch.nn.Linear(n_cond, K * D) for _ in range(3)] + [torch.nn.Linear(n_cond, D)]
    transformer = bg.ConditionalCircularTransformSimple(*nets)
    assert [n for n, _ in transformer.named_children()] == ["_mu", "_log_sigma", "_log_weight", "_log_eps"]
    flow = bg.CouplingFlow(transformer)
    cond, y = torch.randn(9, n_cond), torch.rand(9, D)
    c2, out, dlogp = flow(cond, y)
    assert c2 is cond and out.shape == y.shape and dlogp.shape == (9, 1)
    assert float(out.detach().min()) >= 0.0 and float(out.detach().max()) <= 1.0
    c3, back, dl2 = flow(cond, out.detach(), inverse=True)
    assert float((back - y).abs().max()) < 1e-5 and float((dl2 + dlogp).abs().max()) < 1e-4
    (dlogp.sum() + dl2.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in flow.parameters())
    other = bg.ConditionalCircularTransformSimple(*[torch.nn.Linear(n_cond, K * D) for _ in range(3)], torch.nn.Linear(n_cond, D))
    other.load_state_dict(transformer.state_dict())
    assert torch.equal(other(cond, y)[0], transformer(cond, y)[0])


def test_module_is_exported():
    assert bg.circular is circular and bg.circular_bump_transform is circular_bump_transform
    assert set(circular.FUSED) == {"forward", "inverse", "backward"}


def test_recorded_backward_of_the_kernel_function(monkeypatch):
    """``_CircularBumpFn`` with a stand-in for the launch (the torch formulas without a graph): under create_graph=True its backward
    runs the torch formulas from the saved inputs, never the backward kernel, terminates (the saved output enters it detached: with
    its graph the engine would re-enter the node without end) and gives the general path's first and second derivatives"""
    def launch(y, params, K, inverse):
        with torch.no_grad():
            return circular._transform_torch(y, circular._shaped([p.detach() for p in params], K, y.shape[1]), inverse)

    def refuse(*args, **kwargs):
        raise AssertionError("the backward kernel ran under create_graph=True")

    K, D, mr, ls, lw, le, y, t = well_inputs()
    for inverse in (False, True):
        def derivatives(patched):
            with monkeypatch.context() as m:
                if patched:
                    m.setattr(circular, "_launch", launch)
                    m.setattr(circular, "_launch_backward", refuse)
                    m.setattr(circular, "_kernel_takes", lambda *args: True)
                src = (t if inverse else y).clone().requires_grad_(True)
                params = [v.clone().requires_grad_(True) for v in (mr, ls, lw, le)]
                out, dlogp = circular_bump_transform(src, *params, inverse=inverse)
                assert (type(out.grad_fn).__name__ == "_CircularBumpFnBackward") == patched
                g, = torch.autograd.grad(out.sum() + 0.7 * dlogp.sum(), src, create_graph=True)
                return (g.detach(), *torch.autograd.grad(g.sum(), [src] + params))

        for got, want in zip(derivatives(True), derivatives(False)):
            torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12)
