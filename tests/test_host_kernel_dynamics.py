"""Host (no GPU): ``KernelDynamics`` and ``DiffEqFlow`` -- signatures and parameter names against the reference's recorded metadata, the torch
formulas (``_forward_torch``, the composed fixed-step integration) in f64 against the reference's recorded f64 results
(tests/golden/kernel_dynamics.npz), the C ABI of csrc/bgk_kdyn.hip as the header declares it."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd._abi import abi_signatures
from kdyn_common import CONFIGS, PARAMS, SETS, SHAPES, err_a, err_s, evaluate, flow_of, make_dynamics

SYMBOLS = ("bgk_kdyn_eval", "bgk_kdyn_eval_backward", "bgk_kdyn_integrate")


def positions(golden, n, d):
    return torch.tensor(golden("particles")[f"x_{n}_{d}"]).reshape(150, n * d).double()


def test_signatures_and_parameters_equal_the_references(golden):
    import bgflow_amd.nn.flow.diffeq as diffeq_mod
    assert diffeq_mod.DiffEqFlow is bg.DiffEqFlow and diffeq_mod.KernelDynamics is bg.KernelDynamics
    assert diffeq_mod.DensityDynamics is bg.DensityDynamics and diffeq_mod.InversedDynamics is bg.InversedDynamics
    G = golden("kernel_dynamics")
    meta = json.loads(str(G["meta"]))
    for name in ("KernelDynamics", "DiffEqFlow"):
        params = list(inspect.signature(getattr(bg, name).__init__).parameters.values())[1:]
        assert [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name] for p in params] == meta[name]["parameters"]
    dyn = make_dynamics(G, "ref", 4, 2)
    assert {k: list(v.shape) for k, v in dyn.named_parameters()} == meta["KernelDynamics"]["named_parameters"]
    fresh = bg.KernelDynamics(4, 2, torch.linspace(0, 8, 10), torch.full((10,), 0.3), torch.linspace(0, 1, 5), torch.full((5,), 0.3))
    assert [k for k, _ in fresh.named_parameters()] == ["_weights", "_bias", "_importance"]
    assert float(fresh._bias.detach().abs().max()) == 0.0 and float(fresh._importance.detach().abs().max()) == 0.0 and float(fresh._weights.detach().abs().max()) > 0
    both = bg.KernelDynamics(4, 2, torch.linspace(0, 8, 10), torch.full((10,), 0.3), torch.linspace(0, 1, 5), torch.full((5,), 0.3),
                             optimize_d_gammas=True, optimize_t_gammas=True)
    assert {"_neg_log_gammas", "_neg_log_gammas_time"} <= {k for k, _ in both.named_parameters()}
    torch.testing.assert_close(both._neg_log_gammas.detach(), -torch.log(torch.full((10,), 0.3)))


def test_no_time_kernels_means_no_time_modulation():
    """the deviation from the reference, which raises on mus_time=None: one output column, tau = 1"""
    torch.manual_seed(1)
    dyn = bg.KernelDynamics(3, 2, torch.linspace(0, 4, 6), torch.full((6,), 0.5)).double()
    assert dyn._weights.shape == (6, 1) and dyn._bias.shape == (1, 1) and dyn._n_out == 1
    x = torch.randn(5, 6, dtype=torch.float64)
    f0, d0 = dyn(0.0, x)
    f1, d1 = dyn(0.9, x)
    assert torch.equal(f0, f1) and torch.equal(d0, d1) and f0.abs().max() > 0
    assert torch.equal(dyn(0.0, x, compute_divergence=False), f0)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_torch_formulas_reproduce_the_reference_in_f64(golden, name, n, d):
    G = golden("kernel_dynamics")
    key = f"{name}_{n}_{d}_"
    rows = G[key + "rows"]
    dyn = make_dynamics(G, name, n, d, torch.float64)
    x = positions(golden, n, d)
    for i, t in enumerate(G["times"]):
        r = evaluate(dyn, x, float(t))
        assert r["f"].dtype == np.float64
        errs = {"div": err_s(r["div"], G[key + "div64"][i])}
        if f"{key}f64_t{i}" in G.files:
            errs["f"] = err_a(r["f"][rows], G[f"{key}f64_t{i}"])
        if i == 1:
            errs["gx"] = err_a(r["gx"][rows], G[key + "gx64"])
        for p in PARAMS:
            errs["g" + p] = err_a(r["g" + p], G[f"{key}g64{p}"][i])
        assert max(errs.values()) <= 1e-12, (i, errs)
    assert ("f" in errs) == (n * d <= 64)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_composed_integration_reproduces_the_golden_trajectories_in_f64(golden, name, n, d):
    G = golden("kernel_dynamics")
    key = f"{name}_{n}_{d}_"
    rows = G[key + "rows"]
    dyn = make_dynamics(G, name, n, d, torch.float64)
    x = positions(golden, n, d)
    sub = np.arange(150) if n * d <= 64 else rows[:8]          # the widest shape: eight rows keep the f64 op chain quick
    pos = {int(r): k for k, r in enumerate(rows)}
    x = x[sub]
    seen = 0
    with torch.no_grad():
        for ci, (m, nt, dr) in enumerate(CONFIGS):
            tag = f"{m}{nt}{dr}"
            y, dlogp = flow_of(dyn, m, nt)(x, inverse=dr == "i", temperature=1.0)
            assert y.shape == x.shape and dlogp.shape == (len(sub), 1)
            assert err_s(dlogp.numpy(), G[key + "dlogp64"][ci][sub]) <= 1e-12, tag
            if f"{key}y64_{tag}" in G.files:
                kept = [k for k, r in enumerate(sub) if int(r) in pos]
                assert err_a(y.numpy()[kept], G[f"{key}y64_{tag}"][[pos[int(sub[k])] for k in kept]]) <= 1e-12, tag
                seen += 1
    assert seen == ({"ref": 8, "edge": 4}[name] if n * d <= 64 else int(name == "ref"))


def test_edge_rows_in_f64(golden):
    G = golden("kernel_dynamics")
    dyn = make_dynamics(G, "ref", 4, 3, torch.float64, prefix="edge_")
    r = evaluate(dyn, torch.tensor(G["edge_x"]).reshape(8, 12).double(), float(G["times"][1]))
    assert err_a(r["f"], G["edge_f64"]) <= 1e-12 and err_s(r["div"], G["edge_div64"]) <= 1e-12 and err_a(r["gx"], G["edge_gx64"]) <= 1e-12
    for p in PARAMS:
        assert err_a(r["g" + p], G[f"edge_g64{p}"]) <= 1e-12
    # f32 on the CPU: the far-away particle's pairs underflow to kern = dkern = 0, nothing is NaN
    r32 = evaluate(make_dynamics(G, "ref", 4, 3, prefix="edge_"), torch.tensor(G["edge_x"]).reshape(8, 12), float(G["times"][1]))
    assert all(np.isfinite(v).all() for v in r32.values())


def test_linear_dynamics_log_density():
    """dx = -x has the divergence -dim: RK4 over 20 steps gives dlogp = -dim (the reference's test_nODE property)"""

    class Linear(torch.nn.Module):
        def forward(self, t, x):
            return -x, torch.full((x.shape[0], 1), float(x.shape[1]), dtype=x.dtype)

    dim = 5
    x = torch.randn(7, dim, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    flow = bg.DiffEqFlow(Linear(), use_checkpoints=True, Nt=20, method="RK4")
    y, dlogp = flow(x)
    assert float((dlogp + dim).abs().max()) <= 1e-6
    torch.testing.assert_close(y, x * np.exp(-1.0), rtol=1e-6, atol=0)
    back, dl2 = flow(y, inverse=True)
    torch.testing.assert_close(back, x, rtol=1e-5, atol=0)
    assert float((dl2 - dim).abs().max()) <= 1e-6


def test_adaptive_mode_raises_the_documented_error():
    dyn = bg.KernelDynamics(3, 2, torch.linspace(0, 4, 6), torch.full((6,), 0.5))
    flow = bg.DiffEqFlow(dyn)
    assert (flow._integrator_method, flow._integrator_atol, flow._integrator_rtol, flow._n_time_steps, flow._t_max, flow._use_checkpoints) == (
        "dopri5", 1e-10, 1e-5, 2, 1.0, False)
    with pytest.raises(NotImplementedError, match="use_checkpoints=True"):
        flow(torch.zeros(2, 6))
    with pytest.raises(ValueError, match="RK4 or Euler"):
        bg.DiffEqFlow(dyn, use_checkpoints=True, Nt=2, method="midpoint")(torch.zeros(2, 6))


def test_c_abi_of_the_kernel_dynamics(hip_lib):
    sigs = abi_signatures()
    d, i32, i64, p = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    head = [p, i64, i32, i32, i32, i32, p, p, p, p, p, p, p, d]
    assert sigs["bgk_kdyn_eval"] == (ctypes.c_int, head + [p, p, p])
    assert sigs["bgk_kdyn_eval_backward"] == (ctypes.c_int, head + [p, p, p, p, i32, p, p])
    assert sigs["bgk_kdyn_integrate"] == (ctypes.c_int, head + [i32, i32, i32, p, p, p])
    for name in SYMBOLS:
        assert list(getattr(hip_lib, name).argtypes) == sigs[name][1]
    # argument checks that return before any device work
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def common(n=4, dims=2, K=10, O=5, time=True):
        return (n, dims, K, O, fake, fake, fake, fake, fake, fake if time else None, fake if time else None)

    assert hip_lib.bgk_kdyn_eval(None, 0, *common(), 0.5, None, None, None) == 0                      # an empty batch
    assert hip_lib.bgk_kdyn_integrate(None, 0, *common(), 1.0, 4, 0, 0, None, None, None) == 0
    for kw in (dict(n=65), dict(n=1), dict(dims=4), dict(K=65), dict(O=17), dict(K=0)):
        assert hip_lib.bgk_kdyn_eval(None, 8, *common(**kw), 0.5, None, None, None) == -2
        assert b"envelope" in hip_lib.bgk_last_error()
    assert hip_lib.bgk_kdyn_eval(None, 8, *common(), 0.5, None, None, None) == -1                      # null tensors
    assert hip_lib.bgk_kdyn_eval(None, 8, *common(time=False), 0.5, None, None, None) == -1            # n_out 5 without time kernels
    assert hip_lib.bgk_kdyn_integrate(None, 8, *common(), 1.0, 0, 0, 0, None, None, None) == -1        # no steps
    assert hip_lib.bgk_kdyn_integrate(None, 8, *common(), 1.0, 4, 2, 0, None, None, None) == -1        # unknown method
    assert hip_lib.bgk_kdyn_eval_backward(None, 8, *common(), 0.5, None, None, None, None, 0, None, None) == -1
