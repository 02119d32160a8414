"""Host (no GPU): the particle box -- ``RepulsiveParticles`` / ``HarmonicParticles`` -- names, signatures and defaults against the
reference's recorded metadata, the torch formulas against its f64 energies, gradients, forces and surrogate (tests/golden/box.npz, written
by tests/golden/make_box_goldens.py), the four bgk_box_* prototypes as the header declares them with their argument checks, the plan type,
and the stochastic layers around such a target on their torch paths."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols
from bgflow_amd.distributions import BoxPlan, PairPlan, _kernel_plan, kernel_energy, kl_loss_sums

from box_common import B, KINDS, NSOLVENT, err_g, err_u, make

f64, i32, i64, u32, u64, p = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
HEAD = [p, i64, i64, i32, i32, p, i32, f64]
WANT = {
    "bgk_box_energy": HEAD + [p, p],
    "bgk_box_energy_kl_sums": HEAD + [p, p, i32, p, i32, p, p],
    "bgk_box_energy_backward": HEAD + [p, p, p, p, i32, p, p, i64, p],
    "bgk_box_mcmc": [p, i64, i32, i32, p, i32, p, i32, f64, p, f64, i32, p, p, u64, u32, i64, p, p, i32, p, i32, p],
}


def test_classes_are_exported_with_the_references_signatures_and_defaults(golden):
    import bgflow_amd.distribution.energy as energy_mod
    import bgflow_amd.distribution.energy.particles as particles_mod
    for mod in (energy_mod, particles_mod):
        assert mod.RepulsiveParticles is bg.RepulsiveParticles and mod.HarmonicParticles is bg.HarmonicParticles
    meta = json.loads(str(golden("box")["meta"]))
    assert bg.RepulsiveParticles.params_default == meta["params_default"]
    assert bg.HarmonicParticles.params_default == meta["harmonic_params_default"]
    for name in ("RepulsiveParticles", "HarmonicParticles"):
        params = list(inspect.signature(getattr(bg, name).__init__).parameters.values())[1:]
        assert [[q.name, None if q.default is inspect.Parameter.empty else q.default] for q in params] == meta[name], name
    assert issubclass(bg.HarmonicParticles, bg.RepulsiveParticles) and issubclass(bg.RepulsiveParticles, bg.Energy)


def test_default_constructor_and_reference_attribute_names():
    rep = bg.RepulsiveParticles()                       # (a TypeError in the reference)
    assert rep.params is bg.RepulsiveParticles.params_default and rep.nparticles == 38 and rep.dim == 76
    assert list(rep.event_shape) == [76]
    assert rep.rm == 1.1 and rep.rm12 == 1.1 ** 12
    assert rep.a_surrogate == 21.0 * 1.1 ** 6 / 0.9 ** 8 and rep.b_surrogate == 6.0 * 1.1 ** 6 / 0.9 ** 7 and rep.c_surrogate == 1.1 ** 6 / 0.9 ** 6
    assert rep.mask_matrix.dtype == np.float32 and rep.mask_matrix.shape == (38, 38)
    want = np.ones((38, 38), dtype=np.float32) - np.eye(38, dtype=np.float32)
    want[0, 1] = want[1, 0] = 0.0
    assert np.array_equal(rep.mask_matrix, want) and np.array_equal(rep.mask_matrix_torch.numpy(), want)
    harm = bg.HarmonicParticles()
    assert harm.spring_constant == 200.0 and harm.nparticles == 38
    assert bg.HarmonicParticles(150.0, {**rep.params_default, "nsolvent": 2}).dim == 8
    for name in ("dimer_distance", "LJ_energy_torch", "LJ_energy_surrogate_torch", "LJ_force_torch", "dimer_energy_torch", "dimer_force_torch",
                 "box_energy_torch", "box_force_torch", "_energy", "surrogate_energy", "force"):
        assert callable(getattr(rep, name)), name
    assert callable(harm.harmonic_energy_torch)
    for name in ("forward", "hamiltonian", "surrogate_hamiltonian", "force_autograd", "plot_dimer_energy"):
        assert name not in vars(bg.RepulsiveParticles) and name not in vars(bg.HarmonicParticles), name
    x = torch.tensor([[0.0, 0.0, 3.0, 4.0, 1.0, 1.0, 2.0, 2.0]])
    assert float(bg.RepulsiveParticles({**rep.params_default, "nsolvent": 2}).dimer_distance(x)) == 5.0
    assert float(bg.RepulsiveParticles({**rep.params_default, "nsolvent": 2}).dimer_distance(x.numpy())[0]) == 5.0


def energy_and_grad(energy, x):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x)
    assert u.shape == (x.shape[0], 1) and u.dtype == x.dtype
    (g,) = torch.autograd.grad(u.sum(), x)
    return u.detach().numpy().reshape(-1), g.numpy()


@pytest.mark.parametrize("ns", NSOLVENT)
@pytest.mark.parametrize("kind", KINDS)
def test_torch_formulas_reproduce_the_reference(golden, kind, ns):
    G = golden("box")
    key = f"{kind}_{ns}"
    energy = make(G, kind, ns)
    x = torch.tensor(G[f"x_{ns}"])
    assert x.shape == (B, 2 * (ns + 2))
    rows = G[key + "_g_rows"]
    # f64: the recorded values to 1e-10
    u, g = energy_and_grad(energy, x.double())
    assert err_u(u, G[key + "_u64"]) <= 1e-10 and err_g(g[rows], G[key + "_g64"]) <= 1e-10
    assert np.isfinite(g).all()
    force = energy.force(x.double()).numpy()
    assert force.shape == g.shape and err_g(-force, g) <= 1e-10
    if key + "_force64" in G:
        assert err_g(force[rows], G[key + "_force64"]) <= 1e-10
    if kind == "rep":
        s = energy.surrogate_energy(x.double())
        assert s.shape == (B,) and err_u(s.numpy(), G[key + "_surrogate64"]) <= 1e-10
        parts = energy.LJ_force_torch(x.double()) + energy.dimer_force_torch(x.double()) + energy.box_force_torch(x.double())
        assert torch.equal(parts, energy.force(x.double()))
    half = energy.energy(x.double(), temperature=2.0)
    assert torch.equal(half, energy.energy(x.double()) / 2)
    # f32: within the reference's own f32 errors
    u, g = energy_and_grad(energy, x)
    assert err_u(u, G[key + "_u64"]) <= 4 * float(G[key + "_err_u32"]) + 1e-6
    assert err_g(g[rows], G[key + "_g64"]) <= 4 * float(G[key + "_err_g32"]) + 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_torch_formulas_at_singular_geometry(golden, kind):
    """samples 0 and 1: two coincident solvent particles; sample 2: the dimer 0.3 apart, which no pair term sees"""
    G = golden("box")
    key = f"edge_{kind}"
    energy = make(G, kind, 2)
    x = torch.tensor(G[key + "_x"])
    u, g = energy_and_grad(energy, x.double())
    u64 = G[key + "_u64"]
    fin = np.isfinite(u64)
    assert (np.isfinite(u) == fin).all() and (np.isinf(u[~fin]) & (u[~fin] > 0)).all()
    assert fin[2] and err_u(u[fin], u64[fin]) <= 1e-10
    if kind == "harm":
        assert fin.all() and np.isfinite(g).all() and err_g(g, G[key + "_g64"]) <= 1e-10
        # the harmonic gradient is finite and twice differentiable (the reference's is NaN everywhere)
        xg = x.double().requires_grad_(True)
        (g1,) = torch.autograd.grad(energy.energy(xg).sum(), xg, create_graph=True)
        (g2,) = torch.autograd.grad(g1.pow(2).sum(), xg)
        assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    else:
        assert fin.tolist() == [False, False] + [True] * 6
        assert err_g(g[fin], G[key + "_g64"][fin]) <= 1e-10
    u32, _ = energy_and_grad(energy, x)
    assert (np.isfinite(u32) == np.isfinite(G[key + "_u32"])).all()
    assert err_u(u32[fin], u64[fin]) <= 4 * float(G[key + "_err_u32"]) + 1e-6


def test_the_new_prototypes_are_declared_parsed_and_exported(hip_lib):
    sigs = abi_signatures()
    assert sigs["bgk_pair_energy"][1] == [p, i64, i64, i32, i32, i32, f64, f64, f64, f64, f64, f64, p, p], "no existing prototype changes"
    for name, want in WANT.items():
        assert sigs[name] == (ctypes.c_int, want), name
        assert name in abi_symbols()
        assert list(getattr(hip_lib, name).argtypes) == want
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), name), ctypes.c_void_p).value, f"{name} is not exported"


def test_argument_checks_of_the_new_entries(hip_lib):
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths
    prm = (ctypes.c_float * 12)(0.7, 1.21, 0.9, 0.81, 150.0, -1.0, 25.0, 10.0, 1.5, 20.0, 3.0, 100.0)

    def energy(x=fake, batch=8, n=4, kind=3, params=prm, n_params=12, temperature=1.0, u=fake):
        return hip_lib.bgk_box_energy(x, 2 * n, batch, n, kind, params, n_params, temperature, u, None)

    def sums(x=fake, batch=8, n=4, kind=3, params=prm, n_params=12, temperature=1.0, u=fake, dlogp=fake, partial=fake, out=fake):
        return hip_lib.bgk_box_energy_kl_sums(x, 2 * n, batch, n, kind, params, n_params, temperature, u, dlogp, 0, partial, 4, out, None)

    def backward(x=fake, batch=8, n=4, kind=3, params=prm, n_params=12, temperature=1.0, g_u=fake, g_x=fake):
        return hip_lib.bgk_box_energy_backward(x, 2 * n, batch, n, kind, params, n_params, temperature, g_u, None, None, None, 0, None, g_x,
                                               2 * n, None)

    def mcmc(x=fake, batch=8, n=4, kind=3, params=prm, n_params=12, temperature=1.0, e=fake, std=0.1, steps=2, noise=None, unif=None,
             traj=None, traj_e=None, every=0):
        return hip_lib.bgk_box_mcmc(x, batch, n, kind, params, n_params, e, 0, temperature, None, std, steps, noise, unif, 1, 0, 0, traj,
                                    traj_e, every, None, 0, None)

    for call in (energy, sums, backward, mcmc):
        if call is not sums:                                        # (an empty batch zeroes the loss sums: device work)
            assert call(batch=0) == 0
        for n in (1, 65):
            assert call(n=n) == -2 and b"envelope" in hip_lib.bgk_last_error()
        assert call(batch=-1) == -1
        for kind in (0, 1, 2, 5, -1):                               # the kinds of bgk_pair_energy are not served here
            assert call(kind=kind) == -1
        assert call(params=None) == -1 and call(n_params=11) == -1 and call(n_params=5) == -1
        assert call(x=None) == -1
    assert energy(temperature=0.0) == -1 and energy(u=None) == -1
    assert sums(out=None) == -1 and sums(dlogp=None) == -1
    assert backward(g_u=None) == -1 and backward(g_x=None) == -1    # neither g_u nor the loss form
    assert mcmc(std=-1.0) == -1 and mcmc(noise=fake) == -1 and mcmc(traj_e=fake) == -1 and mcmc(traj=fake, every=0) == -1
    assert mcmc(temperature=0.0) == -1 and mcmc(e=None) == -1
    # ... and the new kinds are not reachable through the old entries
    for kind in (3, 4):
        assert hip_lib.bgk_pair_energy(None, 8, 8, 4, 2, kind, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None) == -1
        assert hip_lib.bgk_pair_mcmc(fake, 8, 4, 2, kind, 1.0, 1.0, 0.0, 0.0, 0.0, fake, 0, 1.0, None, 0.1, 2, None, None, 1, 0, 0, None, None,
                                     0, None, 0, None) == -1


def test_plan_type():
    """a BoxPlan of its own: not a PairPlan (the Langevin / Hessian-vector kernels' licence), not of a field plan's length"""
    rep, harm = bg.RepulsiveParticles(), bg.HarmonicParticles(150.0)
    plan = _kernel_plan(rep, 1.5)
    assert isinstance(plan, BoxPlan) and not isinstance(plan, PairPlan) and len(plan) not in (5, 6, 9)
    assert (plan.kind, plan.n_particles, plan.n_dims, plan.temperature) == (3, 38, 2, 1.5)
    assert plan.params == (1.0, 1.1 ** 2, 0.9, 0.9 ** 2, 0.0, -1.0, 25.0, 10.0, 1.5, 20.0, 3.0, 100.0)
    hp = _kernel_plan(harm, 1.0)
    assert isinstance(hp, BoxPlan) and hp.kind == 4 and hp.params[4] == 150.0 and hp.params[:4] == plan.params[:4]
    big = {**rep.params_default, "nsolvent": 63}
    assert _kernel_plan(bg.RepulsiveParticles(big), 1.0) is None and _kernel_plan(bg.HarmonicParticles(params=big), 1.0) is None
    assert _kernel_plan(bg.RepulsiveParticles({**big, "nsolvent": 62}), 1.0).n_particles == 64
    assert _kernel_plan(rep, torch.tensor(2.0)) is None

    class Shifted(bg.RepulsiveParticles):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    assert _kernel_plan(Shifted(), 1.0) is None
    assert _kernel_plan(bg.LinLogCutEnergy(rep), 1.0) is None
    assert _kernel_plan(bg.ProductDistribution([rep, bg.NormalDistribution(5)]), 1.0) is None
    # CPU tensors never reach the kernel; neither do the stochastic layers' fused paths or the fused chain setup
    x = torch.zeros(4, 76)
    assert kernel_energy(rep, (x,), 1.0) is None and kl_loss_sums(rep, (x,), torch.zeros(4, 1)) is None
    assert bg.MCMCStep(rep)._fused_setup(bg.SamplerState(samples=x)) is None
    for flow in (bg.BrownianFlow(rep), bg.LangevinFlow(rep), bg.MetropolisMCFlow(rep)):
        assert flow._fused_setup(x) is None


def test_stochastic_layers_take_their_torch_paths(golden):
    G = golden("box")
    rep = make(G, "rep", 2)
    x = torch.tensor(G["x_2"])[:16]
    torch.manual_seed(3)
    y, dW = bg.BrownianFlow(rep, nsteps=3, stepsize=1e-4)(x)
    assert y.shape == x.shape and dW.shape == (16, 1) and torch.isfinite(y).all() and torch.isfinite(dW).all()
    y, dW = bg.MetropolisMCFlow(rep, nsteps=3, stepsize=0.02)(x)
    assert y.shape == x.shape and dW.shape == (16, 1) and torch.isfinite(y).all() and torch.isfinite(dW).all()
    q, v, dW = bg.LangevinFlow(rep, nsteps=3, stepsize=1e-3)(x, torch.randn_like(x))
    assert q.shape == x.shape and v.shape == x.shape and dW.shape == (16, 1)
    assert torch.isfinite(q).all() and torch.isfinite(v).all() and torch.isfinite(dW).all()
    # ... and a graph goes through them (the torch formulas are twice differentiable)
    xg = x.clone().requires_grad_(True)
    y, dW = bg.BrownianFlow(make(G, "harm", 2), nsteps=2, stepsize=1e-4)(xg)
    (g,) = torch.autograd.grad(y.sum() + dW.sum(), xg)
    assert torch.isfinite(g).all()
