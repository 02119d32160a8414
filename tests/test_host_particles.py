"""Host (no GPU): the particle-system classes -- names, signatures and event shapes against the reference's recorded metadata, the torch
``_energy`` formulas against its f64 energies (tests/golden/particles.npz), the C ABI of csrc/bgk_pair.hip as the header declares it,
and the plan kinds of ``distributions._kernel_plan``."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd._abi import abi_signatures
from bgflow_amd.distributions import PairPlan, _kernel_plan, kernel_energy, kl_loss_sums

SHAPES = [(2, 1), (4, 2), (13, 3), (55, 3), (64, 3)]
KINDS = ["lj", "ljn", "mdw", "mfn"]
SYMBOLS = ("bgk_pair_energy", "bgk_pair_energy_backward", "bgk_pair_energy_kl_sums")


def make(G, kind, n, d, two_event_dims=True):
    if kind in ("lj", "ljn"):
        eps, rm, osc = (float(v) for v in G["lj_params"])
        return bg.LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=kind == "lj", oscillator_scale=osc, two_event_dims=two_event_dims)
    if kind == "mdw":
        a, b, c, off = (float(v) for v in G["mdw_params"])
        return bg.MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=two_event_dims)
    return bg.MeanFreeNormalDistribution(n * d, n, std=float(G["mfn_std"]), two_event_dims=two_event_dims)


def test_classes_are_exported_with_the_references_signatures(golden):
    import bgflow_amd.distribution.energy.lennard_jones as lj_mod
    import bgflow_amd.distribution.energy.multi_double_well_potential as mdw_mod
    import bgflow_amd.distribution.normal as normal_mod
    assert lj_mod.LennardJonesPotential is bg.LennardJonesPotential
    assert mdw_mod.MultiDoubleWellPotential is bg.MultiDoubleWellPotential
    assert normal_mod.MeanFreeNormalDistribution is bg.MeanFreeNormalDistribution and normal_mod.NormalDistribution is bg.NormalDistribution
    meta = json.loads(str(golden("particles")["meta"]))
    assert set(meta) == {"LennardJonesPotential", "MultiDoubleWellPotential", "MeanFreeNormalDistribution"}
    for name, m in meta.items():
        cls = getattr(bg, name)
        params = list(inspect.signature(cls.__init__).parameters.values())[1:]
        assert [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in params] == m["parameters"], name
        kw = dict(a=1.0, b=1.0, c=1.0, offset=1.0) if name == "MultiDoubleWellPotential" else {}
        assert list(cls(12, 4, **kw).event_shape) == m["event_shape_two_dims"] == [4, 3]
        assert list(cls(12, 4, two_event_dims=False, **kw).event_shape) == m["event_shape_one_dim"] == [12]


def test_reference_attribute_names():
    lj = bg.LennardJonesPotential(39, 13, eps=0.7, rm=1.3, oscillator=False, oscillator_scale=0.5)
    assert (lj._n_particles, lj._n_dims, lj._eps, lj._rm, lj.oscillator, lj._oscillator_scale) == (13, 3, 0.7, 1.3, False, 0.5)
    mdw = bg.MultiDoubleWellPotential(8, 4, 0.9, -4, 0.1, 4)
    assert (mdw._dim, mdw._n_particles, mdw._n_dimensions, mdw._a, mdw._b, mdw._c, mdw._offset) == (8, 4, 2, 0.9, -4, 0.1, 4)
    mfn = bg.MeanFreeNormalDistribution(8, 4, std=0.8, two_event_dims=False)
    assert (mfn._dim, mfn._n_particles, mfn._spacial_dims, mfn._two_event_dims) == (8, 4, 2, False)
    assert "_std" in dict(mfn.named_buffers()) and mfn._std.dtype == torch.float32
    torch.manual_seed(0)
    s = mfn.sample(1000)
    assert s.shape == (1000, 8) and float(s.view(-1, 4, 2).mean(1).abs().max()) < 1e-6
    assert abs(float(s.std()) - 0.8 * (3 / 4) ** 0.5) < 0.03            # the centroid takes one of four degrees of freedom per axis
    assert bg.MeanFreeNormalDistribution(8, 4).sample(5).shape == (5, 4, 2)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_torch_formulas_reproduce_the_reference_in_f64(golden, kind, n, d):
    G = golden("particles")
    x = torch.tensor(G[f"x_{n}_{d}"]).double()
    u64 = G[f"{kind}_{n}_{d}_u64"]
    for two in (True, False):
        energy = make(G, kind, n, d, two)
        u = energy.energy(x if two else x.reshape(-1, n * d))
        assert u.dtype == torch.float64 and u.shape == (x.shape[0], 1)
        assert float(np.max(np.abs(u.numpy().reshape(-1) - u64) / (1.0 + np.abs(u64)))) <= 1e-12
    half = energy.energy(x.reshape(-1, n * d), temperature=2.0)
    assert torch.equal(half, u / 2)


@pytest.mark.parametrize("kind", ["lj", "mdw"])
def test_torch_formulas_with_coincident_particles(golden, kind):
    """f32 on the CPU: the finite / non-finite pattern of the reference's energies; the double-well gradient is finite (0 from the
    coincident pair, as through cdist) and matches the recorded one"""
    G = golden("particles")
    x = torch.tensor(G[f"edge_{kind}_x"]).requires_grad_(True)
    u = make(G, kind, 4, 3).energy(x)
    (g,) = torch.autograd.grad(u.sum(), x)
    assert (np.isfinite(u.detach().numpy().reshape(-1)) == np.isfinite(G[f"edge_{kind}_u32"])).all()
    if kind == "mdw":
        assert torch.isfinite(g).all()
        np.testing.assert_allclose(g.numpy().reshape(8, -1), G["edge_mdw_g64"], rtol=1e-4, atol=1e-4)


def test_c_abi_of_the_pair_kernels(hip_lib):
    sigs = abi_signatures()
    f, d, i32, i64, p = ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    head = [p, i64, i64, i32, i32, i32, d, d, d, d, d, d]
    assert sigs["bgk_pair_energy"] == (ctypes.c_int, head + [p, p])
    assert sigs["bgk_pair_energy_kl_sums"] == (ctypes.c_int, head + [p, p, i32, p, i32, p, p])
    assert sigs["bgk_pair_energy_backward"] == (ctypes.c_int, head + [p, p, p, p, i32, p, p, i64, p])
    assert f is ctypes.c_float
    for name in SYMBOLS:
        assert list(getattr(hip_lib, name).argtypes) == sigs[name][1]
    # argument checks that return before any device work: an empty batch, the envelope, a bad kind
    args = (None, 6, 0, 2, 3, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    assert hip_lib.bgk_pair_energy(*args, None, None) == 0
    assert hip_lib.bgk_pair_energy_backward(*args, None, None, None, None, 0, None, None, 6, None) == -1      # neither g_u nor the loss form
    for n, dims in ((65, 3), (1, 3), (4, 4), (4, 0)):
        assert hip_lib.bgk_pair_energy(None, n * dims, 8, n, dims, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None) == -2
        assert b"envelope" in hip_lib.bgk_last_error()
    assert hip_lib.bgk_pair_energy(None, 6, 8, 2, 3, 3, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None) == -1
    assert hip_lib.bgk_pair_energy(None, 6, 8, 2, 3, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, None, None) == -1          # temperature 0
    assert hip_lib.bgk_pair_energy(None, 6, 8, 2, 3, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None) == -1          # null tensors
    assert hip_lib.bgk_pair_energy_kl_sums(None, 6, 8, 2, 3, 0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, None, None, 0, None, 4, None, None) == -1


def test_plan_kinds():
    """field plans are what they were; a particle system gives a PairPlan, which the callers that fold FIELD plans pass by"""
    log_z = float(5 / 2 * np.log(2 * np.pi * 1.0))
    assert _kernel_plan(bg.NormalDistribution(5), 1.0) == ([(0, None, (0.0, 0.0, 0.0), 0.0)], [5], 0.0, log_z, 1.0)
    assert _kernel_plan(bg.DoubleWellEnergy(6, a=1.0, b=-4.0, c=1.0), 2.0) == ([(1, None, (1.0, -4.0, 1.0), 0.0)], [6], 0.0, 0.0, 2.0)
    lj = bg.LennardJonesPotential(39, 13, eps=0.7, rm=1.3, oscillator_scale=0.5)
    assert _kernel_plan(lj, 1.5) == PairPlan(0, 13, 3, 0.7, 1.3, 0.0, 0.0, 0.5, 1.5)
    assert _kernel_plan(bg.LennardJonesPotential(39, 13, oscillator=False), 1.0).osc_scale == 0.0
    assert _kernel_plan(bg.MultiDoubleWellPotential(8, 4, 0.9, -4, 0.1, 4), 1.0) == PairPlan(1, 4, 2, 0.9, -4.0, 0.1, 4.0, 0.0, 1.0)
    mfn = _kernel_plan(bg.MeanFreeNormalDistribution(8, 4, std=0.8), 1.0)
    assert mfn[:3] == (2, 4, 2) and mfn.osc_scale == 1.0 / float(torch.tensor(0.8) ** 2)
    assert len(_kernel_plan(lj, 1.0)) not in (5, 6)
    # outside the envelope / a tensor-valued temperature / a subclass with its own _energy: the torch formula
    assert _kernel_plan(bg.LennardJonesPotential(195, 65), 1.0) is None
    assert _kernel_plan(bg.LennardJonesPotential(16, 4), 1.0) is None          # four dimensions
    assert _kernel_plan(lj, torch.tensor(2.0)) is None

    class Shifted(bg.LennardJonesPotential):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    assert _kernel_plan(Shifted(39, 13), 1.0) is None
    # the wrappers of clipped.py and a product keep their generic paths around a pair target
    assert _kernel_plan(bg.LinLogCutEnergy(lj), 1.0) is None
    assert _kernel_plan(bg.GradientClippedEnergy(lj, bg.ClipGradient(1.0, 3)), 1.0) is None
    assert _kernel_plan(bg.ProductDistribution([lj, bg.NormalDistribution(5)]), 1.0) is None
    # CPU tensors never reach the kernel
    x = torch.zeros(4, 13, 3)
    assert kernel_energy(lj, (x,), 1.0) is None and kl_loss_sums(lj, (x,), torch.zeros(4, 1)) is None
    cut = bg.LinLogCutEnergy(bg.MultiDoubleWellPotential(8, 4, 0.9, -4, 0.1, 4), 5.0, 8.0)
    xs = torch.randn(6, 4, 2, generator=torch.Generator().manual_seed(1)) * 3
    torch.testing.assert_close(cut.energy(xs, temperature=2.0), bg.linlogcut(cut.delegate._energy(xs), 5.0, 8.0) / 2.0)
