"""CPU: the robust-training wrappers (bgflow_amd/clipped.py: linlogcut, ClipGradient, LinLogCutEnergy, GradientClippedEnergy) on their
torch path against tests/golden/g_clipped.npz, which tests/golden/make_clip_goldens.py wrote by running the unmodified reference;
the kernel plan of the wrapper chains; argument validation of the new entry points (before any launch: no GPU).  Every test here
fails before this feature: the names do not exist."""
import ctypes
import importlib
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd.distributions import _kernel_plan

RTOL = 1e-6          # f32 rounding: same operations as the reference, at most reordered by a vectorised sum


def T(a):
    return torch.as_tensor(np.asarray(a))


def close(t, ref, rtol=RTOL):
    a = t.detach().cpu().numpy()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    np.testing.assert_allclose(a, ref, rtol=rtol, atol=0, equal_nan=True)


def chains(G):
    """name -> energy, as make_clip_goldens.py builds them"""
    normal, well = bg.NormalDistribution(66), bg.DoubleWellEnergy(64)
    cn = lambda: bg.ClipGradient(float(G["n_clip"]), int(G["n_norm_dim"]))       # noqa: E731
    cd = lambda: bg.ClipGradient(float(G["dw_clip"]), int(G["dw_norm_dim"]))     # noqa: E731
    return {
        "n66_cut_clip": (bg.LinLogCutEnergy(bg.GradientClippedEnergy(normal, cn()), 5.0, 8.0), "n66_x"),
        "n66_clip_cut": (bg.GradientClippedEnergy(bg.LinLogCutEnergy(normal, 5.0, 8.0), cn()), "n66_x"),
        "n66h_cut_clip": (bg.LinLogCutEnergy(bg.GradientClippedEnergy(normal, cn()), 70.0, 75.0), "n66_x"),
        "n66h_clip_cut": (bg.GradientClippedEnergy(bg.LinLogCutEnergy(normal, 70.0, 75.0), cn()), "n66_x"),
        "dw64_cut": (bg.LinLogCutEnergy(well, 5.0, 8.0), "dw64_x"),
        "dw64_clip": (bg.GradientClippedEnergy(well, cd()), "dw64_x"),
    }


def test_linlogcut_matches_the_reference(golden):
    G = golden("g_clipped")
    for tag, kw in (("58", dict(high_val=5.0, max_val=8.0)), ("def", {})):
        x = T(G["cut_vals"]).clone().requires_grad_(True)
        y = bg.linlogcut(x, **kw)
        (g,) = torch.autograd.grad(y.sum(), x)
        close(y, G[f"cut_{tag}_out"])
        close(g, G[f"cut_{tag}_grad"])
    # all three branches occur in the recorded data
    g58 = G["cut_58_grad"]
    assert (g58 == 1).any() and (g58 == 0).any() and ((g58 > 0) & (g58 < 1)).any()


@pytest.mark.parametrize("width", [66, 6])
def test_clip_tensor_matches_the_reference(golden, width):
    G = golden("g_clipped")
    g = T(G[f"clip{width}_in"])
    clip = T(G["clip_value"])
    for nd in (1, 3):
        close(bg.ClipGradient.clip_tensor(g, clip, nd), G[f"clip{width}_n{nd}"])
    close(bg.ClipGradient.clip_tensor(g, clip, -1), G[f"clip{width}_m1"])
    close(bg.ClipGradient.clip_tensor(g[:10], clip, -1), G[f"clip{width}_m1f"])
    close(bg.ClipGradient.clip_tensor(g, 1.0, 3), G[f"clip{width}_n3"])           # a python scalar is accepted as well
    # what the reference does with +-inf (recorded, not assumed): by value -> +-clip (to an ulp), in a group of 3 the whole group -> 0,
    # in the whole-tensor norm everything -> 0
    n1, n3 = G[f"clip{width}_n1"], G[f"clip{width}_n3"]
    assert abs(n1[10, 2] - 1) < 1e-6 and abs(n1[10, width - 2] + 1) < 1e-6 and abs(n1[11, 0] + 1) < 1e-6 and n1[11, 3] == 0
    assert not n3[10, 0:3].any() and not n3[11, 0:3].any() and not G[f"clip{width}_m1"].any()


def test_clip_gradient_limits_are_value_errors():
    g = torch.randn(4, 6)
    with pytest.raises(ValueError, match="tensor-valued"):
        bg.ClipGradient.clip_tensor(g, torch.ones(2), 3)
    with pytest.raises(ValueError, match="divide the row width"):
        bg.ClipGradient.clip_tensor(g, torch.tensor(1.0), 4)       # 4 divides 24 elements but not the row of 6: groups would straddle rows
    with pytest.raises(ValueError, match="divide the row width"):
        bg.ClipGradient.clip_tensor(g, 1.0, 0)


def test_clip_gradient_module_state_and_hooks():
    c = bg.ClipGradient(0.25, norm_dim=3)
    assert list(c.state_dict()) == ["clip"] and c.norm_dim == 3 and c._clip_host == 0.25
    c.load_state_dict({"clip": torch.tensor(0.5)})
    assert c._clip_host == 0.5 and float(c.clip) == 0.5           # the host copy follows load_state_dict ...
    c = c.double()
    assert c.clip.dtype == torch.float64 and c._clip_host == 0.5   # ... and _apply
    x, y = torch.full((2, 6), 3.0, requires_grad=True), torch.zeros(2, 3)
    a, b = c(x, y)                      # hooks on the tensors that require a gradient; returned unpacked
    assert a is x and b is y and c(x) is x
    (a * 2.0).sum().backward()
    assert torch.allclose(x.grad, torch.full((2, 6), 0.5 / 3 ** 0.5))
    ref = importlib.import_module("bgflow_amd.utils.train")
    assert ref.ClipGradient is bg.ClipGradient and ref.linlogcut is bg.linlogcut
    ref = importlib.import_module("bgflow_amd.distribution.energy.clipped")
    assert ref.LinLogCutEnergy is bg.LinLogCutEnergy and ref.GradientClippedEnergy is bg.GradientClippedEnergy
    from bgflow_amd.distribution.energy.clipped import GradientClippedEnergy, LinLogCutEnergy      # noqa: F401
    from bgflow_amd.utils.train import ClipGradient, linlogcut                                       # noqa: F401
    e = bg.GradientClippedEnergy(bg.LinLogCutEnergy(bg.NormalDistribution(6), 2.0, max_energy=3.0), bg.ClipGradient(1.0))
    assert sorted(e.state_dict()) == ["clipping.clip", "delegate.delegate._mean"]
    assert e.clipping.norm_dim == 1 and e.delegate.high_energy == 2.0 and e.delegate.max_energy == 3.0 and e.event_shapes == [torch.Size([6])]


def test_wrapped_energies_match_the_reference(golden):
    G = golden("g_clipped")
    for name, (energy, xkey) in chains(G).items():
        for t in G["temperatures"]:
            x = T(G[xkey]).clone().requires_grad_(True)
            u = energy.energy(x, temperature=float(t))
            (g,) = torch.autograd.grad(u.sum(), x)
            close(u, G[f"{name}_T{t}_u"])
            # gradients: rtol on the group norm turns into an absolute bound of the same relative size on the elements of a clipped group
            np.testing.assert_allclose(g.numpy(), G[f"{name}_T{t}_g"], rtol=RTOL, atol=RTOL * float(np.abs(G[f"{name}_T{t}_g"]).max()))
    # the temperature divides the CUT energy of the delegate at T = 1
    e, x = bg.LinLogCutEnergy(bg.NormalDistribution(66), 70.0, 75.0), T(G["n66_x"])
    assert torch.equal(e.energy(x, temperature=1.7), bg.linlogcut(bg.NormalDistribution(66).energy(x), 70.0, 75.0) / 1.7)


def test_kernel_plan_of_the_wrapper_chains():
    normal, well = bg.NormalDistribution(66), bg.DoubleWellEnergy(64)
    clip = bg.ClipGradient(0.05, 3)
    p = _kernel_plan(bg.LinLogCutEnergy(bg.GradientClippedEnergy(normal, clip), 5.0, 8.0), 1.7)
    q = _kernel_plan(bg.GradientClippedEnergy(bg.LinLogCutEnergy(normal, 5.0, 8.0), clip), 1.7)
    assert p is not None and p == q and len(p) == 6
    specs, dims, c_in, c_out, t_eff, (cut, cl) = p
    # the delegate is evaluated at T = 1: its log Z (d / 2 log 2 pi, NOT of T = 1.7) sits inside the cut and the division
    assert dims == [66] and abs(c_in - 33 * np.log(2 * np.pi)) < 1e-12 and c_out == 0.0 and t_eff == 1.7
    assert cut == (5.0, 8.0) and cl == (float(np.float32(0.05)), 3)
    assert _kernel_plan(bg.LinLogCutEnergy(well), 1.0)[5] == ((1e3, 1e9), None)
    assert _kernel_plan(bg.GradientClippedEnergy(well, bg.ClipGradient(1e-4, 1)), 1.0)[5] == (None, (float(np.float32(1e-4)), 1))
    assert _kernel_plan(bg.GradientClippedEnergy(well, bg.ClipGradient(1.0, -1)), 1.0) is not None
    prod = bg.ProductDistribution([bg.NormalDistribution(6), bg.UniformDistribution(torch.zeros(3), torch.ones(3))])
    assert len(_kernel_plan(bg.LinLogCutEnergy(bg.GradientClippedEnergy(prod, bg.ClipGradient(1.0, 3))), 2.0)[0]) == 2
    assert len(_kernel_plan(normal, 1.0)) == 5                                     # plain distributions: unchanged

    # through their own code: overrides, longer chains, what the kernels do not cover
    class MyCut(bg.LinLogCutEnergy):
        def _energy(self, *xs, **kwargs):
            return super()._energy(*xs, **kwargs) + 1.0

    class Shifted(bg.NormalDistribution):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    class Custom(bg.Energy):
        def _energy(self, x):
            return x.pow(2).sum(-1, keepdim=True)

    assert _kernel_plan(MyCut(normal), 1.0) is None
    assert _kernel_plan(bg.LinLogCutEnergy(Shifted(66)), 1.0) is None
    assert _kernel_plan(bg.LinLogCutEnergy(Custom(5)), 1.0) is None
    assert _kernel_plan(bg.LinLogCutEnergy(bg.LinLogCutEnergy(normal)), 1.0) is None
    assert _kernel_plan(bg.GradientClippedEnergy(normal, bg.ClipGradient(1.0, 4)), 1.0) is None     # 4 does not divide 66
    assert _kernel_plan(bg.GradientClippedEnergy(normal, bg.ClipGradient(torch.ones(22), 3)), 1.0) is None
    assert _kernel_plan(bg.ProductDistribution([bg.LinLogCutEnergy(normal), normal]), 1.0) is None
    # ... which still evaluates (torch path), e.g. a custom delegate
    e = bg.GradientClippedEnergy(bg.LinLogCutEnergy(Custom(5), 2.0, 3.0), bg.ClipGradient(0.1, 1))
    x = torch.full((3, 5), 0.5, requires_grad=True)
    e.energy(x, temperature=2.0).sum().backward()
    assert torch.allclose(x.grad, torch.full((3, 5), 0.1))


def test_new_entry_points_validate_before_any_launch(hip_lib):
    L = hip_lib
    P1 = ctypes.c_void_p(0x1000)         # a non-null placeholder, never dereferenced on these paths
    err = lambda: L.bgk_last_error().decode(errors="replace")      # noqa: E731
    assert L.bgk_abi_version() == 1
    # bgk_clip_gradient
    assert L.bgk_clip_gradient(None, 66, 0, 66, 1.0, 3, None, 66, None, 0, None) == 0                       # empty batch
    assert L.bgk_clip_gradient(P1, 66, 4, 66, 1.0, 4, P1, 66, None, 0, None) == -1 and "divisor of the row width" in err()
    assert L.bgk_clip_gradient(P1, 66, 4, 66, 1.0, 0, P1, 66, None, 0, None) == -1
    assert L.bgk_clip_gradient(P1, 60, 4, 66, 1.0, 3, P1, 66, None, 0, None) == -1 and "row stride" in err()
    assert L.bgk_clip_gradient(None, 66, 4, 66, 1.0, 3, P1, 66, None, 0, None) == -1
    assert L.bgk_clip_gradient(P1, 66, 4, 66, -1.0, 3, P1, 66, None, 0, None) == -1 and "non-negative" in err()
    assert L.bgk_clip_gradient(P1, 66, 4, 66, float("nan"), 3, P1, 66, None, 0, None) == -1
    assert L.bgk_clip_gradient(P1, 66, 4, 66, 1.0, -1, P1, 66, None, 0, None) == -1 and "workspace" in err()
    assert L.bgk_clip_gradient(P1, 66, -1, 66, 1.0, 3, P1, 66, None, 0, None) == -1
    # bgk_linlogcut
    assert L.bgk_linlogcut(None, None, 0, 5.0, 8.0, None, None) == 0
    assert L.bgk_linlogcut(None, None, 4, 5.0, 8.0, P1, None) == -1 and "null pointer" in err()
    assert L.bgk_linlogcut(P1, None, 4, float("nan"), 8.0, P1, None) == -1
    # the energy entry points with the wrappers folded in
    x = (ctypes.c_void_p * 1)(0x1000)
    ld = (ctypes.c_int64 * 1)(66)
    d = (ctypes.c_int32 * 1)(66)
    k = (ctypes.c_int32 * 1)(0)
    nd = (ctypes.c_int32 * 1)(4)
    f = (x, ld, d, k, None, None, 1)
    assert L.bgk_energy_fields_cut(*f, 0, 1.0, 0.0, 0.0, 1, 5.0, 8.0, None, None, None, 0, None, 0, None, None) == 0   # empty batch
    assert L.bgk_energy_fields_cut(*f, 4, 0.0, 0.0, 0.0, 1, 5.0, 8.0, P1, P1, None, 0, None, 0, None, None) == -1      # temperature
    assert L.bgk_energy_fields_cut(*f, 4, 1.0, 0.0, 0.0, 1, float("nan"), 8.0, P1, P1, None, 0, None, 0, None, None) == -1 and "cut" in err()
    assert L.bgk_energy_fields_cut(*f, 4, 1.0, 0.0, 0.0, 1, 5.0, 8.0, P1, P1, None, 0, None, 0, P1, None) == -1 and "loss sums" in err()
    k[0] = 3
    assert L.bgk_energy_fields_cut(*f, 4, 1.0, 0.0, 0.0, 1, 5.0, 8.0, P1, P1, None, 0, None, 0, None, None) == -1 and "bad kind" in err()
    k[0] = 0
    g = (ctypes.c_void_p * 1)(0x1000)
    b = (*f, 0, 1.0, 1, 5.0, 8.0, None, 1.0, nd, P1, None, None, None, 0, None, g, ld, None)
    assert L.bgk_energy_fields_cut_backward(*b) == 0                                                             # empty batch
    b = (*f, 4, 1.0, 1, 5.0, 8.0, P1, 1.0, nd, P1, None, None, None, 0, None, g, ld, None)
    assert L.bgk_energy_fields_cut_backward(*b) == -1 and "does not divide the width" in err()
    nd[0] = 3
    b = (*f, 4, 1.0, 1, 5.0, 8.0, None, 1.0, nd, P1, None, None, None, 0, None, g, ld, None)
    assert L.bgk_energy_fields_cut_backward(*b) == -1 and "uncut energies" in err()
    b = (*f, 4, 1.0, 0, 0.0, 0.0, None, -2.0, nd, P1, None, None, None, 0, None, g, ld, None)
    assert L.bgk_energy_fields_cut_backward(*b) == -1 and "non-negative" in err()
    b = (*f, 4, 1.0, 0, 0.0, 0.0, None, 1.0, nd, None, None, None, None, 0, None, g, ld, None)
    assert L.bgk_energy_fields_cut_backward(*b) == -1 and "g_scalar" in err()
    # the optimizer entries
    assert L.bgk_grad_norm_flag(None, 0, P1, P1, 8, P1, None) == -1 and "bgk_grad_norm_flag" in err()
    assert L.bgk_grad_norm_flag(P1, 8, P1, None, 8, P1, None) == -1
    assert L.bgk_grad_norm_flag(P1, 8, P1, P1, 0, P1, None) == -1
    assert L.bgk_adam_step_clipped(P1, P1, P1, P1, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, P1, 1.0, None) == 0      # empty bucket
    assert L.bgk_adam_step_clipped(P1, P1, P1, P1, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, None, 1.0, None) == -1 and "sum of squares" in err()
    assert L.bgk_adam_step_clipped(P1, P1, P1, P1, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, P1, -1.0, None) == -1
    assert L.bgk_adam_step_clipped(P1, P1, P1, P1, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, None, P1, 1.0, None) == -1


def test_clip_forces_still_warns_and_names_a_class_that_exists():
    from bgflow_amd.training import KLTrainer

    class Gen(bg.BoltzmannGenerator):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.w = torch.nn.Parameter(torch.tensor([1.0]))

        def kldiv(self, n_samples, temperature=1.0):
            return (self.w ** 2).expand(n_samples, 1)

    g = Gen()
    tr = KLTrainer(g, optim=torch.optim.SGD(g.parameters(), lr=0.1), train_likelihood=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr.train(1, batchsize=4, clip_forces=10.0)
    msg = [str(x.message) for x in w if issubclass(x.category, DeprecationWarning)]
    assert msg and "GradientClippedEnergy" in msg[0]
    assert issubclass(bg.GradientClippedEnergy, bg.Energy) and bg.GradientClippedEnergy.__module__ == "bgflow_amd.clipped"
