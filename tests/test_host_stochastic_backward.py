"""No GPU: what the fused backward of the stochastic layers (csrc/bgk_langevin.hip, bgk_pair_energy_hvp) shows without a device -- its
three prototypes in the header, in ``abi_signatures`` and in the built library with their argument checks, the fixture
tests/golden/stochastic_grad.npz (keys, shapes, finiteness), the opt-in switch and the unchanged constructor signatures."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib, stochastic
from bgflow_amd._abi import abi_signatures
from bgflow_amd.build import abi_symbols

from stochastic_backward_common import HVP_CASES, LAYER_CASES, grad_key, vectors
from stochastic_common import B

f64, i32, i64, u32, u64, p = ctypes.c_double, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
PLAN = [i64, i32, i32, i32, f64, f64, f64, f64, f64]
RUN = [f64, f64, f64, f64, i32, p, p, u64, u32, i64]
WANT = {
    "bgk_pair_energy_hvp": [p, i64] + PLAN + [f64, p, p, p, p],
    "bgk_pair_langevin_record": [p, p] + PLAN + RUN + [p, i32, p, p, p],
    "bgk_pair_langevin_backward": [p, p, p, p] + PLAN + RUN + [p, p, p, p, i32, p],
}


def test_the_new_prototypes_are_declared_parsed_and_exported(hip_lib):
    sigs = abi_signatures()
    assert sigs["bgk_pair_langevin"][1] == [p, p] + PLAN + RUN + [p, i32, p], "no existing prototype changes"
    for name, want in WANT.items():
        assert sigs[name] == (ctypes.c_int, want), name
        assert name in abi_symbols()
        assert list(getattr(hip_lib, name).argtypes) == want
        assert ctypes.cast(getattr(ctypes.CDLL(_lib.LIB_PATH), name), ctypes.c_void_p).value, f"{name} is not exported"


def test_argument_checks_of_the_new_entries(hip_lib):
    fake = ctypes.c_void_p(64)              # never dereferenced on these paths

    def record(q=fake, v=None, batch=8, n=4, h=0.01, steps=2, w1=None, w2=None, dW=fake, tq=fake, tv=None):
        return hip_lib.bgk_pair_langevin_record(q, v, batch, n, 2, 1, 0.9, -4.0, 0.1, 4.0, 0.0, h, 1.0, 1.0, 1.0, steps, w1, w2, 1, 0, 0, dW, 0,
                                                tq, tv, None)

    def backward(q0=fake, v0=None, tq=fake, tv=None, batch=8, n=4, h=0.01, steps=2, w1=None, w2=None, g=fake, gq=fake, gv=None, carry=fake):
        return hip_lib.bgk_pair_langevin_backward(q0, v0, tq, tv, batch, n, 2, 1, 0.9, -4.0, 0.1, 4.0, 0.0, h, 1.0, 1.0, 1.0, steps, w1, w2, 1,
                                                  0, 0, g, gq, gv, carry, 1, None)

    def hvp(x=fake, u=fake, hu=fake, batch=8, n=4, temperature=1.0):
        return hip_lib.bgk_pair_energy_hvp(x, 8, batch, n, 2, 1, 0.9, -4.0, 0.1, 4.0, 0.0, temperature, u, None, hu, None)

    for call in (record, backward, hvp):
        assert call(batch=0) == 0                                  # an empty batch
        assert call(n=65) == -2 and b"envelope" in hip_lib.bgk_last_error()
        assert call(batch=-1) == -1
    assert record(tq=None) == -1 and record(tv=fake) == -1 and record(v=fake) == -1          # traj_v exactly with velocities
    assert record(h=0.0) == -1 and record(v=fake, tv=fake, w1=fake) == -1
    assert backward(q0=None) == -1 and backward(g=None) == -1 and backward(gq=None) == -1 and backward(carry=None) == -1
    assert backward(tq=None) == -1 and backward(v0=fake) == -1 and backward(gv=fake) == -1 and backward(tv=fake) == -1
    assert backward(h=float("nan")) == -1 and backward(w1=fake, w2=fake) == -1
    assert hvp(x=None) == -1 and hvp(u=None) == -1 and hvp(hu=None) == -1 and hvp(temperature=0.0) == -1


def test_the_fixture(golden):
    G = golden("stochastic_grad")
    for kind, n, d in HVP_CASES:
        key = f"hvp_{kind}_{n}_{d}_"
        rows = G[key + "rows"]
        assert vectors(G, n, d).shape == (B, n * d)                # (checks the recorded sum of u)
        for name in ("g", "hu"):
            a = G[key + name + "64"]
            assert a.dtype == np.float64 and a.shape == (len(rows), n * d) and np.isfinite(a).all()
            err = float(G[key + f"err_{name}32"])
            assert np.isfinite(err) and 0.0 <= err <= 1e-3 * (1 + np.abs(a).max())
        if kind == "mfn":
            assert np.abs(G[key + "hu64"]).max() > 0
    for layer, kind, n, d, nsteps, tag in LAYER_CASES:
        key = grad_key(layer, kind, n, d, nsteps, tag)
        rows = G[key + "rows"]
        assert float(G[key + "stepsize"]) > 0 and G[key + "params"].shape == (3,)
        for name in ("g", "gv") if layer == "langevin" else ("g",):
            a = G[key + name + "64"]
            assert a.dtype == np.float64 and a.shape == (len(rows), n * d) and np.isfinite(a).all()
            err = float(G[key + f"err_{name}32"])
            assert np.isfinite(err) and 0.0 <= err <= 1e-3 * (1 + np.abs(a).max())
        assert (key + "gv64" in G.files) == (layer == "langevin")
    assert np.array_equal(G[grad_key("langevin", "lj", 13, 3, 12, "_p") + "params"], G["params_p"])
    assert np.array_equal(G[grad_key("langevin", "lj", 13, 3, 12) + "params"], np.ones(3))


def test_the_fused_backward_is_opt_in_and_leaves_the_signatures_alone(golden):
    meta = json.loads(str(golden("stochastic")["meta"]))
    for name in ("BrownianFlow", "LangevinFlow", "MetropolisMCFlow"):
        cls = getattr(bg, name)
        got = [[q.name, "<required>" if q.default is inspect.Parameter.empty else q.default]
               for q in inspect.signature(cls.__init__).parameters.values() if q.name != "self"]
        assert got == meta[name], name
        assert cls.fused_backward is False and cls.fused is True
    assert stochastic.LANGEVIN_BACKWARD_MAX_BYTES == 2 ** 30 and stochastic.LANGEVIN_BACKWARD_MAX_STEPS_PER_LAUNCH >= 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_no_fused_training_path_for_cpu_and_f64_inputs(dtype):
    energy = bg.MultiDoubleWellPotential(8, 4, 0.9, -4.0, 0.1, 4.0, two_event_dims=False)
    x = (4.0 * torch.randn(5, 8, dtype=dtype)).requires_grad_(True)
    for flow, xs in ((bg.BrownianFlow(energy, nsteps=2, stepsize=1e-3), (x,)), (bg.LangevinFlow(energy, nsteps=2, stepsize=1e-3), (x, x)),
                     (bg.MetropolisMCFlow(energy, nsteps=2, stepsize=0.1), (x,))):
        flow.fused_backward = True
        assert flow._fused_train_setup(*xs) is None and flow._fused_setup(*xs) is None
        *ys, dW = flow(*xs)                                        # the general path, differentiable as before
        assert dW.dtype == dtype and "Fn" not in type(ys[0].grad_fn).__name__
        (g,) = torch.autograd.grad(dW.sum() + ys[0].sum(), x)
        assert g.shape == x.shape and bool(torch.isfinite(g).all())
