"""MixtureDistribution without a GPU: the general path (the reference's formulas in torch ops) on the CPU against
tests/golden/mixture.npz, the reference's sampling under its seeds, construction, state_dict, the compat import path, the C ABI of the
bgk_mixture_* entries and the plan rules (which mixtures describe themselves to the kernel, and that no caller folding field plans
mistakes a MixturePlan for one)."""
import ctypes

import numpy as np
import pytest
import torch

import bgflow_amd as bg
import mixture_common as mc
from bgflow_amd.distributions import MIXTURE_MAX_COMPONENTS, MIXTURE_MAX_WIDTH, MixturePlan, _kernel_plan


@pytest.fixture(scope="module")
def G(golden):
    return golden("mixture")


@pytest.mark.parametrize("K,d", mc.CASES)
def test_inputs_match_the_fixture(G, K, d):
    assert np.allclose(mc.checksum(mc.inputs(K, d)), G[mc.key(K, d) + "check"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("K,d", mc.CASES)
def test_general_path_f64(G, K, d):
    inp, k = mc.inputs(K, d), mc.key(K, d)
    mix = mc.build(bg, K, d, torch.float64)
    res = mc.evaluate(mix, torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["a"]).double())
    assert all(np.isfinite(v).all() for v in res)
    for name, (bulk, far) in mc.split_errors(*res, G, k).items():
        assert bulk <= 1e-12 and far <= 1e-12, (name, bulk, far)
    if K > 2:
        assert res[3][1] == 0.0 and res[4][1] == 0.0


@pytest.mark.parametrize("K,d", mc.CASES)
def test_general_path_f32(G, K, d):
    inp, k = mc.inputs(K, d), mc.key(K, d)
    mix = mc.build(bg, K, d, torch.float32)
    res = mc.evaluate(mix, torch.from_numpy(inp["x"]), torch.from_numpy(inp["a"]))
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in res)
    mc.assert_within(mc.split_errors(*res, G, k), G, k)


@pytest.mark.parametrize("K,d", [(7, 5), (3, 128)])
def test_general_path_at_a_temperature(G, K, d):
    inp, k = mc.inputs(K, d), mc.key(K, d)
    mix = mc.build(bg, K, d, torch.float64)
    res = mc.evaluate(mix, torch.from_numpy(inp["x"]).double(), torch.from_numpy(inp["a"]).double(), temperature=2.5)
    for name, (bulk, far) in mc.split_errors(*res, G, k, temperature=2.5).items():
        assert bulk <= 1e-12 and far <= 1e-12, (name, bulk, far)


def test_energy_divides_by_the_temperature():
    K, d = 7, 5
    mix = mc.build(bg, K, d, torch.float64)
    x = torch.from_numpy(mc.inputs(K, d)["x"]).double()
    assert torch.equal(mix.energy(x, temperature=2.5), mix.energy(x) / 2.5)
    assert torch.equal(mix.energy(x, temperature=torch.tensor(2.5)), mix.energy(x) / 2.5)


def test_second_derivative_of_the_general_path():
    mix = mc.build(bg, 2, 3, torch.float64)
    x = torch.from_numpy(mc.inputs(2, 3)["x"][:8]).double().requires_grad_(True)
    g, = torch.autograd.grad(mix.energy(x).sum(), x, create_graph=True)
    h, = torch.autograd.grad(g.pow(2).sum(), x)
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def test_reference_sample_under_the_same_seeds(G):
    K, d = mc.SAMPLE_CASE
    inp, counts = mc.inputs(K, d), G["sample_counts"]
    owner = np.repeat(np.arange(K), counts)
    assert counts.sum() == mc.SAMPLE_N and counts[1] == 0

    def draw(mix):
        np.random.seed(mc.SAMPLE_SEED)
        torch.manual_seed(mc.SAMPLE_SEED)
        x = mix.sample(mc.SAMPLE_N)
        assert x.shape == (mc.SAMPLE_N, d) and x.dtype == torch.float32
        return x.numpy()

    # (i) with the components' buffers as the reference stores them, loaded through state_dict: the recorded values.  (The reference
    # decomposes `cov` with linalg.eig, which keeps a diagonal's order -- _rot = 1; this package's NormalDistribution sorts it with eigh,
    # so its _rot is a permutation and the SAME normals land in other columns.)
    mix = mc.build(bg, K, d, torch.float32)
    state = mix.state_dict()
    for k in range(1, K, 2):
        state[f"_components.{k}._rot"] = torch.eye(d)
        state[f"_components.{k}._log_diag"] = (torch.from_numpy(inp["var"][k]) + 1e-6).log().unsqueeze(0)
    mix.load_state_dict(state)
    np.testing.assert_allclose(draw(mix), G["sample_x"], rtol=0, atol=1e-6)
    # (ii) as constructed here: the same counts in the same order -- rows of components without `cov` equal the record, rows of the others
    # carry the record's standardised normals in eigh's column order, up to sign
    x = draw(mc.build(bg, K, d, torch.float32))
    plain = owner % 2 == 0
    np.testing.assert_allclose(x[plain], G["sample_x"][plain], rtol=0, atol=1e-6)
    sd = np.sqrt(inp["var"].astype(np.float64) + 1e-6)
    z, z_ref = ((v[~plain] - inp["mean"][owner[~plain]]) / sd[owner[~plain]] for v in (x, G["sample_x"]))
    order = np.argsort(inp["var"][owner[~plain]], axis=1)          # eigh: ascending variances; normal i lands in column order[i]
    assert (~plain).sum() >= 20
    np.testing.assert_allclose(np.abs(np.take_along_axis(z, order, 1)), np.abs(z_ref), rtol=0, atol=1e-5)


def test_sample_with_a_temperature_is_not_implemented():
    mix = mc.build(bg, 2, 3, torch.float32)
    with pytest.raises(NotImplementedError):
        mix.sample(4, temperature=2.0)


def test_constructor_assertions():
    a, b = bg.NormalDistribution(3), bg.NormalDistribution(4)
    with pytest.raises(AssertionError, match="same dimensionality"):
        bg.MixtureDistribution([a, b])
    with pytest.raises(AssertionError, match="shape"):
        bg.MixtureDistribution([a, bg.NormalDistribution(3)], torch.zeros(1, 2))
    with pytest.raises(AssertionError, match="does not match"):
        bg.MixtureDistribution([a, bg.NormalDistribution(3)], torch.zeros(3))


def test_weights_buffer_parameter_and_state_dict():
    fixed = mc.build(bg, 7, 5, torch.float32, trainable_weights=False)
    train = mc.build(bg, 7, 5, torch.float32, trainable_weights=True)
    assert isinstance(fixed._components, torch.nn.ModuleList)
    assert not isinstance(fixed._unnormed_log_weights, torch.nn.Parameter) and "_unnormed_log_weights" in dict(fixed.named_buffers())
    assert isinstance(train._unnormed_log_weights, torch.nn.Parameter) and list(dict(train.named_parameters())) == ["_unnormed_log_weights"]
    assert torch.allclose(fixed._log_weights.exp().sum(), torch.tensor(1.0))
    # a reference-style state_dict: the weights and the components' buffers under the reference's names, nothing else
    state = fixed.state_dict()
    assert set(state) == ({"_unnormed_log_weights"} | {f"_components.{k}._mean" for k in range(7)}
                          | {f"_components.{k}.{n}" for k in (1, 3, 5) for n in ("_log_diag", "_rot")})
    other = bg.MixtureDistribution([bg.NormalDistribution(5, torch.zeros(5), torch.eye(5) if k % 2 else None) for k in range(7)])
    other.load_state_dict(state)
    x = torch.from_numpy(mc.inputs(7, 5)["x"])
    assert torch.equal(other.energy(x), fixed.energy(x))


def test_compat_import_paths():
    from bgflow_amd.distribution.mixture import MixtureDistribution
    assert MixtureDistribution is bg.MixtureDistribution is bg.distribution.MixtureDistribution is bg.mixture.MixtureDistribution


def test_abi_entries():
    from bgflow_amd._abi import abi_signatures
    from bgflow_amd.build import abi_symbols
    sigs = abi_signatures()
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    table = [p, p, p, p]                       # mu, h, logz, logw
    expected = {
        "bgk_mixture_energy": [p, i64, i64, i32, i32, *table, f64, p, p, p, i32, p, i32, p, p],
        "bgk_mixture_energy_backward": [p, i64, i64, i32, i32, *table, f64, p, p, p, p, i32, p, p, i64, p, p, i32, p],
        "bgk_mixture_sample": [ctypes.c_uint64, ctypes.c_uint32, i64, i64, i32, i32, *table, p, i64, p, p, p],
    }
    for name, args in expected.items():
        assert name in abi_symbols()
        assert sigs[name] == (ctypes.c_int, args), name
    assert (MIXTURE_MAX_COMPONENTS, MIXTURE_MAX_WIDTH) == (64, 128)


def _normals(K, d, **kw):
    return [bg.NormalDistribution(d, torch.full((d,), float(k)), **kw) for k in range(K)]


def test_kernel_plan_of_a_mixture():
    for K, d in mc.CASES:
        mix = mc.build(bg, K, d, torch.float32)
        plan = _kernel_plan(mix, 2.0)
        assert isinstance(plan, MixturePlan) and len(plan) != 5 and plan.dist is mix
        assert (plan.n_components, plan.dim, plan.temperature) == (K, d, 2.0)
    # the tables: a diagonal covariance is recognised from the stored rotation, in whatever order eigh sorted the variances
    inp = mc.inputs(7, 5)
    mu, h, logz = mc.build(bg, 7, 5, torch.float32)._host_tables()
    var = inp["var"].astype(np.float64) + 1e-6
    np.testing.assert_array_equal(mu, inp["mean"])
    np.testing.assert_allclose(h[1::2], 1.0 / var[1::2], rtol=1e-6)
    assert (h[0::2] == 1.0).all()
    np.testing.assert_allclose(logz[1::2], 2.5 * np.log(2 * np.pi) + 0.5 * np.log(var[1::2]).sum(1), rtol=1e-6)
    np.testing.assert_allclose(logz[0::2], 2.5 * np.log(2 * np.pi), rtol=1e-6)


def test_no_kernel_plan_outside_the_envelope():
    d = 3
    assert _kernel_plan(bg.MixtureDistribution(_normals(2, d)), 1.0) is not None
    assert _kernel_plan(bg.MixtureDistribution(_normals(2, d)), torch.tensor(1.0)) is None
    uniform = bg.UniformDistribution(torch.zeros(d), torch.ones(d))
    assert _kernel_plan(bg.MixtureDistribution([bg.NormalDistribution(d), uniform]), 1.0) is None          # a non-normal component
    full = torch.eye(d) + 0.3 * torch.ones(d, d)
    assert _kernel_plan(bg.MixtureDistribution([bg.NormalDistribution(d), bg.NormalDistribution(d, cov=full)]), 1.0) is None
    assert _kernel_plan(bg.MixtureDistribution(_normals(MIXTURE_MAX_COMPONENTS, d)), 1.0) is not None
    assert _kernel_plan(bg.MixtureDistribution(_normals(MIXTURE_MAX_COMPONENTS + 1, d)), 1.0) is None      # K = 65
    assert _kernel_plan(bg.MixtureDistribution(_normals(2, MIXTURE_MAX_WIDTH)), 1.0) is not None
    assert _kernel_plan(bg.MixtureDistribution(_normals(2, MIXTURE_MAX_WIDTH + 1)), 1.0) is None           # d = 129
    f64 = [bg.NormalDistribution(d, torch.zeros(d, dtype=torch.float64)) for _ in range(2)]
    assert _kernel_plan(bg.MixtureDistribution(f64), 1.0) is None

    class Shifted(bg.MixtureDistribution):
        def _energy(self, x):
            return super()._energy(x) + 1.0

    assert _kernel_plan(Shifted(_normals(2, d)), 1.0) is None                                              # a subclass overriding _energy

    class ShiftedNormal(bg.NormalDistribution):
        def energy(self, x, temperature=1.0):
            return super().energy(x, temperature=temperature) + 1.0

    assert _kernel_plan(bg.MixtureDistribution([bg.NormalDistribution(d), ShiftedNormal(d)]), 1.0) is None


def test_tables_follow_the_components_buffers():
    mix = bg.MixtureDistribution(_normals(2, 3))
    first = mix._host_tables()
    assert mix._host_tables() is first                     # cached while nothing changes
    with torch.no_grad():
        mix._components[1]._mean.add_(1.0)
    assert mix._host_tables()[0][1, 0] == 2.0
    mix._components[0].set_cov(torch.diag(torch.tensor([0.5, 2.0, 1.0])))
    np.testing.assert_allclose(mix._host_tables()[1][0], 1.0 / (np.array([0.5, 2.0, 1.0]) + 1e-6), rtol=1e-6)


def test_product_with_a_mixture_has_no_field_plan():
    mix = mc.build(bg, 2, 3, torch.float32)
    prod = bg.ProductDistribution([bg.NormalDistribution(4), mix])
    assert prod._kernel_fields(1.0) is None and _kernel_plan(prod, 1.0) is None
    x0, x1 = torch.randn(6, 4), torch.from_numpy(mc.inputs(2, 3)["x"][8:14])
    expected = bg.NormalDistribution(4).energy(x0) + mix.energy(x1)
    assert torch.allclose(prod.energy(x0, x1), expected) and prod.energy(x0, x1).shape == (6, 1)
