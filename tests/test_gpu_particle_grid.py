"""GPU (-m gpu): the particle kernels -- bgk_pair_energy / _backward / _hvp and bgk_box_energy / _backward (csrc/bgk_pair.hip), bgk_kdyn_eval /
_eval_backward / _integrate (csrc/bgk_kdyn.hip) and the chain kernel that shares csrc/bgk_pair_terms.h -- per element on a grid of (n, d)
that puts a shape on either side of every LDS tile-height switch and runs the D = 1 and D = 2 instantiations at the envelope
(particle_grid_common.py; test_host_particle_grid.py anchors its f64 restatement and shows that its metric rejects planted faults).

Rule for the pair energies: e(kernel) <= 4 e(ref32) + 1e-6 with e(v) = max |v - v64| / (A + 1e-6 (1 + max |v64| of the sample)), A the
absolute-sum scale of the element and e(ref32) the same figure of the classes' own torch formulas in f32 on the CPU, measured per case
(capped at 64 x 2^-24 on the host).  The particle box and the kernel dynamics keep the rules of box_common / kdyn_common, err <= 4 err32 +
1e-6 against the same module in f64 on the CPU, with err32 of its f32 CPU path measured here.  Everything else is bitwise: a row alone
against the row in the batch of 97 on both sides of the first tile boundary, strided rows against contiguous ones, a chain's energies
against the energy kernel.

B = 97 throughout: a partial last tile at every tile height (64, 63, 62, 61, 47, 39, 38, 32, 31, 30 rows)."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd import _lib, particles
from bgflow_amd.distributions import BoxPlan, PairPlan, _kernel_plan

import box_common
from kdyn_common import PARAMS, SETS, err_a, err_s, evaluate, flow_of, kernel_set
from particle_grid_common import (B, BOX_NSOLVENT, GRID, KDYN_SHAPES, KINDS, TEMPERATURES, TILE_SHAPES, bound, cotangent, box_positions,
                                  make, metric, parameters, positions, ref32_errors, rows_backward, rows_forward, rows_hvp, rows_kdyn,
                                  tile_rows, vector, worst)

pytestmark = pytest.mark.gpu

_CASES = {}


def case(G, kind, n, d, temperature):
    """(e(ref32) of u, g, Hu; the f64 restatement with its scales) of a grid case, computed once on the CPU"""
    key = (kind, n, d, temperature)
    if key not in _CASES:
        _CASES[key] = ref32_errors(G, kind, n, d, temperature)
    return _CASES[key]


def target(G, dev, kind, n, d, temperature=1.0):
    """(the class on the device, its PairPlan, x [B, n d] on the device): a case the kernel takes"""
    energy = make(G, kind, n, d).to(dev)
    plan = _kernel_plan(energy, temperature)
    x = positions(G, n, d).to(dev)
    assert isinstance(plan, PairPlan) and particles._pair_rows(plan, (x,)) is not None
    return energy, plan, x


def judge(label, got, want, scale, e_ref32, failures):
    e, b = metric(got, want, scale), bound(e_ref32)
    print(f"{label}: e(kernel) {e:.3g}, e(ref32) {e_ref32:.3g}, bound {b:.3g}")
    if not e <= b:
        failures.append((label, e, b, "worst element (row, column)", tuple(int(i) for i in worst(got, want, scale))))


@pytest.mark.parametrize("n,d", GRID)
@pytest.mark.parametrize("kind", KINDS)
def test_energy_per_sample(hip_lib, dev, golden, kind, n, d):
    G = golden("particles")
    energy, _, x = target(G, dev, kind, n, d)
    failures = []
    for temperature in TEMPERATURES:
        errs, ref = case(G, kind, n, d, temperature)
        u = energy.energy(x, temperature=temperature)
        assert u.shape == (B, 1)
        judge(f"{kind}_{n}_{d} T={temperature} u", u.cpu().numpy().reshape(-1), ref["u"], ref["A_u"], errs["u"], failures)
    assert not failures, failures


@pytest.mark.parametrize("n,d", GRID)
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_per_element_under_a_cotangent_per_row(hip_lib, dev, golden, kind, n, d):
    """autograd of (energy(x, T = 1.7) w).sum() with w cycling through 1, 0, -1, 1e-3, -1e3, 0.37: g_b / w_b under the rule (the bound
    multiplied by |w_b|), exact zeros where w_b = 0"""
    G = golden("particles")
    energy, _, x = target(G, dev, kind, n, d)
    errs, ref = case(G, kind, n, d, 1.7)
    x.requires_grad_(True)
    w = cotangent(dev)
    u = energy.energy(x, temperature=1.7)
    assert type(u.grad_fn).__name__ == "_PairEnergyFnBackward"
    (g,) = torch.autograd.grad((u * w).sum(), x)
    g, w = g.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64).reshape(-1)
    assert g.shape == (B, n * d) and np.isfinite(g).all()
    zero = w == 0
    assert zero.sum() >= B // 6 and not g[zero].any(), "a zero cotangent must give exact zeros"
    keep = ~zero
    failures = []
    judge(f"{kind}_{n}_{d} T=1.7 g / w (backward tile: {rows_backward(n * d)} rows)", g[keep] / w[keep, None], ref["g"][keep], ref["A_g"][keep],
          errs["g"], failures)
    assert not failures, failures


@pytest.mark.parametrize("n,d", GRID)
@pytest.mark.parametrize("kind", KINDS)
def test_hessian_vector_product_per_element(hip_lib, dev, golden, kind, n, d):
    G = golden("particles")
    energy, plan, x = target(G, dev, kind, n, d, 1.7)
    errs, ref = case(G, kind, n, d, 1.7)
    v = vector(n, d).to(dev)
    g, hu = particles.pair_energy_hvp(plan, x, v)
    failures = []
    label = f"{kind}_{n}_{d} T=1.7 hvp ({rows_hvp(n * d)} rows)"
    judge(label + " g", g.cpu().numpy(), ref["g"], ref["A_g"], errs["g"], failures)
    judge(label + " Hu", hu.cpu().numpy(), ref["hu"], ref["A_hu"], errs["hu"], failures)
    if kind == "mfn":                                    # the closed form itself: osc (v - vbar) / T
        osc = parameters(G, kind)[2]
        v64 = v.cpu().numpy().astype(np.float64).reshape(B, n, d)
        closed = (osc * (v64 - v64.mean(axis=1, keepdims=True)) / 1.7).reshape(B, n * d)
        judge(label + " Hu against osc (v - vbar) / T", hu.cpu().numpy(), closed, ref["A_hu"], errs["hu"], failures)
    assert not failures, failures
    # at T = 1: g has the bits of the energy kernel's backward; H 0 = 0 exactly
    plan1 = _kernel_plan(energy, 1.0)
    g1, _ = particles.pair_energy_hvp(plan1, x, v)
    xg = x.clone().requires_grad_(True)
    (g_bwd,) = torch.autograd.grad(energy.energy(xg).sum(), xg)
    assert torch.equal(g1, g_bwd)
    assert not bool(particles.pair_energy_hvp(plan1, x, torch.zeros_like(v))[1].any())


@pytest.mark.parametrize("n,d", TILE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_pair_rows_do_not_depend_on_their_tile(hip_lib, dev, golden, kind, n, d):
    """rows 0, h - 1, h and B - 1 (h: the kernel's tile height at the shape) alone, as batches of one, get the bits they have in the
    batch of 97: bgk_pair_energy, bgk_pair_energy_backward, bgk_pair_energy_hvp"""
    G = golden("particles")
    energy, plan, x = target(G, dev, kind, n, d, 1.7)
    w, v = cotangent(dev), vector(n, d).to(dev)

    def run(rows):
        xs = x[rows].contiguous().requires_grad_(True)
        u = energy.energy(xs, temperature=1.7)
        (g,) = torch.autograd.grad((u * w[rows]).sum(), xs)
        return u.detach(), g, particles.pair_energy_hvp(plan, xs.detach(), v[rows].contiguous())

    u, g, (hg, hu) = run(slice(None))
    heights = {"energy": rows_forward(n * d), "backward": rows_backward(n * d), "hvp": rows_hvp(n * d)}
    print(f"{kind}_{n}_{d}: tile heights {heights}")
    for r in sorted(set(sum((tile_rows(h) for h in heights.values()), []))):
        u1, g1, (hg1, hu1) = run(slice(r, r + 1))
        assert torch.equal(u1, u[r:r + 1]), ("energy", r)
        assert torch.equal(g1, g[r:r + 1]), ("backward", r)
        assert torch.equal(hg1, hg[r:r + 1]) and torch.equal(hu1, hu[r:r + 1]), ("hvp", r)


def strided(src, width, offset, dev):
    """(a [B, width] buffer filled with 7.0, its view at column ``offset`` holding ``src``)"""
    buf = torch.full((src.shape[0], width), 7.0, device=dev)
    view = buf[:, offset:offset + src.shape[1]]
    view.copy_(src)
    assert view.stride(0) == width and view.data_ptr() == buf.data_ptr() + 4 * offset
    return buf, view


def padding_untouched(buf, offset, nd):
    return bool((buf[:, :offset] == 7.0).all()) and bool((buf[:, offset + nd:] == 7.0).all())


@pytest.mark.parametrize("n,d", [(3, 1), (64, 2)])
@pytest.mark.parametrize("kind", ["lj", "mdw"])
def test_row_strides_of_the_pair_entries(hip_lib, dev, golden, kind, n, d):
    """x at column 3 of a [97, n d + 5] tensor (ldx = n d + 5: rows not 16-byte aligned), g_x at column 2 of a [97, n d + 3] one: the
    outputs have the contiguous launch's bits and every padding element keeps its 7.0"""
    G = golden("particles")
    _, plan, x = target(G, dev, kind, n, d, 1.7)
    nd, stream = n * d, _lib.stream_ptr(dev)
    head = (B, plan.n_particles, plan.n_dims, plan.kind, plan.p0, plan.p1, plan.p2, plan.p3, plan.osc_scale, plan.temperature)
    xbuf, xv = strided(x, nd + 5, 3, dev)
    xbuf0 = xbuf.clone()
    g_u, v = cotangent(dev).reshape(-1).contiguous(), vector(n, d).to(dev)

    def launch(xt, ldx, gx, ldg):
        u, hg, hu = torch.empty(B, device=dev), torch.empty(B, nd, device=dev), torch.empty(B, nd, device=dev)
        _lib.check(hip_lib.bgk_pair_energy(_lib.ptr(xt), ldx, *head, _lib.ptr(u), stream), "bgk_pair_energy")
        _lib.check(hip_lib.bgk_pair_energy_backward(_lib.ptr(xt), ldx, *head, _lib.ptr(g_u), None, None, None, 0, None, _lib.ptr(gx), ldg,
                                                    stream), "bgk_pair_energy_backward")
        _lib.check(hip_lib.bgk_pair_energy_hvp(_lib.ptr(xt), ldx, *head, _lib.ptr(v), _lib.ptr(hg), _lib.ptr(hu), stream), "bgk_pair_energy_hvp")
        return u, hg, hu

    gx_c = torch.empty(B, nd, device=dev)
    want = launch(x, nd, gx_c, nd)
    gbuf, gv = strided(torch.full((B, nd), 7.0, device=dev), nd + 3, 2, dev)
    got = launch(xv, nd + 5, gv, nd + 3)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(gv, gx_c)
    assert torch.isfinite(gx_c).all() and bool((gx_c != 7.0).any())
    assert torch.equal(xbuf, xbuf0) and padding_untouched(gbuf, 2, nd)


@pytest.mark.parametrize("kind", box_common.KINDS)
def test_row_strides_of_the_box_entries(hip_lib, dev, golden, kind):
    """the same through bgk_box_energy / bgk_box_energy_backward at 63 particles (S = 127)"""
    ns, nd, stream = 61, 126, _lib.stream_ptr(dev)
    energy = box_common.make(golden("box"), kind, ns).to(dev)
    plan = _kernel_plan(energy, 1.7)
    assert isinstance(plan, BoxPlan)
    x = box_positions(ns).to(dev)
    params = particles._box_params(plan)
    head = (B, plan.n_particles, plan.kind, params, len(plan.params), plan.temperature)
    xbuf, xv = strided(x, nd + 5, 3, dev)
    xbuf0 = xbuf.clone()
    g_u = cotangent(dev).reshape(-1).contiguous()

    def launch(xt, ldx, gx, ldg):
        u = torch.empty(B, device=dev)
        _lib.check(hip_lib.bgk_box_energy(_lib.ptr(xt), ldx, *head, _lib.ptr(u), stream), "bgk_box_energy")
        _lib.check(hip_lib.bgk_box_energy_backward(_lib.ptr(xt), ldx, *head, _lib.ptr(g_u), None, None, None, 0, None, _lib.ptr(gx), ldg, stream),
                   "bgk_box_energy_backward")
        return u

    gx_c = torch.empty(B, nd, device=dev)
    u_c = launch(x, nd, gx_c, nd)
    gbuf, gv = strided(torch.full((B, nd), 7.0, device=dev), nd + 3, 2, dev)
    u_s = launch(xv, nd + 5, gv, nd + 3)
    assert torch.equal(u_s, u_c) and torch.equal(gv, gx_c) and torch.isfinite(gx_c).all() and bool((gx_c != 7.0).any())
    assert torch.equal(xbuf, xbuf0) and padding_untouched(gbuf, 2, nd)


def box_energy_and_grad(energy, x):
    x = x.clone().requires_grad_(True)
    u = energy.energy(x)
    (g,) = torch.autograd.grad(u.sum(), x)
    return u.detach().cpu().numpy().reshape(-1), g.cpu().numpy()


@pytest.mark.parametrize("ns", BOX_NSOLVENT)
@pytest.mark.parametrize("kind", box_common.KINDS)
def test_particle_box_at_the_untested_widths(hip_lib, dev, golden, kind, ns):
    """3 and 63 particles; box_common's rule, err <= 4 err(f32 CPU torch formulas) + 1e-6 against ``_energy`` in f64 on the CPU, for the
    energy, the gradient and ``force``"""
    G = golden("box")
    host = box_common.make(G, kind, ns)
    x = box_positions(ns)
    u64, g64 = box_energy_and_grad(host, x.double())             # CPU tensors: the torch formulas
    u32, g32 = box_energy_and_grad(host, x)
    energy = box_common.make(G, kind, ns).to(dev)
    assert isinstance(_kernel_plan(energy, 1.0), BoxPlan)
    xd = x.to(dev).requires_grad_(True)
    out = energy.energy(xd)
    assert type(out.grad_fn).__name__ == "_PairEnergyFnBackward"
    (g,) = torch.autograd.grad(out.sum(), xd)
    u, g = out.detach().cpu().numpy().reshape(-1), g.cpu().numpy()
    force = energy.force(xd.detach()).cpu().numpy()
    assert np.isfinite(g).all() and np.array_equal(force, -g)    # the same launch with g_u = -1
    checks = [("energy", box_common.err_u(u, u64), box_common.err_u(u32, u64)), ("gradient", box_common.err_g(g, g64), box_common.err_g(g32, g64)),
              ("force", box_common.err_g(force, -g64), box_common.err_g(g32, g64))]
    for what, e, ref in checks:
        print(f"{kind}_{ns} ({rows_backward(2 * (ns + 2))}-row backward tile) {what}: error {e:.3g} (torch f32: {ref:.3g}, bound {4 * ref + 1e-6:.3g})")
    assert not [c for c in checks if not c[1] <= 4 * c[2] + 1e-6], checks


# ---- the kernel dynamics -------------------------------------------------------------------------------------------------------------
def make_dynamics(name, n, d, dtype=torch.float32):
    """KernelDynamics with small seeded parameter values, drawn as tests/golden/make_kernel_dynamics_goldens.py draws them"""
    ks = kernel_set(name, dtype)
    K, O = ks["mus"].shape[0], ks["mus_time"].shape[0]
    rng = np.random.default_rng(100 * n + 10 * d + SETS.index(name))
    values = {"_weights": rng.normal(size=(K, O)) * np.sqrt(1.0 / K) * 0.5 / np.sqrt(n), "_bias": rng.normal(size=(1, O)) * 0.1 / np.sqrt(n),
              "_importance": rng.normal(size=(K,)) * 0.5}
    dyn = bg.KernelDynamics(n, d, optimize_t_gammas=True, **ks).to(dtype)
    with torch.no_grad():
        for p, val in values.items():
            getattr(dyn, p).copy_(torch.tensor(val, dtype=dtype))
    return dyn


def integrate(dyn, x):
    """RK4 with Nt = 2 in both directions without grad: {"yf", "dlogpf", "yi", "dlogpi"} as numpy arrays"""
    flow, res = flow_of(dyn, "rk4", 2), {}
    with torch.no_grad():
        for tag, inverse in (("f", False), ("i", True)):
            y, dlogp = flow(x, inverse=inverse)
            assert y.shape == x.shape and dlogp.shape == (x.shape[0], 1)
            res["y" + tag], res["dlogp" + tag] = y.cpu().numpy(), dlogp.cpu().numpy().reshape(-1)
    return res


@pytest.mark.parametrize("n,d", KDYN_SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_kernel_dynamics_on_the_grid(hip_lib, dev, golden, name, n, d):
    """forces, divergence, g_x, the four parameter gradients (kdyn_common.evaluate at t = 0.37) and the fused RK4 integration with Nt = 2
    in both directions, against the same module in f64 on the CPU: err_s / err_a <= 4 err32 + 1e-6, err32 of its f32 CPU path.  The
    kernels run the batch of 97; the CPU integrates (16 evaluations each in f64 and f32, [rows, n, n - 1, K] tensors) the rows it is
    compared on: the first and last four and both sides of the first tile boundary -- rows are independent there, and the parameter
    gradients, which sum over the batch, come from ``evaluate`` on every row"""
    x = positions(golden("particles"), n, d)
    nd, K = n * d, kernel_set(name)["mus"].shape[0]
    heights = {"eval": rows_kdyn(nd, "eval"), "backward": rows_kdyn(nd, "backward", K), "integrate": rows_kdyn(nd, "integrate")}
    print(f"{name}_{n}_{d}: rows per tile: {heights}")
    rows = sorted(set(range(4)) | set(range(B - 4, B)) | {heights["integrate"] - 1, heights["integrate"]})
    dyn64, dyn32, dyn = make_dynamics(name, n, d, torch.float64), make_dynamics(name, n, d), make_dynamics(name, n, d).to(dev)
    xd = x.to(dev)
    assert dyn._kernel_rows(xd) is not None and dyn32._kernel_rows(x) is None
    r64, r32, r = evaluate(dyn64, x.double(), 0.37), evaluate(dyn32, x, 0.37), evaluate(dyn, xd, 0.37)
    r64.update(integrate(dyn64, x[rows].double()))
    r32.update(integrate(dyn32, x[rows]))
    r.update({key: val[rows] for key, val in integrate(dyn, xd).items()})
    assert all(np.isfinite(val).all() for val in r.values())
    checks = []
    for key in ["f", "div", "gx"] + ["g" + p for p in PARAMS] + ["yf", "dlogpf", "yi", "dlogpi"]:
        err = err_s if key in ("div", "dlogpf", "dlogpi") else err_a
        checks.append((key, err(r[key], r64[key]), err(r32[key], r64[key])))
        print(f"{name}_{n}_{d} {key}: error {checks[-1][1]:.3g} (torch f32: {checks[-1][2]:.3g}, bound {4 * checks[-1][2] + 1e-6:.3g})")
    assert not [c for c in checks if not c[1] <= 4 * c[2] + 1e-6], checks


@pytest.mark.parametrize("n,d", TILE_SHAPES)
@pytest.mark.parametrize("name", SETS)
def test_kernel_dynamics_rows_do_not_depend_on_their_tile(hip_lib, dev, golden, name, n, d):
    """bgk_kdyn_eval and bgk_kdyn_integrate: rows 0, h - 1, h and B - 1 alone get the bits they have in the batch of 97"""
    x = positions(golden("particles"), n, d).to(dev)
    dyn = make_dynamics(name, n, d).to(dev)
    flow = flow_of(dyn, "rk4", 2)
    heights = {"eval": rows_kdyn(n * d, "eval"), "integrate": rows_kdyn(n * d, "integrate")}
    print(f"{name}_{n}_{d}: tile heights {heights}")
    with torch.no_grad():
        f, neg_div = dyn(0.37, x)
        y, dlogp = flow(x)
        for r in sorted(set(sum((tile_rows(h) for h in heights.values()), []))):
            one = x[r:r + 1].contiguous()
            assert dyn._kernel_rows(one) is not None
            f1, neg_div1 = dyn(0.37, one)
            assert torch.equal(f1, f[r:r + 1]) and torch.equal(neg_div1, neg_div[r:r + 1]), ("eval", r)
            y1, dlogp1 = flow(one)
            assert torch.equal(y1, y[r:r + 1]) and torch.equal(dlogp1, dlogp[r:r + 1]), ("integrate", r)


# ---- the chain kernel on the same row functions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(64, 1), (63, 2)])
def test_chain_energies_are_the_energy_kernels_bits(hip_lib, dev, golden, n, d):
    """an IterativeSampler chain on in-kernel Philox, Lennard-Jones, 9 steps: the energies it returns are ``energy.energy`` of the states it
    returns, bit for bit (bgk_mcmc.hip and bgk_pair.hip add up bgk_pair_row_energy's terms alike, in the D = 1 and D = 2 instantiations)"""
    from test_gpu_mcmc import fused_sampler
    torch.manual_seed(4321)
    energy, _, x0 = target(golden("particles"), dev, "lj", n, d)
    sampler, step = fused_sampler(energy, x0, 0.02, 1.0, stream=70)
    frames = sampler.sample(3)
    state = sampler.state.as_dict()
    assert frames.shape == (3, B, n * d) and state["energies_up_to_date"]
    accepted = float(step.n_accepted.float().mean()) / step.n_proposed
    print(f"lj_{n}_{d}: {step.n_proposed} steps, acceptance {accepted:.2f}")
    assert step.n_proposed == 9 and accepted > 0 and not torch.equal(state["samples"][0], x0)        # (a run that moves)
    assert torch.equal(state["energies"], energy.energy(state["samples"][0])[:, 0])
