"""GPU: the robust-training kernels -- bgk_clip_gradient, bgk_linlogcut, bgk_energy_fields_cut(_backward), bgk_grad_norm_flag and
bgk_adam_step_clipped -- behind bgflow_amd.clipped, distributions.kl_loss_sums and FlatAdam(max_grad_norm=...), against the reference's
recorded results (tests/golden/g_clipped.npz) and against the package's f64 torch path on the CPU.

Shapes: B in {1, 65, 4099} (one sample, one past a wave, past the 2048 loss-partial blocks with a ragged last block); widths 66 (22
atoms, no multiple of 4: the staging / group kernels), 64 (the float4 kernels), 6 and 3; row views of a wider tensor."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from bgflow_amd.distributions import kl_loss_sums

pytestmark = pytest.mark.gpu

BATCHES = [1, 65, 4099]
HIGH, MAX = 5.0, 8.0
CLAMP_FROM = HIGH - 1.0 + float(np.exp(MAX - HIGH))          # uncut energy at which linlogcut(., 5, 8) reaches the clamp: 24.0855


def T(a, dev=None):
    return torch.as_tensor(np.asarray(a), device=dev)


def gradient_batch(B, D, seed):
    """gradients whose groups lie below, above and across a threshold of 1; zero rows, NaN and +-inf entries from row 6 on (B >= 65)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g) * torch.logspace(-2, 1, B)[torch.randperm(B, generator=g)][:, None]
    if B >= 65:
        x[6:8] = 0.0
        x[8, 1] = x[9, 0] = float("nan")
        x[10, D - 1] = float("inf")
        x[11, 0] = -float("inf")
    return x


@pytest.mark.parametrize("B", BATCHES)
def test_clip_gradient_kernel_by_group(hip_lib, dev, B):
    """norm_dim 1 / 3 / other divisors against the f64 torch path: rtol 2e-6 (a group's factor is about five f32 roundings: squares,
    their sum, the root, the division, the product); NaN and +-inf entries exactly as the f32 torch path has them; two runs equal bits;
    in place; a row view of a wider tensor."""
    clip = 1.0
    for D, nds in ((66, (1, 3, 6, 66)), (64, (1, 2, 4, 8)), (6, (1, 3)), (3, (1, 3))):
        x = gradient_batch(B, D, 100 * B + D)
        finite = torch.isfinite(x).all(dim=1)
        xd = x.to(dev)
        for nd in nds:
            out = bg.ClipGradient.clip_tensor(xd, clip, nd)
            assert out.is_cuda and torch.equal(out, bg.ClipGradient.clip_tensor(xd, torch.tensor(clip), nd)), (D, nd)
            ref64 = bg.ClipGradient.clip_tensor(x[finite].double(), clip, nd)
            np.testing.assert_allclose(out.cpu()[finite].numpy(), ref64.numpy(), rtol=2e-6, atol=0, err_msg=f"D {D} norm_dim {nd}")
            if not finite.all():        # NaN -> 0; +-inf -> +-clip by value, the whole group -> 0 otherwise: the f32 path's own entries
                ref32 = bg.ClipGradient.clip_tensor(x[~finite], clip, nd)
                np.testing.assert_allclose(out.cpu()[~finite].numpy(), ref32.numpy(), rtol=2e-6, atol=0, err_msg=f"D {D} norm_dim {nd}")
                assert torch.isfinite(out).all()
        # in place, and a view of a wider tensor (rows 4 bytes past a 16-byte boundary: the group kernel whatever the width)
        from bgflow_amd.clipped import clip_launch
        wide = torch.zeros(B, D + 7, device=dev)
        view = wide[:, 1:D + 1]
        view.copy_(xd)
        want = bg.ClipGradient.clip_tensor(xd, clip, nds[1])
        assert torch.equal(bg.ClipGradient.clip_tensor(view, clip, nds[1]), want)
        clip_launch(view, clip, nds[1], out=view)
        assert torch.equal(view, want) and not wide[:, 0].any() and not wide[:, D + 1:].any()


@pytest.mark.parametrize("width", [66, 6])
def test_clip_gradient_kernel_against_the_reference(hip_lib, dev, golden, width):
    """the recorded results of the reference's ClipGradient.clip_tensor, the +-inf and NaN rows included"""
    G = golden("g_clipped")
    g = T(G[f"clip{width}_in"], dev)
    clip = float(G["clip_value"])
    for nd in (1, 3):
        np.testing.assert_allclose(bg.ClipGradient.clip_tensor(g, clip, nd).cpu().numpy(), G[f"clip{width}_n{nd}"], rtol=2e-6, atol=0)
    # norm_dim -1 over a tensor with +-inf entries: the reference's f32 sum of squares overflows and everything comes out 0
    assert not bg.ClipGradient.clip_tensor(g, clip, -1).any() and not G[f"clip{width}_m1"].any()
    np.testing.assert_allclose(bg.ClipGradient.clip_tensor(g[:10], clip, -1).cpu().numpy(), G[f"clip{width}_m1f"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("B", BATCHES)
def test_clip_gradient_kernel_whole_tensor_norm(hip_lib, dev, B):
    """norm_dim -1: the APPLIED factor (least-squares estimate out . in / in . in) against clip / |in|_2 in f64.  Bound: twice the error of
    the reference's own f32 arithmetic (the torch path) on the same inputs, at least 1e-6 relative.  Two runs give equal bits."""
    for D in (66, 64, 3):
        x = gradient_batch(B, D, 7 * B + D)
        x[~torch.isfinite(x)] = float("nan")            # NaN entries count as zeros; +-inf is the recorded case above
        clean = torch.nan_to_num(x, nan=0.0).double()
        clip = 0.37 * float(clean.norm())                 # the factor is 0.37
        f64 = clip / float(clean.norm())
        est = lambda out: float((out.double() * clean).sum() / (clean * clean).sum())     # noqa: E731
        out = bg.ClipGradient.clip_tensor(x.to(dev), clip, -1)
        err = abs(est(out.cpu()) - f64) / f64
        err_ref = abs(est(bg.ClipGradient.clip_tensor(x, clip, -1)) - f64) / f64
        print(f"norm_dim -1, [{B}, {D}]: factor error of the kernel {err:.2e}, of the f32 torch path {err_ref:.2e}")
        assert err <= max(2 * err_ref, 1e-6), (B, D, err, err_ref)
        np.testing.assert_allclose(out.cpu().numpy(), (clean * f64).numpy(), rtol=2e-6, atol=0)
        assert torch.equal(out, bg.ClipGradient.clip_tensor(x.to(dev), clip, -1))
        # below the threshold nothing but the NaN entries changes
        assert torch.equal(bg.ClipGradient.clip_tensor(x.to(dev), 2.0 * float(clean.norm()), -1).cpu(), torch.nan_to_num(x, nan=0.0))


def chains(dev=None, dtype=torch.float32):
    """the golden chains (make_clip_goldens.py) and the input scale that spreads their uncut energies over the cut's three branches"""
    mk = lambda e: (e.to(dev) if dev is not None else e).to(dtype)      # noqa: E731
    n, w = bg.NormalDistribution(66), bg.DoubleWellEnergy(64)
    cn, cd = (lambda: bg.ClipGradient(0.05, 3)), (lambda: bg.ClipGradient(0.02, 1))
    return {
        "n66_cut_clip": mk(bg.LinLogCutEnergy(bg.GradientClippedEnergy(n, cn()), HIGH, MAX)),
        "n66_clip_cut": mk(bg.GradientClippedEnergy(bg.LinLogCutEnergy(n, HIGH, MAX), cn())),
        "n66h_cut_clip": mk(bg.LinLogCutEnergy(bg.GradientClippedEnergy(n, cn()), 70.0, 75.0)),
        "n66h_clip_cut": mk(bg.GradientClippedEnergy(bg.LinLogCutEnergy(n, 70.0, 75.0), cn())),
        "dw64_cut": mk(bg.LinLogCutEnergy(w, HIGH, MAX)),
        "dw64_clip": mk(bg.GradientClippedEnergy(w, cd())),
        "dw64_clip_cut": mk(bg.GradientClippedEnergy(bg.LinLogCutEnergy(w, HIGH, MAX), cd())),
    }


def chain_inputs(name, B, seed=0):
    """inputs whose uncut energies cover all three branches of the chain's cut and keep 1e-4 away from its two branch points (asserted:
    the share of excluded samples is 0).  NormalDistribution(66) cannot go below 33 log 2 pi = 60.6: with (5, 8) all its samples sit on
    the clamp, the n66h chains (70, 75) cover the three branches."""
    g = torch.Generator().manual_seed(1000 * B + seed)
    if name.startswith("n66"):
        x = torch.randn(B, 66, generator=g) * torch.linspace(0.05, 2.7, B)[torch.randperm(B, generator=g)][:, None]
        v = bg.NormalDistribution(66).double().energy(x.double())
        high, max_e = (70.0, 75.0) if name.startswith("n66h") else (HIGH, MAX)
    else:
        x = torch.randn(B, 64, generator=g) * torch.linspace(0.05, 1.3, B)[torch.randperm(B, generator=g)][:, None]
        x[:, 0] = torch.randn(B, generator=g) * 1.5
        v = bg.DoubleWellEnergy(64).energy(x.double())
        high, max_e = HIGH, MAX
    margin = torch.minimum((v - high).abs(), (v - (high - 1.0 + float(np.exp(max_e - high)))).abs())
    assert int((margin <= 1e-4).sum()) == 0, f"{name}, B = {B}: a sample within 1e-4 of a branch point of the cut"
    return x, v


def within(a, want, what):
    """the bound of test_energy_float4_rows_equal_the_staging_kernels: 2e-6 scaled by max(1, |.|)"""
    if want.shape[-1] == 1:
        err = float(((a.double() - want).abs() / want.abs().clamp_min(1.0)).max())
    else:
        err = float((a.double() - want).abs().max()) / max(1.0, float(want.abs().max()))
    assert err <= 2e-6, f"{what}: {err:.2e}"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("temperature", [1.0, 1.7])
def test_wrapped_energies_in_one_launch(hip_lib, dev, B, temperature):
    """energy(x, T) and x.grad of every chain against the f64 torch path; the isolated cut: linlogcut (f64) of the kernel's own uncut
    energy against the fused result, rtol 1e-6"""
    gpu, cpu = chains(dev), chains(dtype=torch.float64)
    w = torch.linspace(0.5, 1.5, B)[:, None]
    for name in gpu:
        x, v = chain_inputs(name, B)
        if B >= 65 and "cut" in name and not name.startswith("n66_"):
            high = 70.0 if name.startswith("n66h") else HIGH
            clamp = high - 1.0 + float(np.exp((75.0 if name.startswith("n66h") else MAX) - high))
            assert (v < high).any() and ((v >= high) & (v < clamp)).any() and (v > clamp).any(), f"{name}: a branch of the cut is not covered"
        xg = x.to(dev).requires_grad_(True)
        u = gpu[name].energy(xg, temperature=temperature)
        assert u.shape == (B, 1) and type(u.grad_fn).__name__ == "_CutEnergyFieldsFnBackward", name          # ONE launch
        (u * w.to(dev)).sum().backward()
        x64 = x.double().requires_grad_(True)
        u64 = cpu[name].energy(x64, temperature=temperature)
        (u64 * w.double()).sum().backward()
        within(u.detach().cpu(), u64.detach(), f"{name} energy")
        within(xg.grad.cpu(), x64.grad, f"{name} gradient")
        if "cut" in name:               # the new arithmetic alone
            delegate = bg.DoubleWellEnergy(64) if name.startswith("dw") else bg.NormalDistribution(66).to(dev)
            uncut = delegate.energy(x.to(dev)).double().cpu()
            high, max_e = (70.0, 75.0) if name.startswith("n66h") else (HIGH, MAX)
            np.testing.assert_allclose(u.detach().cpu().numpy(), (bg.linlogcut(uncut, high, max_e) / temperature).numpy(), rtol=1e-6, atol=0)


def test_wrapped_energies_against_the_reference(hip_lib, dev, golden):
    G = golden("g_clipped")
    gpu = chains(dev)
    for name in ("n66_cut_clip", "n66_clip_cut", "n66h_cut_clip", "n66h_clip_cut", "dw64_cut", "dw64_clip"):
        for t in G["temperatures"]:
            x = T(G["n66_x" if name.startswith("n66") else "dw64_x"], dev).requires_grad_(True)
            u = gpu[name].energy(x, temperature=float(t))
            u.sum().backward()
            within(u.detach().cpu(), T(G[f"{name}_T{t}_u"]).double(), f"{name} T {t} energy")
            within(x.grad.cpu(), T(G[f"{name}_T{t}_g"]).double(), f"{name} T {t} gradient")


def test_wrappers_around_other_delegates_and_other_layouts(hip_lib, dev):
    """a delegate without kernel fields: GradientClippedEnergy hooks its inputs (bgk_clip_gradient), LinLogCutEnergy cuts the [B, 1]
    result (bgk_linlogcut); a whole-tensor clip on the fused chain; a product target; a row view as the input"""
    class Custom(bg.Energy):
        def _energy(self, x):
            return (x ** 2).sum(-1, keepdim=True) * x[:, :1].cos()

    B = 65
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 6, generator=g) * 1.5
    cases = {
        "custom": (lambda: bg.LinLogCutEnergy(bg.GradientClippedEnergy(Custom(6), bg.ClipGradient(0.05, 3)), 2.0, 3.0), [x]),
        "whole": (lambda: bg.GradientClippedEnergy(bg.LinLogCutEnergy(bg.DoubleWellEnergy(6), 2.0, 3.0), bg.ClipGradient(0.3, -1)), [x]),
        "product": (lambda: bg.LinLogCutEnergy(bg.GradientClippedEnergy(bg.ProductDistribution(
            [bg.NormalDistribution(6, mean=torch.linspace(-1, 1, 6)), bg.DoubleWellEnergy(3), bg.UniformDistribution(torch.zeros(3), torch.ones(3))]),
            bg.ClipGradient(0.04, 3)), 9.0, 10.0), [x, torch.randn(B, 3, generator=g), torch.rand(B, 3, generator=g)]),
    }
    for name, (make, xs) in cases.items():
        xg = [t.to(dev).requires_grad_(True) for t in xs]
        u = make().to(dev).energy(*xg, temperature=1.3)
        u.sum().backward()
        x64 = [t.double().requires_grad_(True) for t in xs]
        u64 = make().double().energy(*x64, temperature=1.3)
        u64.sum().backward()
        within(u.detach().cpu(), u64.detach(), name)
        for a, b in zip(xg, x64):
            if b.grad is not None:
                within(a.grad.cpu(), b.grad, name)
    wide = torch.randn(B, 80, generator=g).to(dev)
    e = bg.GradientClippedEnergy(bg.DoubleWellEnergy(64), bg.ClipGradient(0.02, 1))
    a, b = wide[:, 8:72].detach().requires_grad_(True), wide[:, 8:72].contiguous().requires_grad_(True)
    e.energy(a).sum().backward(); e.energy(b).sum().backward()
    assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("B", BATCHES)
def test_kl_loss_sums_of_wrapped_targets(hip_lib, dev, B):
    """kl_loss_sums on every chain: the sums against (energy - dlogp) summed in f64, the gradients to x and dlogp against the per-sample
    path; one injected non-finite row is dropped on request (kept count - 1, zero gradients on that row)"""
    gpu = chains(dev)
    for name, target in gpu.items():
        x, _ = chain_inputs(name, B, seed=1)
        dl = torch.randn(B, 1, generator=torch.Generator().manual_seed(B))
        for drop in (False, True):
            bad = B // 2 if drop else None
            if drop:
                dl = dl.clone(); dl[bad] = float("inf")
            xg, dg = x.to(dev).requires_grad_(True), dl.to(dev).requires_grad_(True)
            res = kl_loss_sums(target, (xg,), dg, 1.7, drop)
            assert res is not None, f"{name}: no kernel plan"
            sums, u = res
            (sums[0] * 0.25).backward()
            xp, dp_ = x.to(dev).requires_grad_(True), dl.to(dev).requires_grad_(True)
            per = target.energy(xp, temperature=1.7) - dp_
            keep = torch.isfinite(per) if drop else torch.ones_like(per, dtype=torch.bool)
            (torch.where(keep, per, torch.zeros_like(per)).sum() * 0.25).backward()
            want = per.detach().double()[keep].sum()
            assert float(sums[1]) == B - int(drop)
            assert abs(float(sums[0]) - float(want)) <= 2e-6 * max(1.0, float(per.detach().double()[keep].abs().sum())), name
            assert torch.equal(u, target.energy(x.to(dev), temperature=1.7))
            within(xg.grad.cpu(), xp.grad.double().cpu(), f"{name} x gradient")
            assert torch.equal(dg.grad, dp_.grad)
            if drop:
                assert not xg.grad[bad].any() and float(dg.grad[bad]) == 0.0


def _grad_errors(got, ref):
    num = sum(float(((got[n] - ref[n]) ** 2).sum()) for n in ref)
    den = sum(float((ref[n] ** 2).sum()) for n in ref)
    worst = max((float((got[n] - ref[n]).abs().max()) / max(float(ref[n].norm()), 1e-30), n) for n in ref)
    return (num / den) ** 0.5, worst


def test_one_kl_step_with_a_wrapped_target(hip_lib, dev):
    """BASELINE cfg 2 (8 affine couplings, dim 64) at B = 4099 with GradientClippedEnergy(LinLogCutEnergy(DoubleWellEnergy(64)),
    ClipGradient(1e-4, 1)) -- the threshold bites: |dL/dx| = |de/dx| / B exceeds it for most elements: the flat gradient of one
    KLTrainer + FlatAdam step (fused kldiv_mean path) against f64 autograd of the reference's op chain with the wrappers' torch path on
    the same samples, within the bound of the cfg-2 KL gradient test (relative L2 5e-5, every tensor within 3e-4 of its norm)."""
    from bgflow_amd import configs
    from bgflow_amd.training import FlatAdam, KLTrainer
    from oracle import torch_flow as tfl
    B = 4099
    make_target = lambda: bg.GradientClippedEnergy(bg.LinLogCutEnergy(bg.DoubleWellEnergy(64)), bg.ClipGradient(1e-4, 1))     # noqa: E731
    gen, gen_cpu = configs.make_affine8_generator(device=dev), configs.make_affine8_generator().double()
    gen._target = make_target().to(dev)
    opt = FlatAdam([p for p in gen.parameters() if p.requires_grad], lr=1e-3, max_grad_norm=1.0)
    tr = KLTrainer(gen, optim=opt, train_likelihood=False)
    before = opt.flat.clone()
    torch.manual_seed(11)
    tr.train(1, batchsize=B)
    got = {n: p.grad.detach().cpu().double() for n, p in gen.flow.named_parameters()}
    assert not torch.equal(opt.flat, before) and opt.skipped_steps() == 0
    torch.manual_seed(11)
    z = gen.prior.sample(B)
    for p in gen_cpu.flow.parameters():
        p.grad = None
    xs, dl = tfl.run_flow(gen_cpu.flow, [z.cpu().double()], grad=True)
    xs[0].retain_grad()
    target64 = make_target().double()
    loss64 = (target64.energy(xs[0]) - dl).mean()
    loss64.backward()
    clipped = float((xs[0].grad.abs() >= float(np.float32(1e-4)) * (1 - 1e-9)).double().mean())       # (the f32 threshold; clipped entries sit on it)
    assert 0.2 < clipped < 0.999, f"share of clipped gradient elements {clipped:.3f}: the threshold does not bite / bites everywhere"
    ref = {n: p.grad.clone() for n, p in gen_cpu.flow.named_parameters()}
    assert set(ref) == set(got)
    rel, worst = _grad_errors(got, ref)
    print(f"wrapped cfg-2 KL step: flat gradient relative L2 {rel:.2e}, worst tensor {worst[1]} {worst[0]:.2e} of its norm; "
          f"{clipped:.1%} of dL/dx clipped; loss {float(tr.reporter.recent()[0][0]):.6f} vs f64 {float(loss64):.6f}")
    assert rel <= 5e-5 and worst[0] <= 3e-4
    assert abs(float(tr.reporter.recent()[0][0]) - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64)))
    norm = float(sum((v ** 2).sum() for v in ref.values()) ** 0.5)
    assert abs(float(opt.last_grad_norm()) - norm) <= 1e-4 * norm


def test_flat_adam_with_norm_clipping(hip_lib, dev):
    """FlatAdam(max_grad_norm=m) == torch.optim.Adam after clip_grad_norm_(., m) on CPU f32: 3036 parameters in odd-sized tensors, five
    steps whose gradient norms lie on both sides of m.  Bound: 1e-6 of a tensor's largest entry (one update rounds at 6e-8 |p|; the
    coefficient comes from an f64 norm here, an f32 one there: 1e-7 relative on a step of lr).  An inf gradient skips the step."""
    from bgflow_amd.training import FlatAdam
    shapes = [(37, 41), (613,), (29, 31), (7,)]
    m = 1.0
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(*s, generator=g) for s in shapes]
    scales = [0.01, 10.0, 0.3, 5.0, 0.001]
    grads = [[torch.randn(*s, generator=g) * sc / 55.0 for s in shapes] for sc in scales]        # norms ~ scale
    cpu = [torch.nn.Parameter(t.clone()) for t in init]
    gpu = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    plain = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    plain_none = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = torch.optim.Adam(cpu, lr=1e-2, weight_decay=1e-3)
    opt = FlatAdam(gpu, lr=1e-2, weight_decay=1e-3, max_grad_norm=m)
    o1, o2 = FlatAdam(plain, lr=1e-2, weight_decay=1e-3), FlatAdam(plain_none, lr=1e-2, weight_decay=1e-3, max_grad_norm=None)
    seen = []
    for step in grads:
        for ps, o in ((gpu, opt), (plain, o1), (plain_none, o2)):
            o.zero_grad()
            for p, t in zip(ps, step):
                p.grad.copy_(t.to(dev))
        for p, t in zip(cpu, step):
            p.grad = t.clone()
        kept = opt.grad.clone()
        total = torch.nn.utils.clip_grad_norm_(cpu, m)
        ref.step(); opt.step(); o1.step(); o2.step()
        seen.append(float(total) > m)
        assert torch.equal(opt.grad, kept), "the bucket itself stays unscaled"
        assert abs(float(opt.last_grad_norm()) - float(total)) <= 1e-6 * float(total)
        for a, b in zip(gpu, cpu):
            assert float((a.detach().cpu() - b.detach()).abs().max()) <= 1e-6 * float(b.detach().abs().max())
    assert any(seen) and not all(seen)
    assert torch.equal(o1.flat, o2.flat) and not torch.equal(o1.flat, opt.flat)          # None: today's step, bit for bit
    # an inf gradient: the norm is not finite, the step is skipped and counted (torch would write NaN)
    before = opt.flat.clone()
    opt.zero_grad()
    gpu[1].grad[17] = float("inf")
    opt.step()
    assert opt.skipped_steps() == 1 and torch.equal(opt.flat, before) and not torch.isfinite(opt.last_grad_norm())
    sd = opt.state_dict()
    assert sd["flat_adam"]["max_grad_norm"] == m and o1.state_dict()["flat_adam"]["max_grad_norm"] is None
    opt.load_state_dict(sd)
    with pytest.raises(RuntimeError):
        o1.last_grad_norm()
