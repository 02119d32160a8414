"""GPU (-m gpu): the constraint layers on the column-map kernel (bgk_colmap, csrc/bgk_colmap.hip) against the reference's golden
vectors (tests/golden/g_constraints.npz), the Philox oracle (oracle/philox.py) and f64 autograd of the reference's op chain.
Every kind of the kernel is one or two correctly rounded IEEE operations or an exact fmod in torch's order: equality of bits."""
import numpy as np
import pytest
import torch

import bgflow_amd as bg
from test_host_constraints import T, constraint_builder, same

pytestmark = pytest.mark.gpu


def _philox_u(flow, rows, n, call, row0=0):
    """the uniforms IncreaseMultiplicityFlow's kernel draws at call ``call``: oracle/philox.py on the flow's key"""
    from oracle import philox
    from bgflow_amd import dp
    stream = flow.__dict__["_philox_state"][0]
    seed = (dp.rank_seed(torch.initial_seed()) + 0x9E3779B97F4A7C15 * (stream + 1)) & (2 ** 64 - 1)
    return philox.sample_field(seed, call, 0, rows, n, 0, row0=row0)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
    except Exception as e:          # no kernel tracer on this box
        pytest.skip(f"torch.profiler unavailable: {e!r}")
    names = [e.key for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA for _ in range(e.count)]
    if not names:
        pytest.skip("torch.profiler recorded no device kernels")
    return names


def _aten(names):
    return [n for n in names if "at::native" in n or "elementwise" in n or "copyBuffer" in n or "fillBuffer" in n or "Memset" in n or "Memcpy" in n]


def test_each_flow_alone_matches_the_reference(hip_lib, dev, golden):
    G = golden("g_constraints")
    with torch.no_grad():
        f = bg.CircularShiftFlow(T(G["shifts"])).to(dev)
        y, d = f(T(G["shift_x"], dev))
        xi, di = f(T(G["shift_x"], dev), inverse=True)
        assert same(y, G["shift_fwd"]) and same(xi, G["shift_inv"]) and same(d, G["shift_dlogp"]) and same(di, G["shift_dlogp_inv"])
        assert f.check_unit_interval() == 0           # 0, 1 and values within 1e-6 outside [0, 1] are allowed
        f = bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev)
        y, d = f(T(G["mult_x"], dev), sheaf_uniforms=T(G["mult_u"], dev))
        xi, di = f(T(G["mult_x"], dev), inverse=True)
        assert same(y, G["mult_fwd"]) and same(xi, G["mult_inv"]) and same(d, G["mult_dlogp"]) and same(di, G["mult_dlogp"])
        assert f.check_unit_interval() == 0
        f = bg.TorchTransform(torch.distributions.AffineTransform(loc=T(G["aff_loc"], dev), scale=T(G["aff_scale"], dev)), 1)
        y, d = f(T(G["aff_x"], dev))
        xi, di = f(T(G["aff_x"], dev), inverse=True)
        assert same(y, G["aff_fwd"]) and same(xi, G["aff_inv"])
        # log-det: the kernel writes the f64 sum rounded once; the reference sums f32 logarithms.  A correctly rounded value is at
        # least as close to the f64 sum as any other f32, so the bound is the reference's own error (here the two differ or not
        # by rounding only); printed before it is asserted
        ld64 = float(G["aff_logdet64"])
        e_ours, e_ref = abs(float(d[0, 0].double()) - ld64), abs(float(np.float64(G["aff_dlogp"][0, 0])) - ld64)
        print(f"affine log-det error vs f64: kernel {e_ours:.3e}, reference f32 {e_ref:.3e}")
        assert d.shape == (256, 1) and bool((d == d[0]).all()) and bool((di == -d).all()) and e_ours <= e_ref
        f = bg.TorchTransform(torch.distributions.AffineTransform(loc=0.25, scale=-3.0), 1)
        y, d = f(T(G["aff_x"], dev))
        assert same(y, G["affs_fwd"]) and abs(float(d[0, 0].double()) - 17 * np.log(3.0)) <= abs(float(np.float64(G["affs_dlogp"][0, 0])) - 17 * np.log(3.0))


def test_builder_flow_matches_the_reference(hip_lib, dev, golden):
    G = golden("g_constraints")
    flow = constraint_builder(G, device=dev).build_flow()
    assert [label for label, _ in flow.segments()][0] == "constant merge"
    zs = [T(G[f"flow_z{k}"], dev) for k in range(4)]
    with torch.no_grad():
        *ys, d = flow(*zs, sheaf_uniforms=T(G["flow_u"], dev))
        *zi, di = flow(*[T(G[f"flow_y{k}"], dev) for k in range(4)], inverse=True)
    for k in range(4):
        assert same(ys[k], G[f"flow_y{k}"]), f"forward, tensor {k}"
        assert same(zi[k], G[f"flow_zi{k}"]), f"inverse, tensor {k}"
    assert same(d, G["flow_dlogp"]) and same(di, G["flow_dlogp_inv"])       # 2 ln 0.5: exact in either summation
    # drawing on the device: the same chain on the CPU with the sheaves the Philox oracle predicts
    mult = flow[2]._flow
    mult.set_philox_stream(11, calls=4)
    with torch.no_grad():
        *ys2, d2 = flow(*zs)
        *ref, dr = constraint_builder(G).build_flow()(*[z.cpu() for z in zs], sheaf_uniforms=torch.from_numpy(_philox_u(mult, 256, 17, 4)))
    for a, b in zip(ys2, ref):
        assert torch.equal(a.cpu(), b)
    assert torch.equal(d2.cpu(), dr)


def test_multiplicity_forward_draws_the_philox_stream(hip_lib, dev, golden):
    G = golden("g_constraints")
    m = G["mults"].astype(np.float32)
    x = T(G["mult_x"], dev)[8:]                          # rows without the edge values
    B = x.shape[0]
    f = bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev)
    f.set_philox_stream(3)
    torch.manual_seed(77)
    with torch.no_grad():
        y0, _ = f(x)
        y1, _ = f(x)
        xb, _ = f(y0, inverse=True)
    for call, y in ((0, y0), (1, y1)):
        u = _philox_u(f, B, 17, call)
        sheaf = np.floor(u * m)
        got = np.rint(y.cpu().numpy() * m - x.cpu().numpy())
        assert np.array_equal(got, sheaf), f"call {call}: sheaf index differs from the oracle's prediction"
        assert np.array_equal(y.cpu().numpy(), (x.cpu().numpy() + sheaf) / m)          # one f32 addition, one f32 division
    assert not torch.equal(y0, y1)                       # two calls draw different sheaves
    # inverse(forward(x)) = the chain (x + s) / m -> remainder(., 1 / m) * m evaluated on the CPU with the predicted sheaves
    s0 = torch.from_numpy(np.floor(_philox_u(f, B, 17, 0) * m))
    mt = torch.from_numpy(m)
    chain = torch.remainder((x.cpu() + s0) / mt, 1 / mt) * mt
    assert torch.equal(xb.cpu(), chain)
    print("multiplicity round trip: max |inverse(forward(x)) - x| =", float((xb.cpu() - x.cpu()).abs().max()))
    # a shard of the batch draws what the whole batch draws
    f.set_philox_stream(3, calls=0)
    with torch.no_grad():
        lo, _ = f(x[:100].contiguous())
        f.set_philox_stream(3, calls=0)
        hi, _ = f(x[100:].contiguous(), row0=100)
    assert torch.equal(torch.cat([lo, hi]), y0)
    assert f.state_dict()["_philox_state"].tolist() == [3, 1]


def test_constraint_merge_is_one_launch_equal_to_the_two_blocks(hip_lib, dev, golden):
    G = golden("g_constraints")
    flow = constraint_builder(G, device=dev).build_flow()[:2]
    z = T(G["flow_z0"], dev)
    rest = [T(G[f"flow_z{k}"], dev) for k in (1, 2, 3)]
    free = np.setdiff1d(np.arange(17), G["c_idx"])
    with torch.no_grad():
        y, *_, d = flow(z, *rest)
        zb, *_, db = flow(y, *rest, inverse=True)
        flow.FUSE_CONSTANT_MERGE = False
        y2, *_, d2 = flow(z, *rest)
        zb2, *_, db2 = flow(y, *rest, inverse=True)
        flow.FUSE_CONSTANT_MERGE = True
    assert same(y, G["merge_fwd"]) and same(zb, G["merge_inv"]) and same(d, G["merge_dlogp"]) and same(db, G["merge_dlogp"])
    assert np.array_equal(y.cpu().numpy()[:, G["c_idx"]], np.broadcast_to(G["c_val"], (256, 2)))
    assert np.array_equal(y.cpu().numpy()[:, free], G["flow_z0"]) and torch.equal(zb, z)
    assert torch.equal(y, y2) and torch.equal(zb, zb2) and torch.equal(d, d2) and torch.equal(db, db2)


def test_constraint_layers_launch_no_aten_kernel(hip_lib, dev, golden):
    G = golden("g_constraints")
    merge = constraint_builder(G, device=dev).build_flow()[:2]
    z = [T(G[f"flow_z{k}"], dev) for k in range(4)]
    x = T(G["mult_x"], dev)
    cases = {
        "set constant + merge": lambda: merge(*z),
        "circular shift": lambda f=bg.CircularShiftFlow(T(G["shifts"])).to(dev): f(x),
        "multiplicity forward": lambda f=bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev): f(x),
        "multiplicity inverse": lambda f=bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev): f(x, inverse=True),
        "affine": lambda f=bg.TorchTransform(torch.distributions.AffineTransform(T(G["aff_loc"], dev), T(G["aff_scale"], dev)), 1): f(x),
    }
    with torch.no_grad():
        for what, fn in cases.items():
            names = _kernel_names(fn)
            print(what, "->", names)
            assert any("colmap" in n for n in names), f"{what}: no colmap kernel among {names}"
            assert not _aten(names), f"{what}: aten / copy / fill launches {_aten(names)}"
            assert len(names) == 1, f"{what}: {len(names)} launches"


def test_backward_matches_f64_autograd_of_the_reference_chain(hip_lib, dev, golden):
    G = golden("g_constraints")
    flow = constraint_builder(G, device=dev).build_flow()
    mult = flow[2]._flow
    mult.set_philox_stream(21)
    gen = torch.Generator().manual_seed(5)
    w = [torch.randn(256, n, generator=gen) for n in (17, 17, 17, 9)]
    zs = [T(G[f"flow_z{k}"], dev).requires_grad_(True) for k in range(4)]
    *ys, d = flow(*zs)
    loss = sum((y * wk.to(dev)).sum() for y, wk in zip(ys, w))
    grads = torch.autograd.grad(loss, zs)
    # the reference's op chain in f64 on the CPU, with the sheaves the kernel drew
    z64 = [T(G[f"flow_z{k}"]).double().requires_grad_(True) for k in range(4)]
    free = torch.as_tensor(np.setdiff1d(np.arange(17), G["c_idx"]))
    b17 = torch.empty(256, 17, dtype=torch.float64)
    b17 = b17.index_copy(1, free, z64[0]).index_copy(1, T(G["c_idx"]), T(G["c_val"]).double().repeat(256, 1))
    m, shift = T(G["mults"]).double(), T(G["shifts"]).double()
    sheaves = torch.from_numpy(np.floor(_philox_u(mult, 256, 17, 0) * G["mults"].astype(np.float32))).double()
    t = (z64[2] + sheaves) / m
    t = (t + shift) % 1
    loc, scale = torch.zeros(17, dtype=torch.float64), torch.ones(17, dtype=torch.float64)
    loc[T(G["halpha"])], scale[T(G["halpha"])] = 0.5, 0.5
    t = loc + scale * t
    out64 = [b17, z64[1], t, z64[3]]
    assert float((ys[0].detach().cpu().double() - b17.detach()).abs().max()) < 1e-7
    g64 = torch.autograd.grad(sum((y * wk.double()).sum() for y, wk in zip(out64, w)), z64)
    for k, (a, b) in enumerate(zip(grads, g64)):
        assert torch.equal(a.cpu(), b.float()), f"gradient of tensor {k}"
    assert grads[0].shape == (256, 15)                   # the constrained columns contribute nothing
    # each flow alone, both directions: a copy, one multiplication or one division of the incoming gradient
    x = T(G["mult_x"], dev)[8:].contiguous()
    gy = torch.randn(x.shape, generator=gen)
    aff = bg.TorchTransform(torch.distributions.AffineTransform(T(G["aff_loc"], dev), T(G["aff_scale"], dev)), 1)
    sc = T(G["aff_scale"]).double()
    cases = [(bg.CircularShiftFlow(T(G["shifts"])).to(dev), False, gy.double()), (bg.CircularShiftFlow(T(G["shifts"])).to(dev), True, gy.double()),
             (bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev), False, gy.double() / m), (bg.IncreaseMultiplicityFlow(T(G["mults"])).to(dev), True, gy.double() * m),
             (aff, False, gy.double() * sc), (aff, True, gy.double() / sc)]
    for f, inverse, expect in cases:
        xr = x.clone().requires_grad_(True)
        y, d = f(xr, inverse=inverse)
        g, = torch.autograd.grad(y, xr, gy.to(dev))
        assert torch.equal(g.cpu(), expect.float()), f"{type(f).__name__}, inverse={inverse}"
        assert not d.requires_grad
    # a second derivative raises instead of returning a wrong one
    xr = x.clone().requires_grad_(True)
    y, _ = aff(xr)
    g, = torch.autograd.grad((y * y).sum(), xr, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), xr)


def test_range_check_counts_on_the_device(hip_lib, dev):
    for make in (lambda: bg.CircularShiftFlow(0.3), lambda: bg.IncreaseMultiplicityFlow(2)):
        for inverse in (False, True):
            f = make().to(dev)
            x = torch.full((70, 5), 0.5, device=dev)
            x[65, 2] = 1 + 5e-7
            with torch.no_grad():
                f(x, inverse=inverse)
                assert f.check_unit_interval() == 0
                x[65, 2] = 1.1
                f(x, inverse=inverse)                   # counted in the kernel; raised when the counter is polled ...
                with pytest.raises(ValueError):
                    f.check_unit_interval()
                assert f.check_unit_interval() == 0     # ... which resets it
                f.SYNC_RANGE_CHECK = True               # ... or in the call itself
                x[65, 2] = -0.1
                with pytest.raises(ValueError):
                    f(x, inverse=inverse)


def test_affine_logdet_lands_in_the_running_buffer(hip_lib, dev, golden):
    """inside a SequentialFlow pass the constant log-det is added by the kernel to the pass's one buffer: equal to the block-wise sum"""
    G = golden("g_constraints")
    aff = lambda: bg.TorchTransform(torch.distributions.AffineTransform(T(G["aff_loc"], dev), T(G["aff_scale"], dev)), 1)   # noqa: E731
    blocks = [bg.CircularShiftFlow(T(G["shifts"])).to(dev), aff(), bg.InverseFlow(aff()), aff(), bg.CircularShiftFlow(0.5).to(dev)]
    flow = bg.SequentialFlow(blocks)
    x = T(G["shift_x"], dev)
    with torch.no_grad():
        for inverse in (False, True):
            y, d = flow(x, inverse=inverse)
            flow.ACCUMULATE_IN_KERNELS = False
            y2, d2 = flow(x, inverse=inverse)
            flow.ACCUMULATE_IN_KERNELS = True
            total, z = torch.zeros(x.shape[0], 1, device=dev), x
            for b in (reversed(blocks) if inverse else blocks):
                z, dd = b(z, inverse=inverse)
                total = total + dd
            assert d.shape == (256, 1) and torch.equal(y, z) and torch.equal(y, y2)
            assert torch.equal(d, total) and torch.equal(d, d2)
            assert float(d[0].abs()) > 0.1
        # a zero-log-det map as the first writer zeroes the buffer; later ones leave it alone
        y, d = bg.SequentialFlow([blocks[0], blocks[4]])(x)
        assert bool((d == 0).all())


def test_outside_the_envelope_runs_the_torch_form(hip_lib, dev, golden):
    G = golden("g_constraints")
    f = bg.CircularShiftFlow(T(G["shifts"])).to(dev)
    x = T(G["shift_x"], dev)
    with torch.no_grad():
        y64, _ = f(x.double())
        assert y64.dtype == torch.float64
        yt, _ = f(x.t().contiguous().t())                 # non-contiguous rows
        assert same(yt, G["shift_fwd"])
        wide = torch.rand(64, 300, device=dev)
        yw, dw = bg.CircularShiftFlow(0.25).to(dev)(wide)
        assert torch.equal(yw, (wide + 0.25) % 1) and dw.shape == (64, 1)
        edge = torch.rand(130, 256, device=dev)           # the widest field of the envelope, a partial last tile
        ye, _ = bg.CircularShiftFlow(0.25).to(dev)(edge)
        assert torch.equal(ye, (edge + 0.25) % 1)
        with pytest.raises(ValueError):
            f(torch.full((4, 17), 1.1, device=dev).double())
