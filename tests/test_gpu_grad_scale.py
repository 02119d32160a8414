"""GPU (-m gpu): the hand-off of gradient tensors and their published maxima along the training backward.  Every producer
(bgk_rqs_backward in its register, packed and walked forms, the recompute backward, bgk_dense_backward_dx / bgk_mlp_backward_dx,
bgk_affine_backward, bgk_absmax) publishes 'the largest magnitude I wrote' as a device float; the consumers turn it into the power-of-two
scale of an f16 hi + lo split with a margin of 2 to the f16 maximum.  Section A: the published float IS the maximum of what was written
(bit equality), at every tile boundary, with the maximum in the first lane's element and in the partial tile's last float, under NaN
rows and poisoned padding.  Section B: per-element accuracy of the GEMM chain and the weight gradients when the rows of the cotangent
differ by up to 2^45 (per-sample KL cotangents with outlier rows), against an f64 chain and a bound derived from the design.
References and input builders: tests/grad_scale_common.py (checked on the CPU by test_host_grad_scale.py)."""
import numpy as np
import pytest
import torch

import grad_scale_common as gc
from test_gpu_parity import t
from test_gpu_round5 import _fields, _spline_layer

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def dev_max(x):
    """largest magnitude of a device tensor as torch computes it, NaNs skipped like the kernels' maxima"""
    a = x.detach().abs()
    return torch.where(torch.isnan(a), torch.zeros_like(a), a).max().reshape(1) if a.numel() else torch.zeros(1, device=x.device)


def assert_published(buf, x, what):
    want = dev_max(x)
    assert torch.equal(buf.reshape(1), want), f"{what}: published {float(buf):.9g}, largest magnitude written {float(want):.9g}"
    assert not bool(torch.signbit(buf).any())


def padded(a, dev, extra_rows=3, col_fill=gc.COL_FILL):
    """[B, w] device view of a longer and wider allocation: rows past the end 1e30, columns past the width NaN, row pitch > w and a
    multiple of 4 floats (the 16-byte pieces of bgk_dense_backward_dx stay aligned)"""
    a = np.asarray(a, np.float32)
    B, w = a.shape
    buf = np.full((B + extra_rows, (w // 4 + 2) * 4), gc.ROW_FILL, np.float32)
    buf[:B, w:] = col_fill
    buf[:B, :w] = a
    return t(buf, dev)[:B, :w]


def pitched(a, dev):
    """the same row pitch without the poison: zeros behind the width, no rows behind the batch"""
    return padded(a, dev, extra_rows=0, col_fill=0.0)


def padded_rows(a, dev, extra_rows=3):
    """[B, ...] leading rows of a longer allocation whose other rows are 1e30 (tensors a kernel takes without a row pitch)"""
    a = np.asarray(a, np.float32)
    buf = np.full((a.shape[0] + extra_rows,) + a.shape[1:], gc.ROW_FILL, np.float32)
    buf[:a.shape[0]] = a
    return t(buf, dev)[:a.shape[0]]


def canary(dev, B, w, ld=None, extra_rows=2):
    """(buffer [B + extra, ld] full of the canary value, its [B, w] view)"""
    buf = torch.full((B + extra_rows, ld or w), gc.CANARY, dtype=torch.float32, device=dev)
    return buf, buf[:B, :w]


def assert_canaries(buf, B, w, what):
    assert bool((buf[B:] == gc.CANARY).all()) and bool((buf[:B, w:] == gc.CANARY).all()), f"{what}: written past the batch or the width"


def bits(x):
    return x.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# A.1  bgk_rqs_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _pack_element_major(params, Kb, circ):
    """[B, P] in the reference's column order -> [B, d (3 K + 1)]: an element's widths | heights | slopes | slot in one run"""
    B, d = params.shape[0], len(circ)
    out = np.zeros((B, d * (3 * Kb + 1)), np.float32)
    cols = gc.element_columns(Kb, d, circ)
    for j in range(d):
        ok = cols[j] >= 0
        out[:, j * (3 * Kb + 1):(j + 1) * (3 * Kb + 1)][:, ok] = params[:, cols[j][ok]]
    return out


def _rqs_raw(dev, Kb, inverse, y, params, g_out, g_dl, absmax, packed, pad):
    """bgk_rqs_backward through the C ABI on buffers of the test's own: inputs as views of poisoned allocations (``pad``), outputs
    inside canaries.  Returns (g_y, g_params) views; raises if a canary was touched."""
    from bgflow_amd import _lib
    from bgflow_amd.utils import row_pitch
    from oracle.oracle import nc_slots
    circ = gc.CIRC7
    B, d = y.shape
    P = gc.n_params(Kb, circ)
    wrap = (lambda a: padded(a, dev)) if pad else (lambda a: t(a, dev))
    p_host = _pack_element_major(params, Kb, circ) if packed else params
    yd, pd, god = wrap(y), wrap(p_host), wrap(g_out)
    gld = padded_rows(g_dl, dev) if pad else t(g_dl, dev)
    slots = t(nc_slots(circ, d), dev)
    ldgp = row_pitch(P)
    gy_buf, gy = canary(dev, B, d, ld=d + (3 if pad else 0))
    gp_buf, gp = canary(dev, B, P, ld=ldgp)
    s = gc.SETTINGS
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_rqs_backward(
            _lib.ptr(yd), yd.stride(0), _lib.ptr(pd), pd.stride(0), P, _lib.ptr(slots), B, d, Kb, int(inverse), 0.0, 1.0, 0.0, 1.0,
            s["min_bin_width"], s["min_bin_height"], s["min_derivative"], 1, _lib.ptr(god), god.stride(0), _lib.ptr(gld),
            _lib.ptr(gy_buf), gy_buf.stride(0), _lib.ptr(gp_buf), ldgp, _lib.ptr(absmax), int(packed), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_rqs_backward")
    assert_canaries(gy_buf, B, d, "g_y")
    assert_canaries(gp_buf, B, P, "g_params")
    return gy, gp


RQS_FORMS = [("K8", 8, False), ("K32", 32, False), ("K6-walked", 6, False), ("K72-walked-compensated", 72, False), ("K8-element-major", 8, True)]


@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("form,Kb,packed", RQS_FORMS)
def test_rqs_backward_publishes_the_maximum_it_wrote(hip_lib, dev, form, Kb, packed, inverse, B):
    """d = 7, circular mask [1,0,1,1,0,0,1]: register instances (K = 8, 32), the walked form (K = 6; K = 72: compensated sums), and
    the element-major parameter layout of the fused forward.  Also the metamorphic form: the arithmetic is elementwise f32 without a
    scale, so a row's cotangents times 2^k scale that row's gradients bit-exactly and leave every other row alone."""
    from bgflow_amd.transformer import rqs_backward
    from oracle.oracle import nc_slots
    P = gc.n_params(Kb, gc.CIRC7)
    zero = lambda: torch.zeros(1, dtype=torch.float32, device=dev)      # noqa: E731

    def run(inputs, buf=None, pad=True):
        buf = zero() if buf is None else buf
        gy, gp = _rqs_raw(dev, Kb, inverse, *inputs, buf, packed, pad)
        return gy, gp, buf

    base = gc.rqs_absmax_inputs(Kb, B)
    gy0, gp0, buf = run(base)
    assert_published(buf, gp0, "moderate cotangents")
    assert bool(torch.isfinite(gp0).all()) and float(buf) > 0
    # the padding has no part in the result: the same inputs as plain contiguous tensors, and through the package's own wrapper
    gy1, gp1, buf1 = run(base, pad=False)
    assert same_bits(gy1, gy0) and same_bits(gp1, gp0) and torch.equal(buf1, buf)
    y, p, go, gl = base
    cfg = (Kb, inverse, 0.0, 1.0, 0.0, 1.0, gc.SETTINGS)
    buf2 = zero()
    gy2, gp2 = rqs_backward(t(y, dev), t(_pack_element_major(p, Kb, gc.CIRC7) if packed else p, dev), t(nc_slots(gc.CIRC7, 7), dev), cfg,
                            t(go, dev), t(gl, dev), absmax=buf2, packed_width=P if packed else None)
    assert same_bits(gy2, gy0) and same_bits(gp2, gp0) and torch.equal(buf2, buf)
    # the maximum in the first lane's element / in the last float of the (partial) last tile
    for put in (gc.put_maximum_first, gc.put_maximum_last):
        inputs = tuple(a.copy() for a in base)
        r, c = put(*inputs, Kb)
        _, gp, b = run(inputs)
        assert_published(b, gp, put.__name__)
        am = int(gp.abs().argmax())
        assert (am // P, am % P) == (r, c), f"{put.__name__}: the fixture's maximum sits at {(am // P, am % P)}, not {(r, c)}"
    # a buffer already larger than anything written stays as it is
    big = (2.0 * buf).clone()
    _, gp, b = run(base, buf=big.clone())
    assert torch.equal(b, big) and same_bits(gp, gp0)
    # all cotangents zero: +0.0 stays, exact zeros everywhere
    gy, gp, b = run((y, p, np.zeros_like(go), np.zeros_like(gl)))
    assert int(bits(b)) == 0 and not bool(gy.any()) and not bool(gp.any())
    # one row of the cotangents NaN: the maximum of the finite entries; every other row as without the poison
    r = B // 2
    go_n, gl_n = go.copy(), gl.copy()
    go_n[r], gl_n[r] = np.nan, np.nan
    gy, gp, b = run((y, p, go_n, gl_n))
    assert_published(b, gp, "a NaN row")
    keep = torch.arange(B, device=dev) != r
    assert same_bits(gy[keep], gy0[keep]) and same_bits(gp[keep], gp0[keep])
    assert bool(torch.isnan(gy[r]).all()) and bool(torch.isnan(gp[r]).any())
    # metamorphic: row r times 2^k
    for k in (-20, 7):
        go_k, gl_k = go.copy(), gl.copy()
        go_k[r] *= np.float32(2.0 ** k)
        gl_k[r] *= np.float32(2.0 ** k)
        gy, gp, b = run((y, p, go_k, gl_k))
        assert same_bits(gy[keep], gy0[keep]) and same_bits(gp[keep], gp0[keep])
        assert same_bits(gy[r], gy0[r] * 2.0 ** k) and same_bits(gp[r], gp0[r] * 2.0 ** k)
        assert_published(b, gp, f"row {r} times 2^{k}")


# ---------------------------------------------------------------------------------------------------------------------------------
# A.2  bgk_absmax
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("w", [1, 7, 425])
def test_absmax_of(hip_lib, dev, B, w):
    """bgk_absmax (dense.absmax_of: the scale source of gradients that came from outside the library): bit-equal to torch's maximum --
    in the first and in the last element, negative, through a row pitch with poisoned padding, NaNs skipped, zeros -> +0.0, None
    entries left at 0, and raised, never lowered"""
    from bgflow_amd import _lib
    from bgflow_amd.dense import absmax_of
    from bgflow_amd.utils import synth
    a = synth(40 + w, B, w)
    for where in ((0, 0), (B - 1, w - 1), (B // 2, w // 2)):
        for sign in (1.0, -1.0):
            b = a.copy()
            b[where] = sign * 77.5
            for x in (t(b, dev), padded(b, dev)):
                out = absmax_of(x, None, x)
                assert out.shape == (3,) and float(out[1]) == 0.0
                assert_published(out[0], x, f"maximum at {where}")
                assert float(out[0]) == 77.5 and torch.equal(out[0], out[2])
    b = a.copy()
    b[B // 2] = np.nan
    x = padded(b, dev)
    assert_published(absmax_of(x)[0], x, "a NaN row")
    z = absmax_of(torch.zeros(B, w, device=dev))
    assert int(bits(z)) == 0
    # the kernel raises what the buffer holds
    x = t(a, dev)
    for preset in (1e9, 1e-9):
        out = torch.full((1,), preset, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().bgk_absmax(_lib.ptr(x), x.stride(0), B, w, _lib.ptr(out), _lib.stream_ptr(dev)), "bgk_absmax")
        assert torch.equal(out, torch.maximum(dev_max(x), torch.full_like(out, preset)))


# ---------------------------------------------------------------------------------------------------------------------------------
# A.3  bgk_dense_backward_dx / bgk_mlp_backward_dx
# ---------------------------------------------------------------------------------------------------------------------------------
class _Conditioner:
    """DenseNet [n_in, H, H, P] with weights from hash_init_, its transposed operands and scale table, and the pre-activations of a
    plain f32 forward on a closed-form input"""

    def __init__(self, dev, P, d_c, periodic, act, H=128):
        import bgflow_amd as bg
        from bgflow_amd import _lib, packing
        from bgflow_amd.utils import hash_init_
        self.dev, self.P, self.d_c, self.periodic, self.act, self.H = dev, P, d_c, bool(periodic), act, H
        self.n_in = 2 * d_c if periodic else d_c
        net = hash_init_(bg.DenseNet([self.n_in, H, H, P], activation={1: torch.nn.SiLU(), 3: torch.nn.Tanh()}[act]))
        lins = [m for m in net._layers if isinstance(m, torch.nn.Linear)]
        self.W = [l.weight.detach().clone() for l in lins]
        self.b = [l.bias.detach().clone() for l in lins]
        es = [packing._h2_scale_exp(W, b) for W, b in zip(self.W, self.b)]
        self.cs = torch.tensor([v for e in es for v in (2.0 ** e, 2.0 ** -e)], dtype=torch.float32, device=dev)
        self.Wd = [W.to(dev) for W in self.W]
        self.bufs = {}
        packing._t_operand_bufs(self.bufs, P, self.n_in, dev)
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_pack_mlp_h2_t(_lib.ptr(self.Wd[0]), self.n_in, H, _lib.ptr(self.Wd[1]), H, _lib.ptr(self.Wd[2]), P, _lib.ptr(self.cs),
                                              _lib.ptr(self.bufs["T0"]), _lib.ptr(self.bufs["T1"]), _lib.ptr(self.bufs["T2"]), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_pack_mlp_h2_t")

    def inputs(self, B):
        from bgflow_amd.utils import synth
        x = synth(50 + self.P, B, self.d_c, uniform=True)
        z0, z1 = gc.conditioner_pre_activations(x, self.W[0].numpy(), self.b[0].numpy(), self.W[1].numpy(), self.b[1].numpy(), self.act, self.periodic)
        return x, z0, z1

    def dx_raw(self, g, absmax, z1, z0, x, B):
        """bgk_dense_backward_dx (H = 128) / bgk_mlp_backward_dx (H = 64) through the C ABI, outputs inside canaries"""
        from bgflow_amd import _lib
        dev, H = self.dev, self.H
        gz1_buf, gz1 = canary(dev, B, H)
        gz0_buf, gz0 = canary(dev, B, H)
        gx_buf, gx = canary(dev, B, self.d_c, ld=self.d_c + 3)
        T = self.bufs
        common = (_lib.ptr(x), x.stride(0), self.d_c, int(self.periodic), _lib.ptr(T["T0"]), _lib.ptr(T["T1"]), _lib.ptr(T["T2"]), _lib.ptr(self.cs),
                  self.act, B, _lib.ptr(gz1_buf), _lib.ptr(gz0_buf), None, None, _lib.ptr(gx_buf), gx_buf.stride(0), None, 0, _lib.ptr(absmax),
                  _lib.ptr(absmax[1:]), _lib.stream_ptr(dev))
        with torch.cuda.device(dev):
            if H == 128:
                st = _lib.lib().bgk_dense_backward_dx(_lib.ptr(g), g.stride(0), self.P, _lib.ptr(z1), _lib.ptr(z0), *common)
            else:
                st = _lib.lib().bgk_mlp_backward_dx(_lib.ptr(g), g.stride(0), self.P, _lib.ptr(z1), _lib.ptr(z0), H, *common)
        _lib.check(st, "bgk_dense_backward_dx")
        for buf, w, what in ((gz1_buf, H, "g_z1"), (gz0_buf, H, "g_z0"), (gx_buf, self.d_c, "g_x")):
            assert_canaries(buf, B, w, what)
        return gz1, gz0, gx


DX_SHAPES = [("P425-silu", 425, 17, 0, 1, 128), ("P225-periodic-tanh", 225, 17, 1, 3, 128), ("P425-tanh", 425, 17, 0, 3, 128),
             ("P225-periodic-silu", 225, 17, 1, 1, 128), ("P18-tanh-64-units", 18, 9, 0, 3, 64)]


@pytest.fixture(scope="module")
def conditioners(dev, hip_lib):
    return {name: _Conditioner(dev, P, d_c, per, act, H) for name, P, d_c, per, act, H in DX_SHAPES}


@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("shape", [s[0] for s in DX_SHAPES])
def test_dense_backward_dx_publishes_the_maxima_it_wrote(hip_lib, dev, conditioners, shape, B):
    """absmax[1] == max |g_z1| and absmax[2] == max |g_z0| of what the launch wrote, absmax[0] (read only) untouched -- the spline
    conditioners' shapes on bgk_dense_backward_dx, a 64-unit network on bgk_mlp_backward_dx (row pitch 64).  A NaN row of the
    gradient moves no scale and stays in its own MFMA column: every other row of every output is bit-identical to a clean run."""
    from bgflow_amd.dense import _dense_backward_dx, absmax_of
    c = conditioners[shape]
    x, z0, z1 = c.inputs(B)
    g = np.random.default_rng(B + c.P).standard_normal((B, c.P)).astype(np.float32) * np.float32(3e-4)

    def run(g_host, preset=(0.0, 0.0), pad=True):
        gd = padded(g_host, dev) if pad else pitched(g_host, dev)
        xd = padded(x, dev) if pad else t(x, dev)
        z1d, z0d = (padded_rows(z, dev) if pad else t(z, dev) for z in (z1, z0))
        buf = torch.cat([absmax_of(gd), torch.tensor(preset, dtype=torch.float32, device=dev)])
        before = buf.clone()
        gz1, gz0, gx = c.dx_raw(gd, buf, z1d, z0d, xd, B)
        assert torch.equal(buf[:1], before[:1]), "absmax[0] is read, not written"
        return gz1, gz0, gx, buf

    ref = run(g)
    assert_published(ref[3][1], ref[0], "g_z1")
    assert_published(ref[3][2], ref[1], "g_z0")
    assert all(bool(torch.isfinite(v).all()) for v in ref[:3]) and float(ref[3][1]) > 0 and float(ref[3][2]) > 0
    plain = run(g, pad=False)
    assert all(same_bits(a, b) for a, b in zip(plain, ref)), "poisoned padding changed a result"
    if c.H == 128:      # the package's own wrapper
        buf = torch.cat([absmax_of(pitched(g, dev)), torch.zeros(2, device=dev)])
        res = _dense_backward_dx(pitched(g, dev), t(z1, dev), t(z0, dev), t(x, dev), *c.Wd, c.cs, c.act, c.periodic, True, {}, want_h=False, absmax=buf)
        assert same_bits(res[0], ref[0]) and same_bits(res[1], ref[1]) and same_bits(res[4], ref[2]) and torch.equal(buf, ref[3])
    for r in (0, B - 1):                                   # the maximum in the first row / in the last row of the (partial) last tile
        gr = g.copy()
        gr[r] *= np.float32(2.0 ** 9)
        gz1, gz0, gx, buf = run(gr)
        assert_published(buf[1], gz1, f"g_z1, outlier row {r}")
        assert_published(buf[2], gz0, f"g_z0, outlier row {r}")
        assert int(gz1.abs().argmax()) // c.H == r and int(gz0.abs().argmax()) // c.H == r
    big = (2.0 * float(ref[3][1]), 2.0 * float(ref[3][2]))
    gz1, gz0, gx, buf = run(g, preset=big)
    assert torch.equal(buf[1:].cpu(), torch.tensor(big)) and same_bits(gz1, ref[0]) and same_bits(gz0, ref[1])
    gz1, gz0, gx, buf = run(np.zeros_like(g))
    assert not bool(bits(buf).any()) and not bool(gz1.any()) and not bool(gz0.any()) and not bool(gx.any())
    r = B // 2
    gn = g.copy()
    gn[r] = np.nan
    gz1, gz0, gx, buf = run(gn)
    assert_published(buf[1], gz1, "g_z1, a NaN row")
    assert_published(buf[2], gz0, "g_z0, a NaN row")
    keep = torch.arange(B, device=dev) != r
    for got, want in zip((gz1, gz0, gx), ref[:3]):
        assert same_bits(got[keep], want[keep]) and bool(torch.isnan(got[r]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# A.4  bgk_affine_backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("d,pv,inverse", [(18, 0, 0), (18, 0, 1), (17, 0, 0), (18, 1, 0), (17, 1, 1)])
def test_affine_backward_publishes_the_maxima_it_wrote(hip_lib, dev, B, d, pv, inverse):
    """g_mu_absmax == max |g_mu| and g_s_absmax == max |g_s|: the one-pass pair kernel (even d), the tile kernel (odd d, volume
    preservation)"""
    from bgflow_amd import _lib
    from bgflow_amd.utils import synth
    y, mu, s_raw, go, gl = synth(60, B, d), synth(61, B, d), synth(62, B, d, scale=2.0), synth(63, B, d), synth(64, B)
    la = torch.tensor([-0.3], device=dev)

    def run(go_h, gl_h, preset=(0.0, 0.0), pad=True):
        ins = [(padded(a, dev) if pad else t(a, dev)) for a in (y, mu, s_raw, go_h)]      # (the padded pitch is even: d = 18 keeps the pair kernel)
        gld = padded_rows(gl_h, dev) if pad else t(gl_h, dev)
        ld = (d // 4 + 2) * 4 if pad else d
        outs = [canary(dev, B, d, ld=ld) for _ in range(3)]
        bm, bs = (torch.tensor([v], dtype=torch.float32, device=dev) for v in preset)
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_affine_backward(
                _lib.ptr(ins[0]), ins[0].stride(0), _lib.ptr(ins[1]), ins[1].stride(0), _lib.ptr(ins[2]), ins[2].stride(0), _lib.ptr(la), pv, 0,
                inverse, B, d, _lib.ptr(ins[3]), ins[3].stride(0), _lib.ptr(gld), _lib.ptr(outs[0][0]), ld, _lib.ptr(outs[1][0]), ld,
                _lib.ptr(outs[2][0]), ld, None, _lib.ptr(bm), _lib.ptr(bs), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_affine_backward")
        for (buf, _), what in zip(outs, ("g_y", "g_mu", "g_s")):
            assert_canaries(buf, B, d, what)
        return outs[0][1], outs[1][1], outs[2][1], bm, bs

    ref = run(go, gl)
    assert_published(ref[3], ref[1], "g_mu")
    assert_published(ref[4], ref[2], "g_s")
    plain = run(go, gl, pad=False)
    assert all(same_bits(a, b) for a, b in zip(plain, ref))
    for r in (0, B - 1):
        go_r, gl_r = go.copy(), gl.copy()
        go_r[r] *= np.float32(2.0 ** 9)
        gl_r[r] *= np.float32(2.0 ** 9)
        _, gm, gs, bm, bs = run(go_r, gl_r)
        assert_published(bm, gm, f"g_mu, outlier row {r}")
        assert_published(bs, gs, f"g_s, outlier row {r}")
        assert int(gm.abs().argmax()) // d == r
    big = (2.0 * float(ref[3]), 2.0 * float(ref[4]))
    _, gm, gs, bm, bs = run(go, gl, preset=big)
    assert (float(bm), float(bs)) == big and same_bits(gm, ref[1]) and same_bits(gs, ref[2])
    gy, gm, gs, bm, bs = run(np.zeros_like(go), np.zeros_like(gl))
    assert int(bits(bm)) == 0 and int(bits(bs)) == 0 and not bool(gy.any()) and not bool(gm.any()) and not bool(gs.any())
    r = B // 2
    go_n, gl_n = go.copy(), gl.copy()
    go_n[r], gl_n[r] = np.nan, np.nan
    gy, gm, gs, bm, bs = run(go_n, gl_n)
    assert_published(bm, gm, "g_mu, a NaN row")
    assert_published(bs, gs, "g_s, a NaN row")
    keep = torch.arange(B, device=dev) != r
    for got, want in zip((gy, gm, gs), ref[:3]):
        assert same_bits(got[keep], want[keep])


@pytest.mark.parametrize("B", [1, 33, 257])
@pytest.mark.parametrize("inverse", [False, True])
def test_affine_layer_backward_hands_its_maxima_on(hip_lib, dev, monkeypatch, inverse, B):
    """The same two producers through the package's own calls (dense._affine_train_backward: bgk_affine_backward, then per network
    dense._affine_net_backward: bgk_mlp_backward_dx on [B, 64] arrays) inside an affine coupling under autograd -- 64-unit Tanh
    networks, 40 transformed dims (outside the one-launch kernels' envelope).  What bgk_affine_backward published for a network is the
    maximum of the gradient that network's chain then reads; what the chain raised behind it equals, bit for bit, what the kernel
    publishes and writes when called through the C ABI on the wrapper's own operands and buffers, inside canaries."""
    from bgflow_amd import dense, _lib
    from test_gpu_round6 import _affine_layer
    from bgflow_amd.utils import synth
    n_c, d = 9, 40
    flow = _affine_layer(n_c, (64, 64), d, (torch.nn.Tanh, torch.nn.Tanh)).to(dev)
    calls = []
    real = dense._affine_net_backward

    def spy(e, plan, g_net, ldg, z1, z0, x2, ldc, absmax, *rest):
        before = absmax.clone()
        res = real(e, plan, g_net, ldg, z1, z0, x2, ldc, absmax, *rest)
        calls.append(dict(e=e, plan=plan, g_net=g_net, ldg=ldg, z1=z1, z0=z0, x2=x2, ldc=ldc, before=before, after=absmax.clone()))
        return res
    monkeypatch.setattr(dense, "_affine_net_backward", spy)
    xg, yg = t(synth(91, B, n_c), dev).requires_grad_(True), t(synth(92, B, d), dev).requires_grad_(True)
    _, out, dl = flow(xg, yg, inverse=inverse)
    torch.autograd.backward([out, dl], [t(synth(93, B, d), dev), t(synth(94, B, 1), dev)])
    assert len(calls) == 2, "shift and scale network, each through dense._affine_net_backward"
    for c in calls:
        plan, e = c["plan"], c["e"]
        assert plan["ldz"] == 64 and not plan["periodic"]
        g = c["g_net"][:, :d]
        assert_published(c["before"][0], g, "bgk_affine_backward's maximum of a network's output gradient")
        assert not bool(bits(c["before"][1:]).any()) and torch.equal(c["after"][:1], c["before"][:1])
        gz1_buf, gz1 = canary(dev, B, 64)
        gz0_buf, gz0 = canary(dev, B, 64)
        buf = c["before"].clone()
        T = e["tbufs"]
        with torch.cuda.device(dev):
            st = _lib.lib().bgk_mlp_backward_dx(
                _lib.ptr(c["g_net"]), c["ldg"], d, _lib.ptr(c["z1"]), _lib.ptr(c["z0"]), 64, _lib.ptr(c["x2"]), c["ldc"], plan["d_c"], 0,
                _lib.ptr(T["T0"]), _lib.ptr(T["T1"]), _lib.ptr(T["T2"]), _lib.ptr(e["cs"]), e["act"], B, _lib.ptr(gz1_buf), _lib.ptr(gz0_buf),
                None, None, None, plan["d_c"], None, 0, _lib.ptr(buf), _lib.ptr(buf[1:]), _lib.stream_ptr(dev))
        _lib.check(st, "bgk_mlp_backward_dx")
        assert_canaries(gz1_buf, B, 64, "g_z1")
        assert_canaries(gz0_buf, B, 64, "g_z0")
        assert torch.equal(buf, c["after"]), "the wrapper's chain and the C ABI call publish the same maxima"
        assert_published(buf[1], gz1, "g_z1")
        assert_published(buf[2], gz0, "g_z0")


def _rc_raw(lc, y, z1, P, nc_dev, g_out, g_dlogp, absmax):
    """bgk_coupling_rqs_dense_h2_backward through the C ABI with the arguments dense._rqs_backward_recompute builds, outputs inside
    canaries.  Returns (g_y, g_params) views."""
    from bgflow_amd import _lib
    from bgflow_amd.utils import row_pitch
    n_bins, inverse, left, right, bottom, top, s = lc.rcfg
    A2, c2, circ_mask = lc.recompute
    y2, ldy = _lib.rowmajor(y)
    B, d = y2.shape
    dev = y.device
    g_out2, g_dl = g_out.reshape(-1, d).contiguous(), g_dlogp.reshape(-1).contiguous()
    assert z1.is_contiguous() and z1.shape == (B, 128)
    ldgp = row_pitch(P)
    gy_buf, gy = canary(dev, B, d)
    gp_buf, gp = canary(dev, B, P, ld=ldgp)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_coupling_rqs_dense_h2_backward(
            _lib.ptr(z1), _lib.ptr(A2), c2, _lib.ptr(lc.cs), 128, lc.act, _lib.ptr(y2), ldy, B, d, n_bins, P, circ_mask, int(inverse),
            left, right, bottom, top, s["min_bin_width"], s["min_bin_height"], s["min_derivative"],
            int(s.get("enable_identity_init", False)), _lib.ptr(g_out2), d, _lib.ptr(g_dl), _lib.ptr(gy_buf), d, _lib.ptr(gp_buf), ldgp,
            _lib.ptr(absmax), _lib.stream_ptr(dev))
    _lib.check(st, "bgk_coupling_rqs_dense_h2_backward")
    assert_canaries(gy_buf, B, d, "g_y")
    assert_canaries(gp_buf, B, P, "g_params")
    return gy, gp


# ---------------------------------------------------------------------------------------------------------------------------------
# A.5  the recompute backward (bgk_fused2.hip) and the chain behind it, inside a fused spline coupling layer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("option", [1, 2])
def test_recompute_backward_and_its_chain_publish_their_maxima(hip_lib, dev, monkeypatch, option, B):
    """A BONDS-on-ANGLES spline coupling (d = 17, every dim with a slot) under autograd with per-sample cotangents: the [3] floats the
    layer's backward hands from bgk_coupling_rqs_dense_h2_backward to bgk_dense_backward_dx to bgk_dense_weight_grad equal the maxima
    of g_params, g_z1 and g_z0 as written.  bgk_set_option(3, 1) (deterministic VJP forms): absmax[0] also equals the maximum of the
    saved-parameter path's g_params (bgk_rqs_backward) bit for bit; (3, 2) (shipped hardware forms): to 2e-4, the bound of
    test_spline_backward_with_recomputed_parameters_equals_the_saved_parameters."""
    from bgflow_amd import dense, transformer, _lib
    layer = _spline_layer(dev, what="BONDS", on="ANGLES")
    ti = int(layer.transformed_indices[0])
    d = 17
    seen = {}
    real_rc, real_dx, real_rqs = dense._rqs_backward_recompute, dense._dense_backward_dx, transformer.rqs_backward

    def spy_rc(lc, y, z1, P, nc_dev, g_out, g_dlogp, absmax):
        res = real_rc(lc, y, z1, P, nc_dev, g_out, g_dlogp, absmax)
        seen.update(g_p=res[1], g_y=res[0], absmax=absmax, after_rc=absmax.clone(), rc_args=(lc, y, z1, P, nc_dev, g_out, g_dlogp))
        return res

    def spy_rqs(*a, **kw):
        res = real_rqs(*a, **kw)
        seen.update(g_p=res[1], absmax=kw.get("absmax"), after_rc=kw["absmax"].clone())
        return res

    def spy_dx(*a, **kw):
        res = real_dx(*a, **kw)
        seen.update(g_z1=res[0], g_z0=res[1])
        return res
    monkeypatch.setattr(dense, "_rqs_backward_recompute", spy_rc)
    monkeypatch.setattr(transformer, "rqs_backward", spy_rqs)
    monkeypatch.setattr(dense, "_dense_backward_dx", spy_dx)

    def run(g_out, g_dl, recompute=True):
        monkeypatch.setattr(dense, "RECOMPUTE_PARAMS", recompute)
        old = _lib.lib().bgk_set_option(3, option)
        try:
            for p in layer.parameters():
                p.grad = None
            xs = _fields(dev, B)
            *outs, dl = layer(*xs)
            assert layer.transformer._fused_cache.get("params_recompute") is recompute
            seen.clear()
            torch.autograd.backward([outs[ti], dl], [t(g_out, dev), t(g_dl, dev)[:, None]])
        finally:
            _lib.lib().bgk_set_option(3, old)
        return dict(seen)

    from bgflow_amd.utils import synth
    go, gl = synth(70, B, d), synth(71, B)

    def check(s, what):
        assert torch.equal(s["after_rc"][1:], torch.zeros(2, device=dev)), "the spline backward writes absmax[0] alone"
        assert_published(s["absmax"][0], s["g_p"], what + ": g_params")
        assert_published(s["absmax"][1], s["g_z1"], what + ": g_z1")
        assert_published(s["absmax"][2], s["g_z0"], what + ": g_z0")

    ref = run(go, gl)
    check(ref, "moderate cotangents")
    saved = run(go, gl, recompute=False)
    check(saved, "saved parameters")
    if option == 1:
        assert same_bits(ref["g_p"], saved["g_p"]) and torch.equal(ref["absmax"], saved["absmax"])
    else:
        assert abs(float(ref["absmax"][0]) - float(dev_max(saved["g_p"]))) <= 2e-4 * float(dev_max(saved["g_p"]))
    for r in (0, B - 1):
        go_r, gl_r = go.copy(), gl.copy()
        go_r[r] *= np.float32(2.0 ** 9)
        gl_r[r] *= np.float32(2.0 ** 9)
        s = run(go_r, gl_r)
        check(s, f"outlier row {r}")
        assert int(s["g_p"].abs().argmax()) // s["g_p"].shape[1] == r
    s = run(np.zeros_like(go), np.zeros_like(gl))
    assert not bool(bits(s["absmax"]).any()) and not any(bool(s[k].any()) for k in ("g_p", "g_y", "g_z1", "g_z0"))
    r = B // 2
    go_n, gl_n = go.copy(), gl.copy()
    go_n[r], gl_n[r] = np.nan, np.nan
    s = run(go_n, gl_n)
    check(s, "a NaN row")
    keep = torch.arange(B, device=dev) != r
    for k in ("g_p", "g_y", "g_z1", "g_z0"):
        assert same_bits(s[k][keep], ref[k][keep]), k
    # the kernel itself with the wrapper's arguments: poisoned padding (the input as a view of a wider allocation, the pre-activations
    # as the leading rows of a longer one), canaries behind both outputs; and a buffer that already holds more, which stays
    lc, y, z1, P, nc_dev, g_out, g_dlogp = ref["rc_args"]
    old = _lib.lib().bgk_set_option(3, option)
    try:
        buf = torch.zeros(3, device=dev)
        gy, gp = _rc_raw(lc, padded(y.detach().cpu().numpy(), dev), padded_rows(z1.cpu().numpy(), dev), P, nc_dev, g_out, g_dlogp, buf)
        big = torch.tensor([2.0 * float(ref["after_rc"][0]), 0.0, 0.0], device=dev)
        preset = big.clone()
        gy_b, gp_b = _rc_raw(lc, y.detach(), z1, P, nc_dev, g_out, g_dlogp, preset)
    finally:
        _lib.lib().bgk_set_option(3, old)
    assert same_bits(gy, ref["g_y"]) and same_bits(gp, ref["g_p"]) and torch.equal(buf, ref["after_rc"])
    assert same_bits(gy_b, ref["g_y"]) and same_bits(gp_b, ref["g_p"]) and torch.equal(preset, big)


@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("option", [1, 2])
@pytest.mark.parametrize("inverse", [False, True])
def test_recompute_backward_maximum_in_the_first_element_and_in_the_last_slot(hip_lib, dev, monkeypatch, inverse, option, B):
    """The LDS VJP folds the slot's gradient into its maximum in code of its own (bgk_rqs_vjp_element_lds).  d = 7, mask
    [1,0,1,1,0,0,1]: the output layer of the conditioner with zero weights and put_maximum_first's / put_maximum_last's parameter
    row as bias emits that row for every sample; only the fixture's row carries a cotangent, so the launch's largest gradient is the
    first float of g_params / the slot of the last non-circular dim in the last row of the partial tile -- published bit for bit,
    canaries behind the outputs intact."""
    import bgflow_amd as bg
    from bgflow_amd import dense, _lib
    from bgflow_amd.utils import hash_init_, synth
    Kb, d, d_c = 8, 7, 9
    P = gc.n_params(Kb, gc.CIRC7)
    seen = {}
    real_rc = dense._rqs_backward_recompute

    def spy_rc(*a):
        res = real_rc(*a)
        seen.update(args=a[:7], g_p=res[1], absmax=a[7])
        return res
    monkeypatch.setattr(dense, "_rqs_backward_recompute", spy_rc)
    monkeypatch.setattr(dense, "RECOMPUTE_PARAMS", True)
    x = t(synth(32, B, d_c, uniform=True), dev)
    for put in (gc.put_maximum_first, gc.put_maximum_last):
        y, p, go, gl = gc.rqs_absmax_inputs(Kb, B)
        r, c = put(y, p, go, gl, Kb)
        g_out, g_dl = np.zeros_like(go), np.zeros_like(gl)
        g_out[r] = go[r]
        net = bg.DenseNet([d_c, 128, 128, P], activation=torch.nn.SiLU())
        tr = hash_init_(bg.ConditionalSplineTransformer(net, is_circular=torch.tensor(gc.CIRC7))).to(dev)
        with torch.no_grad():
            net._layers[-1].weight.zero_()
            net._layers[-1].bias.copy_(torch.as_tensor(p[r]))
        old = _lib.lib().bgk_set_option(3, option)
        try:
            yd = t(y, dev).requires_grad_(True)
            out, dl = tr(x, yd, inverse=inverse)
            assert tr._fused_cache.get("params_recompute") is True, "the fused training forward must have run without saving parameters"
            torch.autograd.backward([out, dl], [t(g_out, dev), t(g_dl, dev)[:, None]])
            assert_published(seen["absmax"][0], seen["g_p"], put.__name__)
            buf = torch.zeros(3, device=dev)
            gy, gp = _rc_raw(*seen["args"], buf)
        finally:
            _lib.lib().bgk_set_option(3, old)
        assert same_bits(gp, seen["g_p"]) and same_bits(gy, yd.grad)
        assert_published(buf[0], gp, put.__name__ + " (C ABI)")
        assert not bool(bits(buf[1:]).any())
        am = int(gp.abs().argmax())
        assert (am // P, am % P) == (r, c), f"{put.__name__}: the fixture's maximum sits at {(am // P, am % P)}, not {(r, c)}"
        keep = torch.arange(B, device=dev) != r
        assert not bool(gp[keep].any()) and not bool(gy[keep].any())


# ---------------------------------------------------------------------------------------------------------------------------------
# B  per-element accuracy of the GEMM chain under mixed row scales
# ---------------------------------------------------------------------------------------------------------------------------------
def _chained_cotangent(dev, P, d, buf):
    """g_params [97, P] with the mixed row scales, written by bgk_rqs_backward (which publishes its maximum into buf[0]): spline
    cotangents are linear in (g_out, g_dlogp), so row r's times 2^-s[r] scale the row"""
    from bgflow_amd.transformer import rqs_backward
    from bgflow_amd.utils import synth
    B = gc.B_MIXED
    circ = np.zeros(d, bool)
    assert gc.n_params(8, circ) == P
    sc = (2.0 ** -gc.mixed_row_exponents()).astype(np.float32)
    y, p = synth(81, B, d, uniform=True), synth(82, B, P, scale=0.7)
    go, gl = synth(83, B, d) * sc[:, None], synth(84, B) * sc
    slots = torch.arange(d, dtype=torch.int32, device=dev)
    _, g_p = rqs_backward(t(y, dev), t(p, dev), slots, (8, False, 0.0, 1.0, 0.0, 1.0, gc.SETTINGS), t(go, dev), t(gl, dev), absmax=buf)
    return g_p


@pytest.mark.parametrize("source", ["absmax_of", "rqs_backward"])
@pytest.mark.parametrize("shape", [s[0] for s in DX_SHAPES if s[5] == 128])
def test_dx_chain_and_weight_grads_per_row_under_mixed_row_scales(hip_lib, dev, conditioners, shape, source):
    """bgk_dense_backward_dx and, fed with its outputs and its published maxima, bgk_dense_weight_grad, B = 97 (three 32-row tiles and a
    row), rows of the cotangent at 2^0 .. 2^-45 of the largest (grad_scale_common.mixed_row_exponents) -- absmax[0] measured by
    bgk_absmax on a random cotangent, or published by bgk_rqs_backward in a chained run.  Every element of g_z1, g_z0 and g_x against the
    f64 chain within the design's bound (grad_scale_common.gemm_bound: the f16 hi + lo split under the tensor's / the 32-row tile's
    power-of-two scale, 22-bit weights, f32 accumulation, the bound carried from stage to stage); rows 5 and 6 (2^-38, 2^-45 below the
    maximum: the absolute floor) by the same inequality, and finite.  Weight gradients: relative L2 per tensor against f64 g^T h within 8
    times (22 against 24 bits, times a margin of 2) what a plain f32 evaluation reaches; two calls bit-equal.
    MI355X, worst error / bound over the four conditioners and both sources: g_z1 0.029, g_z0 0.003, g_x < 0.001 (the rows at 2^-30: the same);
    weight gradients 0.7 - 5.0e-7 relative L2 where plain f32 reaches 1.1 - 2.0e-7.  That bound is a worst case over signs and far from tight: with the
    tensor's maximum in place of the tile's in the second GEMM (a wrong kernel built for the purpose) g_z0 rises to 0.30 and stays
    inside it.  Hence the second GEMM on its own, tile by tile, relative L2 against the f64 stage from the kernel's own g_z1 within 8
    times a plain f32 evaluation: measured 1.2 - 2.7e-7 where plain f32 reaches 1.7 - 3.2e-7, every tile alike; the wrong kernel: 1.08 on
    the rows at 2^-30."""
    from bgflow_amd.dense import _dense_backward_dx, _dense_weight_grad, absmax_of
    c = conditioners[shape]
    B = gc.B_MIXED
    x, z0, z1 = c.inputs(B)
    buf = torch.zeros(3, dtype=torch.float32, device=dev)
    if source == "absmax_of":
        g_d = padded(gc.mixed_cotangent(c.P, seed=c.P), dev)
        buf[:1] = absmax_of(g_d)
    else:
        g_d = _chained_cotangent(dev, c.P, {425: 17, 225: 9}[c.P], buf)
    assert_published(buf[0], g_d, "the cotangent's maximum")
    g = g_d.cpu().numpy()
    s = gc.mixed_row_exponents()
    row_max = np.abs(g).max(1)
    assert np.all(row_max <= 2.0 ** (6.0 - s) * row_max.max()) and row_max[5] < 2.0 ** -30 * row_max.max()      # the rows sit where the case wants them
    xd, z1d, z0d = t(x, dev), t(z1, dev), t(z0, dev)
    bufs = {}
    g_z1, g_z0, _, _, g_x = _dense_backward_dx(g_d, z1d, z0d, xd, *c.Wd, c.cs, c.act, c.periodic, True, bufs, want_h=False, absmax=buf)
    assert_published(buf[1], g_z1, "g_z1")
    assert_published(buf[2], g_z0, "g_z0")
    ref = gc.dx_chain_reference(g, float(buf[0]), z1, z0, x, *(W.numpy() for W in c.W), c.act, c.periodic)
    worst = {}
    for name, got in (("g_z1", g_z1), ("g_z0", g_z0), ("g_x", g_x)):
        got = got.cpu().numpy()
        want, bound = ref[name]
        ratio = np.abs(got.astype(np.float64) - want) / bound
        worst[name] = float(ratio.max())
        print(f"{shape} / {source}: {name} worst error / bound {ratio.max():.3f} at row {int(ratio.max(1).argmax())}; rows 5, 6: "
              f"{ratio[5].max():.3f}, {ratio[6].max():.3f}; per row exponent "
              f"{ {int(e): round(float(ratio[s == e].max()), 3) for e in np.unique(s)} }")
        assert np.isfinite(got).all()
    assert max(worst.values()) <= 1.0, worst
    # Inside the design's stated range the bound above is far from tight (it is a worst case over signs; the sums are random walks).
    # The second GEMM on its own, tile by tile: every element of a tile is scaled by the TILE's maximum, so a tile 2^-30 below the
    # tensor's largest is as accurate, relative to itself, as the first one.  Reference: the f64 stage from the kernel's own g_z1;
    # yardstick: a plain f32 evaluation of the same stage, as for the weight gradients (22 against 24 bits, times a margin of 2).
    gz1_k = g_z1.cpu().numpy()
    d0 = gc.act_f64(z0, c.act)[1]
    want = (gz1_k.astype(np.float64) @ c.W[1].numpy().astype(np.float64)) * d0
    plain = (torch.as_tensor(gz1_k) @ c.W[1]).numpy() * d0.astype(np.float32)
    got = g_z0.cpu().numpy().astype(np.float64)
    for b0 in range(0, B, 32):
        if b0 == 0:
            rows = np.setdiff1d(np.arange(32), [5, 6])          # (rows 5, 6 sit 2^-38 / 2^-45 below their tile's maximum: outside the range)
        elif b0 == 32:
            rows = np.arange(32, 33)                            # (row 32 governs tile 1; its other rows sit 2^-20 below it)
        else:
            rows = np.arange(b0, min(b0 + 32, B))
        n = np.linalg.norm(want[rows])
        e_k, e_32 = np.linalg.norm(got[rows] - want[rows]) / n, np.linalg.norm(plain[rows].astype(np.float64) - want[rows]) / n
        print(f"{shape} / {source}: second GEMM alone, rows {rows[0]}..{rows[-1]}: relative L2 {e_k:.2e}, plain f32 {e_32:.2e}")
        assert e_k <= 8.0 * e_32, f"rows {rows[0]}..{rows[-1]}: relative L2 {e_k:.2e} against f64, a plain f32 evaluation reaches {e_32:.2e}"
    # weight gradients from the chain's outputs and its published maxima
    need = [True] * 8
    res = _dense_weight_grad(g_d, g_z1, g_z0, z1d, z0d, xd, c.periodic, c.n_in, need, bufs, h_act=c.act, absmax=buf)
    res2 = _dense_weight_grad(g_d, g_z1, g_z0, z1d, z0d, xd, c.periodic, c.n_in, need, bufs, h_act=c.act, absmax=buf)
    assert all(same_bits(a, b) for a, b in zip(res, res2)), "deterministic"
    want, f32_err = gc.weight_grad_reference(g, g_z1.cpu().numpy(), g_z0.cpu().numpy(), z1, z0, x, c.act, c.periodic)
    for got, w, e32, name in zip(res, want, f32_err, ("gW0", "gb0", "gW1", "gb1", "gW2", "gb2")):
        err = float(np.linalg.norm(got.cpu().numpy().astype(np.float64) - w) / np.linalg.norm(w))
        print(f"{shape} / {source}: {name} relative L2 {err:.2e}, plain f32 {e32:.2e}")
        assert err <= 8.0 * e32, f"{name}: relative L2 {err:.2e} against f64, a plain f32 evaluation reaches {e32:.2e}"
