"""Operand layouts of the conditioner GEMMs: the contract between the host and the coupling / layer kernels, written once.

The torch packers here are the layouts' reference (tests/test_host_packing.py pins their output bit for bit) and what the plans of
dense.py call for the shapes that have no device-side packer; ``pack_dense_for_fused_h2_device`` / ``pack_linear_layer_device`` are the
device-side twins.  Nothing in this module knows about transformers, plans or module switches.
"""
import numpy as np
import torch

from . import _lib

# ---- MFMA operand packing for bgk_coupling_rqs_dense ------------------------------------------------
# One k-step of the f32 MFMA (v_mfma_f32_32x32x2_f32, A = weights) over 4 output tiles consumes, per
# lane l (i = l & 31, h = l >> 5), the four values W[32*m + i][k(step, h)], m = 0..3: stored as one
# float4 -> a packed layer is [steps + 1][64 lanes][4] floats; the extra last step carries the bias in
# the lower half-wave (A = bias, B = 1.0) and zeros in the upper one.
#   layer 0 (input from LDS, natural order):            k(t, h) = 2 t + h
#   hidden layers (input = accumulator registers):      k(16 kb + r, h) = 32 kb + (r & 3) + 8 (r >> 2) + 4 h
_LANE_I = torch.arange(64) & 31
_LANE_H = torch.arange(64) >> 5


def _pack_steps(W, bias, k_of_step):
    """W [128, n_in] (rows = output features), k_of_step [S, 2] (k index for half-wave 0 / 1, -1 = none)"""
    S = k_of_step.shape[0]
    dev = W.device
    rows = (32 * torch.arange(4, device=dev)[None, None, :] + _LANE_I.to(dev)[None, :, None]).expand(S, 64, 4)
    kk = k_of_step.to(dev)[:, _LANE_H.to(dev)][:, :, None].expand(S, 64, 4)
    vals = W[rows.reshape(-1), kk.clamp_min(0).reshape(-1)].reshape(S, 64, 4)
    vals = torch.where(kk >= 0, vals, torch.zeros_like(vals))
    bstep = torch.zeros(1, 64, 4, dtype=W.dtype, device=dev)
    bstep[0, :32, :] = bias.reshape(4, 32).t()
    return torch.cat([vals, bstep], dim=0).contiguous()


def _k_natural(n_in):
    T = ((n_in + 1) // 2 + 3) & ~3          # k-steps padded to a multiple of 4 (zero weights)
    k = torch.arange(2 * T).reshape(T, 2)
    return torch.where(k < n_in, k, torch.full_like(k, -1))


def _k_hidden():
    s = torch.arange(64)
    kb, r = s // 16, s % 16
    k0 = 32 * kb + (r & 3) + 8 * (r >> 2)
    return torch.stack([k0, k0 + 4], dim=1)


def _src_col_table(d, n_bins, nc_slot_host, device, row_order=1):
    """packed row -> source row of the output layer (-1 = padding) in row order ``row_order`` (bgk_pack_rqs_columns_v)"""
    ncp = _lib.lib().bgk_pack_rqs_columns_v(d, n_bins, None, row_order, None, None)
    if ncp <= 0:
        raise ValueError(f"no row order {row_order} for {n_bins} bins")
    src = np.empty(ncp, dtype=np.int32)
    slots = np.ascontiguousarray(nc_slot_host, dtype=np.int32)
    _lib.lib().bgk_pack_rqs_columns_v(d, n_bins, slots.ctypes.data, row_order, src.ctypes.data, None)
    return torch.as_tensor(src, device=device)


def rqs_row_perm(row_order):
    """[128] int32: position within a 128-row chunk of row order ``row_order`` -> row of order 1 within the chunk (-1 = unused)"""
    perm = np.empty(128, dtype=np.int32)
    if _lib.lib().bgk_pack_rqs_columns_v(1, 8, None, row_order, None, perm.ctypes.data) <= 0:
        raise ValueError(f"no row order {row_order}")
    return perm


def _gather_rows(W, b, src_t):
    """rows of the output layer (= reference params columns) regrouped per transformed dim by the table ``src_t`` (-1: a zero row)"""
    src_t = src_t.to(torch.int64)
    Wr = torch.where(src_t[:, None] >= 0, W[src_t.clamp_min(0)], torch.zeros((), dtype=W.dtype, device=W.device))
    br = torch.where(src_t >= 0, b[src_t.clamp_min(0)], torch.zeros((), dtype=b.dtype, device=b.device))
    return Wr, br


def pack_dense_for_fused(linears, nc_slot_host, d, n_bins):
    """Pack the three Linear layers of a DenseNet([n_in, 128, 128, P]) for bgk_coupling_rqs_dense.
    Returns (W0p, W1p, W2p) float32 device tensors."""
    l0, l1, l2 = linears
    W0p = _pack_steps(l0.weight.detach().float(), l0.bias.detach().float(), _k_natural(l0.in_features))
    W1p = _pack_steps(l1.weight.detach().float(), l1.bias.detach().float(), _k_hidden())
    W2r, b2r = _gather_rows(l2.weight.detach().float(), l2.bias.detach().float(), _src_col_table(d, n_bins, nc_slot_host, l2.weight.device))
    chunks = [_pack_steps(W2r[c * 128:(c + 1) * 128], b2r[c * 128:(c + 1) * 128], _k_hidden()) for c in range(W2r.shape[0] // 128)]
    return W0p, W1p, torch.cat(chunks, dim=0).contiguous()


# ---- split-f16 operand packing for bgk_coupling_rqs_dense_h2 ---------------------------------------
# v = hi + lo with hi = rne_f16(v), lo = rne_f16(v - hi); weights are first scaled by 2^s (exact) so that
# max(|W|, |b|) lands in [2^14, 2^15).  One 1 KiB block = 64 lanes x 8 f16; block(s, m, p) = (s*4 + m)*2 + p
# holds, for lane l = 32 kb + i, W'[32 m + i][k(s, kb, e)], e = 0..7, part p; after the S k16-steps follow 4
# bias blocks (lanes < 32: {b_hi, b_lo, 0, ...}).  See bgk_fused.hip (coupling_rqs_dense_h2_kernel).


def _h2_scale_exp(*tensors):
    m = max(float(t.abs().max()) for t in tensors if t.numel())
    if not np.isfinite(m) or m <= 0.0:
        return 0
    return int(np.clip(np.floor(np.log2(32768.0 / m)), -16, 24))


def _h2_split(v):
    hi = v.to(torch.float16)
    lo = (v - hi.to(torch.float32)).to(torch.float16)
    return hi, lo


def _h2_k_natural(S):
    s, kb, e = torch.meshgrid(torch.arange(S), torch.arange(2), torch.arange(8), indexing="ij")
    return 16 * s + 8 * kb + e


def _h2_k_hidden(HT=4):
    s, kb, e = torch.meshgrid(torch.arange(2 * HT), torch.arange(2), torch.arange(8), indexing="ij")
    return 32 * (s >> 1) + (e & 3) + 8 * (2 * (s & 1) + (e >> 2)) + 4 * kb


def _pack_h2(Ws, bs, kidx, NT=4):
    """Ws [32 NT, Kdim] scaled f32 weights, bs [32 NT] scaled bias or None, kidx [S, 2, 8] -> f16 tensor of
    (S * NT * 2 [+ NT]) blocks x 64 lanes x 8."""
    dev = Ws.device
    S = kidx.shape[0]
    lane_i, lane_kb = _LANE_I.to(dev), _LANE_H.to(dev)
    rows = 32 * torch.arange(NT, device=dev)[:, None] + lane_i[None, :]                 # [NT, 64]
    k = kidx.to(dev)[:, lane_kb, :]                                                      # [S, 64, 8]
    vals = Ws[rows[None, :, :, None].expand(S, NT, 64, 8), k[:, None, :, :].expand(S, NT, 64, 8)]
    hi, lo = _h2_split(vals)
    blocks = torch.stack([hi, lo], dim=2).reshape(S * NT * 2, 64, 8)                     # [S, NT, 2, 64, 8]
    if bs is None:
        return blocks.contiguous()
    bb = torch.zeros(NT, 64, 8, dtype=torch.float16, device=dev)
    bhi, blo = _h2_split(bs.reshape(NT, 32))
    bb[:, :32, 0] = bhi
    bb[:, :32, 1] = blo
    return torch.cat([blocks, bb], dim=0).contiguous()


def _pad_rows(W, b, R):
    Wp = torch.zeros(R, W.shape[1], dtype=torch.float32, device=W.device)
    bp = torch.zeros(R, dtype=torch.float32, device=W.device)
    Wp[:W.shape[0]] = W
    bp[:b.shape[0]] = b
    return Wp, bp


class _PaddedLinear:
    """weight / bias of a Linear zero-padded to (out_to, in_to): the stand-in the packers read.  Padded hidden units have weight 0
    and bias 0, so they hold act(0) = 0 (SiLU / ReLU / Tanh) and feed zero columns of the next layer: same function."""

    def __init__(self, lin, out_to, in_to):
        W, b = lin.weight.detach(), lin.bias.detach()
        self.weight = torch.zeros((out_to, in_to), dtype=W.dtype, device=W.device)
        self.weight[:W.shape[0], :W.shape[1]] = W
        self.bias = torch.zeros((out_to,), dtype=b.dtype, device=b.device)
        self.bias[:b.shape[0]] = b
        self.in_features, self.out_features = in_to, out_to


def _pad_hidden(linears, H):
    """the Linear chain with every hidden width zero-padded to H (input and output widths unchanged)"""
    n = len(linears)
    return tuple(_PaddedLinear(lin, H if i < n - 1 else lin.out_features, H if i > 0 else lin.in_features)
                 for i, lin in enumerate(linears))


# The three layer kinds of a conditioner in the split-f16 layout.  Each scales the layer by its own 2^e in f32 first (weights and bias
# together), then splits into hi / lo (_pack_h2), and returns (blocks, the unscale factor 2^-e).  ``groups``: the layer's rows are
# packed 32 NT at a time, the groups back to back -- the two 128-row halves of the width-256 kernel, the 128-row parameter chunks.


def _h2_scaled(lin):
    W, b = lin.weight.detach().float(), lin.bias.detach().float()
    e = _h2_scale_exp(W, b)
    return W * 2.0 ** e, b * 2.0 ** e, 2.0 ** -e


def _pack_h2_groups(Ws, bs, kidx, NT, groups):
    R = 32 * NT
    return torch.cat([_pack_h2(Ws[g * R:(g + 1) * R], None if bs is None else bs[g * R:(g + 1) * R], kidx, NT)
                      for g in range(groups)], dim=0).contiguous()


def _h2_first_layer(lin, NT=4, groups=1):
    """layer 0 (input from LDS): rows zero-padded to 32 NT per group, 16 S0 columns in natural k order, the bias as one more column; no
    bias blocks"""
    W, b, c = _h2_scaled(lin)
    n_in = lin.in_features
    S0 = (n_in + 1 + 15) // 16
    W0e = torch.zeros(32 * NT * groups, 16 * S0, dtype=torch.float32, device=W.device)
    W0e[:W.shape[0], :n_in] = W
    W0e[:W.shape[0], n_in] = b                          # column of the constant-1 feature
    return _pack_h2_groups(W0e, None, _h2_k_natural(S0), NT, groups), c


def _h2_hidden_layer(lin, HT=4, NT=None, groups=1):
    """a layer fed from the accumulator registers of HT input tiles (k order _h2_k_hidden(HT)): hidden -> hidden (NT = HT output tiles
    per group), or the affine kernels' output layer (rows zero-padded to NT = OT tiles); bias blocks"""
    NT = HT if NT is None else NT
    W, b, c = _h2_scaled(lin)
    Wp, bp = _pad_rows(W, b, 32 * NT * groups)
    return _pack_h2_groups(Wp, bp, _h2_k_hidden(HT), NT, groups), c


def _h2_hidden_stack(lins, HT=4):
    """hidden -> hidden layers back to back: (blocks or None when there is none, [unscale factor per layer])"""
    packed = [_h2_hidden_layer(lin, HT) for lin in lins]
    return (torch.cat([A for A, _ in packed], dim=0).contiguous() if packed else None), [c for _, c in packed]


def _h2_param_chunks(lin, src_t, HT=4):
    """the spline kernels' output layer: rows gathered through the table ``src_t`` (_src_col_table; -1: a zero row), in 128-row chunks"""
    W, b, c = _h2_scaled(lin)
    Wr, br = _gather_rows(W, b, src_t)
    return _pack_h2_groups(Wr, br, _h2_k_hidden(HT), 4, src_t.numel() // 128), c


def pack_dense_for_affine_h2(linears):
    """Pack DenseNet([n_in, H, H, d]) (H = 64 | 128, d <= 96) for bgk_coupling_affine_dense_h2, or DenseNet([n_in, H, H, H, d])
    for bgk_coupling_affine_dense_h3.  Returns (A0, A1, A2 f16 device tensors, (c0, c1, c2)[, A1b, c1b])."""
    l0, l1, l2 = linears[0], linears[1], linears[-1]
    HT, OT = l0.out_features // 32, (l2.out_features + 31) // 32
    A0, c0 = _h2_first_layer(l0, HT)
    A1, c1 = _h2_hidden_layer(l1, HT)
    A2, c2 = _h2_hidden_layer(l2, HT, NT=OT)
    if len(linears) == 3:
        return A0, A1, A2, (c0, c1, c2)
    (l1b,) = linears[2:-1]
    A1b, c1b = _h2_hidden_layer(l1b, l1b.out_features // 32)
    return A0, A1, A2, (c0, c1, c2), A1b, c1b


def pack_dense_for_affine_deep(linears):
    """Pack DenseNet([n_in, H, ..., H, d]) with 1 .. 8 hidden layers (H = 64 | 128, d <= 96) for bgk_coupling_affine_dense_deep: layer 0
    and the output layer as pack_dense_for_affine_h2, the hidden -> hidden layers back to back.  Returns (A0, A1 | None, A2, c0, [c1 per
    hidden -> hidden layer], c2)."""
    l0, l_out = linears[0], linears[-1]
    HT, OT = l0.out_features // 32, (l_out.out_features + 31) // 32
    A0, c0 = _h2_first_layer(l0, HT)
    A1, c1s = _h2_hidden_stack(linears[1:-1], HT)
    A2, c2 = _h2_hidden_layer(l_out, HT, NT=OT)
    return A0, A1, A2, c0, c1s, c2


def pack_dense_for_fused_h2(linears, nc_slot_host, d, n_bins, row_order=1):
    """Pack DenseNet([n_in, 128, 128, P]) for bgk_coupling_rqs_dense_h2.
    Returns (A0, A1, A2 f16 device tensors, (c0, c1, c2) unscale factors).  ``row_order``: order of the output layer's rows
    (bgk_pack_rqs_columns_v): 1 = what every kernel reads; 2 = the permutation the split-f16 inference kernel reads with
    operand_dtype 2 (8 bins; widths / heights of a lane's element in that lane's accumulator registers)."""
    l0, l1, l2 = linears
    A0, c0 = _h2_first_layer(l0)
    A1, c1 = _h2_hidden_layer(l1)
    A2, c2 = _h2_param_chunks(l2, _src_col_table(d, n_bins, nc_slot_host, l2.weight.device, row_order))
    return A0, A1, A2, (c0, c1, c2)


def pack_dense_for_fused_w256(linears, nc_slot_host, d, n_bins):
    """Pack DenseNet([n_in, 256, 256, P]) for the width-256 kernel behind bgk_coupling_rqs_dense_h2 (H0 = H1 = 256;
    bgk_fused.hip::coupling_rqs_dense_w256_kernel): every GEMM produces 128 output rows at a time, so layer 0 and layer 1 are packed as
    two 128-row halves (rows 0..127, then 128..255), each in the width-128 block layout with 16 k16-steps over the 256 hidden inputs
    (k order = the accumulator layout of 8 tiles), the parameter chunks likewise.  Returns (A0, A1, A2 f16 device tensors, (c0, c1, c2))."""
    l0, l1, l2 = linears
    assert l0.weight.shape[0] == 256 and l1.weight.shape == (256, 256) and l2.weight.shape[1] == 256
    A0, c0 = _h2_first_layer(l0, groups=2)
    A1, c1 = _h2_hidden_layer(l1, HT=8, NT=4, groups=2)
    A2, c2 = _h2_param_chunks(l2, _src_col_table(d, n_bins, nc_slot_host, l2.weight.device), HT=8)
    return A0, A1, A2, (c0, c1, c2)


DEEP_MAX_HIDDEN = 8     # hidden layers bgk_coupling_rqs_dense_deep takes (DEEP_MAX_HH + 1 in bgk_fused.hip)


def pack_dense_for_fused_deep(linears, nc_slot_host, d, n_bins):
    """Pack DenseNet([n_in, 128, ..., 128, P]) with 1 .. 8 hidden layers for bgk_coupling_rqs_dense_deep: layer 0 and the parameter chunks
    as pack_dense_for_fused_h2, the hidden -> hidden layers back to back in A1.  Returns (A0, A1 | None, A2, c0, [c1 per layer], c2)."""
    l0, l_out = linears[0], linears[-1]
    A0, c0 = _h2_first_layer(l0)
    A1, c1s = _h2_hidden_stack(linears[1:-1])
    A2, c2 = _h2_param_chunks(l_out, _src_col_table(d, n_bins, nc_slot_host, l_out.weight.device))
    return A0, A1, A2, c0, c1s, c2


def pack_dense_for_fused_h2_device(linears, src_col_dev, n_chunks, bufs=None, bf16=False):
    """Device-side twin of pack_dense_for_fused_h2 (bgk_pack_dense_h2): returns (A0, A1, A2, cs) with cs the
    device scale table {2^s, 2^-s} x 3.  ``bufs`` = previous result to overwrite in place."""
    l0, l1, l2 = linears
    dev = l0.weight.device
    n_in = l0.in_features
    S0 = (n_in + 1 + 15) // 16
    if bufs is None:
        A0 = torch.empty((S0 * 8, 64, 8), dtype=torch.float16, device=dev)
        A1 = torch.empty((8 * 8 + 4, 64, 8), dtype=torch.float16, device=dev)
        A2 = torch.empty((n_chunks * (8 * 8 + 4), 64, 8), dtype=torch.float16, device=dev)
        cs = torch.empty(6, dtype=torch.float32, device=dev)
    else:
        A0, A1, A2, cs = bufs
    ws = [t.detach().contiguous() for lin in linears for t in (lin.weight, lin.bias)]
    assert all(w.dtype == torch.float32 for w in ws)
    with torch.cuda.device(dev):
        st = _lib.lib().bgk_pack_dense_h2(
            _lib.ptr(ws[0]), _lib.ptr(ws[1]), n_in, 128, _lib.ptr(ws[2]), _lib.ptr(ws[3]), _lib.ptr(ws[4]), _lib.ptr(ws[5]),
            l2.out_features, _lib.ptr(src_col_dev), n_chunks, 4, int(bf16), _lib.ptr(A0), _lib.ptr(A1), _lib.ptr(A2), _lib.ptr(cs),
            _lib.stream_ptr(dev))
    _lib.check(st, "bgk_pack_dense_h2")
    return A0, A1, A2, cs


T_OPERAND_MAX_IN = 96     # widest conditioner input bgk_pack_dense_h2_t / bgk_dense_backward_dx take (three 32-feature output tiles)


def _t_operand_bufs(bufs, P, n_in, dev):
    """transposed-weight operands T0..T2 of bgk_dense_backward_dx for a conditioner [n_in, 128, 128, P] (allocated once per plan)"""
    FT, S2 = (n_in + 31) // 32, ((P + 15) // 16 + 3) // 4 * 4      # T2: whole groups of 4 k-steps (zero blocks behind ceil(P / 16))
    key = (P, n_in, str(dev))
    if bufs.get("key") != key:
        bufs.clear()
        bufs.update(key=key, T0=torch.empty((8 * FT * 2 + FT, 64, 8), dtype=torch.float16, device=dev),
                    T1=torch.empty((8 * 8 + 4, 64, 8), dtype=torch.float16, device=dev),
                    T2=torch.empty((S2 * 8 + 4, 64, 8), dtype=torch.float16, device=dev))
    return bufs["T0"], bufs["T1"], bufs["T2"]


def pack_linear_layer(weight):
    """Operands of bgk_dense_layer for ``weight`` [n_out, n_in]: a list of passes (A f16 [G * S * 8, 64, 8], S, c, k0, k1), one per
    block of <= 256 input columns [k0, k1): the block scaled by a power of two (largest magnitude into [2^14, 2^15)), zero-padded to
    16 S columns and 128 G rows, per 128-row group in the split-f16 block layout of the coupling kernels (natural k order)."""
    W = weight.detach().float()
    n_out, n_in = W.shape
    G = (n_out + 127) // 128
    passes = []
    for k0 in range(0, n_in, 256):
        k1 = min(n_in, k0 + 256)
        S = int(_lib.lib().bgk_dense_layer_steps(k1 - k0))
        Wb = W[:, k0:k1]
        e = _h2_scale_exp(Wb)
        Wp = torch.zeros(128 * G, 16 * S, dtype=torch.float32, device=W.device)
        Wp[:n_out, :k1 - k0] = Wb * 2.0 ** e
        A = torch.cat([_pack_h2(Wp[g * 128:(g + 1) * 128], None, _h2_k_natural(S)) for g in range(G)], dim=0).contiguous()
        passes.append((A, S, 2.0 ** -e, k0, k1))
    return passes


def pack_linear_layer_device(weight):
    """Device-side twin of pack_linear_layer (bgk_pack_linear_layer: no host synchronisation): passes (A, S, cs, k0, k1) with cs the
    device pair {largest magnitude, unscale factor} of the block"""
    W = weight.detach()
    assert W.is_cuda and W.dtype == torch.float32 and W.dim() == 2 and W.stride(1) == 1
    n_out, n_in = W.shape
    G = (n_out + 127) // 128
    passes = []
    with torch.cuda.device(W.device):
        for k0 in range(0, n_in, 256):
            k1 = min(n_in, k0 + 256)
            S = int(_lib.lib().bgk_dense_layer_steps(k1 - k0))
            A = torch.empty((G * S * 8, 64, 8), dtype=torch.float16, device=W.device)
            cs = torch.empty(2, dtype=torch.float32, device=W.device)
            st = _lib.lib().bgk_pack_linear_layer(W.data_ptr() + 4 * k0, W.stride(0), n_out, k1 - k0, _lib.ptr(A), _lib.ptr(cs),
                                                  _lib.stream_ptr(W.device))
            _lib.check(st, "bgk_pack_linear_layer")
            passes.append((A, S, cs, k0, k1))
    return passes
