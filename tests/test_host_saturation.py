"""Host (no GPU): the reproducible activation forms of csrc/bgk_detmath.h (the oracle compiles the same header the kernels do) where
they saturate or their exp overflows -- SiLU / tanh / softplus, the affine tail's log sigma = tanh(s_raw) exp(log_alpha) and its
VJP, DenseNet layers -- against f64 restatements of the reference's ops (nn/flow/transformer/affine.py:35-70, nn/dense.py:30-48).
The kernels' own hardware forms are pinned on the device by tests/test_gpu_saturation.py."""
import numpy as np
import pytest

# pre-activations where the forms saturate: 44.36 is where exp2 of the tanh argument (2 |x| log2 e) overflows in f32, 88.72 where
# that of SiLU (-x log2 e) does
SAT = np.array([0.5, 20.0, 44.0, 44.36, 44.5, 45.0, 50.0, 88.0, 88.72, 89.0, 100.0, 1e4], np.float32)
S = np.concatenate([SAT, -SAT])
HUGE = np.array([1e30, -1e30], np.float32)


def _silu64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


SOFTPLUS_BETA = 0.69384102162        # the beta bgo_detmath_probe / bgk_detmath_probe pass (softplus(x, beta, threshold=20))


def _softplus64(x):
    x = np.asarray(x, np.float64)
    z = x * SOFTPLUS_BETA
    return np.where(z > 20.0, x, np.log1p(np.exp(np.minimum(z, 20.0))) / SOFTPLUS_BETA)


REF = {"silu": _silu64, "tanh": np.tanh, "softplus": _softplus64}


@pytest.mark.parametrize("which", ["silu", "tanh", "softplus"])
def test_detmath_activations_saturate_like_f64(oracle, which):
    """over S: finite, within 6e-7 of f64 relative to |x| (the bound of the device layer tests with one input and weight 1); tanh is
    exactly +-1 from |x| = 20 on, SiLU is (sub)normally tiny below -100; at +-1e30: finite, the right sign, within 1e-4 of f64 (the
    +-80 clamp of bgk_expf leaves SiLU(-1e30) at -1.8e-5)"""
    got = oracle.detmath_probe(S, which).astype(np.float64)
    ref = REF[which](S.astype(np.float64))
    assert np.isfinite(got).all(), (which, S[~np.isfinite(got)])
    assert (np.abs(got - ref) <= 6e-7 * np.maximum(np.abs(S.astype(np.float64)), 1.0)).all(), (which, got, ref)
    if which == "tanh":
        sat = np.abs(S) >= 20.0
        assert np.array_equal(got[sat], np.sign(S[sat]).astype(np.float64)), got[sat]
    if which == "silu":
        assert (np.abs(got[S <= -100.0]) <= 1e-30).all(), got[S <= -100.0]
    big = oracle.detmath_probe(HUGE, which).astype(np.float64)
    ref_big = REF[which](HUGE.astype(np.float64))
    assert np.isfinite(big).all()
    assert big[0] > 0 and (big[1] <= 0.0 if which != "softplus" else big[1] >= 0.0)
    assert (np.abs(big - ref_big) <= 1e-4 * np.maximum(np.abs(ref_big), 1.0)).all(), (which, big, ref_big)


def test_detmath_exp_and_its_clamp(oracle):
    """exp within 2 ulp of f64 for |x| <= 80; beyond, the documented clamp: exp(+-80) exactly as the form computes it there"""
    x = np.concatenate([np.linspace(-80.0, 80.0, 20001, dtype=np.float32), np.array([-80.0, 80.0, 0.0, -0.0], np.float32)])
    got = oracle.detmath_probe(x, "exp").astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    assert (np.abs(got - ref) <= 2.0 * np.spacing(ref.astype(np.float32)).astype(np.float64)).all()
    edge = oracle.detmath_probe(np.array([-80.0, 80.0], np.float32), "exp")
    far = np.array([80.5, 88.72, 89.0, 100.0, 1e4, 1e30, np.inf], np.float32)
    assert np.array_equal(oracle.detmath_probe(far, "exp"), np.full(far.shape, edge[1], np.float32))
    assert np.array_equal(oracle.detmath_probe(-far, "exp"), np.full(far.shape, edge[0], np.float32))
    assert np.isfinite(edge).all() and edge[0] > 0


def _affine64(y, mu, s_raw, log_alpha, preserve_volume, inverse):
    """affine.py:35-70 in f64: (out, dlogp) and the intermediates the VJP below needs"""
    th = np.tanh(s_raw)
    alpha = np.exp(log_alpha)
    ls = th * alpha
    if preserve_volume:
        ls = ls - ls.mean(axis=1, keepdims=True)
    sgn = -1.0 if inverse else 1.0
    e = np.exp(sgn * ls)
    out = e * (y - mu) if inverse else e * y + mu
    dlogp = sgn * ls.sum(axis=1, keepdims=True)
    return out, dlogp, th, alpha, e, sgn


def _affine_vjp64(y, mu, s_raw, log_alpha, preserve_volume, inverse, go, gl):
    """(out, dlogp, g_y, g_mu, g_s_raw, g_log_alpha) for the loss sum(go out) + sum(gl dlogp), the chain rule written out"""
    out, dlogp, th, alpha, e, sgn = _affine64(y, mu, s_raw, log_alpha, preserve_volume, inverse)
    g_y = go * e
    g_mu = -go * e if inverse else go
    g_ls = sgn * go * e * ((y - mu) if inverse else y) + sgn * gl
    if preserve_volume:
        g_ls = g_ls - g_ls.mean(axis=1, keepdims=True)
    g_s = g_ls * alpha * (1.0 - th * th)
    g_la = float((g_ls * th).sum() * alpha)
    return out, dlogp, g_y, g_mu, g_s, g_la


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("preserve_volume", [False, True])
def test_affine_tail_with_saturated_log_sigma(oracle, inverse, preserve_volume):
    """the oracle's affine tail (bgo_affine / bgo_affine_backward) with s_raw over S: y', dlogp and every gradient within f32 rounding
    of the f64 restatement, all finite, and g_s exactly 0 wherever tanh is saturated (the f64 value: 1 - tanh^2 = 0 there)"""
    rng = np.random.default_rng(7 + 2 * inverse + preserve_volume)
    B, d = 64, S.size
    s_raw = np.stack([np.roll(S, i) for i in range(B)]).astype(np.float32)
    s_raw[:, ::3] = rng.standard_normal((B, (d + 2) // 3)).astype(np.float32)          # unsaturated units in between
    y = rng.standard_normal((B, d)).astype(np.float32)
    mu = rng.standard_normal((B, d)).astype(np.float32)
    go = rng.standard_normal((B, d)).astype(np.float32)
    gl = rng.standard_normal((B, 1)).astype(np.float32)
    la = np.float32(0.25)
    f = [a.astype(np.float64) for a in (y, mu, s_raw, go, gl)]
    r_out, r_dl, r_gy, r_gmu, r_gs, r_gla = _affine_vjp64(f[0], f[1], f[2], float(la), preserve_volume, inverse, f[3], f[4])
    out, dl = oracle.affine(y, mu, s_raw, log_alpha=la, preserve_volume=preserve_volume, inverse=inverse)
    g_y, g_mu, g_s, g_la = oracle.affine_backward(y, mu, s_raw, go, gl, log_alpha=la, preserve_volume=preserve_volume, inverse=inverse)
    for name, a in (("out", out), ("dlogp", dl), ("g_y", g_y), ("g_mu", g_mu), ("g_s", g_s)):
        assert np.isfinite(a).all(), name
    assert np.isfinite(g_la)
    np.testing.assert_allclose(out, r_out, rtol=0, atol=2e-5 * max(1.0, np.abs(r_out).max()))
    np.testing.assert_allclose(dl, r_dl, rtol=0, atol=1e-5 * max(1.0, np.abs(r_dl).max()))
    for name, a, b in (("g_y", g_y, r_gy), ("g_mu", g_mu, r_gmu), ("g_s", g_s, r_gs)):
        assert np.linalg.norm(a - b) <= 5e-6 * np.linalg.norm(b), name
    assert abs(g_la - r_gla) <= 5e-6 * max(abs(r_gla), 1.0)
    sat = np.abs(s_raw) >= 20.0
    assert sat.sum() > B and np.all(g_s[sat] == 0.0) and np.all(r_gs[sat] == 0.0)


@pytest.mark.parametrize("act", ["silu", "tanh"])
def test_oracle_dense_layers_at_saturation(oracle, act):
    """oracle.linear / oracle.dense_net with SiLU / Tanh whose pre-activations (set through the bias) run over S and +-1e30: finite,
    within 6e-7 (sum |x||W| + |b|) of f64 per row, tanh exactly +-1 from |pre| = 20 on, and a two-layer net agrees with f64"""
    rng = np.random.default_rng(3)
    B, n_in = 33, 24
    b = np.concatenate([S, HUGE]).astype(np.float32)
    n_out = b.size
    W = (rng.standard_normal((n_out, n_in)) * 1e-3).astype(np.float32)
    x = rng.standard_normal((B, n_in)).astype(np.float32)
    y = oracle.linear(x, W, b, act).astype(np.float64)
    pre = x.astype(np.float64) @ W.T.astype(np.float64) + b.astype(np.float64)
    ref = REF[act](pre)
    bound = 6e-7 * (np.abs(x.astype(np.float64)) @ np.abs(W.T.astype(np.float64)) + np.abs(b.astype(np.float64)))
    assert np.isfinite(y).all()
    huge = np.abs(b) > 1e29
    assert (np.abs(y - ref)[:, ~huge] <= bound[:, ~huge]).all()
    assert (np.abs(y - ref)[:, huge] <= 1e-4 * np.maximum(np.abs(ref[:, huge]), 1.0)).all()
    if act == "tanh":
        sat = np.abs(pre) >= 20.0
        assert np.array_equal(y[sat], np.sign(pre[sat]))
    else:
        assert (np.abs(y[(pre <= -100.0) & ~huge[None, :]]) <= 1e-30).all()
    W2 = (rng.standard_normal((5, n_out)) * 0.01).astype(np.float32)
    b2 = rng.standard_normal(5).astype(np.float32)
    z = oracle.dense_net(x, [W, W2], [b, b2], [act, None]).astype(np.float64)
    z_ref = ref @ W2.T.astype(np.float64) + b2
    assert np.isfinite(z).all()
    np.testing.assert_allclose(z, z_ref, rtol=0, atol=1e-5 * max(1.0, np.abs(z_ref).max()))
