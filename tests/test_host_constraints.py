"""CPU: the builder's constraint layers (add_merge_constraints, add_constrain_chirality, add_torsion_multiplicities,
add_torsion_shifts; reference factory/generator_builder.py:461-526) and the flows behind them (nn/flow/modulo.py,
nn/flow/torchtransform.py) against tests/golden/g_constraints.npz, which tests/golden/make_constraint_goldens.py wrote by running
the unmodified reference.  Every operation is one or two correctly rounded IEEE operations or an exact fmod evaluated in the
reference's order, so every comparison is equality of bits."""
import warnings

import numpy as np
import pytest
import torch

import bgflow_amd as bg


def T(a, device=None):
    return torch.as_tensor(np.asarray(a), device=device)


def same(t, ref):
    """bit equality of a tensor with a golden array (np.array_equal: -0.0 == 0.0, which the f32 results here never mix)"""
    a = t.detach().cpu().numpy()
    return a.shape == ref.shape and a.dtype == ref.dtype and np.array_equal(a, ref)


def constraint_builder(G, device=None):
    """the four constraint layers on the 15 / 17 / 17 / 9 alanine-dipeptide shapes, as make_constraint_goldens.py builds them"""
    shapes = bg.ShapeDictionary()
    shapes[bg.BONDS], shapes[bg.ANGLES], shapes[bg.TORSIONS], shapes[bg.FIXED] = (15,), (17,), (17,), (9,)
    b = bg.BoltzmannGeneratorBuilder(shapes, device=device)
    b.add_merge_constraints(G["c_idx"], G["c_val"])
    b.add_torsion_multiplicities(torch.tensor(G["mults"]))
    b.add_torsion_shifts(torch.tensor(G["shifts"]))
    b.add_constrain_chirality(G["halpha"])
    return b


def test_builder_constraint_layers_match_the_reference(golden):
    """fails before this feature: the first call raised NotImplementedError"""
    G = golden("g_constraints")
    b = constraint_builder(G)
    assert b.current_dims[bg.BONDS] == (15 + len(G["c_idx"]),)
    assert list(b.current_dims) == [bg.BONDS, bg.ANGLES, bg.TORSIONS, bg.FIXED]
    flow = b.build_flow()
    assert [type(f).__name__ for f in flow] == ["SetConstantFlow", "WrapFlow", "WrapFlow", "WrapFlow", "WrapFlow"]
    assert [type(f._flow).__name__ for f in list(flow)[1:]] == ["MergeFlow", "IncreaseMultiplicityFlow", "CircularShiftFlow", "TorchTransform"]
    zs = [T(G[f"flow_z{k}"]) for k in range(4)]
    torch.manual_seed(int(G["seed"]) + 2)
    with torch.no_grad():
        *ys, d = flow(*zs)
        *zi, di = flow(*[T(G[f"flow_y{k}"]) for k in range(4)], inverse=True)
    for k in range(4):
        assert same(ys[k], G[f"flow_y{k}"]), f"forward, tensor {k}"
        assert same(zi[k], G[f"flow_zi{k}"]), f"inverse, tensor {k}"
    assert same(d, G["flow_dlogp"]) and same(di, G["flow_dlogp_inv"])
    assert float(d[0]) == np.float32(2 * np.log(0.5))
    # the constants sit bit-exact at the constrained indices, the inputs elsewhere; the inverse drops them
    free = np.setdiff1d(np.arange(17), G["c_idx"])
    assert np.array_equal(ys[0].numpy()[:, G["c_idx"]], np.broadcast_to(G["c_val"], (zs[0].shape[0], 2)))
    assert np.array_equal(ys[0].numpy()[:, free], G["flow_z0"]) and np.array_equal(zi[0].numpy(), G["flow_y0"][:, free])


def test_builder_constraint_arguments():
    shapes = bg.ShapeDictionary()
    shapes[bg.BONDS], shapes[bg.TORSIONS] = (4,), (6,)
    b = bg.BoltzmannGeneratorBuilder(shapes)
    with pytest.warns(UserWarning, match="skipped"):
        b.add_merge_constraints([], [])
    assert not b.layers
    with pytest.raises(AssertionError):
        b.add_merge_constraints([1, 2], [0.1])
    with pytest.raises(AssertionError):
        b.add_merge_constraints([1], [0.1], field=bg.ANGLES)
    with pytest.raises(NotImplementedError):      # the reference has no defaults here: a missing argument is an error
        b.add_merge_constraints([1])
    b.add_constrain_chirality([True, False, False, True, False, False], right_handed=True)
    t = b.layers[-1]._flow._delegate_transform.base_transform
    assert t.loc.tolist() == [0.0] * 6 and t.scale.tolist() == [0.5, 1, 1, 0.5, 1, 1]
    b.add_torsion_multiplicities(3)
    b.add_torsion_shifts(0.25)
    sd = b.build_flow().state_dict()
    assert {k.split(".")[-1] for k in sd} == {"_multiplicities", "_shift"}       # the reference's buffer names


def test_each_flow_alone_matches_the_reference(golden):
    G = golden("g_constraints")
    with torch.no_grad():
        f = bg.CircularShiftFlow(T(G["shifts"]))
        y, d = f(T(G["shift_x"]))
        xi, di = f(T(G["shift_x"]), inverse=True)
        assert same(y, G["shift_fwd"]) and same(xi, G["shift_inv"]) and same(d, G["shift_dlogp"]) and same(di, G["shift_dlogp_inv"])
        f = bg.IncreaseMultiplicityFlow(T(G["mults"]))
        torch.manual_seed(int(G["seed"]) + 1)                 # the same torch.rand call shape as the reference
        y, d = f(T(G["mult_x"]))
        xi, _ = f(T(G["mult_x"]), inverse=True)
        assert same(y, G["mult_fwd"]) and same(xi, G["mult_inv"]) and same(d, G["mult_dlogp"])
        y2, _ = f(T(G["mult_x"]), sheaf_uniforms=T(G["mult_u"]))
        assert same(y2, G["mult_fwd"])
        f = bg.TorchTransform(torch.distributions.AffineTransform(loc=T(G["aff_loc"]), scale=T(G["aff_scale"])), 1)
        y, d = f(T(G["aff_x"]))
        xi, di = f(T(G["aff_x"]), inverse=True)
        assert same(y, G["aff_fwd"]) and same(xi, G["aff_inv"]) and same(d, G["aff_dlogp"]) and same(di, G["aff_dlogp_inv"])
        f = bg.TorchTransform(torch.distributions.AffineTransform(loc=0.25, scale=-3.0), 1)
        y, d = f(T(G["aff_x"]))
        assert same(y, G["affs_fwd"]) and same(d, G["affs_dlogp"])
        # any other transform, and an affine without reinterpreted dimensions, go through torch as in torchtransform.py
        f = bg.TorchTransform(torch.distributions.SigmoidTransform())
        y, d = f(T(G["aff_x"]))
        assert torch.equal(y, torch.sigmoid(T(G["aff_x"]))) and d.shape == (*y.shape, 1)


def test_range_check_raises_on_cpu():
    for f in (bg.CircularShiftFlow(0.3), bg.IncreaseMultiplicityFlow(2)):
        for inverse in (False, True):
            x = torch.full((3, 5), 0.5)
            x[1, 2] = 1 + 5e-7
            f(x, inverse=inverse)
            x[1, 2] = 1.1
            with pytest.raises(ValueError):
                f(x, inverse=inverse)
            x[1, 2] = -0.1
            with pytest.raises(ValueError):
                f(x, inverse=inverse)


def test_column_tables_and_their_backward():
    from bgflow_amd import modulo as mo
    t = mo.ColumnTable(3, [(mo.COPY, 2, 0, 0), (mo.CONST, 0, 7.5, 0), (mo.AFFINE_FWD, 0, 1.0, -2.0), (mo.MULT_INV, 1, 3.0, 1 / 3)], logdet=0.5)
    assert (t.n_in, t.n_out, t.checks_range, t.draws) == (3, 4, True, False)
    assert t.host.itemsize == 16
    b = t.backward()
    assert (b.n_in, b.n_out, b.logdet) == (4, 3, 0.0)
    assert b.host.tolist() == [(mo.AFFINE_FWD, 2, 0.0, -2.0), (mo.AFFINE_FWD, 3, 0.0, 3.0), (mo.COPY, 0, 0.0, 0.0)]
    with pytest.raises(ValueError):
        mo.ColumnTable(2, [(mo.COPY, 2, 0, 0)])
    assert mo.COLMAP_MAX_WIDTH == 256
    # the pair matcher: only SetConstant -> Wrap(Merge(indices)) over the inserted slot
    G = {"c_idx": np.array([1]), "c_val": np.array([0.1], np.float32)}
    shapes = bg.ShapeDictionary()
    shapes[bg.BONDS], shapes[bg.ANGLES] = (3,), (4,)
    b2 = bg.BoltzmannGeneratorBuilder(shapes)
    b2.add_merge_constraints(G["c_idx"], G["c_val"])
    flow = b2.build_flow()
    assert [label for label, _ in flow.segments()] == ["constant merge"]
    assert [label for label, _ in flow.segments(inverse=True)] == ["constant merge"]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")
        x = torch.rand(5, 3)
        y, a, d = flow(x, torch.rand(5, 4))          # on CPU tensors the segment runs the two blocks
        assert y.shape == (5, 4) and torch.equal(y[:, 1], torch.full((5,), 0.1)) and torch.equal(y[:, [0, 2, 3]], x)
        xb, _, _ = flow(y, a, inverse=True)
        assert torch.equal(xb, x)
    flow.FUSE_CONSTANT_MERGE = False
    assert [label for label, _ in flow.segments()] == ["SetConstantFlow", "WrapFlow"]


def test_compat_paths_and_state_dict():
    from bgflow_amd.nn.flow.modulo import CircularShiftFlow, IncreaseMultiplicityFlow
    from bgflow_amd.nn.flow.torchtransform import TorchTransform
    assert CircularShiftFlow is bg.CircularShiftFlow and IncreaseMultiplicityFlow is bg.IncreaseMultiplicityFlow and TorchTransform is bg.TorchTransform
    f = bg.IncreaseMultiplicityFlow(torch.tensor([1, 2, 3]))
    assert list(f.state_dict()) == ["_multiplicities"]              # no Philox state before the first device draw
    f.set_philox_stream(5, calls=3)
    sd = f.state_dict()
    assert sd["_philox_state"].tolist() == [5, 3]
    g = bg.IncreaseMultiplicityFlow(torch.tensor([1, 1, 1]))
    with pytest.warns(RuntimeWarning):                              # the stream id is held by the live `f`
        g.load_state_dict(sd)
    assert g._multiplicities.tolist() == [1, 2, 3] and g.__dict__["_philox_state"] == [5, 3]
