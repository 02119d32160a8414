"""CPU: the operands the torch packers write (f32 layout, split-f16 block layout of the spline and affine coupling kernels) are bit for
bit those recorded in tests/golden/packed_operand_digests.json (cases and digest: tests/golden/make_packing_digests.py)."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_packing_digests", os.path.join(HERE, "golden", "make_packing_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_packed_operands_are_bit_identical_to_the_recorded_ones(hip_lib):
    gen = _generator()
    with open(gen.PATH) as f:
        want = json.load(f)
    got = gen.digests()
    assert sorted(got) == sorted(want)
    assert {k: v for k, v in got.items() if v != want[k]} == {}
