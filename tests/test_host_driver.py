"""No GPU: bgflow_amd._driver, the host plumbing free_energy.py, umbrella.py and analysis.py share -- the record loop against a fake
enqueue on a CPU record, the ``path=`` resolver, the per-tensor rule, and that the three modules hold the driver's tables."""
import math

import pytest
import torch

from bgflow_amd import _driver, analysis, umbrella
from bgflow_amd import free_energy as fe

DONE = 4


class FakeSolver:
    """advances a CPU record one step at a time; the phase turns DONE at step ``done_at`` and later steps are empty, as the kernels' are"""

    def __init__(self, done_at):
        self.done_at, self.calls, self.steps, self.records = done_at, 0, 0, []

    def __call__(self, record, n_steps):
        assert record.dtype == torch.float64 and record.device.type == "cpu" and record.shape == (6,)
        if self.calls == 0:
            assert float(record.abs().max()) == 0.0                 # the start state is all zeros
        self.calls += 1
        self.records.append(record)
        for _ in range(n_steps):
            if int(record[_driver.R_PHASE]) == DONE:
                continue
            self.steps += 1
            record[5] = self.steps
            if self.steps == self.done_at:
                record[_driver.R_PHASE], record[_driver.R_STATUS] = DONE, _driver.BUDGET
        return 0


@pytest.mark.parametrize("chunk", [1, 5, 16])
def test_readbacks_are_the_chunks_up_to_the_done_step(chunk):
    for s in (1, chunk, chunk + 1):
        fake = FakeSolver(s)
        record, host, reads = _driver.solve_record(fake, 6, DONE, 100, chunk, torch.device("cpu"), "fake_steps")
        assert reads == math.ceil(s / chunk) == fake.calls             # one read-back per call, none past the first done one
        assert all(r is record for r in fake.records)                 # one record from start to end
        assert int(host[_driver.R_PHASE]) == DONE and int(host[_driver.R_STATUS]) == _driver.BUDGET and int(host[5]) == s == fake.steps


@pytest.mark.parametrize("chunk", [1, 5, 16])
def test_a_record_that_is_never_done_raises_past_the_budget(chunk):
    budget = 7
    fake = FakeSolver(10 ** 9)
    with pytest.raises(RuntimeError) as e:
        _driver.solve_record(fake, 6, DONE, budget, chunk, torch.device("cpu"), "fake_steps", unit="iterations")
    enqueued = fake.calls * chunk
    assert enqueued > budget + chunk >= enqueued - chunk              # the first call that ends more than a chunk past the budget
    assert str(e.value) == f"fake_steps: the record is not done after {enqueued} iterations (budget {budget})"
    with pytest.raises(RuntimeError, match=r"fake_steps: the record is not done after \d+ steps \(budget 7\)"):
        _driver.solve_record(FakeSolver(10 ** 9), 6, DONE, budget, chunk, torch.device("cpu"), "fake_steps")
    # done exactly at the last step the budget allows for: no error
    last = (budget // chunk + 2) * chunk
    assert _driver.solve_record(FakeSolver(last), 6, DONE, budget, chunk, torch.device("cpu"), "fake_steps")[2] == last // chunk


def test_a_failed_entry_stops_the_loop(hip_lib):
    with pytest.raises(RuntimeError, match="fake_steps failed"):
        _driver.solve_record(lambda record, n: -1, 6, DONE, 10, 4, torch.device("cpu"), "fake_steps")


def test_path_resolver():
    takes = "tensors it likes"
    assert _driver.use_kernel(None, True, "f", takes) is True and _driver.use_kernel(None, False, "f", takes) is False
    assert _driver.use_kernel("kernel", True, "f", takes) is True
    assert _driver.use_kernel("torch", True, "f", takes) is False and _driver.use_kernel("torch", False, "f", takes) is False
    with pytest.raises(ValueError, match="f: unknown path 'fastest'"):
        _driver.use_kernel("fastest", True, "f", takes)
    with pytest.raises(ValueError, match="f: unknown path 'Kernel'"):
        _driver.use_kernel("Kernel", True, "f", takes)
    with pytest.raises(ValueError, match="f: the kernel path takes tensors it likes"):
        _driver.use_kernel("kernel", False, "f", takes)


def test_per_tensor_rule_on_the_cpu():
    t = torch.zeros(4)
    assert not _driver.kernel_takes(t) and not _driver.kernel_takes(t.numpy()) and not _driver.kernel_takes(None)      # not on a HIP device
    assert _driver.same_kind([t, t.clone()]) and not _driver.same_kind([t, t.double()])


def test_the_modules_hold_the_drivers_tables():
    codes = {torch.float32: 0, torch.float64: 1}
    assert _driver.DTYPE_CODES == codes
    assert fe._DTYPE_CODES is _driver.DTYPE_CODES and umbrella._DTYPE_CODES is _driver.DTYPE_CODES and analysis._DTYPE_CODES is _driver.DTYPE_CODES
    assert (fe.CONVERGED, fe.BUDGET, fe.NO_ROOT, fe.NOT_A_NUMBER) == (0, 1, 2, 3) == (_driver.CONVERGED, _driver.BUDGET, _driver.NO_ROOT, _driver.NOT_A_NUMBER)
    assert (umbrella.CONVERGED, umbrella.BUDGET, umbrella.NOT_A_NUMBER) == (0, 1, 3)
    assert fe.STATUS_NAMES is _driver.STATUS_NAMES == ("converged", "budget exhausted", "no root", "nan")
    assert (fe.RECORD_DOUBLES, fe.PHASE_DONE, fe.BAR_CHUNK, fe.MAX_BLOCKS) == (18, 4, 16, 512)
    assert (umbrella.RECORD_DOUBLES, umbrella.PHASE_DONE, umbrella.MBAR_CHUNK, umbrella.MAX_BLOCKS, umbrella.MAX_WINDOWS) == (8, 1, 32, 512, 256)
    assert (fe.R_UPPER, fe.R_LOWER, fe.R_UNCERTAINTY) == (2, 3, 17) and (umbrella.R_N_ITER, umbrella.R_ERR, umbrella.R_N) == (2, 3, 5)
