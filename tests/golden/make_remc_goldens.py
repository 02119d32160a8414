#!/usr/bin/env python
"""Generate tests/golden/remc.npz by IMPORTING the reference (CPU, never on the GPU box):

    BGFLOW_REFERENCE=<checkout of the reference> python tests/golden/make_remc_goldens.py

What runs: the UNMODIFIED reference class ``ReplicaExchangeMetropolisGauss`` (distribution/sampling/_mcmc/metropolis.py:138-188) with its
``MetropolisGauss``, with the import shims of make_goldens.py.  The fixture holds DATA only.  Settings and random numbers: tests/remc_common.py.

(a) Seeded run: ``np.random.seed(A_SEED)``, the 2-d double well of remc_common.py, K = 5 temperatures, ``burnin=3``, ``stride=2``, 20 epochs
    of 4 steps.  Stored: ``a_traj`` = np.array(sampler.traj_) [frames, 5, 2], ``a_etraj`` [frames, 5], ``a_toggle``.

(b) Recorded numbers: ``np.random.randn`` / ``np.random.rand`` are patched to hand out the numbers of remc_common.recorded_numbers
    (Philox field 0: noise; field 1: one acceptance number per ladder and step; field 2: the exchange number at the pair's lower slot).
    The reference runs ONE ladder per object: L = 50 objects per case, ladder l started at x_{n}_{d}[l] of particles.npz tiled K = 3
    times (chains 3 l .. 3 l + 2 of the batch of 150), 10 epochs of 3 steps, on the reference's torch energies (parameters of
    particles.npz, ``two_event_dims=False``) wrapped as numpy functions.  The patched ``rand`` also reads, without changing anything, what
    the objects hold at that moment: the acceptance margin |-log r - (E_prop - E) / T| of every walker, the exchange margin |-log r - c|,
    both decisions, and -- at the exchange's draw -- the state BEFORE the exchange (the reference's own ``traj_`` keeps a reference to the
    array the exchange then edits in place).  Per case, from the f64 run:

      x64 [rows, n d]   final states (after the last exchange); rows = all 150, for n d > 64 G_ROWS_WIDE (``rows``)
      e64 [150]         final energies            acc / exch [150]  accepted steps per slot / accepted exchanges at the pair's lower slot
      frames64 [10, 6, n d], frames_e64 [10, 6]   the state of the first two ladders after every epoch's steps, before its exchange
      keep [50]         per LADDER: every Metropolis and exchange margin of its chains >= 1e-3
      err_x32 / err_e32 max |x32 - x64| over final states and frames / max |e32 - e64| / (1 + |e64|), kept ladders, x32 the reference's own
                        f32 run on the same numbers
      std, temps        the settings

Asserted here: keep covers >= 2/3 of the ladders of every case; the f32 run decides like the f64 run on every kept ladder; the Metropolis
acceptance is within 25-80 % and the exchange acceptance within 10-90 %.
"""
import os
import sys

import numpy

numpy.infty = numpy.inf  # numpy-2 shim

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.environ["BGFLOW_REFERENCE"])

import nflows_stub  # noqa: E402

nflows_stub.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgflow.distribution.energy.lennard_jones import LennardJonesPotential  # noqa: E402
from bgflow.distribution.energy.multi_double_well_potential import MultiDoubleWellPotential  # noqa: E402

import remc_common as C  # noqa: E402


def load_reference(name):
    """a module of the reference's _mcmc package by path (the package's __init__ imports modules that do not exist)"""
    import importlib.util
    path = os.path.join(os.environ["BGFLOW_REFERENCE"], "bgflow", "distribution", "sampling", "_mcmc", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ReplicaExchangeMetropolisGauss = load_reference("metropolis").ReplicaExchangeMetropolisGauss


def make(kind, n, d, P):
    if kind == "lj":
        eps, rm, osc = (float(v) for v in P["lj_params"])
        return LennardJonesPotential(n * d, n, eps=eps, rm=rm, oscillator=True, oscillator_scale=osc, two_event_dims=False)
    a, b, c, off = (float(v) for v in P["mdw_params"])
    return MultiDoubleWellPotential(n * d, n, a, b, c, off, two_event_dims=False)


def seeded_run():
    np.random.seed(C.A_SEED)
    re = ReplicaExchangeMetropolisGauss(C.double_well, C.A_X0, C.A_TEMPS, noise=C.A_NOISE, burnin=C.A_BURNIN, stride=C.A_STRIDE)
    re.run(nepochs=C.A_EPOCHS, nsteps_per_epoch=C.A_STEPS)
    return np.array(re.sampler.traj_), np.array(re.sampler.etraj_), re.toggle


class Recorded:
    """np.random.randn / np.random.rand for one ladder: hands out the recorded numbers and looks at what the objects hold"""

    def __init__(self, ladder, noise, unif, exch, dtype):
        self.rows = slice(C.K * ladder, C.K * ladder + C.K)
        self.noise, self.unif, self.exch, self.dtype = noise, unif, exch, dtype
        self.re = None
        self.step = self.in_epoch = self.exchange = 0
        self.acc = np.zeros(C.K, np.int32)
        self.exc = np.zeros(C.K, np.int32)
        self.margin = np.inf
        self.decisions = []
        self.frames, self.frames_e = [], []

    def randn(self, rows, cols):
        return self.noise[self.step, self.rows].astype(self.dtype)

    def _log(self, r):
        return np.log(r.astype(self.dtype)) if self.dtype == np.float32 else np.log(np.float64(r))

    def rand(self):
        s = self.re.sampler
        if self.in_epoch < C.EVERY:                    # the acceptance draw of a step
            r = self.unif[self.step, self.rows][0]
            v = (s.E_prop - s.E) / s.temperature
            dec = -self._log(r) > v
            self.acc += dec
            self.margin = min(self.margin, float(np.abs(-np.log(np.float64(r)) - v.astype(np.float64)).min()))
            self.decisions += list(dec)
            self.step += 1
            self.in_epoch += 1
        else:                                          # the one exchange draw of an epoch (K = 3: one pair)
            k = self.re.toggle
            assert k + 2 >= C.K - 1
            r = self.exch[self.exchange, self.rows][k]
            T = self.re.temperatures
            c = -(s.E[k + 1] - s.E[k]) * (1.0 / T[k + 1] - 1.0 / T[k])
            dec = -self._log(r) > c
            self.exc[k] += dec
            self.margin = min(self.margin, float(abs(-np.log(np.float64(r)) - np.float64(c))))
            self.decisions.append(bool(dec))
            self.frames.append(s.x.copy())
            self.frames_e.append(s.E.copy())
            self.exchange += 1
            self.in_epoch = 0
        return r.astype(self.dtype) if self.dtype == np.float32 else float(r)


def run_case(energy, x0, numbers, std, temps, dtype):
    """the reference on the recorded numbers, ladder by ladder"""
    noise, unif, exch = numbers
    tdtype = torch.float32 if dtype == np.float32 else torch.float64

    def energy_function(x):
        assert x.dtype == dtype, x.dtype
        return energy.energy(torch.from_numpy(np.ascontiguousarray(x)).to(tdtype))[:, 0].detach().numpy()

    out = dict(x=[], e=[], acc=[], exch=[], margin=[], decisions=[], frames=[], frames_e=[])
    randn, rand = np.random.randn, np.random.rand
    try:
        for ladder in range(C.L):
            rec = Recorded(ladder, noise, unif, exch, dtype)
            np.random.randn, np.random.rand = rec.randn, rec.rand
            re = ReplicaExchangeMetropolisGauss(energy_function, x0[ladder].reshape(1, -1).astype(dtype), np.array(temps, dtype), noise=std)
            rec.re = re
            re.run(nepochs=C.N_EXCHANGES, nsteps_per_epoch=C.EVERY)
            assert rec.step == C.N_STEPS and rec.exchange == C.N_EXCHANGES and re.sampler.x.dtype == dtype and re.sampler.E.dtype == dtype
            out["x"].append(re.sampler.x.copy()); out["e"].append(re.sampler.E.copy()); out["acc"].append(rec.acc); out["exch"].append(rec.exc)
            out["margin"].append(rec.margin); out["decisions"].append(rec.decisions)
            out["frames"].append(np.stack(rec.frames)); out["frames_e"].append(np.stack(rec.frames_e))
    finally:
        np.random.randn, np.random.rand = randn, rand
    return dict(x=np.concatenate(out["x"]), e=np.concatenate(out["e"]), acc=np.concatenate(out["acc"]), exch=np.concatenate(out["exch"]),
                margin=np.array(out["margin"]), decisions=np.array(out["decisions"]),
                frames=np.concatenate(out["frames"], axis=1), frames_e=np.concatenate(out["frames_e"], axis=1))


def main():
    P = np.load(os.path.join(HERE, "particles.npz"))
    traj, etraj, toggle = seeded_run()
    out = {"a_traj": traj, "a_etraj": etraj, "a_toggle": np.int64(toggle)}
    print(f"(a) {traj.shape[0]} frames, final toggle {toggle}")
    for key, (kind, n, d, std, temps) in C.CASES.items():
        nd = n * d
        numbers = C.recorded_numbers(nd)
        x0 = P[f"x_{n}_{d}"].reshape(-1, nd)[:C.L]
        energy = make(kind, n, d, P)
        r64 = run_case(energy, x0, numbers, std, temps, np.float64)
        r32 = run_case(energy, x0, numbers, std, temps, np.float32)
        assert r64["x"].dtype == np.float64 and r32["x"].dtype == np.float32 and np.isfinite(r64["e"]).all()
        keep = r64["margin"] >= C.MARGIN
        assert keep.mean() >= 2 / 3, (key, keep.mean())
        assert (r32["decisions"][keep] == r64["decisions"][keep]).all(), key
        rate = r64["acc"].mean() / C.N_STEPS
        pairs = sum(len(range(j & 1, C.K - 1, 2)) for j in range(C.N_EXCHANGES))
        xrate = r64["exch"].sum() / (C.L * pairs)
        rows = C.G_ROWS_WIDE if nd > 64 else np.arange(C.B)
        kc = np.repeat(keep, C.K)
        fr = C.FRAME_LADDERS * C.K
        err_x = max(np.abs(r32["x"][rows][kc[rows]] - r64["x"][rows][kc[rows]]).max(initial=0.0),
                    np.abs(r32["frames"][:, :fr][:, kc[:fr]] - r64["frames"][:, :fr][:, kc[:fr]]).max(initial=0.0))
        err_e = np.max(np.abs(r32["e"][kc] - r64["e"][kc]) / (1.0 + np.abs(r64["e"][kc])))
        k_ = key + "_"
        out[k_ + "x64"], out[k_ + "rows"], out[k_ + "e64"] = r64["x"][rows], rows.astype(np.int32), r64["e"]
        out[k_ + "acc"], out[k_ + "exch"], out[k_ + "keep"] = r64["acc"].astype(np.int32), r64["exch"].astype(np.int32), keep
        out[k_ + "frames64"], out[k_ + "frames_e64"] = r64["frames"][:, :fr], r64["frames_e"][:, :fr]
        out[k_ + "err_x32"], out[k_ + "err_e32"] = np.float64(err_x), np.float64(err_e)
        out[k_ + "std"], out[k_ + "temps"] = np.float64(std), np.array(temps, np.float64)
        print(f"{key}: acceptance {rate:.2f}, exchanges {xrate:.2f}, kept {int(keep.sum())} / {C.L} ladders, f32 = f64 decisions on all: "
              f"{bool((r32['decisions'] == r64['decisions']).all())}, err_x32 {err_x:.3g}, err_e32 {err_e:.3g}")
        assert 0.25 <= rate <= 0.80, (key, rate)
        assert 0.10 <= xrate <= 0.90, (key, xrate)
    path = os.path.join(HERE, "remc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
