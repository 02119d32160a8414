"""Time ``HungarianMapper`` (bgflow_amd/permutation.py) on 2^18 samples: the kernel path (csrc/bgk_assign.hip, HIP events around one call,
3 warm-up calls, 20 repeats, median / min / max) against the general path (scipy per sample on the host, timed on 4096 of the same rows
and scaled, labelled as scaled), on box samples from the chain kernel (n = 38, m = 36, d = 2), on the same samples with the solvent
labels shuffled, and at m = 64, d = 3.  With ``--one-per-wave-lib`` also the packing A/B of DESIGN.md "Permutation reduction": this
library against a build of the same source with one sample per wavefront for every m,

    BGK_EXTRA_FLAGS=-DBGK_ASSIGN_PACK=0 BGK_EXTRA_TU=bgk_assign.hip python -m bgflow_amd.build --out /tmp/libbgflow_amd_one_per_wave.so

both loaded into this process, blocks of 5 repeats alternated 4 times.  One JSON line per measurement.

    python tools/assign_time.py [--one-per-wave-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import bgflow_amd as bg                      # noqa: E402
from bgflow_amd import _lib                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--one-per-wave-lib", default=None)
opts = ap.parse_args()
assert torch.cuda.is_available(), "needs a HIP device"
dev = torch.device("cuda:0")
REPEATS = 20
print(json.dumps({"device": torch.cuda.get_device_name(0)}))


def timed(fn, repeats=REPEATS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def raw(handle, mapper, rows, y, status):
    """the map launch through a given library handle"""
    m = len(mapper.identical_particles)
    ref = mapper._device_ref[rows.device]
    rc = handle.bgk_assign_particles(_lib.ptr(rows), rows.stride(0), rows.shape[0], mapper.n_particles, mapper.dim, _lib.ptr(ref),
                                     mapper._host_index, m, _lib.ptr(y), y.stride(0), None, None, _lib.ptr(status), None, _lib.stream_ptr(dev))
    assert rc == 0, rc


def say(key, value):
    print(json.dumps({key: value}), flush=True)


B = 1 << 18
# ---- box samples from the chain kernel -----------------------------------------------------------------------------------------------
G = np.load(os.path.join(ROOT, "tests", "golden", "box.npz"))
params = {**bg.RepulsiveParticles.params_default, "nsolvent": 36, "eps": float(G["eps"])}
energy = bg.HarmonicParticles(spring_constant=float(G["spring_constant"]), params=params).to(dev)
start = torch.tensor(G["x_36"][:1], device=dev)
x = start.repeat(B, 1).contiguous()
STD, STEPS = 0.08, 400
step = bg.MCMCStep(energy, proposal=bg.GaussianProposal(noise_std=STD), target_temperatures=1.0, n_steps=STEPS).set_philox_stream(11)
torch.cuda.synchronize()
t0 = time.perf_counter()
X = step(bg.SamplerState(samples=x)).as_dict()["samples"][0].contiguous()
torch.cuda.synchronize()
say("chain", dict(B=B, steps=STEPS, noise_std=STD, seconds=time.perf_counter() - t0, accept_rate=float(step.n_accepted.float().mean()) / STEPS))
mapper = bg.HungarianMapper(start[0], dim=2, identical_particles=np.arange(2, 38))
assert mapper._takes_kernel(X)
moved = mapper.is_permuted(X)
say("box_fraction_permuted", float(moved.float().mean()))
perm, _ = mapper.assignment(X[:4096])
say("box_mean_particles_moved", float((perm != torch.arange(36, device=dev)).sum(1).float().mean()))
say("box_map_call", timed(lambda: mapper.map(X)))
say("box_map_launch", timed(lambda: mapper._launch(X, y=True, status=True)))
say("box_is_permuted_launch", timed(lambda: mapper._launch(X, permuted=True)))
# shuffled labels: the long-path case
gen = torch.Generator(device=dev).manual_seed(1)
order = torch.rand(B, 36, device=dev, generator=gen).argsort(dim=1)
Xs = X.clone()
Xs.view(B, 38, 2)[:, 2:] = torch.gather(X.view(B, 38, 2)[:, 2:], 1, order[:, :, None].expand(B, 36, 2))
say("box_shuffled_map_launch", timed(lambda: mapper._launch(Xs, y=True, status=True)))
# the general path on the host, 4096 of the same rows
for name, data in (("box", X), ("box_shuffled", Xs)):
    host = data[:4096].cpu().numpy()
    secs = []
    for _ in range(3):
        t0 = time.perf_counter()
        Yh = mapper.map(host)
        secs.append(time.perf_counter() - t0)
    say(name + "_general_path_4096_rows_s", dict(median=statistics.median(secs), min=min(secs), scaled_to_2p18_s=statistics.median(secs) * B / 4096))
    Yk = mapper.map(data[:4096]).cpu().numpy()
    say(name + "_rows_equal_to_general_path", int((Yk == Yh).all(axis=1).sum()))

# ---- m = 64, d = 3 ---------------------------------------------------------------------------------------------------------------------
def synthetic(m, d, n, noise, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ref = (torch.rand(n, d, device=dev, generator=g) * 10 - 5)
    data = ref[None] + noise * torch.randn(B, n, d, device=dev, generator=g)
    ip = np.arange(n - m, n)
    order = torch.rand(B, m, device=dev, generator=g).argsort(dim=1)
    data[:, n - m:] = torch.gather(data[:, n - m:], 1, order[:, :, None].expand(B, m, d))
    return bg.HungarianMapper(ref.reshape(-1), dim=d, identical_particles=ip), data.reshape(B, n * d).contiguous()


mp, data = synthetic(64, 3, 64, 0.5, 2)
say("m64_d3_map_launch", timed(lambda: mp._launch(data, y=True, status=True)))
host = data[:1024].cpu().numpy()
t0 = time.perf_counter()
mp.map(host)
secs = time.perf_counter() - t0
say("m64_d3_general_path_1024_rows_s", dict(seconds=secs, scaled_to_2p18_s=secs * B / 1024))

# ---- packing: this library (packed) against the one-sample-per-wavefront build, alternating --------------------------------------------
if opts.one_per_wave_lib:
    alt = ctypes.CDLL(opts.one_per_wave_lib)
    res, args = _lib._SIGNATURES["bgk_assign_particles"]
    alt.bgk_assign_particles.restype, alt.bgk_assign_particles.argtypes = res, args
    here = _lib.lib()
    for m, d in ((8, 2), (16, 2), (16, 3), (32, 2), (24, 3)):
        mp, data = synthetic(m, d, m + 2, 0.5, 10 + m)
        mp._launch(data[:4], y=True, status=True)                # uploads the reference
        y1, s1 = torch.empty_like(data), torch.empty(B, dtype=torch.int32, device=dev)
        y2, s2 = torch.empty_like(data), torch.empty(B, dtype=torch.int32, device=dev)
        rounds = {"packed": [], "one_per_wave": []}
        for _ in range(4):                                       # alternate blocks of 5 repeats
            rounds["packed"].append(timed(lambda: raw(here, mp, data, y1, s1), repeats=5, warmup=1))
            rounds["one_per_wave"].append(timed(lambda: raw(alt, mp, data, y2, s2), repeats=5, warmup=1))
        summary = {k: dict(median_ms=statistics.median(r["median_ms"] for r in v), min_ms=min(r["min_ms"] for r in v),
                           max_ms=max(r["max_ms"] for r in v)) for k, v in rounds.items()}
        summary["same_output"] = bool(torch.equal(y1, y2) and torch.equal(s1, s2))
        say(f"packing_m{m}_d{d}", summary)

