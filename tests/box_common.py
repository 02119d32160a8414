"""Shared by test_host_box.py and test_gpu_box.py: the cases of tests/golden/box.npz (written by tests/golden/make_box_goldens.py) rebuilt
with this package's classes."""
import numpy as np

import bgflow_amd as bg

B = 150
NSOLVENT = [0, 2, 36, 62]
KINDS = ["rep", "harm"]
MC_NSOLVENT = [2, 36, 62]


def make(G, kind, nsolvent):
    """the target of a case with the fixture's parameters: params_default but for nsolvent and eps, and the spring constant"""
    params = {**bg.RepulsiveParticles.params_default, "nsolvent": nsolvent, "eps": float(G["eps"])}
    if kind == "rep":
        return bg.RepulsiveParticles(params)
    return bg.HarmonicParticles(spring_constant=float(G["spring_constant"]), params=params)


def err_u(v, u64):
    return float(np.max(np.abs(v.astype(np.float64) - u64) / (1.0 + np.abs(u64))))


def err_g(v, g64):
    return float(np.max(np.abs(v.astype(np.float64) - g64)) / (1.0 + np.max(np.abs(g64))))
