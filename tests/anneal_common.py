"""Shared by test_host_anneal.py and test_gpu_anneal.py: the cases of tests/golden/anneal.npz (written by
tests/golden/make_anneal_goldens.py) rebuilt with this package's classes, and their random numbers regenerated from oracle/philox.py."""
import numpy as np
import torch

import bgflow_amd as bg

from mcmc_common import make as make_pair, random_numbers

B = 150
K = 2
EPS, SPRING = 0.7, 150.0
UMBRELLA_K, UMBRELLA_M = 50.0, 1.5
# case: (end A, end B); an end is (kind, n, d) or (box kind, nsolvent) -- the table of make_anneal_goldens.py without the settings
CASES = {
    "mfn_lj_2_1": (("mfn", 2, 1), ("lj", 2, 1)), "mfn_lj_13_3": (("mfn", 13, 3), ("lj", 13, 3)), "mfn_lj_64_3": (("mfn", 64, 3), ("lj", 64, 3)),
    "lj_mdw_4_2": (("lj", 4, 2), ("mdw", 4, 2)), "lj_mdw_64_3": (("lj", 64, 3), ("mdw", 64, 3)), "mdw_mfn_13_3": (("mdw", 13, 3), ("mfn", 13, 3)),
    "lj_lj_13_3": (("lj", 13, 3), ("lj", 13, 3)), "rep_biased_2": (("rep", 2), ("biased", 2)), "rep_biased_62": (("rep", 62), ("biased", 62)),
    "rep_harm_36": (("rep", 36), ("harm", 36)),
}


def make_end(P, end):
    """the energy of one end with the parameters of particles.npz / make_box_goldens.py"""
    kind = end[0]
    if kind in ("rep", "biased", "harm"):
        params = {**bg.RepulsiveParticles.params_default, "nsolvent": end[1], "eps": EPS}
        if kind == "harm":
            return bg.HarmonicParticles(spring_constant=SPRING, params=params)
        system = bg.RepulsiveParticles(params)
        return bg.biased_system(system, UMBRELLA_K, UMBRELLA_M) if kind == "biased" else system
    return make_pair(P, kind, end[1], end[2])


def start_state(golden, end):
    x = golden("box")[f"x_{end[1]}"] if len(end) == 2 else golden("particles")[f"x_{end[1]}_{end[2]}"]
    return np.ascontiguousarray(x).reshape(B, -1)


def case_numbers(G, nd):
    """the case's random numbers (noise [12, B, nd], uniforms [12, B]), checked against the sums the fixture recorded"""
    n_steps = (len(G["lambdas"]) - 1) * int(G["n_steps"])
    noise, unif = random_numbers(int(G["seed"]), nd, n_steps, B)
    assert abs(noise.astype(np.float64).sum() - float(G[f"noise_sum_{nd}"])) <= 1e-9 * noise.size
    assert float(np.abs(noise).max()) == float(G[f"noise_absmax_{nd}"])
    assert abs(unif.astype(np.float64).sum() - float(G["unif_sum"])) <= 1e-12 * unif.size and float(unif.max()) == float(G["unif_absmax"])
    return noise, unif


def switching(golden, key, device="cpu", dtype=torch.float32):
    """(the case's AnnealedSwitching with its random numbers fed, its start state) on ``device`` in ``dtype``"""
    G, P = golden("anneal"), golden("particles")
    end_a, end_b = CASES[key]
    x0 = start_state(golden, end_a)
    noise, unif = case_numbers(G, x0.shape[1])
    sw = bg.AnnealedSwitching(make_end(P, end_a).to(device), make_end(P, end_b).to(device), G["lambdas"].tolist(), n_steps=int(G["n_steps"]),
                              noise_std=float(G[key + "_std"]), temperature_a=float(G[key + "_t_a"]), temperature_b=float(G[key + "_t_b"]))
    sw.feed_noise(torch.tensor(noise, device=device), torch.tensor(unif, device=device))
    return sw, torch.tensor(x0, device=device).to(dtype)


def bar_check(prior, target, forward_x0, reverse_x0, fused, stream=None):
    """the statistical check with an analytic answer: 16 linear stages x 4 steps at noise_std 0.3 from sigma_A = 1 to sigma_B = 0.8 of
    4 particles in 2 dimensions; forward and reverse work into bennett_acceptance_ratio.  Returns (estimate, uncertainty, exact)."""
    import math
    lambdas = [i / 16 for i in range(17)]
    sw = bg.AnnealedSwitching(prior, target, lambdas, n_steps=4, noise_std=0.3)
    sw.fused = fused
    rv = sw.reverse()
    if stream is not None:
        sw.set_philox_stream(stream)
        rv.set_philox_stream(stream + 1)
    _, w_f = sw(forward_x0)
    _, w_r = rv(reverse_x0)
    df, ddf = bg.bennett_acceptance_ratio(w_f, w_r)
    return float(df), float(ddf), -6 * math.log(0.8), sw, rv
