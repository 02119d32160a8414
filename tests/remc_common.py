"""Shared by tests/golden/make_remc_goldens.py, test_host_remc.py and test_gpu_remc.py: the settings of tests/golden/remc.npz, the random
numbers of its recorded cases regenerated from oracle/philox.py, and the small numpy target of its seeded run.  No import of the package
here: the fixture's script runs the reference with these."""
import functools

import numpy as np

from oracle import philox

# ---- (a) the seeded run of the numpy class
A_SEED, A_TEMPS, A_NOISE, A_BURNIN, A_STRIDE, A_EPOCHS, A_STEPS = 4711, np.array([1.0, 1.6, 2.5, 4.0, 6.5]), 0.4, 3, 2, 20, 4
A_X0 = np.array([[-1.7, 0.2]])


def double_well(x):
    """a tilted double well along x and a harmonic well along y: x [walkers, 2] -> [walkers]"""
    return x[:, 0] ** 4 - 6.0 * x[:, 0] ** 2 + x[:, 0] + 0.5 * x[:, 1] ** 2


# ---- (b) the recorded cases: L ladders of K temperatures, chain b = slot b % K of ladder b // K
SEED = 20263
K, L = 3, 50
B = K * L
N_STEPS, EVERY = 30, 3
N_EXCHANGES = N_STEPS // EVERY
FRAME_LADDERS = 2
MARGIN = 1e-3
G_ROWS_WIDE = np.r_[0:9, 117:150]              # whole ladders: 0..2 and 39..49
# case: (kind, n, d, noise_std, temperatures)
CASES = {
    "mdw_4_2": ("mdw", 4, 2, 0.3, (1.0, 1.5, 2.25)),
    "lj_13_3": ("lj", 13, 3, 0.05, (1.0, 2.0, 4.0)),
    "lj_64_3": ("lj", 64, 3, 0.02, (1.0, 1.5, 2.25)),
}


@functools.lru_cache(maxsize=None)
def recorded_numbers(nd, seed=SEED, n_steps=N_STEPS, batch=B, n_replicas=K, every=EVERY):
    """f32 (noise [n_steps, batch, nd], uniforms [n_steps, batch], exchange_uniforms [n_steps // every, batch]): Philox fields 0, 1, 2
    at offset = the step; the acceptance number of a ladder and step is that of its slot 0, repeated over the ladder (the reference draws
    one for all walkers of a run); the exchange after step s (0-based, s + 1 a multiple of ``every``) reads field 2 at offset s"""
    noise = np.stack([philox.sample_field(seed, s, 0, batch, nd, 1).astype(np.float32) for s in range(n_steps)])
    unif = np.stack([philox.sample_field(seed, s, 1, batch, 1, 0)[:, 0] for s in range(n_steps)])
    unif = np.repeat(unif[:, ::n_replicas], n_replicas, axis=1)
    exch = np.stack([philox.sample_field(seed, s, 2, batch, 1, 0)[:, 0] for s in range(every - 1, n_steps, every)])
    assert noise.dtype == np.float32 and unif.dtype == np.float32 and exch.dtype == np.float32
    return noise, unif, exch
