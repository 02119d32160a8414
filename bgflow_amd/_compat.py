"""Dotted import paths of the reference package, mapped onto this package's flat modules.

bgflow code often imports through sub-packages (``from bgflow.nn.flow.crd_transform.ic import ...``,
``from bgflow.factory.tensor_info import BONDS``).  ``register(root)`` installs lightweight alias modules under
``<root>.nn...``, ``<root>.distribution...``, ``<root>.factory...`` so that such imports resolve to the accelerated classes
when this package stands in for bgflow (``import bgflow_amd as bgflow`` or ``sys.modules["bgflow"] = bgflow_amd``).
Only the modules on the accelerated hot path are mapped; anything else raises ImportError as before.
"""
import sys
import types

# reference module path (relative to the package root) -> name of the flat module here that holds its public names (a tuple: several)
_MAP = {
    "nn": None,
    "nn.dense": "dense",
    "nn.periodic": "dense",
    "nn.flow": "flow",
    "nn.flow.base": "flow",
    "nn.flow.sequential": "flow",
    "nn.flow.coupling": "flow",
    "nn.flow.inverted": "flow",
    "nn.flow.cdf": "cdf",
    "nn.flow.modulo": "modulo",
    "nn.flow.circular": "circular",
    "nn.flow.torchtransform": "modulo",
    "nn.flow.diffeq": "dynamics",
    "nn.flow.stochastic": ("flow", "stochastic"),
    "nn.flow.stochastic.augment": "flow",
    "nn.flow.stochastic.langevin": "stochastic",
    "nn.flow.stochastic.mcmc": "stochastic",
    "nn.flow.transformer": "transformer",
    "nn.flow.transformer.base": "transformer",
    "nn.flow.transformer.affine": "transformer",
    "nn.flow.transformer.spline": "transformer",
    "nn.flow.crd_transform": "ic",
    "nn.flow.crd_transform.ic": "ic",
    "nn.flow.crd_transform.pca": "ic",
    "distribution": ("distributions", "particles", "sampling", "mixture"),
    "distribution.distributions": "distributions",
    "distribution.normal": ("distributions", "particles"),
    "distribution.product": "distributions",
    "distribution.mixture": "mixture",
    "distribution.energy": ("distributions", "particles"),
    "distribution.energy.lennard_jones": "particles",
    "distribution.energy.multi_double_well_potential": "particles",
    "distribution.energy.particles": "particles",
    "distribution.energy.base": "distributions",
    "distribution.energy.double_well": "distributions",
    "distribution.energy.clipped": "clipped",
    "distribution.sampling": ("distributions", "sampling"),
    "distribution.sampling.iterative": "sampling",
    "distribution.sampling.mcmc": "sampling",
    "distribution.sampling.base": "distributions",
    "distribution.sampling.dataset": "training",
    "distribution.sampling._mcmc": ("permutation", "analysis", "umbrella"),
    "distribution.sampling._mcmc.permutation": "permutation",
    "distribution.sampling._mcmc.analysis": "analysis",
    "distribution.sampling._mcmc.umbrella_sampling": "umbrella",
    "distribution.sampling._mcmc.metropolis": "umbrella",
    "nn.training": "training",
    "nn.training.trainers": "training",
    "factory.tensor_info": "factory",
    "factory.generator_builder": "factory",
    "factory.conditioner_factory": "factory",
    "factory.transformer_factory": "factory",
    "factory.distribution_factory": "factory",
    "factory.icmarginals": "factory",
    "utils.types": "utils",
    "utils.train": "clipped",
    "utils.free_energy": "free_energy",
}


def register(root, package):
    """Install the alias modules under the dotted name ``root`` (``package`` = the imported bgflow_amd package)."""
    for rel, flat in sorted(_MAP.items(), key=lambda kv: kv[0].count(".")):
        full = f"{root}.{rel}"
        if full in sys.modules:
            continue
        mod = types.ModuleType(full, f"alias of {package.__name__}.{flat}" if flat else "namespace")
        mod.__path__ = []          # behaves like a package: sub-imports go through sys.modules
        for flat in ((flat,) if isinstance(flat, str) else flat or ()):
            src = getattr(package, flat)
            names = getattr(src, "__all__", None) or [n for n in vars(src) if not n.startswith("__")]
            for n in names:
                setattr(mod, n, getattr(src, n))
            for n in vars(src):        # private helpers a few reference call sites reach for (e.g. _tuple)
                if n.startswith("_") and not n.startswith("__") and not hasattr(mod, n):
                    setattr(mod, n, getattr(src, n))
        sys.modules[full] = mod
        parent, _, leaf = full.rpartition(".")
        if parent in sys.modules and not hasattr(sys.modules[parent], leaf):
            setattr(sys.modules[parent], leaf, mod)
