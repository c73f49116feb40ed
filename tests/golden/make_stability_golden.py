"""Generate ``stability_pairs.npz`` by executing the reference's own ``utils.match_signatures_pair``.

Run where the reference is checked out next to the build (``python tests/golden/make_stability_golden.py``); a no-op where
it is not.  Nothing here is imported by the product or by the tests -- the tests read the arrays it wrote.

How the reference is executed (as ``make_golden.py`` does it): ``utils.py`` is loaded by file path
with ``numba.njit`` replaced by the identity decorator and placeholder modules for its absent optional imports; the function
itself runs on the installed pandas, scikit-learn and SciPy, as in the reference.

Output (arrays only):
  stability_pairs.npz   for each of the pairs: ``first_i``, ``second_i`` (K x V signature matrices, float64) and
                        ``indices_i``, what ``match_signatures_pair(first, second)`` returned (cosine metric): the order
                        of ``second``'s rows that matches ``first``'s
"""

from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(1, 96, 0.3), (2, 96, 0.3), (5, 96, 0.05), (5, 83, 0.3), (8, 96, 0.3), (12, 83, 0.6), (16, 96, 0.3), (16, 96, 0.6)]  # K, V, noise


def load_reference_utils():
    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    for name, attrs in (("numba", {"njit": njit}), ("mudata", {"MuData": type("MuData", (), {})}), ("anndata", {"AnnData": type("AnnData", (), {})})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("salamander_reference_utils", os.path.join(REF, "src", "salamander", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(REF):
        print("no reference here: nothing to do")
        return
    import pandas as pd

    utils = load_reference_utils()
    rng = np.random.default_rng(20240)
    out = {"n_pairs": np.array(len(PAIRS))}
    for i, (K, V, cv) in enumerate(PAIRS):
        base = rng.dirichlet(np.full(V, 0.2), size=K)
        shape = 1.0 / cv**2
        first = base * rng.gamma(shape, 1.0 / shape, size=(K, V))
        second = (base * rng.gamma(shape, 1.0 / shape, size=(K, V)))[rng.permutation(K)]
        first /= first.sum(axis=1, keepdims=True)
        second /= second.sum(axis=1, keepdims=True)
        out[f"first_{i}"], out[f"second_{i}"] = first, second
        out[f"indices_{i}"] = np.asarray(utils.match_signatures_pair(pd.DataFrame(first), pd.DataFrame(second)), dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "stability_pairs.npz"), **out)
    print("wrote stability_pairs.npz")


if __name__ == "__main__":
    main()
