#!/usr/bin/env python3
"""Generate tests/golden/pf_sample.npz by IMPORTING the reference's ``SequenceDataset(..., pf_sample=True)``
(osrl/common/dataset.py:736-737 -> compute_sample_prob :399-436, never copying it) on the six cases of
tests/augment_cases.py that fit a Pareto frontier.  Build container only (needs the reference checkout and scipy):

    python tests/golden/make_golden_pf_sample.py

Same stubs as make_golden_augment.py (gymnasium / logger stubs, the ``oapackage`` ParetoDoubleLong stand-in) and the
same seeds, so the augmented trajectories are those of augment.npz.  The ``minimize`` the reference module sees is
wrapped: per trajectory the file keeps the start point (the cost return), the solver's ``sol.x``, scipy's success
flag and the distance the reference derives from it (its own closure evaluated at ``max(0, sol.x)``), next to the
returns, the frontier coefficients and the resulting ``sample_prob``.  Data only.
"""
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from augment_cases import RNG_SEED, SEQ_CASES  # noqa: E402
from augment_cases import make_augment_dataset  # noqa: E402
from make_golden import REF, _install_stubs  # noqa: E402
from make_golden_augment import _install_oapackage  # noqa: E402

PF_CASES = ("d0_p50", "d1_p20", "d2_p50", "d3_p20", "d4_p20", "single_pf")


class MinimizeRecorder:
    """Wraps ``minimize`` as the reference module sees it; one row per call, in call order."""

    def __init__(self, module):
        self.module, self.orig = module, module.minimize
        self.x0, self.x, self.dist, self.ok = [], [], [], []
        self.seconds = 0.0  # spent inside the reference's solves

    def __enter__(self):
        def wrapped(fun, x0, **kw):
            t0 = time.perf_counter()
            sol = self.orig(fun, x0=x0, **kw)
            self.seconds += time.perf_counter() - t0
            x = np.max([0, (sol.x)[0]])  # what compute_sample_prob does with the result (dataset.py:431-432)
            self.x0.append(float(x0))
            self.x.append(float(sol.x[0]))
            self.dist.append(float(np.sqrt(fun(x))))
            self.ok.append(bool(sol.success))
            return sol

        self.module.minimize = wrapped
        return self

    def __exit__(self, *exc):
        self.module.minimize = self.orig


def main():
    _install_stubs()
    _install_oapackage()
    sys.path.insert(0, REF)
    import scipy
    import osrl.common.dataset as D
    out = {"meta": np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}", f"rng_seed {RNG_SEED}",
                             "oapackage: stub, dominance >= all and > one, ties kept"])}
    for name in PF_CASES:
        dkw, skw = SEQ_CASES[name]
        random.seed(RNG_SEED)
        np.random.seed(RNG_SEED)
        with MinimizeRecorder(D) as rec:
            ds = D.SequenceDataset(make_augment_dataset(**dkw), seq_len=10, pf_sample=True, **skw)
        n = len(ds.dataset)
        assert len(rec.x) == n
        out[f"{name}_coef"] = np.asarray(ds.pareto_frontier.coeffs, np.float64)
        out[f"{name}_c"] = np.array([t["cost_returns"][0] for t in ds.dataset], np.float32)
        out[f"{name}_r"] = np.array([t["returns"][0] for t in ds.dataset], np.float32)
        assert np.array_equal(out[f"{name}_c"].astype(np.float64), np.asarray(rec.x0))
        out[f"{name}_sol_x"] = np.asarray(rec.x, np.float64)
        out[f"{name}_dist"] = np.asarray(rec.dist, np.float64)
        out[f"{name}_success"] = np.asarray(rec.ok, np.bool_)
        out[f"{name}_prob"] = np.asarray(ds.sample_prob, np.float64)
        out[f"{name}_n_original"] = np.array(len(ds.original_data), np.int64)
        print(name, "trajectories", n, "deg", len(out[f"{name}_coef"]) - 1, "scipy success",
              float(np.mean(rec.ok)), "seconds in the reference's solves", round(rec.seconds, 2))
    path = os.path.join(HERE, "pf_sample.npz")
    np.savez_compressed(path, **out)
    print("wrote pf_sample.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
