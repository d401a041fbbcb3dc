#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by IMPORTING the reference's dataset functions (never copying them):
SequenceDataset's augmentation paths (osrl/common/dataset.py:633-747 -> augmentation :282-396, get_nearest_point
:186-236, grid_filter :239-272, random_augmentation :557-630), compute_cost_sample_prob (:439-459) and
process_bc_dataset's "frontier" mode (:30-134) on the datasets of tests/augment_cases.py.  Build container only
(needs the reference checkout):

    python tests/golden/make_golden_augment.py

oapackage is not installed here, so an ``oapackage`` stub is put in ``sys.modules`` first: ParetoDoubleLong keeps the
indices whose value no other value dominates (>= in every component and > in one; every index of a tied optimum is
kept), in insertion order.  That dominance rule is an ASSUMPTION about oapackage the goldens rest on.

Every random draw the reference makes is recorded so the tests can inject the same stream: random.sample -> the
positions kept inside each bin; np.random.uniform / np.random.choice -> the raw random_sample() doubles they
consumed (replayed from a state snapshot); np.random.normal -> the values it returned.
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from augment_cases import BC_COST_LIMIT, BC_KINDS, RNG_SEED, SEQ_CASES, make_augment_dataset, make_bc_frontier_dataset  # noqa: E402,E501
from make_golden import REF, _install_stubs  # noqa: E402


class ParetoDoubleLong:
    def __init__(self):
        self.vals, self.idx = [], []

    def addvalue(self, w, i):
        self.vals.append(tuple(float(v) for v in w))
        self.idx.append(int(i))

    def show(self, verbose=0):
        pass

    def allindices(self):
        v = np.asarray(self.vals, np.float64).reshape(-1, 2)
        keep = []
        for k in range(v.shape[0]):  # is any value >= in both components and > in one?
            dom = np.all(v >= v[k], axis=1) & np.any(v > v[k], axis=1)
            if not dom.any():
                keep.append(self.idx[k])
        return keep


def _install_oapackage():
    m = types.ModuleType("oapackage")
    m.ParetoDoubleLong = ParetoDoubleLong
    m.doubleVector = lambda t: tuple(t)
    sys.modules["oapackage"] = m


class Recorder:
    """Wraps the four samplers; ``log`` collects (kind, values) in call order."""

    def __init__(self):
        self.log = []
        self._orig = (random.sample, np.random.uniform, np.random.choice, np.random.normal)

    def _raw(self, fn, *a, **kw):
        st = np.random.get_state()
        out = fn(*a, **kw)
        after = np.random.get_state()
        np.random.set_state(st)
        raw = np.random.random_sample(np.size(out))
        now = np.random.get_state()
        assert now[2] == after[2] and np.array_equal(now[1], after[1]), "the sampler consumed other than size doubles"
        np.random.set_state(after)
        return out, raw

    def __enter__(self):
        sample, uniform, choice, normal = self._orig

        def w_sample(pop, k):
            out = sample(pop, k)
            self.log.append(("pick", np.array([pop.index(e) for e in out], np.int32)))
            return out

        def w_uniform(*a, **kw):
            out, raw = self._raw(uniform, *a, **kw)
            self.log.append(("uniform", raw))
            return out

        def w_choice(*a, **kw):
            out, raw = self._raw(choice, *a, **kw)
            self.log.append(("choice", raw))
            return out

        def w_normal(*a, **kw):
            out = normal(*a, **kw)
            self.log.append(("normal", np.asarray(out, np.float64).ravel()))
            return out

        random.sample, np.random.uniform, np.random.choice, np.random.normal = w_sample, w_uniform, w_choice, w_normal
        return self

    def __exit__(self, *exc):
        random.sample, np.random.uniform, np.random.choice, np.random.normal = self._orig

    def cat(self, kind, dtype=np.float64):
        v = [x for k, x in self.log if k == kind]
        return np.concatenate(v).astype(dtype) if v else np.zeros(0, dtype)




def main():
    _install_stubs()
    _install_oapackage()
    sys.path.insert(0, REF)
    import torch
    from osrl.common.dataset import SequenceDataset, compute_cost_sample_prob, process_bc_dataset
    out = {"meta": np.array([f"numpy {np.__version__}", f"torch {torch.__version__}", f"rng_seed {RNG_SEED}",
                             "oapackage: stub, dominance >= all and > one, ties kept"])}
    for name, (dkw, skw) in SEQ_CASES.items():
        random.seed(RNG_SEED)
        np.random.seed(RNG_SEED)
        with Recorder() as rec:
            ds = SequenceDataset(make_augment_dataset(**dkw), seq_len=10, **skw)
        n_orig = len(ds.original_data)
        out[f"{name}_n_original"] = np.array(n_orig, np.int64)
        out[f"{name}_len"] = np.array([len(t["costs"]) for t in ds.dataset], np.int64)
        aug = ds.dataset[n_orig:]  # the original rows are process_sequence_dataset's (pinned by ingest.npz)
        for k in ("observations", "actions", "rewards", "costs", "returns", "cost_returns"):
            out[f"{name}_aug_{k}"] = np.concatenate([t[k] for t in aug]) if aug else np.zeros(0, np.float32)
        if hasattr(ds, "idx"):
            out[f"{name}_idx"] = np.asarray(ds.idx, np.int64)
        if hasattr(ds, "indices"):
            out[f"{name}_indices"] = np.asarray(ds.indices, np.int64)
        if hasattr(ds, "pareto_frontier"):
            out[f"{name}_coef"] = np.asarray(ds.pareto_frontier.coeffs, np.float64)
            # the Pareto set of the filtered returns, from the same stub the reference used
            fc = np.array([ds.original_data[i]["cost_returns"][0] for i in ds.indices], np.float64)
            fr = np.array([ds.original_data[i]["returns"][0] for i in ds.indices], np.float64)
            p = ParetoDoubleLong()
            for i in range(fc.shape[0]):
                p.addvalue((-fc[i], fr[i]), i)
            out[f"{name}_pareto"] = np.array(sorted(p.allindices()), np.int64)
        out[f"{name}_pick"] = rec.cat("pick", np.int32)
        if "random_aug" in skw:
            out[f"{name}_u_cr"] = rec.cat("uniform")
            nz = [x for k, x in rec.log if k == "normal"]  # per trajectory: the cost rows, then the reward rows
            out[f"{name}_noise_c"] = np.concatenate(nz[0::2]) if nz else np.zeros(0)
            out[f"{name}_noise_r"] = np.concatenate(nz[1::2]) if nz else np.zeros(0)
        else:
            out[f"{name}_u_rew"] = rec.cat("uniform")
            out[f"{name}_u_part"] = rec.cat("choice")
        out[f"{name}_prob50"] = np.asarray(compute_cost_sample_prob(ds.dataset, lambda x: 50 - x), np.float64)
        print(name, "orig", n_orig, "aug", len(ds.aug_data), "filtered", len(getattr(ds, "indices", [])),
              "partner draws", len(rec.cat("choice")), "picks", len(rec.cat("pick")),
              "pareto", len(out.get(f"{name}_pareto", [])))
    for kind in BC_KINDS:
        for gamma in (1.0, 0.99):
            data = make_bc_frontier_dataset(kind)
            data["index"] = np.arange(data["rewards"].shape[0])
            process_bc_dataset(data, BC_COST_LIMIT, gamma, "frontier")
            tag = f"bc_{kind}_{gamma}"
            for k in ("index", "observations", "cost_returns", "rew_returns"):
                out[f"{tag}_{k}"] = data[k]
    np.savez_compressed(os.path.join(HERE, "augment.npz"), **out)
    print("wrote augment.npz:", os.path.getsize(os.path.join(HERE, "augment.npz")), "bytes")


if __name__ == "__main__":
    main()
