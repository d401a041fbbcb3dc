"""Timings of the CDT dataset recipe on device: ``SequenceStore.from_dataset`` without augmentation, with the Pareto
augmentation (augment_percent = 0.2, cost_sample, the reference's CDT defaults) and with random_aug = 0.2, at 1 M
transitions x obs 76 (arrays already resident, as profiles/r1_ingest_bench.json); and the numpy restatement of the
augmentation step (tests/augment_oracle.py, reference-shaped host loops) on the same tables.

    python tools/augment_probe.py > profiles/augment_probe.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import augment_oracle as AO
    from augment_cases import make_augment_dataset
    from oracle import ingest_oracle as IO
    from osrl_amd.common.replay import SequenceStore
    data = make_augment_dataset(seed=0, n_traj=1000, od=76, ad=2, max_len=2000)
    n = int(data["rewards"].shape[0])
    dev = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
    torch.cuda.synchronize()

    def timed(fn, reps=7):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    out = {"transitions": n, "obs_dim": 76, "trajectories": 1000, "rows": []}
    mk = lambda **kw: SequenceStore.from_dataset(dev, 10, "cuda:0", cost_sample=True, seed=1, **kw)  # noqa: E731
    base = timed(lambda: mk())
    out["rows"].append(dict(what="from_dataset(cost_sample=True)", seconds=round(base, 6)))
    st = mk(augment_percent=0.2)
    t = timed(lambda: mk(augment_percent=0.2))
    out["rows"].append(dict(what="from_dataset(cost_sample=True, augment_percent=0.2)", seconds=round(t, 6),
                            added_seconds=round(t - base, 6), augmented_trajectories=st.n_augmented,
                            rows=int(st.ret.shape[0])))
    st = mk(random_aug=0.2)
    t = timed(lambda: mk(random_aug=0.2))
    out["rows"].append(dict(what="from_dataset(cost_sample=True, random_aug=0.2)", seconds=round(t, 6),
                            added_seconds=round(t - base, 6), augmented_trajectories=st.n_augmented))
    trajs = IO.process_sequence_dataset(data, False)
    tabs = {k: np.concatenate([tr[k] for tr in trajs]) for k in AO.KEYS}
    lens = np.array([len(tr["costs"]) for tr in trajs], np.int64)
    tabs["traj_len"], tabs["traj_start"] = lens, np.concatenate([[0], np.cumsum(lens)[:-1]])
    rs = np.random.RandomState(0)
    draws = dict(pick=np.tile(np.arange(10, dtype=np.int32), 600), u_rew=rs.uniform(size=6000),
                 u_part=rs.uniform(size=6000))
    t0 = time.perf_counter()
    AO.augmentation(tabs, deg=3, augment_percent=0.2, min_reward=5, draws=draws)
    out["rows"].append(dict(what="numpy restatement of augmentation() on the host (tables in host memory)",
                            seconds=round(time.perf_counter() - t0, 6)))
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
