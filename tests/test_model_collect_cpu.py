"""CPU-side checks of the recorded model rollouts: the pinned ring as a pure function, the condition the GPU oracle-parity
test relies on (with the oracle alone), the refusals that need no device, and the C ABI of the two new entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import model_collect_cases as K
import model_env_cases as MC
from model_env_oracle import OracleDynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the pinned ring -------------------------------------------------------------------------------------------------
def _brute(cursor, m, capacity, pinned):
    """Row i of the chunk goes to pinned + (cursor - pinned + i) % (capacity - pinned): who ends up where."""
    ring = np.full(capacity, -1, np.int64)
    for i in range(m):
        ring[pinned + (cursor - pinned + i) % (capacity - pinned)] = i
    return ring


def test_ring_spans_pinned_against_a_brute_force_ring():
    from osrl_amd.common.replay import ring_spans, ring_spans_pinned
    rs = np.random.RandomState(0)
    longer = 0
    for _ in range(400):
        capacity = int(rs.randint(1, 40))
        pinned = int(rs.randint(0, capacity))
        cursor = int(rs.randint(pinned, capacity))
        m = int(rs.randint(0, 3 * capacity + 2))
        longer += m > capacity - pinned
        spans = ring_spans_pinned(cursor, m, capacity, pinned)
        assert len(spans) <= 2
        ring = np.full(capacity, -1, np.int64)
        for dst, src, n in spans:
            assert n > 0 and pinned <= dst and dst + n <= capacity and 0 <= src and src + n <= m
            assert (ring[dst:dst + n] == -1).all(), "two spans write one row"
            ring[dst:dst + n] = np.arange(src, src + n)
        np.testing.assert_array_equal(ring, _brute(cursor, m, capacity, pinned), err_msg=str((cursor, m, capacity, pinned)))
        assert (ring[:pinned] == -1).all()
        if pinned == 0:
            assert spans == ring_spans(cursor, m, capacity)
    assert longer > 50  # chunks longer than the ring are among the cases
    for bad in ((3, 1, 8, 4), (8, 1, 8, 4), (0, 1, 4, 4), (0, 1, 4, -1)):
        with pytest.raises(ValueError):
            ring_spans_pinned(*bad)


def _rows(n, od=4, ad=2, seed=0):
    return K.store_rows(n, od, ad, seed)


def test_a_pinned_store_on_the_host():
    """The constructor's checks, the ring and the checkpoint dictionary, on a CPU store (torch copies only)."""
    from osrl_amd.common.replay import ReplayStore
    d = _rows(10)
    for kw in (dict(pinned_rows=11, capacity=32), dict(pinned_rows=10, capacity=10), dict(pinned_rows=4),
               dict(pinned_rows=-2, capacity=32)):
        with pytest.raises(ValueError):
            ReplayStore(d, "cpu", **kw)
    plain, s = ReplayStore(d, "cpu", capacity=16), ReplayStore(d, "cpu", capacity=16, pinned_rows=6)
    assert plain.pinned_rows == 0 and "pinned_rows" not in plain.state_dict() and s.state_dict()["pinned_rows"] == 6
    assert s._cursor == 10 and ReplayStore(d, "cpu", capacity=10, pinned_rows=6)._cursor == 6
    keep = [t[:6].clone() for t in s.tables]
    ring = s.tables[0].numpy().copy()
    cursor = 10
    for i, m in enumerate((5, 9, 23, 1)):
        chunk = _rows(m, seed=10 + i)
        s.append(chunk)
        for j in range(m):
            ring[6 + (cursor - 6 + j) % 10] = chunk["observations"][j]
        cursor = 6 + (cursor - 6 + m) % 10
        assert s._cursor == cursor and s.n_rows == min(10 + sum((5, 9, 23, 1)[:i + 1]), 16) and int(s._live.item()) == s.n_rows
        np.testing.assert_array_equal(s.tables[0].numpy(), ring)
        for t, k in zip(s.tables, keep):
            assert torch.equal(t[:6], k)
    twin = ReplayStore(d, "cpu", capacity=16, pinned_rows=6)
    twin.load_state_dict(s.state_dict())
    more = _rows(7, seed=20)
    s.append(more)
    twin.append(more)
    for a, b in zip(s.tables, twin.tables):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        plain.load_state_dict(s.state_dict())
    with pytest.raises(ValueError):
        s.load_state_dict(plain.state_dict())


# ---- what the GPU oracle-parity test relies on -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mean", "member"])
def test_case_b_cost_margin_with_the_oracle_alone(mode):
    """Case B's weights, starts and actions (constant policy, injected noise), rolled out by the oracle: at most 2 % of the
    rows within 1e-3 of the cost threshold, and both cost values occur."""
    c = K.CASES["B"]
    o = OracleDynamics(MC.dyn_state_dict(c["od"], c["ad"], c["hidden"], c["M"], K.DYN_SEED["B"]))
    s = MC.start_rows(K.E, c["od"]).astype(np.float64)
    acts = K.host_actions(c["ad"])
    raw = []
    for t in range(K.HORIZON):
        r = o.env_step(s, acts[t], mode, 2, clamp=True, lam=K.LAMBDA, max_action=MC.MAX_ACTION)
        raw.append(r["cost_raw"])
        s = r["s_next"]
    raw = np.concatenate(raw)
    near = int((np.abs(raw - 0.5) <= 1e-3).sum())
    print(f"case B {mode}: {near} of {raw.size} rows within 1e-3 of the threshold, {int((raw > 0.5).sum())} costs of 1, "
          f"closest {np.abs(raw - 0.5).min():.4f}")
    assert near <= 0.02 * raw.size and 0 < (raw > 0.5).sum() < raw.size
    assert (K.sigma() == 0).sum() >= 3 and (K.sigma() > 0).sum() >= 3
    assert np.isnan(K.eps_rows(c["ad"], poison=True)[:, K.sigma() == 0]).all()


# ---- refusals that need no device ------------------------------------------------------------------------------------
def test_check_model_target_on_the_host():
    from osrl_amd.common.replay import ReplayStore
    from osrl_amd.engine.collect import check_model_target
    od, ad, rows = 4, 2, 12
    d = _rows(10)
    grows = lambda **kw: ReplayStore(d, "cpu", capacity=64, **kw)  # noqa: E731
    weighted = grows()
    weighted.weighted = True  # (the flag alone: building the cdf is device work)
    start = grows()
    assert check_model_target(None, None, od, ad, rows, None) is None
    assert check_model_target(grows(), start, od, ad, rows, None) is None
    assert check_model_target(grows(state_init=True), None, od, ad, rows, None) is None
    w = check_model_target(weighted, start, od, ad, rows, 2.5)
    assert w.dtype == torch.float64 and w.shape == (rows,) and (w == 2.5).all()
    assert torch.equal(check_model_target(weighted, None, od, ad, rows, np.arange(rows)), torch.arange(rows, dtype=torch.float64))
    for into, st, sp in ((grows(state_init=True), start, None), (weighted, None, None), (grows(), None, 1.0),
                         (None, None, 1.0), (weighted, None, np.ones(rows + 1)), (weighted, None, -1.0),
                         (ReplayStore(d, "cpu"), None, None), (grows(), ReplayStore(_rows(10, od + 1), "cpu"), None),
                         (ReplayStore(_rows(10, od + 1), "cpu", capacity=64), None, None),
                         (ReplayStore(_rows(10, od, ad + 1), "cpu", capacity=64), None, None),
                         (None, np.zeros((3, od), np.float32), None)):
        with pytest.raises(ValueError):
            check_model_target(into, st, od, ad, rows, sp)


def test_cdt_has_no_collect_model_and_the_mlp_trainers_do():
    from osrl_amd.algorithms import BCQLTrainer, BCTrainer, BEARLTrainer, CDTTrainer, COptiDICETrainer, CPQTrainer
    assert not hasattr(CDTTrainer, "collect_model")
    for t in (BCTrainer, CPQTrainer, BCQLTrainer, BEARLTrainer, COptiDICETrainer):
        assert callable(getattr(t, "collect_model")) and callable(getattr(t, "model_collector"))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """-1 for a missing table, descriptor or pointer: the checks run before the first HIP call (no device here)."""
    from osrl_amd import _lib as L
    lib = L.load()
    env, rec = L.ModelEnvT(), L.CollectT()
    one = 0x1000  # (never dereferenced: every call below fails a check first)
    assert lib.osrl_model_env_collect(None, rec, one, one, one, 4, one, one, None, 1, None) == -1
    assert lib.osrl_model_env_collect(env, None, one, one, one, 4, one, one, None, 1, None) == -1
    env.episode_len = 3
    assert lib.osrl_model_env_collect(env, rec, one, one, one, 4, one, one, None, 1, None) == -1  # no tables
    for k, _ in L.CollectT._fields_[:11]:
        setattr(rec, k, one)
    rec.seed = None
    assert lib.osrl_model_env_collect(env, rec, one, one, one, 4, one, one, None, 1, None) == -1  # neither seed nor eps_in
    rec.seed = one
    assert lib.osrl_model_env_collect(env, rec, one, one, one, 4, one, one, None, 1, None) == -1  # an empty model descriptor
    for k in range(11):
        rec2 = L.CollectT.from_buffer_copy(rec)
        setattr(rec2, L.CollectT._fields_[k][0], None)
        if L.CollectT._fields_[k][0] == "seed":
            continue
        assert lib.osrl_model_env_collect(env, rec2, one, one, one, 4, one, one, None, 1, None) == -1
    ok = [one, 8, None, 0, 4, one, 0, one, one, 4, one, one, one, one, 2, None]
    for i, badv in ((0, None), (1, 0), (3, -1), (4, 0), (5, None), (7, None), (8, None), (9, 3), (10, None), (11, None),
                    (12, None), (13, None), (14, 0)):
        args = list(ok)
        args[i] = badv
        assert lib.osrl_model_env_branch(*args) == -1, i


# ---- header <-> _lib.py ----------------------------------------------------------------------------------------------
def _ctype_of(decl):
    from osrl_amd import _lib as L
    decl = re.sub(r"/\*.*?\*/", "", decl).strip()
    structs = {"osrl_model_env_t": L.ModelEnvT, "osrl_collect_t": L.CollectT}
    if "*" in decl:
        base = decl.replace("const", "").split("*")[0].strip()
        return C.POINTER(structs[base]) if base in structs else C.c_void_p
    base = decl.replace("const", "").split()[0]
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float}[base]


@pytest.mark.parametrize("name", ["osrl_model_env_collect", "osrl_model_env_branch"])
def test_prototypes_agree_with_the_header(name):
    from osrl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "osrl_amd.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.S)
    assert m, name
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    want = [_ctype_of(p) for p in params]
    assert L.PROTOTYPES[name] == want, (name, L.PROTOTYPES[name], want)
    assert hasattr(L.load(), name)


def test_struct_layouts_agree_with_the_compiled_header(tmp_path):
    from osrl_amd import _lib as L
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc is not None, "a C compiler is required"
    pairs = [("osrl_collect_t", L.CollectT), ("osrl_model_env_t", L.ModelEnvT)]
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
        for cname, cls in pairs:
            f.write(f'  printf("{cname} %zu", sizeof({cname}));\n')
            for fname, _ in cls._fields_:
                f.write(f'  printf(" %zu", offsetof({cname}, {fname}));\n')
            f.write('  printf("\\n");\n')
        f.write("  return 0;\n}\n")
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (cname, cls) in zip(out, pairs):
        tok = line.split()
        assert tok[0] == cname
        assert [int(x) for x in tok[1:]] == [C.sizeof(cls)] + [getattr(cls, fname).offset for fname, _ in cls._fields_], cname
