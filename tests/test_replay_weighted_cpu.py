"""Weighted transition sampling (ReplayStore.set_sample_prob, include/osrl_amd.h osrl_replay_gather_w) without a GPU:
the draw rule restated in numpy (tests/replay_weighted_util.py) never lands on a zero-weight row, the new entry points are
declared, mirrored and refuse bad arguments before any launch, and bad weights raise before any device work."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from replay_weighted_util import (U64_MAX, make_weights, philox4x32_10, replay_words, table_from_weights,  # noqa: E402
                                  uniform_indices, weighted_indices)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("osrl_replay_gather_w", "osrl_step_begin_w", "osrl_step_begin_peer_w", "osrl_weights_cum_u64",
       "osrl_weights_cum_u64_ws_elems")


def test_philox_restatement_known_answers():
    """Philox4x32-10's published known-answer vectors (Random123 kat_vectors): all-zero and all-ones counter / key."""
    r = philox4x32_10(np.zeros((1, 4), np.uint32), 0, 0)[0]
    assert [int(v) for v in r] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    r = philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert [int(v) for v in r] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    w = replay_words(11 * 1000003, 3, 8)
    assert w.dtype == np.uint64 and len(set(w.tolist())) == 8
    assert ((uniform_indices(w, 5000) >= 0) & (uniform_indices(w, 5000) < 5000)).all()


TABLES = {
    "leading": [0, 0, 0, 1, 2, 3],
    "trailing": [1, 2, 3, 0, 0, 0],
    "interior": [1, 0, 0, 0, 2, 0, 3, 0, 0, 4],
    "all three": [0, 0, 5, 0, 0, 0, 1, 1, 0, 7, 0, 0],
    "one row": [3.5],
    "one heavy row": [0, 1e-30, 0, 1e30, 0, 1.0, 0],
    "random": None,
}


@pytest.mark.parametrize("name", list(TABLES))
def test_a_zero_weight_row_is_never_drawn(name):
    """Every word that could sit on an edge of the rule: 0, 2^64 - 1, every table entry and its two neighbours."""
    w = np.asarray(make_weights(200, seed=4) if TABLES[name] is None else TABLES[name], np.float64)
    cum = table_from_weights(w)
    assert (np.diff(cum.astype(object)) >= 0).all() and cum[-1] == U64_MAX
    zero = np.flatnonzero(w == 0)
    assert (cum[zero] == np.concatenate([[np.uint64(0)], cum])[zero]).all()  # a zero row repeats its predecessor
    words = {0, 2 ** 64 - 1, 2 ** 64 - 2, 1, 2 ** 63}
    for c in cum.tolist():
        words |= {c, max(c - 1, 0), min(c + 1, 2 ** 64 - 1)}
    words = np.array(sorted(words), np.uint64)
    idx = weighted_indices(cum, words)
    assert idx.min() >= 0 and idx.max() < len(w)
    assert (w[idx] > 0).all(), (name, words[w[idx] == 0], idx[w[idx] == 0])
    assert (np.diff(idx) >= 0).all()  # (the index is a non-decreasing function of the word)
    # ... and it is the rule as stated: the first entry that exceeds min(word, 2^64 - 2)
    for u, i in zip(words.tolist(), idx.tolist()):
        u = min(u, 2 ** 64 - 2)
        assert int(cum[i]) > u and (i == 0 or int(cum[i - 1]) <= u)
    # every row the table resolves (an entry above its predecessor's) is reachable
    reach, prev = set(idx.tolist()), np.concatenate([[np.uint64(0)], cum])
    assert reach == set(np.flatnonzero(cum > prev[:-1]).tolist())


def test_frequencies_of_the_restatement_with_the_gpu_tests_seed():
    """The condition test_gpu_replay_weighted.py's frequency test asserts on the device's draws, checked here on the
    restatement with the same seed, weights, batch and steps: zero rows never, every other count within six standard
    deviations of N p.  (The bound is a condition on the rule and the generator, fixed before any GPU ran it.)"""
    w = np.array([1, 2, 3, 4, 0, 0, 5, 5], np.float64)
    cum = table_from_weights(w)
    B, steps, seed = 2000, 100, 5 * 1000003
    counts = np.zeros(8, np.int64)
    for s in range(1, steps + 1):
        counts += np.bincount(weighted_indices(cum, replay_words(seed, s, B)), minlength=8)
    N, p = B * steps, w / w.sum()
    assert counts[4] == 0 and counts[5] == 0 and counts.sum() == N
    assert (np.abs(counts - N * p) <= 6 * np.sqrt(N * p * (1 - p))).all(), (counts, N * p)


def test_header_prototypes_and_restypes_agree():
    from osrl_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, "include", "osrl_amd.h")).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        m = re.search(r'\b(int|int64_t)\s+' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, name
        args = [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
        assert len(args) == len(L.PROTOTYPES[name]), name
        assert (m.group(1) == "int64_t") == (name in L.RESTYPES), name
        assert hasattr(lib, name)
        # the weighted form is the old prototype plus the table, in front of the stream
        old = name[:-2]
        if name.endswith("_w") and old in L.PROTOTYPES:
            assert len(L.PROTOTYPES[name]) == len(L.PROTOTYPES[old]) + 1
            mo = re.search(r'\bint\s+' + old + r'\s*\(([^)]*)\)\s*;', hdr)
            a_old = [" ".join(a.split()) for a in mo.group(1).split(",")]
            a_new = [" ".join(a.split()) for a in m.group(2).split(",")]
            assert a_new == a_old[:-1] + ["const uint64_t* cum"] + a_old[-1:], name


def test_step_descriptor_mirror_matches_the_header(tmp_path):
    """osrl_mlp_step_t gained the trailing table pointer: its ctypes mirror against the C header."""
    from osrl_amd import _lib as L
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    names = {"in_": "in"}
    with open(src, "w") as f:
        f.write('#include "osrl_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n')
        f.write('  printf("%zu", sizeof(osrl_mlp_step_t));\n')
        for fname, _ in L.MlpStepT._fields_:
            f.write(f'  printf(" %zu", offsetof(osrl_mlp_step_t, {names.get(fname, fname)}));\n')
        f.write('  printf("\\n");\n  return 0;\n}\n')
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    want = [C.sizeof(L.MlpStepT)] + [getattr(L.MlpStepT, fname).offset for fname, _ in L.MlpStepT._fields_]
    assert [int(x) for x in out] == want
    assert L.MlpStepT._fields_[-1][0] == "cum" and L.MlpStepT.cum.offset + 8 == C.sizeof(L.MlpStepT)
    assert L.MlpStepT().cum is None  # zero = uniform


def test_bad_arguments_are_refused_before_any_launch():
    from osrl_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(16)  # (never dereferenced: every call below fails its argument check first)
    assert lib.osrl_weights_cum_u64_ws_elems(1) >= 2 and lib.osrl_weights_cum_u64_ws_elems(1 << 27) >= (1 << 15) + 1
    assert lib.osrl_weights_cum_u64(None, 8, one, one, None) == -1
    assert lib.osrl_weights_cum_u64(one, 8, None, one, None) == -1
    assert lib.osrl_weights_cum_u64(one, 8, one, None, None) == -1
    assert lib.osrl_weights_cum_u64(one, 0, one, one, None) == -1
    assert lib.osrl_weights_cum_u64(one, (1 << 28) + 1, one, one, None) == -1
    src, dst = (C.c_void_p * 1)(16), (C.c_void_p * 1)(16)
    w, sc = (C.c_int32 * 1)(1), (C.c_float * 1)(1.0)
    g = lambda nf, s, d, ww, n, B: lib.osrl_replay_gather_w(nf, s, d, ww, sc, n, B, None, 0, 1, None, one, None)  # noqa: E731
    assert g(0, src, dst, w, 8, 4) == -1 and g(9, src, dst, w, 8, 4) == -1
    assert g(1, None, dst, w, 8, 4) == -1 and g(1, src, None, w, 8, 4) == -1 and g(1, src, dst, None, 8, 4) == -1
    assert g(1, src, dst, w, 0, 4) == -1 and g(1, src, dst, w, 8, 0) == -1
    assert g(1, (C.c_void_p * 1)(None), dst, w, 8, 4) == -1 and g(1, src, dst, (C.c_int32 * 1)(0), 8, 4) == -1
    b = lambda st, nf, s, n, B: lib.osrl_step_begin_w(st, 0.9, 0.999, 0, None, None, 1, 1, None, 0, 0, 0, nf, s, dst, w, sc, n, B,  # noqa: E731
                                                     0, 1, one, None)
    assert b(None, 1, src, 8, 4) == -1 and b(one, 9, src, 8, 4) == -1 and b(one, 1, None, 8, 4) == -1
    assert b(one, 1, src, 0, 4) == -1 and b(one, 1, src, 8, 0) == -1
    bp = lambda st, peer, nf, n: lib.osrl_step_begin_peer_w(st, peer, 0.9, 0.999, 0, None, None, 1, 1, None, 0, 0, 0, nf, src,  # noqa: E731
                                                            dst, w, sc, n, 4, 0, 1, one, None)
    assert bp(None, None, 1, 8) == -1 and bp(one, one, 1, 8) == -1 and bp(one, None, -1, 8) == -1 and bp(one, None, 1, 0) == -1


class _NoDevice:
    """A ReplayStore shell without tables: set_sample_prob must refuse bad host weights before it touches a device."""

    def __new__(cls, n, shard=slice(None)):
        from osrl_amd.common.replay import ReplayStore
        s = ReplayStore.__new__(ReplayStore)
        s.n_total, s._shard, s.weighted, s.sample_epoch = n, shard, False, 0
        s._cum_buf = s._cum_ws = s._w64 = None
        s.n_rows = len(range(n)[shard])
        s.device = "cuda:0"
        return s


@pytest.mark.parametrize("bad", ["negative", "nan", "inf", "length", "zero", "zero shard"])
def test_bad_weights_raise_before_any_device_work(bad, monkeypatch):
    from osrl_amd import _lib as L
    monkeypatch.setattr(L, "load", lambda: pytest.fail("the library was reached"))
    n = 10
    w = np.ones(n)
    store = _NoDevice(n)
    if bad == "negative":
        w[3] = -1e-9
    elif bad == "nan":
        w[3] = np.nan
    elif bad == "inf":
        w[3] = np.inf
    elif bad == "length":
        w = np.ones(n + 1)
    elif bad == "zero":
        w[:] = 0
    else:  # all of rank 1's mass is zero: every rank normalises its own shard
        store = _NoDevice(n, slice(1, n, 2))
        w[1::2] = 0
    with pytest.raises(ValueError):
        store.set_sample_prob(w)
    import torch
    with pytest.raises(ValueError):
        store.set_sample_prob(torch.as_tensor(w))
    assert store.cum is None and not store.weighted and store.sample_epoch == 0
    store.set_sample_prob(None)  # uniform -> uniform: nothing to do, no epoch
    assert store.sample_epoch == 0


def test_sample_prob_is_a_trailing_keyword():
    import inspect
    from osrl_amd.common.replay import ReplayStore
    params = list(inspect.signature(ReplayStore.__init__).parameters.values())
    assert params[-1].name == "sample_prob" and params[-1].default is None
    assert list(inspect.signature(ReplayStore.set_sample_prob).parameters) == ["self", "weights"]
