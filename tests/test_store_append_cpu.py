"""Stores that grow (ReplayStore(capacity=) / append, include/osrl_amd.h osrl_replay_gather_n) without a GPU: the ring
placement against a brute-force modular one, the ring's table contents and ``is_init`` on a host-resident store (append
is torch copies only), the refusals that must come before any device work, and the C boundary of the new entry points.
The device's draws over a grown store are tests/test_gpu_store_append.py."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from osrl_amd import _lib as L  # noqa: E402
from osrl_amd.common.replay import FIELDS, ReplayStore, ring_spans, synthetic_transitions  # noqa: E402

NEW = ("osrl_replay_gather_n", "osrl_step_begin_peer_n")


@pytest.mark.parametrize("cursor", range(7))
@pytest.mark.parametrize("m", range(0, 23))
def test_ring_spans_is_the_modular_placement(cursor, m):
    """Capacity 7, every cursor, chunks from empty to three laps: applying the spans in order == writing row i to
    (cursor + i) % 7 one by one (later rows win); at most two spans, each contiguous and inside both arrays."""
    cap = 7
    want = np.full(cap, -1, np.int64)
    for i in range(m):
        want[(cursor + i) % cap] = i
    spans = ring_spans(cursor, m, cap)
    assert len(spans) <= 2
    got = np.full(cap, -1, np.int64)
    chunk = np.arange(m)
    for dst, src, n in spans:
        assert n > 0 and 0 <= dst and dst + n <= cap and 0 <= src and src + n <= m
        got[dst:dst + n] = chunk[src:src + n]
    np.testing.assert_array_equal(got, want)
    assert sum(n for _, _, n in spans) == min(m, cap)


@pytest.mark.parametrize("bad", [(7, 1, 7), (-1, 1, 7), (0, -1, 7), (0, 1, 0)])
def test_ring_spans_refuses_nonsense(bad):
    with pytest.raises(ValueError):
        ring_spans(*bad)


def _data(n, seed, od=5, ad=2):
    d = synthetic_transitions(n, od, ad, seed=seed)
    d["timeouts"] = (np.arange(n) % 9 == 8).astype(np.float32)
    return d


def _done(d):
    return np.logical_or(d["terminals"] == 1, d["timeouts"] == 1).astype(np.float32)


def _init(d):
    return np.concatenate([[1.0], _done(d)[:-1]]).astype(np.float32)


def test_ring_contents_on_a_host_store():
    """Capacity 16, 10 rows, then chunks of 4, 9 (wraps) and 40 (laps twice): all seven tables equal the numpy ring,
    ``is_init`` restarting with 1 at every chunk; the live count saturates, ``version`` counts the appends, ``live(i)``
    is the live slice, and the tables never move."""
    cap = 16
    d0 = _data(10, 1)
    s = ReplayStore(d0, "cpu", state_init=True, capacity=cap, reward_scale=0.5)
    assert (s.n_rows, s.capacity, s.version, s.n_fields) == (10, cap, 0, 7) and int(s._live[0]) == 10
    ptrs = [t.data_ptr() for t in s.tables]
    cols = lambda d: [np.asarray(x, np.float32).reshape(len(d["rewards"]), -1) for x in  # noqa: E731
                      [d[k] for k in FIELDS[:5]] + [_done(d), _init(d)]]
    ring = [np.zeros((cap, w), np.float32) for w in s.widths]
    for r, c in zip(ring, cols(d0)):
        r[:10] = c
    cursor, live = 10, 10
    for v, (m, seed) in enumerate([(4, 2), (9, 3), (40, 4)], 1):
        d = _data(m, seed)
        if v == 2:  # tensors and the ``done`` key are taken as well
            d = {k: torch.from_numpy(x) for k, x in d.items()}
            d["done"] = torch.from_numpy(_done({k: x.numpy() for k, x in d.items()}))
            dn = {k: x.numpy() for k, x in d.items()}
        else:
            dn = d
        s.append(d)
        for r, c in zip(ring, cols(dn)):
            for i in range(m):
                r[(cursor + i) % cap] = c[i]
        cursor, live = (cursor + m) % cap, min(live + m, cap)
        assert (s.n_rows, s.version, s._cursor) == (live, v, cursor) and int(s._live[0]) == live
        for i, r in enumerate(ring):
            np.testing.assert_array_equal(s.tables[i].numpy(), r, err_msg=f"append {v}, table {i}")
            np.testing.assert_array_equal(s.live(i).numpy(), r[:live])
    assert [t.data_ptr() for t in s.tables] == ptrs
    s.append(_data(0, 5))  # an empty chunk changes nothing
    assert s.version == 3 and s.n_rows == cap


def test_launch_arguments_carry_the_capacity_and_the_live_word():
    fixed = ReplayStore(_data(10, 1), "cpu")
    grown = ReplayStore(_data(10, 1), "cpu", capacity=32)
    dst = [torch.zeros(4, w) for w in fixed.widths]
    a, b = fixed.gather_args(dst), grown.gather_args(dst)
    assert a[5] == 10 and a[-1] is None and fixed.capacity is None and fixed.live(0).shape[0] == 10
    assert b[5] == 32 and b[-1] == grown._live.data_ptr() and grown._live.dtype == torch.int64
    grown.append(_data(7, 2))
    assert grown.gather_args(dst)[-1] == b[-1] and grown.gather_args(dst)[5] == 32 and grown.n_rows == 17
    assert "n_rows_dev" in dict(L.MlpStepT._fields_) and L.MlpStepT().n_rows_dev is None  # zero = a fixed store


def test_refusals_come_before_any_work():
    d = _data(10, 1)
    with pytest.raises(ValueError):
        ReplayStore(d, "cpu", capacity=9)
    with pytest.raises(ValueError):
        ReplayStore(d, "cpu", capacity=32, rank=0, world=2)
    with pytest.raises(ValueError):
        ReplayStore(d, "cpu").append(_data(3, 2))  # a fixed store
    s = ReplayStore(d, "cpu", capacity=32)
    before = [t.clone() for t in s.tables]
    with pytest.raises(ValueError):
        s.append(_data(3, 2, od=6))
    with pytest.raises(ValueError):
        s.append(_data(3, 2, ad=3))
    short = _data(3, 2)
    short["rewards"] = short["rewards"][:2]
    with pytest.raises(ValueError):
        s.append(short)
    for k in ("observations", "costs", "timeouts"):
        miss = _data(3, 2)
        del miss[k]
        with pytest.raises(ValueError):
            s.append(miss)
    with pytest.raises(ValueError):
        s.append(_data(3, 2), sample_prob=np.ones(3))  # a uniform store takes no weights
    with pytest.raises(ValueError):
        s.check_append_widths(observations=6)
    s.check_append_widths(observations=5, next_observations=5, actions=2)
    assert s.n_rows == 10 and s.version == 0 and all(torch.equal(a, b) for a, b in zip(before, s.tables))


def test_header_declares_the_new_entry_points_and_the_mirror_knows_them():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, "include", "osrl_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f"{name} is not declared in include/osrl_amd.h"
        assert name in L.PROTOTYPES, name
    # one more pointer than the call each extends, just before the stream
    for new, old in zip(NEW, ("osrl_replay_gather_w", "osrl_step_begin_peer_w")):
        assert len(L.PROTOTYPES[new]) == len(L.PROTOTYPES[old]) + 1
        assert L.PROTOTYPES[new][:len(L.PROTOTYPES[old]) - 1] == L.PROTOTYPES[old][:-1]
    step_t = re.search(r'typedef\s+struct\s*{([^}]*)}\s*osrl_mlp_step_t', hdr).group(1)
    assert re.search(r'const\s+int64_t\s*\*\s*n_rows_dev\s*;', step_t)
    # the window gather has ONE entry point: the live word is a field of its descriptor, NULL on a fixed store
    names = re.findall(r'\bint\s+(osrl_seq_window_gather\w*)\s*\(', hdr)
    assert names == ["osrl_seq_window_gather"] and [n for n in L.PROTOTYPES if n.startswith("osrl_seq_window_gather")] == names
    seq_t = re.search(r'typedef\s+struct\s*{([^}]*)}\s*osrl_seq_gather_t', hdr).group(1)
    assert re.search(r'const\s+int32_t\s*\*\s*n_traj_dev\s*;', seq_t) and L.SeqGatherT().n_traj_dev is None


def test_the_window_gather_refuses_bad_descriptors_before_any_launch():
    """A null descriptor, every null table or output pointer, and n_traj / B / T below 1: -1, nothing launched."""
    lib = L.load()
    required = ("obs", "act", "returns", "cost_returns", "costs", "traj_start", "traj_len", "o_states", "o_actions",
                "o_returns", "o_cost_returns", "o_time_steps", "o_mask", "o_episode_cost", "o_costs")

    def desc(**over):  # (16: never dereferenced, every call below fails its argument check first)
        g = L.SeqGatherT()
        for k in required:
            setattr(g, k, 16)
        g.n_traj, g.B, g.T, g.od, g.ad = 3, 2, 4, 5, 2
        for k, v in over.items():
            setattr(g, k, v)
        return g
    assert lib.osrl_seq_window_gather(None, None, None) == -1
    for k in required:
        assert lib.osrl_seq_window_gather(desc(**{k: None}), None, None) == -1, k
    for k in ("n_traj", "B", "T"):
        assert lib.osrl_seq_window_gather(desc(**{k: 0}), None, None) == -1, k
