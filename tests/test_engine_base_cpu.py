"""The step engines' shared base (osrl_amd/engine/_step.py): what of it needs no device."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_noise_layout_views_one_flat_buffer_back_to_back():
    from osrl_amd.engine._step import StepEngine
    flat, views = StepEngine.noise_layout({"a": (3, 5), "b": (2,), "c": (1, 1, 3)}, "cpu")
    assert flat.dtype == torch.float32 and flat.numel() == 20 and not flat.any()
    assert list(views) == ["a", "b", "c"]
    assert [tuple(v.shape) for v in views.values()] == [(3, 5), (2,), (1, 1, 3)]
    assert [(v.data_ptr() - flat.data_ptr()) // 4 for v in views.values()] == [0, 15, 17]
    views["b"][1] = 7.0  # a write through a view lands in the flat buffer (what the Philox fill and the kernels share)
    views["c"][0, 0, 2] = -2.0
    assert flat[16].item() == 7.0 and flat[19].item() == -2.0 and flat.count_nonzero().item() == 2
    flat[0] = 3.0
    assert views["a"][0, 0].item() == 3.0


def test_noise_layout_pads_to_four_floats_and_takes_an_empty_mapping():
    from osrl_amd.engine._step import StepEngine
    flat, views = StepEngine.noise_layout({"x": (5,), "y": (2, 2)}, "cpu")  # 9 floats -> 12
    assert flat.numel() == 12 and (views["y"].data_ptr() - flat.data_ptr()) // 4 == 5
    flat, views = StepEngine.noise_layout({}, "cpu")
    assert flat.numel() == 0 and views == {}
