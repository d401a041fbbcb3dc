"""Host side of the CDT act latency path (csrc/cdt_act.hip, include/osrl_amd.h ``osrl_cdt_policy_*``).

``CDTTrainer.rollout`` (cdt.py:436-518) on a host environment asks for one action per env step over the window of the
last ``seq_len`` timesteps.  ``CDTFastPolicy`` keeps that window on the device, with every token's cached hidden state:
``reset`` / ``step`` write the observation into a pinned, device-mapped block through a numpy view, make one C call
(the step's launch chain + a spin on the published sequence number) and read the action back through another view.
Window updates use the existing loop's fp32 expressions (``returns - float(reward)``, ``costs - cost``), on device.

The kernels read the packed forward weight copies and the biases of the model's flat group -- the buffers the fused
AdamW step, ``load_state_dict`` and ``repack()`` keep current -- so training between evaluations needs no rebuild.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib as L
from .core import cur_stream

MAX_TOKENS, MAX_E, MAX_HEAD_DIM = 256, 512, 128


def unsupported(model) -> Optional[str]:
    """Why ``model`` is outside the fast path's domain (None: inside)."""
    S = model.seq_repeat * model.seq_len + int(model.cost_prefix)
    if S > MAX_TOKENS:
        return f"{S} tokens per sequence > {MAX_TOKENS} (seq_repeat * seq_len + cost_prefix)"
    if model.embedding_dim > MAX_E:
        return f"embedding_dim {model.embedding_dim} > {MAX_E}"
    if model.embedding_dim // model.num_heads > MAX_HEAD_DIM:
        return f"head_dim {model.embedding_dim // model.num_heads} > {MAX_HEAD_DIM}"
    if model.action_head_layers > L.MAX_LAYERS:
        return f"action_head_layers {model.action_head_layers} > {L.MAX_LAYERS}"
    if 2 * model.action_dim > 1024:
        return f"action_dim {model.action_dim} > 512"
    return None


class CDTFastPolicy:
    def __init__(self, model):
        why = unsupported(model)
        if why is not None:
            raise NotImplementedError("the CDT act latency path does not support: " + why)
        m = self.model = model
        g = m.groups["cdt"]
        self.device = torch.device(m.device)
        pk = lambda key: g.pf.data_ptr() + 4 * g.f_off[key]  # noqa: E731  packed forward copy
        cv = lambda key: g.view(key).data_ptr()  # noqa: E731  canonical tensor
        d = L.CdtPolicyT()
        d.state_dim, d.action_dim, d.seq_len = m.state_dim, m.action_dim, m.seq_len
        d.embedding_dim, d.num_layers, d.num_heads = m.embedding_dim, m.num_layers, m.num_heads
        d.use_rew, d.use_cost, d.cost_prefix = int(m.use_rew), int(m.use_cost), int(m.cost_prefix)
        d.cost_transform = int(m.cost_transform_on)
        d.add_cost_feat, d.mul_cost_feat, d.cat_cost_feat = int(m.add_cost_feat), int(m.mul_cost_feat), int(m.cat_cost_feat)
        chain = list(m.head_hidden_keys) + [m.head_out_key]
        d.head_layers = len(chain)
        d.head_out_width = 2 * m.action_dim if m.stochastic else m.action_dim
        d.max_action = float(m.max_action)
        if m.time_emb:
            d.te = cv("cdt.timestep_emb.weight")
            d.te_rows = g.layout["cdt.timestep_emb.weight"][1][0]
        d.state_w, d.state_b = cv("cdt.state_emb.weight"), cv("cdt.state_emb.bias")
        d.action_w, d.action_b = cv("cdt.action_emb.weight"), cv("cdt.action_emb.bias")
        if m.use_rew:
            d.return_w, d.return_b = cv("cdt.return_emb.weight"), cv("cdt.return_emb.bias")
        if m.use_cost:
            d.cost_w, d.cost_b = cv("cdt.cost_emb.weight"), cv("cdt.cost_emb.bias")
        if m.cost_prefix:
            d.prefix_w, d.prefix_b = cv("cdt.prefix_emb.weight"), cv("cdt.prefix_emb.bias")
        d.emb_g, d.emb_b = cv("cdt.emb_norm.weight"), cv("cdt.emb_norm.bias")
        d.out_g, d.out_b = cv("cdt.out_norm.weight"), cv("cdt.out_norm.bias")
        for i, key in enumerate(chain):
            d.head_w[i], d.head_b[i] = pk(key), cv(key[:-len("weight")] + "bias")
        layers = (L.CdtLayerT * m.num_layers)()
        for l in range(m.num_layers):
            p, y = f"cdt.blocks.{l}.", layers[l]
            y.ln1_g, y.ln1_b = cv(p + "norm1.weight"), cv(p + "norm1.bias")
            y.w_qkv, y.b_qkv = pk(p + "attention.in_proj_weight"), cv(p + "attention.in_proj_bias")
            y.w_o, y.b_o = pk(p + "attention.out_proj.weight"), cv(p + "attention.out_proj.bias")
            y.ln2_g, y.ln2_b = cv(p + "norm2.weight"), cv(p + "norm2.bias")
            y.w_1, y.b_1 = pk(p + "mlp.0.weight"), cv(p + "mlp.0.bias")
            y.w_2, y.b_2 = pk(p + "mlp.2.weight"), cv(p + "mlp.2.bias")
        lib = L.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(lib.osrl_cdt_policy_create(C.byref(d), layers, C.byref(h)), "osrl_cdt_policy_create")
        self._h, self._lib = h, lib
        ptrs = [C.POINTER(C.c_float)() for _ in range(3)]
        L.check(lib.osrl_cdt_policy_io(h, *[C.byref(p) for p in ptrs]), "osrl_cdt_policy_io")
        od, ad = m.state_dim, m.action_dim
        self.od, self.ad, self.T = od, ad, m.seq_len
        self._obs = np.ctypeslib.as_array(ptrs[0], shape=(od,))  # numpy views of PINNED memory
        self._act_in = np.ctypeslib.as_array(ptrs[1], shape=(ad,))
        self._act_out = np.ctypeslib.as_array(ptrs[2], shape=(ad,))
        self._t, self._episode_len = -1, 0
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)

    # a pinned, device-mapped block behind a ctypes pointer: not copyable; a copied / unpickled model builds its own
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (type(None), ())

    def _stream(self):
        return self._raw_stream(self._dev_index) if self._raw_stream is not None else cur_stream()

    def _put_obs(self, obs) -> None:
        if np.shape(obs) != self._obs.shape:  # numpy would broadcast a scalar silently
            raise ValueError(f"expected one observation of shape {self._obs.shape}, got {np.shape(obs)}")
        self._obs[:] = obs  # float32 (round to nearest), as torch.as_tensor(obs) written into the fp32 window

    def reset(self, obs, target_return: float, target_cost: float) -> np.ndarray:
        """Starts an episode (cdt.py:470-478) and returns the first action."""
        if self._h is None:
            raise RuntimeError("CDTFastPolicy is closed")
        self._episode_len = int(self.model.episode_len)
        self.model.repack()  # in-place edits of the parameters since the last step (CDT.forward does the same)
        self._put_obs(obs)
        self._t = 0
        rc = self._lib.osrl_cdt_policy_reset(self._h, float(target_return), float(target_cost), self._stream())
        if rc != 0:
            self._t = -1
            L.check(rc, "osrl_cdt_policy_reset")
        return self._act_out.copy()

    def step(self, obs, reward, cost, action=None) -> np.ndarray:
        """Records the action taken at the previous step (``action``, default: the one returned), the new observation
        and that step's reward and cost (``info["cost"] * cost_scale``, or its cost_reverse form); returns the next
        action."""
        if self._t < 0:
            raise RuntimeError("call reset() before step()")
        if self._t + 1 >= self._episode_len:
            raise RuntimeError(f"the episode is over: {self._episode_len} steps (model.episode_len)")
        self._put_obs(obs)
        host = 0
        if action is not None:
            if np.shape(action) != self._act_in.shape:
                raise ValueError(f"expected one action of shape {self._act_in.shape}, got {np.shape(action)}")
            self._act_in[:] = action
            host = 1
        rc = self._lib.osrl_cdt_policy_step(self._h, float(reward), float(cost), host, self._stream())
        if rc != 0:
            L.check(rc, "osrl_cdt_policy_step")
        self._t += 1
        return self._act_out.copy()

    def window(self) -> Dict[str, np.ndarray]:
        """numpy copies of the current window (oldest timestep first), as the model saw it for the last action."""
        T, od, ad = self.T, self.od, self.ad
        s, a = np.zeros((T, od), np.float32), np.zeros((T, ad), np.float32)
        r, c, ts = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.int64)
        n = C.c_int32(0)
        f = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        L.check(self._lib.osrl_cdt_policy_window(self._h, f(s), f(a), f(r), f(c), f(ts), C.byref(n), self._stream()),
                "osrl_cdt_policy_window")
        k = n.value
        return dict(states=s[:k].copy(), actions=a[:k].copy(), returns=r[:k].copy(), costs=c[:k].copy(),
                    time_steps=ts[:k].copy())

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            self._lib.osrl_cdt_policy_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass
