"""CPU-side checks of the member-parallel environment step (csrc/model_env_split.hip, ``osrl_model_env_step_split``,
``ModelVecEnv(split_members=)``): the entry's refusals before any launch, the compile-time budgets of its kernels (hipcc
cross-compiles gfx950 assembly without a GPU) and the keyword on an environment that never saw a device."""
import ctypes as C

import pytest

from test_isa_halt_model_env_cpu import listing


def test_entry_refuses_bad_arguments_before_any_launch():
    """One table of refusals for ``osrl_model_env_step`` and ``osrl_model_env_step_split``: the two entries state one
    contract (csrc/model_env_args.h), the split one with ``member_out`` / ``arrive`` appended."""
    from osrl_amd import _lib as L
    lib = L.load()
    one = 0x1000  # (never dereferenced: every call below fails a check first)
    env, gauss, pess, rec = L.ModelEnvT(), L.ModelEnvGaussT(), L.ModelEnvPessT(), L.CollectT()
    tail = [one, one, one, 40, one, one, None, 17]  # act, state, obs, obs_ld, acc, unc, step_out, episodes

    for split in (False, True):
        def call(e=env, g=None, p=None, r=None, member_out=one, arrive=one, split=split, **kw):
            t = list(tail)
            for i, v in kw.items():
                t[int(i[1:])] = v
            head = (None if e is None else C.byref(e), None if g is None else C.byref(g), p, r, None)
            if split:
                return lib.osrl_model_env_step_split(*head, *t, member_out, arrive, None)
            return lib.osrl_model_env_step(*head, *t, None)

        assert call(e=None) == -1 and call(g=gauss) == -1          # neither, both
        if split:
            assert call(member_out=None) == -1 and call(arrive=None) == -1
        assert call() == -1 and call(e=None, g=gauss) == -1        # zeroed descriptors: n_models == 0
        assert call(r=C.byref(rec)) == -1                          # a recorder without tables
        for i in (0, 1, 2, 4, 5):                                  # the step's own pointers
            assert call(**{f"a{i}": None}) == -1, i
        assert call(a7=0) == -1 and call(p=C.byref(pess)) == -1
    assert L.model_env_split_row(37, False) == 40 and L.model_env_split_row(37, True) == 80


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return listing(tmp_path_factory.mktemp("isa_model_env_split"), "model_env_split.hip")


def test_sixteen_kernels_within_their_budgets(kernels):
    """Eight instantiations and their descriptor-pointer twins; no scratch, static LDS within 160 KB, fp32 MFMA layers,
    and no more registers than the plain kernel of the same flags (198 / 209 / 208: tests' docstrings of model_env.hip)."""
    k = {n: v for n, v in kernels.items() if "menv_split_kernel" in n}
    assert len(k) == 16 and sum("menv_split_kernel_p" in n for n in k) == 8, list(kernels)
    assert not any(o in n for n in kernels for o in ("model_env_kernel", "model_rec_kernel", "halt_env", "halt_rec"))
    for n, v in k.items():
        print(n, v)
        assert v["scratch"] == 0 and 0 <= v["lds"] <= 160 * 1024 and v["mfma"] >= 4, (n, v)
        assert 0 < v["vgpr"] <= 198, (n, v)


def test_keyword_on_a_stub():
    from osrl_amd.common.model_env import ModelVecEnv
    v = ModelVecEnv.__new__(ModelVecEnv)
    v._own_epoch, v._split, v.member_out, v.arrive = 0, False, object(), object()  # (buffers "allocated": no device)
    assert v.split_members is False
    v.split_members = True
    assert v.split_members is True and v.launch_epoch == 1
    v.split_members = True
    assert v.launch_epoch == 1
    v.split_members = False
    assert v.launch_epoch == 2 and v.member_out is not None
