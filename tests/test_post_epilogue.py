"""vnl_env_step_post -- the rollout post-processing as the epilogue of the env step kernel -- on the host build of the
product source (float32), against the two launches it replaces: vnl_env_step, then vnl_rollout_post.  First the entry
itself, on a case in which all four decision branches occur and the ops cover the shapes an op can have; then an unroll
through acting.generate_unroll with acting._POST_EPILOGUE on and off; then the validation of the descriptor, which is
vnl_rollout_post's (tests/test_abi.py: the same codes and messages)."""
import ctypes as C

import torch

import helpers as H
import model_cases as M
import post_epilogue_cases as PE
from vnl_brax_imitation_amd import _lib


def test_step_with_epilogue_equals_step_then_post_on_every_buffer():
    two = PE.direct_case(H.hostsim_env(5, "float"), fused=False)
    one = PE.direct_case(H.hostsim_env(5, "float"), fused=True)
    PE.assert_same(one, two)


def test_unroll_with_epilogue_equals_the_two_launch_unroll():
    dev = torch.device("cpu")
    runs = [PE.unroll_case(lambda: H.hostsim_env(5, "float"), dev, epilogue) for epilogue in (False, True)]
    PE.assert_unrolls_same(*runs)
    datas, _ = runs[1]
    trunc = datas[0][-1]  # (leaves: ..., state_extras sorted: traj, truncation)
    assert trunc.shape == (3, 5) and float(trunc.sum()) > 0  # episodes of 2 steps did end inside the unroll


def test_an_env_that_works_on_the_state_after_its_step_keeps_the_two_launches():
    """AntTracking.step assembles the observation AFTER the kernel: the post-processing must see it, so the unroll must not
    take the epilogue there -- switch on and off give the same unroll, and no step carries a descriptor."""
    dev, seen = torch.device("cpu"), []

    def hook(base):
        orig = base.step

        def step(st, a):
            seen.append(getattr(base, "_post_desc", None) is not None)
            return orig(st, a)

        base.step = step

    runs = [PE.unroll_case(lambda: M.ant_env(5), dev, epilogue, hook=hook) for epilogue in (False, True)]
    PE.assert_unrolls_same(*runs)
    assert seen == [False] * 6


def test_the_fused_entry_validates_the_descriptor_as_vnl_rollout_post_does():
    base = H.hostsim_env(2, "float")
    L = base._L
    st = base.reset(torch.Generator().manual_seed(0))
    before = {k: v.clone() for k, v in PE.state_tensors(st).items()}
    p = base._ptrs(st)
    action = torch.zeros(2, int(base.dims.nu))
    call = lambda desc: L.vnl_env_step_post(base._env_h, action.data_ptr(), C.byref(p), desc, None)  # noqa: E731

    def message_of_post(desc):
        assert L.vnl_rollout_post(desc, 2, None) == -1
        return L.vnl_last_error()

    d = _lib.PostDesc()
    assert call(None) == -1 and L.vnl_last_error() == message_of_post(None)
    assert call(C.byref(d)) == -1 and b"null" in L.vnl_last_error() and L.vnl_last_error() == message_of_post(C.byref(d))
    d.done = C.c_void_p(8)  # never dereferenced: validation fails first
    d.num_ops = _lib.POST_MAX_OPS + 1
    assert call(C.byref(d)) == -1 and b"too many" in L.vnl_last_error() and L.vnl_last_error() == message_of_post(C.byref(d))
    d.num_ops = -1
    assert call(C.byref(d)) == -1 and b"too many" in L.vnl_last_error()
    d.num_ops = 1  # op 0 has no source
    assert call(C.byref(d)) == -1 and b"bad op" in L.vnl_last_error() and L.vnl_last_error() == message_of_post(C.byref(d))
    d.ops[0].src, d.ops[0].width = C.c_void_p(8), 0
    assert call(C.byref(d)) == -1 and b"bad op" in L.vnl_last_error()
    d.num_ops, d.log_reward = 0, C.c_void_p(8)
    assert call(C.byref(d)) == -1 and b"log_reward" in L.vnl_last_error()
    assert L.vnl_env_step_post(None, action.data_ptr(), C.byref(p), C.byref(d), None) == -1
    PE.assert_same(PE.state_tensors(st), before)  # nothing ran
