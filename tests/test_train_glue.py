"""vnl_gather_rows, vnl_adam_step and vnl_ppo_head of the host simulation against the references of
tests/train_glue_cases.py (the same cases as tests/test_gpu_train_glue.py runs on the device).  The host build runs every
kernel with one thread per block: it pins the arithmetic and the indexing, not the lane groups, block sums and strides."""
import pytest

import helpers as H
import train_glue_cases as G


def _lib():
    return H.hostsim_library("float")


@pytest.mark.parametrize("N,M,permutation,all_ops", [(37, 11, False, False), (16, 16, True, False), (5, 16, False, False),
                                                     (37, 11, False, True)],
                         ids=["37-11", "16-16-permutation", "5-16-repeats", "37-11-all-24-ops"])
def test_gather_of_the_host_build_equals_index_select(N, M, permutation, all_ops):
    G.check_gather(_lib(), "cpu", N, M, permutation, all_ops)


@pytest.mark.parametrize("n,count,hyper", G.ADAM_CASES, ids=[f"n{n}-t{c}-lr{h['lr']}" for n, c, h in G.ADAM_CASES])
def test_adam_of_the_host_build_within_the_rounding_bounds(n, count, hyper):
    G.check_adam(_lib(), "cpu", n, count, hyper)


def test_adam_in_two_segments_of_the_host_build_equals_one_call():
    G.check_adam_segments(_lib(), "cpu")


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw-advantages"])
@pytest.mark.parametrize("shape", G.HEAD_SHAPES, ids=["x".join(map(str, s)) for s in G.HEAD_SHAPES])
def test_head_of_the_host_build_matches_float64_autograd(shape, normalize):
    G.check_head(_lib(), "cpu", *shape, normalize)


def test_head_of_the_host_build_with_other_min_std_and_var_scale():
    G.check_head(_lib(), "cpu", 9, 5, 33, 3, True, min_std=0.01, var_scale=0.5)


def test_head_of_the_host_build_all_truncated_leaves_the_entropy_term():
    G.check_head(_lib(), "cpu", 9, 5, 33, 3, False, all_truncated=True)
