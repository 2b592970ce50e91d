"""vnl_rollout_post of the host simulation against the torch restatement of tests/test_gpu_rollout_post.py (the same cases;
the device runs them there)."""
import pytest

import helpers as H
import test_gpu_rollout_post as R


@pytest.mark.parametrize("logs", [True, False], ids=["log_rows", "no_log_rows"])
@pytest.mark.parametrize("B", [5, 67])
def test_rollout_post_of_the_host_build_equals_its_restatement(B, logs):
    R._check(H.hostsim_library("float"), "cpu", B, logs)
