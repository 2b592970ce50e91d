"""vnl_rollout_post of the host simulation against the torch restatement of tests/rollout_post_cases.py (the same cases as
tests/test_gpu_rollout_post.py runs on the device)."""
import pytest

import helpers as H
from rollout_post_cases import check


@pytest.mark.parametrize("logs", [True, False], ids=["log_rows", "no_log_rows"])
@pytest.mark.parametrize("B", [5, 67])
def test_rollout_post_of_the_host_build_equals_its_restatement(B, logs):
    check(H.hostsim_library("float"), "cpu", B, logs)
