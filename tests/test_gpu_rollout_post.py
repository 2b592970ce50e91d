"""vnl_rollout_post (csrc/vnl_lib.hip: vnl_post_kernel) against a torch restatement of include/vnl.h's description, exact
equality: widths below, at and above one pass of the 256 threads, an op whose destination is its own source, ops without
destination, without first state, with and without log rows, finished and running envs mixed, step counts crossing the
episode length.  The cases and the restatement are in tests/rollout_post_cases.py, which the host simulation is put through
as well."""
import pytest

from rollout_post_cases import check
from vnl_brax_imitation_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("logs", [True, False], ids=["log_rows", "no_log_rows"])
@pytest.mark.parametrize("B", [5, 67])
def test_rollout_post_equals_its_restatement(B, logs):
    check(_lib.load_library(), DEV, B, logs)
