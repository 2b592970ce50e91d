"""Run by tests/test_body_domain.py under LD_PRELOAD=libasan.so:libubsan.so: body-randomised envs (rodent, rodent with a
four-field domain too, ant) and a rejected domain through the host build of the kernels compiled with
-fsanitize=address,undefined (argv[1])."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import body_domain_cases as BD  # noqa: E402
import domain_cases as D  # noqa: E402
import helpers as H  # noqa: E402
from vnl_brax_imitation_amd import _lib  # noqa: E402
from vnl_brax_imitation_amd.envs.ant import AntTracking  # noqa: E402
from vnl_brax_imitation_amd.envs.rodent import RodentTracking  # noqa: E402

lib = _lib.load_library(sys.argv[1], env_only=True)
ctx = H.backend(lib)
ctx.__enter__()  # every env below binds to the sanitizer build of the host library
rng = np.random.default_rng(0)


def run(env, nu, steps=2):
    st = env.reset(5)
    for _ in range(steps):
        st = env.step(st, torch.from_numpy(np.clip(0.3 * rng.standard_normal((env.num_envs, nu)), -1, 1).astype(np.float32)))
    return bool(torch.isfinite(st.obs).all())


base = RodentTracking(H.reference_clip(), num_envs=3, device="cpu", **H.env_kwargs())
env = base.with_body_domain(BD.random_body_domain(base.sys, 3, 1))
print("rodent ok", run(env, 30), [tuple(env.domain_table(k).shape) for k in ("dom_mass", "dom_ipos", "dom_inertia6", "dom_tminv")])
both = env.with_domain(D.random_domain(base.sys, 3, 2))
print("both ok", run(both, 30), sorted(both.domain))
am = BD.packaged("ant")
a = AntTracking(dict(solver="newton", iterations=1, ls_iterations=4), model=am, num_envs=2, device="cpu")
print("ant ok", run(a.with_body_domain(BD.random_body_domain(am, 2, 3)), 8))
bad = BD.identity(base.sys, 3)["body_mass"]
bad[2, 1:] = 0.0
try:
    base.with_body_domain({"body_mass": bad})
except ValueError as e:
    print("bad ok", str(e)[:80])
