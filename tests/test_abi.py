"""The C-ABI library loads without a GPU and exports every symbol include/vnl.h declares;
compute entry points fail loudly when no HIP device exists (there is no CPU fallback)."""
import ctypes as C
import os
import re

import pytest
import torch

import helpers as H
from vnl_brax_imitation_amd import _lib
from vnl_brax_imitation_amd.model import blob

HEADER = os.path.join(H.ROOT, "include", "vnl.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vnl_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_all_exported():
    lib = _lib.load_library()  # built by __graft_entry__.build()
    names = _declared()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), n
    assert set(_lib.EXPORTS) == set(names)
    assert lib.vnl_version() == 1


def test_missing_library_is_a_loud_error(tmp_path):
    with pytest.raises(_lib.VnlError, match="no CPU fallback"):
        _lib.load_library(str(tmp_path / "nope.so"))


def test_bad_blob_and_missing_device_are_reported():
    lib = _lib.load_library()
    h = C.c_void_p()
    bad = C.create_string_buffer(b"garbage" * 10)
    assert lib.vnl_model_create(bad, 70, C.byref(h)) == -2
    assert b"magic" in lib.vnl_last_error()
    good = blob.to_blob(H.model())
    buf = C.create_string_buffer(good, len(good))
    assert lib.vnl_model_create(buf, len(good), C.byref(h)) == 0
    if not torch.cuda.is_available():
        from vnl_brax_imitation_amd.envs.rodent import RodentTracking

        with pytest.raises(_lib.VnlError, match="no CPU fallback|HIP device"):
            RodentTracking(H.reference_clip(), num_envs=2, device="cpu", **H.env_kwargs())
        with pytest.raises(_lib.VnlError, match="no HIP device|hipSetDevice|HIP"):
            with H.backend(lib):
                RodentTracking(H.reference_clip(), num_envs=2, device="cpu", **H.env_kwargs())
    lib.vnl_model_destroy(h)


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(H.ROOT, "vnl-brax-imitation_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"import\s+oracle|from\s+oracle|oracle[/.]oracle|liborc|vnl_oracle|orc_", txt), \
                    os.path.join(dp, f)


def test_argument_validation_of_the_helper_entry_points():
    """vnl_rollout_post / vnl_ppo_head / vnl_policy_forward reject malformed descriptors with an error code and a
    message instead of launching (checked on the product library: validation happens before any HIP call)."""
    lib = _lib.load_library()
    d = _lib.PostDesc()
    assert lib.vnl_rollout_post(C.byref(d), 4, None) == -1 and b"null" in lib.vnl_last_error()
    d.done = C.c_void_p(8)  # never dereferenced: validation fails first
    d.num_ops = _lib.POST_MAX_OPS + 1
    assert lib.vnl_rollout_post(C.byref(d), 4, None) == -1 and b"too many" in lib.vnl_last_error()
    d.num_ops = 1  # op 0 has no source
    assert lib.vnl_rollout_post(C.byref(d), 4, None) == -1 and b"bad op" in lib.vnl_last_error()
    assert lib.vnl_rollout_post(None, 4, None) == -1
    a = _lib.PPOHeadArgs()
    work = C.c_void_p(8)
    assert lib.vnl_ppo_head(C.byref(a), work, None) == -1 and b"sizes" in lib.vnl_last_error()
    a.T, a.B, a.act, a.latent = 2, 2, 3, 4
    assert lib.vnl_ppo_head(C.byref(a), work, None) == -1 and b"null buffer" in lib.vnl_last_error()
    assert lib.vnl_policy_forward(None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, None,
                                  None, None, None, None) == -1


def test_argument_validation_of_gather_and_adam():
    """vnl_gather_rows / vnl_adam_step reject malformed arguments with VNL_ERR_ARG and a message, and launch nothing: on the
    host build a launch would run at once, read the pointers below (never dereferenceable) and write the buffers watched."""
    lib = H.hostsim_library("float")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    src, idx = torch.arange(12, dtype=torch.float32).reshape(1, 4, 3), torch.tensor([2, 0], dtype=torch.int64)
    dst = torch.full((1, 2, 3), -7.0)

    def desc(**over):
        d = _lib.GatherDesc()
        d.idx, d.N, d.M, d.num_ops = ptr(idx), 4, 2, 1
        d.ops[0].dst, d.ops[0].src, d.ops[0].T, d.ops[0].width = ptr(dst), ptr(src), 1, 3
        for k, v in over.items():
            setattr(d.ops[0] if k in ("dst", "src", "T", "width") else d, k, v)
        return d

    def rejected(d, message):
        rc = lib.vnl_gather_rows(C.byref(d) if d is not None else None, None)
        return rc == -1 and message in lib.vnl_last_error() and bool((dst == -7.0).all())

    assert rejected(None, b"bad descriptor")
    for over in (dict(idx=None), dict(N=0), dict(N=-1), dict(M=0), dict(M=-3), dict(num_ops=_lib.POST_MAX_OPS + 1)):
        assert rejected(desc(**over), b"bad descriptor"), over
    for over in (dict(dst=None), dict(src=None), dict(T=0), dict(T=-1), dict(width=0), dict(width=-2)):
        assert rejected(desc(**over), b"bad op"), over
    assert lib.vnl_gather_rows(C.byref(desc()), None) == 0 and torch.equal(dst, src[:, idx])  # (the descriptor they all vary)

    p, g, mu, nu = (torch.full((3,), v) for v in (1.0, 0.5, 0.25, 0.125))
    count = torch.tensor([1], dtype=torch.int64)
    good = [ptr(p), ptr(g), ptr(mu), ptr(nu), ptr(count)]
    for k in range(5):
        args = list(good)
        args[k] = None
        assert lib.vnl_adam_step(*args, 3, 1e-3, 0.9, 0.999, 1e-8, None) == -1 and b"vnl_adam_step" in lib.vnl_last_error(), k
    for n in (0, -5):
        assert lib.vnl_adam_step(*good, n, 1e-3, 0.9, 0.999, 1e-8, None) == -1 and b"vnl_adam_step" in lib.vnl_last_error(), n
    assert all(bool((t == v).all()) for t, v in ((p, 1.0), (g, 0.5), (mu, 0.25), (nu, 0.125))) and int(count) == 1
