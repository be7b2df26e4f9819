"""dg_sample_rows and the loss's route for label-size signals without a GPU: the export, the entry's refusals (made on the host in
front of any launch, so host memory serves), the CPU route of ops.sample_rows against the numpy restatement, and what the plan
reserves for feature maps above 16384 positions - rows, no channel-last copies - up to the new limit of 65536."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT  # noqa: E402
from sample_rows_reference import (SAMPLE_ROWS_SHAPES, check_rows, sample_coords, sample_map,  # noqa: E402
                                   sample_rows_reference)


def _err():
    from depthg_amd import _lib
    return _lib.load().dg_last_error().decode()


def test_export_is_declared_listed_and_exported():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    assert "int dg_sample_rows(" in header and "src/modules.py:822-825" in header[header.index("int dg_label_onehot("):header.index("int dg_sample_rows(")]
    assert "dg_sample_rows" in _lib.EXPORTS and "dg_sample_rows" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "dg_sample_rows")
    assert lib.dg_version() == _lib.DG_VERSION == 119


def test_refusals_on_host_memory():
    """Every refusal is made before a launch: the pointers are host arrays and nothing dereferences them."""
    from depthg_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float64)                      # 8-byte aligned host memory
    base = buf.ctypes.data
    assert base % 8 == 0
    p = lambda off=0: ctypes.c_void_p(base + off)
    ok = dict(map=p(), coords=p(64), srcidx=p(128), B=2, K=5, h=3, w=3, S=2, Sh=2, Kout=8, as_bf16=0, out=p(256))

    def call(**over):
        a = {**ok, **over}
        return lib.dg_sample_rows(a["map"], a["coords"], a["srcidx"], a["B"], a["K"], a["h"], a["w"], a["S"], a["Sh"], a["Kout"], a["as_bf16"],
                                  a["out"], None)

    cases = [(dict(map=None), "null"), (dict(coords=None), "null"), (dict(out=None), "null"),
             (dict(map=p(2)), "4-byte"), (dict(coords=p(66)), "4-byte"), (dict(out=p(257)), "4-byte"), (dict(srcidx=p(132)), "8-byte"),
             (dict(h=1, w=65537), "too large"), (dict(h=257, w=256), "too large"),
             (dict(Kout=4), "Kout"), (dict(Kout=6), "Kout"), (dict(Kout=10), "Kout"),
             (dict(B=0), "non-positive"), (dict(K=0), "non-positive"), (dict(S=0), "non-positive"), (dict(Sh=0), "non-positive"),
             (dict(h=0), "non-positive"), (dict(B=65536), "65535")]
    for over, word in cases:
        rc = call(**over)
        assert rc < 0 and "dg_sample_rows" in _err() and word in _err(), (over, rc, _err())


def test_the_entries_that_keep_the_old_limit_refuse_by_name():
    """dg_sampled_sumsq and dg_corr_forward_extnorm (the route of maps wider than 768 channels) and the intra-feats entry stay at
    16384 positions; each names itself and the limit, in front of any launch."""
    from depthg_amd import _lib, ops
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.dg_sampled_sumsq(2, 8, 129, 128, 4, 0, p, p, None, 0, p, None) < 0
    assert "dg_sampled_sumsq" in _err() and "16384" in _err()
    kw = dict(pointwise=True, zero_clamp=True, stabalize=False, depth_term=False, need_grad=False, shared_coords=False, shifts=(0.1,) * 4)
    desc = ops.make_desc(2, 600, 16, 129, 128, 14, 1, **kw)
    assert lib.dg_corr_forward_extnorm(ctypes.byref(desc), p, p, p, p, None, p, p, p, p, p, p, 64, None) < 0
    assert "dg_corr_forward_extnorm" in _err() and "16384" in _err()
    with pytest.raises(RuntimeError, match=r"dg_corr_forward_intra_feats: feature map 129x128 too large \(max 16384"):
        ops.workspace_bytes(ops.make_desc(2, 28, 16, 129, 128, 4, 1, **kw), intra_feats=True)
    assert ops.workspace_bytes(ops.make_desc(2, 28, 16, 128, 128, 4, 1, **kw), intra_feats=True) > 0


@pytest.mark.parametrize("B,K,h,w", SAMPLE_ROWS_SHAPES)
@pytest.mark.parametrize("bf16", [False, True])
def test_cpu_route_equals_the_restatement(B, K, h, w, bf16):
    from depthg_amd import ops
    t = sample_map(11, B, K, h, w)
    worst = 0.0
    for S, Sh, mapped in ((1, 1, False), (4, 4, False), (11, 11, False), (7, 1, False), (4, 4, True)):
        coords = sample_coords(100 + S + Sh, B, S, Sh, h, w)
        idx = np.arange(B)[::-1].copy() if mapped else None
        got = ops.sample_rows(torch.from_numpy(t), torch.from_numpy(coords), None if idx is None else torch.from_numpy(idx), bf16=bf16)
        assert tuple(got.shape) == (B, S * Sh, (K + 127) // 128 * 128 if bf16 else (K + 3) // 4 * 4)
        assert got.dtype == (torch.bfloat16 if bf16 else torch.float32)
        want, tapmax = sample_rows_reference(t, coords, idx)
        worst = max(worst, check_rows(got.to(torch.float64).numpy(), want, tapmax, K, bf16))
    print(f"\n  sample_rows CPU route {(B, K, h, w)} {'bf16' if bf16 else 'fp32'}: max |got - want| / bound = {worst:.3f}")


def test_cpu_route_argument_checks():
    from depthg_amd import ops
    t, c = torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 2, 2)
    with pytest.raises(ValueError, match="sample_rows takes"):
        ops.sample_rows(t[0], c)
    with pytest.raises(ValueError, match="sample_rows takes"):
        ops.sample_rows(t, c[:1])
    with pytest.raises(ValueError, match="srcidx"):
        ops.sample_rows(t, c, torch.zeros(2, dtype=torch.int32))


# ---- the plan: what a label-size signal reserves -----------------------------------------------------------------------------------
_KW = dict(pointwise=True, zero_clamp=True, stabalize=False, depth_term=True, need_grad=True, shared_coords=False,
           shifts=(0.1, 0.2, 0.3, 0.4), depth_hw=(224, 224))


ONE_COPY = 32 * 50176 * 28 * 4          # bytes of one channel-last fp32 copy of one 224 x 224 signal map at B = 32, K = 28


@pytest.mark.parametrize("h,w", [(224, 224), (129, 128)])
def test_workspace_of_a_large_signal_holds_rows_not_copies(h, w):
    """B = 32, C = 28 one-hot channels, D = 70, the signal over 28 x 28 code maps, S = 11, five negatives, with gradients: served (the
    call returned 0 bytes before), in less than ONE channel-last copy of one 224 x 224 signal map.  A route that still reserved the
    two copies would miss that at both sizes: at 129 x 128 they are 2 x 59 MB on top of the 99 MB every size needs."""
    from depthg_amd import ops
    desc = ops.make_desc(32, 28, 70, h, w, 11, 5, code_hw=(28, 28), **_KW)
    n = ops.workspace_bytes(desc)
    assert 0 < n < ONE_COPY
    # nothing the plan reserves grows with the signal map
    assert n == ops.workspace_bytes(ops.make_desc(32, 28, 70, 256, 256, 11, 5, code_hw=(28, 28), **_KW))
    # S = 14 (the blob path behind k_gather_norm) the same
    assert 0 < ops.workspace_bytes(ops.make_desc(32, 28, 70, h, w, 14, 5, code_hw=(28, 28), **_KW)) < ONE_COPY
    assert ops.corr_main_kernel_name(desc) == "k_corr_small"


def test_nothing_changes_at_the_old_limit_and_the_new_one_is_named():
    from depthg_amd import ops
    # 128 x 128 still copies: its workspace holds both channel-last signal maps
    at_limit = ops.workspace_bytes(ops.make_desc(2, 28, 70, 128, 128, 11, 5, code_hw=(28, 28), **_KW))
    assert at_limit > 2 * 2 * 128 * 128 * 28 * 4
    assert ops.workspace_bytes(ops.make_desc(2, 28, 70, 256, 256, 11, 5, code_hw=(28, 28), **_KW)) < at_limit
    with pytest.raises(RuntimeError, match=r"feature map 257x256 too large \(max 65536 positions\)"):
        ops.workspace_bytes(ops.make_desc(2, 28, 70, 257, 256, 11, 5, code_hw=(28, 28), **_KW))
    # the code maps' limit stays
    with pytest.raises(RuntimeError, match="code map 200x200 too large"):
        ops.workspace_bytes(ops.make_desc(2, 28, 70, 224, 224, 11, 5, code_hw=(200, 200), **_KW))
    with pytest.raises(RuntimeError, match="code map 129x128 too large"):
        ops.workspace_bytes(ops.make_desc(2, 28, 70, 129, 128, 11, 5, **_KW))
