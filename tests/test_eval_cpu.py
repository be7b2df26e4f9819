"""CPU-side checks of the probes' predictions and confusion counts (dg_segment_predict, ops.segment_predict,
evaluation.predict_and_score): the export, the refusals before any launch, the fixture's internal consistency and the audit of
dg_eval.hip's generated code."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def test_segment_predict_is_exported_and_declared():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    assert re.search(r"\bdg_segment_predict\s*\(", header)
    assert "dg_segment_predict" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "dg_segment_predict") and lib.dg_version() == 119


def _call(B=2, D=8, h=4, w=4, n=3, m=4, H=8, W=8, n_store=0, ptr=16, scratch_bytes=1 << 30):
    """The C ABI with dummy addresses: every case here is refused before anything is launched or dereferenced."""
    from depthg_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(ptr) if ptr else ctypes.c_void_p(0)
    rc = lib.dg_segment_predict(p, None, B, D, h, w, p, None, n, p, m, p, H, W, None, None, n_store, None, None, p,
                                scratch_bytes, None)
    return rc, lib.dg_last_error().decode()


def test_c_abi_refuses_bad_dimensions_and_limits():
    for kw in (dict(B=0), dict(D=0), dict(h=0), dict(w=0), dict(n=0), dict(m=0), dict(H=0), dict(W=0), dict(n_store=-1)):
        rc, msg = _call(**kw)
        assert rc == -1 and "dimensions" in msg, (kw, rc, msg)
    rc, msg = _call(D=1025)
    assert rc == -2 and "D <= 1024" in msg
    rc, msg = _call(n=200, m=57)
    assert rc == -2 and "n + m <= 256" in msg
    rc, msg = _call(n=128, m=128, w=65)                # 65 * 256 floats of one blended score row > 64 KiB
    assert rc == -2 and "w * (n + m" in msg
    rc, _ = _call(n=128, m=128, w=64, ptr=0)          # at the limit: passes the checks, then refused for the null pointers
    assert rc == -1
    rc, msg = _call(scratch_bytes=2 * 16 * 8 * 4 - 1)  # B*h*w*(4 + 4)*4 bytes needed
    assert rc == -3 and "scratch" in msg
    rc, msg = _call(ptr=8)
    assert rc == -1 and "aligned" in msg


def test_segment_predict_refuses_cpu_tensors_and_bad_shapes():
    from depthg_amd import ops
    from depthg_amd.evaluation import predict_and_score
    from depthg_amd.head import ClusterLookup
    from depthg_amd.metrics import UnsupervisedMetrics
    code, label = torch.randn(2, 8, 4, 4), torch.zeros(2, 16, 16, dtype=torch.long)
    lin_w, lin_b, clusters = torch.randn(5, 8), torch.randn(5), torch.randn(7, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.segment_predict(code, label, lin_w, lin_b, clusters, n_store=1)
    linear, cluster = torch.nn.Conv2d(8, 5, 1), ClusterLookup(8, 7)
    with pytest.raises(RuntimeError, match="GPU"):
        predict_and_score(code, label, linear, cluster, UnsupervisedMetrics("a/", 5, 0, False), UnsupervisedMetrics("b/", 5, 2, True))
    bad = [dict(code=code[0]), dict(code_flip=code[:, :, :, :3]), dict(lin_w=torch.randn(5, 9)), dict(lin_b=torch.randn(4)),
           dict(clusters=torch.randn(7, 9)), dict(label=torch.zeros(3, 16, 16, dtype=torch.long)),
           dict(stats_lin=torch.zeros(5, 5, dtype=torch.int32)), dict(stats_lin=torch.zeros(4, 5, dtype=torch.long)),
           dict(stats_clu=torch.zeros(7, 6, dtype=torch.long)), dict(n_store=-1)]
    for over in bad:
        kw = dict(code=code, label=label, lin_w=lin_w, lin_b=lin_b, clusters=clusters)
        kw.update(over)
        with pytest.raises(ValueError):
            ops.segment_predict(**kw)
    with pytest.raises(ValueError, match="classes"):
        predict_and_score(code, label, linear, cluster, UnsupervisedMetrics("a/", 6, 0, False))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_eval_fixture_stats_are_the_counts_of_its_predictions(case):
    g = load_golden("eval.npz")
    B, D, h, w, H, W, n, e, flip, _ = (int(v) for v in g[f"{case}_cfg"])
    lab = g[f"{case}_label"].astype(np.int64).reshape(-1)
    assert {-1, 255, n} <= set(np.unique(lab).tolist())
    for key, rows in (("linear", n), ("cluster", n + e)):
        pred = g[f"{case}_{key}_preds"].astype(np.int64).reshape(-1)
        assert g[f"{case}_{key}_preds"].shape == (B, H, W) and pred.max() < rows
        ok = (lab >= 0) & (lab < n) & (pred < n)
        want = np.zeros((rows, n), np.int64)
        np.add.at(want, (pred[ok], lab[ok]), 1)
        assert np.array_equal(g[f"{case}_stats_{'lin' if key == 'linear' else 'clu'}"], want)
    assert (f"{case}_code_flip" in g) == bool(flip)


def test_eval_kernels_use_no_scratch_and_no_flat_memory(tmp_path):
    """The audit of tests/test_host_cpu.py::test_byte_movers_use_no_scratch_and_no_flat_loads on dg_eval.hip: a kernel argument
    struct spilled to scratch or a pointer without address space (FLAT loads, which also count as LDS operations) would slow the
    LDS-bound score loop several-fold without changing a result."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "depthg_amd", "csrc", "dg_eval.hip")
    out = tmp_path / "dg_eval.s"
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    text = out.read_text()
    flat = [l.strip() for l in text.splitlines() if re.match(r"\s+flat_(load|store|atomic)", l)]
    assert not flat, f"dg_eval: FLAT memory instructions: {flat[:3]}"
    scratch = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) == 4, scratch                     # k_seg_project<flip / not>, k_seg_score<LDS histogram / not>
    bad = {k: v for k, v in scratch.items() if v > 0}
    assert not bad, f"dg_eval: kernels with scratch (bytes per thread): {bad}"
