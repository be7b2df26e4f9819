"""dg_sample_rows (k_sample_direct) on the GPU against the numpy restatement of sample() (tests/sample_rows_reference.py): every element
of outputs poisoned with 0xFF bytes, both row types, square and line grids, a reversed batch map, coordinates on and beyond the border
and on pixel centres.  Bounds: SAMPLE_ROWS_ULPS * 2^-24 * max|tap| per fp32 element, + 2^-8 |want| for bf16 (derived there); the
measured maxima (printed with -s) are recorded in profiles/sample_rows_parity.md."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sample_rows_reference import (SAMPLE_ROWS_SHAPES, check_rows, sample_coords, sample_map,  # noqa: E402
                                   sample_rows_reference)

pytestmark = pytest.mark.gpu

# (S, Sh, reversed batch map): S = 1, 4 and 11, a line grid, a reversed batch map
GRIDS = [(1, 1, False), (4, 4, False), (11, 11, False), (11, 1, False), (4, 4, True), (11, 1, True)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


_MAPS = {}


def _map(shape, dev):
    """The map of a shape, its device copy and the restatement's rows per grid: computed once, shared by both row types."""
    if shape not in _MAPS:
        t = sample_map(11, *shape)
        cases = []
        for S, Sh, mapped in GRIDS:
            coords = sample_coords(100 + S + Sh, shape[0], S, Sh, shape[2], shape[3])
            idx = np.arange(shape[0])[::-1].copy() if mapped else None
            cases.append((coords, idx) + sample_rows_reference(t, coords, idx))
        _MAPS[shape] = (torch.from_numpy(t).to(dev), cases)
    return _MAPS[shape]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,K,h,w", SAMPLE_ROWS_SHAPES)
def test_sample_rows_against_the_restatement(B, K, h, w, bf16, dev, monkeypatch):
    from depthg_amd import ops
    monkeypatch.setattr(ops, "POISON", True)                 # every output is 0xFF bytes until the kernel writes it
    t, cases = _map((B, K, h, w), dev)
    worst = 0.0
    for coords, idx, want, tapmax in cases:
        got = ops.sample_rows(t, torch.from_numpy(coords).to(dev), None if idx is None else torch.from_numpy(idx).to(dev), bf16=bf16)
        S, Sh = coords.shape[1], coords.shape[2]
        assert tuple(got.shape) == (B, S * Sh, (K + 127) // 128 * 128 if bf16 else (K + 3) // 4 * 4) and got.is_contiguous()
        assert got.dtype == (torch.bfloat16 if bf16 else torch.float32)
        worst = max(worst, check_rows(got.to(torch.float64).cpu().numpy(), want, tapmax, K, bf16))
    print(f"\n  dg_sample_rows {(B, K, h, w)} {'bf16' if bf16 else 'fp32'}: max |got - want| / bound = {worst:.3f}")


def test_two_calls_give_equal_bits_and_the_cpu_route_agrees(dev):
    from depthg_amd import ops
    t, cases = _map(SAMPLE_ROWS_SHAPES[1], dev)
    coords, idx = cases[2][0], None
    c = torch.from_numpy(coords).to(dev)
    a, b = ops.sample_rows(t, c), ops.sample_rows(t, c)
    assert torch.equal(a, b)
    cpu = ops.sample_rows(t.cpu(), torch.from_numpy(coords))
    assert float((a.cpu() - cpu).abs().max()) <= 16 * 2.0 ** -24 * float(t.abs().max())       # both within 8 ulps of the restatement
