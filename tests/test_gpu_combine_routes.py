"""k_combine_out's routed lists against the oracle: batch maps that are NOT permutations (super_perm's output need not be one,
quirk Q6), so that one destination image collects many routed tiles and others none, with the list lengths around the 64 pairs a
wave tests per ballot; a narrow code (D = 16: two of the three channel groups partly or wholly padding) beside the requests the
kernel issues before it knows its list; the smallest routed case.  Every case runs the step twice and asks for bit-equal results:
the list's order, and with it the order of the floating-point sums, must not depend on timing.
Shape, reference and bounds of test_gpu_sweep.py::test_dense_grid_shapes (src/modules.py:1184-1188 super_perm, :1323-1367 forward)."""
import functools

import pytest
import torch

from test_gpu_parity import _relclose, dev  # noqa: F401

pytestmark = pytest.mark.gpu

C = 384
#          B   D  hw  N  batch maps: an image index = every map constant; "draw" = O.super_perm; else the maps themselves
ROUTES = [(3, 70, 13, 5, 1),            # image 1 collects 15 routed tiles, images 0 and 2 none; P = 169: ragged tiles everywhere
          (8, 70, 13, 8, 0),            # DG_MAX_NEG maps: 64 entries on one destination = exactly one full ballot
          (9, 70, 13, 8, 0),            # 72 entries: a second, partial ballot
          (5, 16, 16, 3, "draw"),       # the ordinary case; DP = 96 with D = 16: the `ok` predicate beside the early requests
          (2, 70, 13, 1, ((1, 0),))]    # the smallest routed case


@functools.lru_cache(maxsize=None)
def _case(B, D, hw, N, maps):
    """Inputs and the oracle's losses and gradients of one case, computed once (CPU tensors; nobody writes to them)."""
    from oracle import depthg_oracle as O
    g = torch.Generator().manual_seed(77 * B + hw)
    f, fp = torch.randn(B, C, hw, hw, generator=g), torch.randn(B, C, hw, hw, generator=g)
    c, cp = torch.randn(B, D, hw, hw, generator=g), torch.randn(B, D, hw, hw, generator=g)
    d = torch.randint(0, 256, (B, 1, 4 * hw, 4 * hw), generator=g).float()
    d[:, :, :7, :9] = 0.0
    if maps == "draw":
        perms = [O.super_perm(B, g) for _ in range(N)]
    elif isinstance(maps, int):
        perms = [torch.full((B,), maps, dtype=torch.int64) for _ in range(N)]
    else:
        perms = [torch.tensor(m, dtype=torch.int64) for m in maps]
    assert len(perms) == N and all(p.shape == (B,) for p in perms)
    cfg = O.default_cfg(feature_samples=hw, neg_samples=N, dim=D, dg_outputs="reduced", dg_dense_grid=True)
    coords = O.identity_coords(B, hw)
    cr, cpr = c.clone().requires_grad_(True), cp.clone().requires_grad_(True)
    ref = O.forward(cfg, f, fp, cr, cpr, d, d, coords1=coords, coords2=coords, perms=perms)
    O.total_loss(cfg, ref).backward()
    means = {i: float(ref[i].detach().mean()) for i in (0, 2, 4, 6)}
    return cfg, (f, fp, c, cp, d, coords, perms), means, (cr.grad.detach(), cpr.grad.detach())


def _gpu_step(cfg, inputs, dev):
    from depthg_amd import ContrastiveCorrelationLoss
    from oracle import depthg_oracle as O
    f, fp, c, cp, d, coords, perms = inputs
    cg, cpg = c.to(dev).requires_grad_(True), cp.to(dev).requires_grad_(True)
    out = ContrastiveCorrelationLoss(cfg).forward_with(f.to(dev), fp.to(dev), cg, cpg, d.to(dev), coords.to(dev), coords.to(dev),
                                                       [p.to(dev) for p in perms], shared_coords=True, identity_grid=True)
    O.total_loss(cfg, out).backward()
    torch.cuda.synchronize()
    return {i: out[i].detach().float().mean().cpu() for i in (0, 2, 4, 6)}, (cg.grad.cpu(), cpg.grad.cpu())


@pytest.mark.parametrize("B,D,hw,N,maps", ROUTES)
def test_routed_lists_of_any_batch_map(B, D, hw, N, maps, dev):
    cfg, inputs, ref_means, ref_grads = _case(B, D, hw, N, maps)
    means, grads = _gpu_step(cfg, inputs, dev)
    means2, grads2 = _gpu_step(cfg, inputs, dev)
    for i in (0, 2, 4, 6):
        print(f"tuple[{i}]: got {float(means[i]):.9e} want {ref_means[i]:.9e}")
    for got, want, name in zip(grads, ref_grads, ("code", "code_pos")):
        print(f"grad {name}: relative L2 {float((got - want).norm() / want.norm()):.3e}")
    for i in (0, 2, 4, 6):
        _relclose(means[i], ref_means[i], 1e-3, 1e-5, f"tuple[{i}]")
    for got, want, name in zip(grads, ref_grads, ("code", "code_pos")):
        assert torch.isfinite(got).all(), name
        rel = (got - want).norm() / want.norm()
        assert rel < 3e-2, (name, float(rel))
    # the same call again: bit for bit (the routed list's order is the pair order, whichever wave is first)
    for i in (0, 2, 4, 6):
        assert torch.equal(means[i], means2[i]), f"tuple[{i}] differs between two runs"
    for got, again, name in zip(grads, grads2, ("code", "code_pos")):
        assert torch.equal(got, again), f"grad {name} differs between two runs"
