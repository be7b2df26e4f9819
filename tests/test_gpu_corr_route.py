"""ops.corr_forward against the C entry it selects, called directly on the loaded library: the same tensors, batch maps and seed,
a fresh workspace each - equal bits in `out`, in the drawn batch maps and in what dg_corr_backward_total forms from the two
workspaces.  Shapes, the smallest that reach each route's kernels: 8 x 8 maps with S = 5 on sampled coordinates (the fused small-grid
kernel), 14 x 14 maps with S = 14 (196 positions, the blob path) - on the shared identity grid for the masked entry, on sampled
coordinates per image for the extnorm and the intra entry."""
import ctypes
import functools

import pytest
import torch

from depthg_amd import _lib, ops
from oracle import depthg_oracle as O

pytestmark = pytest.mark.gpu

B, C, D, N = 2, 64, 16, 2
SEED = 20240611


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(shape, dev):
    """(desc factory, the seven maps but depth, depth, perms, the extras' tensors) of one of the three shapes, drawn once."""
    hw, S = (8, 5) if shape == "small" else (14, 14)
    dense = shape == "dense"
    g = torch.Generator().manual_seed({"small": 1, "dense": 2, "blob": 3}[shape])
    T = lambda *s: torch.randn(*s, generator=g).to(dev)
    f, fp, c, cp, aug = T(B, C, hw, hw), T(B, C, hw, hw), T(B, D, hw, hw), T(B, D, hw, hw), T(B, C, hw, hw)
    depth = torch.randint(0, 256, (B, 1, 32, 32), generator=g).float().to(dev)
    c1 = (O.identity_coords(B, hw) if dense else torch.rand(B, S, S, 2, generator=g) * 2 - 1).to(dev)
    c2 = c1 if dense else (torch.rand(B, S, S, 2, generator=g) * 2 - 1).to(dev)
    perms = torch.stack([O.super_perm(B, g) for _ in range(N)]).to(dev)
    keep = (torch.rand(B, C, generator=g) > 0.25).float().to(dev)           # a keep row with zeros in it
    assert 0 < int((keep[0] == 0).sum()) < C
    feat_inv = (0.05 + 0.1 * torch.rand(2 + N, B, S * S, generator=g)).to(dev)

    def desc(depth_term):
        return ops.make_desc(B, C, D, hw, hw, S, N, pointwise=True, zero_clamp=True, stabalize=False, depth_term=depth_term, need_grad=True,
                             shared_coords=dense, identity_grid=dense, shifts=(0.18, 0.12, 0.46, 0.05 if depth_term else 0.0),
                             depth_hw=(32, 32) if depth_term else (0, 0), weights=(0.67, 0.25, 0.63, 0.19 if depth_term else 0.0))
    return desc, (f, fp, c, cp, c1, c2), depth, perms, dict(keep=(keep, None, 1.0 / 0.75), feat_inv=feat_inv, intra_feats=aug)


# (entry, shape, the extra, draws its batch maps)
SELECTIONS = [
    ("dg_corr_forward", "small", None, False),
    ("dg_corr_forward_draw", "small", None, True),
    ("dg_corr_forward_intra_feats", "small", "intra_feats", True),
    ("dg_corr_forward_intra_feats", "blob", "intra_feats", False),
    ("dg_corr_forward_masked", "dense", "keep", False),
    ("dg_corr_forward_masked", "dense", "keep", True),
    ("dg_corr_forward_extnorm", "blob", "feat_inv", False),
]


@pytest.mark.parametrize("entry, shape, extra, draw", SELECTIONS, ids=[f"{e[8:]}-{s}-{'draw' if d else 'given'}" for e, s, _, d in SELECTIONS])
def test_one_route_and_the_entry_called_directly_give_equal_bits(entry, shape, extra, draw, dev):
    make, (f, fp, c, cp, c1, c2), depth, perms, extras = _inputs(shape, dev)
    intra = extra == "intra_feats"
    desc = make(depth_term=not intra)
    depth = None if intra else depth
    kw = {extra: extras[extra]} if extra else {}

    torch.manual_seed(SEED)
    got, got_perms, got_ws = ops.corr_forward(desc, f, fp, c, cp, depth, c1, c2, None if draw else perms, **kw)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0

    torch.manual_seed(SEED)
    seed = ops._cpu_seed() if draw else 0          # (the one host draw corr_forward makes for a drawing call)
    P = ops._ptr
    ws = ops.alloc_workspace(desc, dev, intra_feats=intra)
    out = ops._empty(_lib.DG_OUT_COUNT, torch.float32, dev)
    pm = ops._empty((N, B), torch.long, dev) if draw else perms
    mid = {None: (seed, None) if draw else (),
           "keep": (int(draw), seed, None, P(extras["keep"][0]), P(extras["keep"][1]), extras["keep"][2]),
           "feat_inv": (P(extras["feat_inv"]),),
           "intra_feats": (int(draw), seed, None, P(extras["intra_feats"]))}[extra]
    rc = getattr(_lib.load(), entry)(ctypes.byref(desc), P(f), P(fp), P(c), P(cp), P(depth), P(c1), P(c2), P(pm), *mid, P(out), P(ws),
                                     ws.numel(), ops._stream(dev))
    _lib.check(rc, entry)

    assert torch.equal(got, out)
    assert torch.equal(got_perms, pm) and (draw or got_perms is perms)
    assert got_ws is not ws and got_ws.numel() == ws.numel()
    # need_grad: the two workspaces hold the same gradient pieces
    gt = torch.tensor(0.7, device=dev)
    a = ops.corr_backward_total(desc, gt, c1, c2, got_perms, got_ws, tuple(c.shape))
    b = ops.corr_backward_total(desc, gt, c1, c2, pm, ws, tuple(c.shape))
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0 and torch.equal(x, y)
