"""GPU parity of the HIP head and probes (depthg_amd/head.py) against vectors from the imported
reference (tests/golden/head.npz) and the CPU oracle (oracle/head_oracle.py).

Tolerances: the head's 1x1 convolutions run as bf16 x bf16 MFMA products with fp32 accumulation (operands rounded to 8 bits of
mantissa, as the north_star prescribes for the correlation): code elements within 1.5e-2 of the largest |code| and 6e-3 relative
L2 (measured ~2e-3); gradients of the head tensors 2e-2 relative L2 (bf16 operands again; 6e-2 behind the ReLU, whose mask flips
where the bf16 pre-activation is within its rounding error of zero).  Dropout2d itself is exact (zeroed
weight columns, fp32 scale), the returned feats are the fp32 product.  ClusterLookup and the probe loss are fp32 kernels: 1e-5.

These shapes keep B <= 4: every k_head_dh2 block processes one tile and every split of k_head_wgrad3 one or two steps.  The loops of
the persistent kernels, the other route combinations of the backward's plan and bounds per row, column and element (on inputs whose
ReLU masks cannot flip, so cluster2.0 is held to the same figures as the rest) live in tests/test_gpu_head_margin.py, with
tests/head_margin_inputs.py and tests/test_head_margin_inputs_cpu.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("proj", ["nonlinear", "linear"])
def test_head_eval_matches_reference_vectors(proj, dev):
    from depthg_amd.head import ProjectionHead
    fx = load_golden("head.npz")
    t = torch.from_numpy(fx["tokens"])
    feat = t[:, 1:, :].reshape(2, 6, 6, -1).permute(0, 3, 1, 2).contiguous().to(dev)
    head = ProjectionHead(48, 12, proj).to(dev)
    with torch.no_grad():
        mods = list(head.cluster1.parameters()) + (list(head.cluster2.parameters()) if proj == "nonlinear" else [])
        for i, prm in enumerate(mods):
            prm.copy_(torch.from_numpy(fx[f"{proj}_w{i}"]))
    head.eval()
    code, feats = head(feat)
    want = torch.from_numpy(fx[f"{proj}_code"])
    assert feats is feat                                                   # eval: Dropout2d is the identity (src/modules.py:133-137)
    assert (code.cpu() - want).abs().max() < 1.5e-2 * want.abs().max() and _rel(code.cpu(), want) < 6e-3


@pytest.mark.parametrize("B,C,D,hw,proj", [(4, 384, 70, 28, "nonlinear"), (2, 768, 100, 28, "nonlinear"), (3, 384, 90, 14, "nonlinear"),
                                            (2, 384, 70, 15, "nonlinear"), (3, 384, 70, 28, "linear"), (2, 64, 16, 9, "nonlinear"),
                                            (2, 256, 70, 28, "nonlinear"), (2, 320, 33, 28, "nonlinear"), (1, 384, 70, 56, "nonlinear"),
                                            (2, 200, 24, 28, "linear"), (2, 384, 90, 28, "nonlinear"), (2, 384, 70, 20, "nonlinear"),
                                            (3, 352, 96, 24, "nonlinear"), (1, 384, 70, 8, "nonlinear")])
def test_head_train_forward_backward_vs_oracle(B, C, D, hw, proj, dev):
    """training pass with given Dropout2d draws: code, the returned feats and the six parameter gradients against the oracle;
    28x28 (the recipes), 14x14 / 15x15 / 9x9 (position counts that are not multiples of 8 or 4: the guarded paths), ViT-B width;
    widths below 384 on 28x28 / 56x56 maps (the 112-position, eight-wave forward with padded channel groups; the paired weight-gradient
    launch with partial tiles).  Round 6 - the backward of the headline widths (k_head_dh2 with d W2b inside, k_head_wgrad3): D = 90 /
    96 (six row blocks of d code, four-piece d code rows), 20 x 20 (400 positions: a ragged last step of 16 and a ragged last tile),
    C = 352 (clamped rows of both tiles), 8 x 8 at B = 1 (two steps per image: fewer steps than eight splits, the launches of round 5)."""
    from depthg_amd.head import ProjectionHead, draw_keep_masks
    from oracle import head_oracle as HO
    g = torch.Generator().manual_seed(100 * C + hw)
    feat = torch.randn(B, C, hw, hw, generator=g) * 2.0
    torch.manual_seed(C + hw)                               # (the head's initial weights)
    head = ProjectionHead(C, D, proj).to(dev).train()
    keeps = tuple((torch.rand(B, C, generator=g) > 0.1).float() for _ in range(3))
    code, feats = head(feat.to(dev), True, tuple(k.to(dev) for k in keeps))
    up = torch.randn(B, D, hw, hw, generator=g)
    (code * up.to(dev)).sum().backward()
    prm = [p.detach().cpu().clone().requires_grad_(True) for p in head.parameters()]
    nl = proj == "nonlinear"
    code_r, feats_r = HO.head_forward(feat, prm[0], prm[1], *(prm[2:] if nl else (None,) * 4), keeps=keeps, p=0.1)
    (code_r * up).sum().backward()
    assert torch.allclose(feats.cpu(), feats_r, rtol=1e-6, atol=0)
    zero_ch = keeps[2] == 0
    assert bool((feats.cpu().abs().sum((2, 3))[zero_ch] == 0).all())
    assert (code.cpu() - code_r).abs().max() < 1.5e-2 * code_r.abs().max() and _rel(code.detach().cpu(), code_r.detach()) < 6e-3
    for got, want, (name, _) in zip(head.parameters(), prm, head.named_parameters()):
        assert got.grad is not None and torch.isfinite(got.grad).all(), name
        # cluster2's first convolution sits behind the ReLU: where the bf16 pre-activation and the oracle's fp32 one differ in
        # sign (|pre| below the bf16 product error, ~0.2 % of the elements) the mask flips - the same mechanism as the clamp mask of
        # the loss; measured 3.4-3.9e-2
        tol = 6e-2 if name.startswith("cluster2.0") else 2e-2
        assert _rel(got.grad.cpu(), want.grad) < tol, (name, _rel(got.grad.cpu(), want.grad))
    # a dropped input channel gets no weight gradient (its column was zeroed)
    gw1 = head.cluster1[0].weight.grad.cpu().reshape(D, C)
    dropped_everywhere = (keeps[0] == 0).all(0)
    assert bool((gw1[:, dropped_everywhere] == 0).all())


def test_head_is_deterministic_and_draws_its_own_masks(dev):
    from depthg_amd.head import ProjectionHead
    torch.manual_seed(0)
    head = ProjectionHead(384, 70).to(dev).train()
    feat = torch.randn(4, 384, 28, 28, device=dev)
    torch.manual_seed(1)
    c1, f1 = head(feat)
    torch.manual_seed(1)
    c2, f2 = head(feat)
    assert torch.equal(c1, c2) and torch.equal(f1, f2)                    # same draws, same bits
    c3, f3 = head(feat)
    assert not torch.equal(c1, c3) and not torch.equal(f1, f3)
    frac = float((f1.abs().sum((2, 3)) == 0).float().mean())
    assert 0.05 < frac < 0.16                                              # Dropout2d(p=.1) zeroes whole channels (quirk Q10)


@pytest.mark.parametrize("proj,feats_dropout", [("linear", True), ("nonlinear", False), ("linear", False), (None, True)])
def test_head_random_stream_follows_the_reference(proj, feats_dropout, dev):
    """only the Dropout2d uses that exist draw (src/modules.py:122-132), so with projection_type "linear" the returned
    feats carry the SECOND draw of the pass, with cfg.dropout off nothing is drawn for them, and whatever is drawn next comes
    from the same generator position as behind the reference's nn.Dropout2d sequence.  Also: features that require grad are
    refused (no d/d image_feat kernel), and under no_grad the head keeps no hidden tile."""
    from depthg_amd.head import ProjectionHead
    torch.manual_seed(0)
    head = ProjectionHead(64, 16, proj).to(dev).train()
    feat = torch.randn(3, 64, 9, 9, device=dev)
    torch.manual_seed(21)
    code, feats = head(feat, feats_dropout)
    nxt = torch.rand(4, device=dev)
    torch.manual_seed(21)
    drop = torch.nn.Dropout2d(0.1).train()
    ones = torch.ones(3, 64, 1, 1, device=dev)
    ndraws = (0 if proj is None else (2 if proj == "nonlinear" else 1)) + (1 if feats_dropout else 0)
    draws = [drop(ones) for _ in range(ndraws)]
    nxt_ref = torch.rand(4, device=dev)
    assert torch.equal(nxt, nxt_ref)
    if feats_dropout:
        assert torch.allclose(feats, feat * draws[-1], rtol=1e-6, atol=0)
    else:
        assert feats is feat
    if proj is None:
        assert code is feat
        return
    with pytest.raises(RuntimeError, match="require grad"):
        head(feat.clone().requires_grad_(True))
    with torch.no_grad():
        c2, _ = head(feat, feats_dropout)
    assert c2.grad_fn is None and torch.isfinite(c2).all()


def test_cluster_lookup_matches_reference_vectors(dev):
    from depthg_amd.head import ClusterLookup
    fx = load_golden("head.npz")
    cl = ClusterLookup(12, 5).to(dev)
    with torch.no_grad():
        cl.clusters.copy_(torch.from_numpy(fx["cl_clusters"]))
    x = torch.from_numpy(fx["cl_x"]).to(dev).requires_grad_(True)
    loss_h, probs_h = cl(x, None)
    loss_s, probs_s = cl(x, 2.0)
    logp = cl(x, 2.0, log_probs=True)
    (loss_h + loss_s).backward()
    assert abs(float(loss_h) - float(fx["cl_loss_hard"])) < 1e-6 and abs(float(loss_s) - float(fx["cl_loss_soft"])) < 1e-6
    assert np.array_equal(probs_h.cpu().numpy(), fx["cl_probs_hard"])
    assert np.abs(probs_s.detach().cpu().numpy() - fx["cl_probs_soft"]).max() < 1e-6
    assert np.abs(logp.detach().cpu().numpy() - fx["cl_logp"]).max() < 1e-5
    assert np.abs(x.grad.cpu().numpy() - fx["cl_grad_x"]).max() < 1e-6
    assert np.abs(cl.clusters.grad.cpu().numpy() - fx["cl_grad_clusters"]).max() < 1e-6


@pytest.mark.parametrize("alpha", [None, 3.0])
def test_cluster_lookup_at_training_size(alpha, dev):
    from depthg_amd.head import ClusterLookup
    from oracle import head_oracle as HO
    g = torch.Generator().manual_seed(9)
    B, D, n, hw = 8, 70, 27, 28
    x = torch.randn(B, D, hw, hw, generator=g)
    cl = ClusterLookup(D, n).to(dev)
    xr = x.clone().requires_grad_(True)
    cr = cl.clusters.detach().cpu().clone().requires_grad_(True)
    loss_r, probs_r = HO.cluster_lookup(xr, cr, alpha)
    loss_r.backward()
    xg = x.to(dev).requires_grad_(True)
    loss, probs = cl(xg, alpha)
    loss.backward()
    assert abs(float(loss) - float(loss_r)) < 1e-6
    assert (probs.cpu() - probs_r).abs().max() < 1e-5 if alpha is not None else float((probs.cpu() != probs_r).float().mean()) < 1e-4
    assert _rel(cl.clusters.grad.cpu(), cr.grad) < 1e-4 and _rel(xg.grad.cpu(), xr.grad) < (1e-4 if alpha is not None else 2e-3)


@pytest.mark.parametrize("B,n,hw,HW", [(3, 27, 28, 224), (2, 27, 28, 320), (2, 3, 14, 100), (2, 27, 40, 320), (1, 6, 7, 50)])
def test_probe_cross_entropy_vs_oracle(B, n, hw, HW, dev):
    """resize (align_corners=False) + masked cross entropy: 224 and 320 label sizes of the recipes, a non-integer scale (100 / 14,
    50 / 7), labels with -1 (unlabelled) and out-of-range entries"""
    from depthg_amd.head import probe_cross_entropy
    from oracle import head_oracle as HO
    g = torch.Generator().manual_seed(HW + n)
    logits = torch.randn(B, n, hw, hw, generator=g) * 3
    label = torch.randint(-1, n + 1, (B, HW, HW), generator=g)
    lr = logits.clone().requires_grad_(True)
    want = HO.probe_cross_entropy(lr, label, n)
    want.backward()
    lg = logits.to(dev).requires_grad_(True)
    got = probe_cross_entropy(lg, label.to(dev))
    (got * 1.5).backward()
    assert abs(float(got) - float(want)) < 1e-5 * abs(float(want))
    assert _rel(lg.grad.cpu(), 1.5 * lr.grad) < 1e-4


@pytest.mark.parametrize("B,C,D,hw,proj", [(4, 384, 70, 28, "nonlinear"), (3, 384, 70, 15, "nonlinear"), (2, 384, 70, 28, "linear"),
                                            (5, 64, 16, 9, "nonlinear"), (2, 384, 70, 28, None)])
def test_head_pair_equals_two_calls(B, C, D, hw, proj, dev):
    """ProjectionHead.forward_pair = the two featurizer passes of a training step (src/train_segmentation.py:303-306: net(img),
    net(img_pos), same weights) as one set of launches.  Against two forward() calls with the same keep masks: code, code_pos, feats,
    feats_pos BIT-identical (the same kernels on the same tiles); the six parameter gradients - summed over both passes by one
    split reduction instead of by autograd's addition of two - within 1e-5 relative; the torch generator ends where it ends
    behind two calls; odd batch sizes, position counts off the fast paths, the linear head and projection_type None included."""
    from depthg_amd.head import ProjectionHead, draw_keep_masks_pair
    g = torch.Generator().manual_seed(31 * C + hw + B)
    f, fp = (torch.randn(B, C, hw, hw, generator=g) * 2.0).to(dev), (torch.randn(B, C, hw, hw, generator=g) * 2.0).to(dev)
    up, up_pos = torch.randn(B, D if proj else C, hw, hw, generator=g).to(dev), torch.randn(B, D if proj else C, hw, hw, generator=g).to(dev)
    torch.manual_seed(C + hw)
    head = ProjectionHead(C, D, proj).to(dev).train()
    torch.manual_seed(77)
    keeps = draw_keep_masks_pair(B, C, dev, 0.1, use=(proj is not None, proj == "nonlinear", True))
    end_pair = torch.rand(3, device=dev)
    ka = tuple(k[:B] if k is not None else None for k in keeps)
    kb = tuple(k[B:] if k is not None else None for k in keeps)
    # two calls
    c1, f1 = head(f, True, ka)
    c2, f2 = head(fp, True, kb)
    if proj is not None:
        ((c1 * up).sum() + (c2 * up_pos).sum()).backward()
        want = [p.grad.clone() for p in head.parameters()]
        for p in head.parameters():
            p.grad = None
    # one pair call
    (pc1, pf1), (pc2, pf2) = head.forward_pair(f, fp, True, keeps)
    assert torch.equal(pc1, c1) and torch.equal(pc2, c2) and torch.equal(pf1, f1) and torch.equal(pf2, f2)
    if proj is not None:
        ((pc1 * up).sum() + (pc2 * up_pos).sum()).backward()
        for p, w, (name, _) in zip(head.parameters(), want, head.named_parameters()):
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            assert _rel(p.grad, w) < 1e-5, (name, _rel(p.grad, w))
        # one pass alone in the loss: the other's upstream is absent, not an error
        for p in head.parameters():
            p.grad = None
        (qc1, _), (qc2, _) = head.forward_pair(f, fp, True, keeps)
        (qc1 * up).sum().backward()
        assert all(torch.isfinite(p.grad).all() for p in head.parameters())
    # masks drawn inside: the generator advances as for two calls
    torch.manual_seed(77)
    head.forward_pair(f, fp, True)
    end_inside = torch.rand(3, device=dev)
    torch.manual_seed(77)
    head(f, True)
    head(fp, True)
    end_two = torch.rand(3, device=dev)
    assert torch.equal(end_inside, end_two) and torch.equal(end_pair, end_two)
    with pytest.raises(ValueError, match="depthg_amd"):
        head.forward_pair(f, fp[:, :, : hw - 1], True) if proj is not None else (_ for _ in ()).throw(ValueError("depthg_amd: n/a"))


def test_keep_masks_from_the_device_generator(dev):
    """ops.keep_masks_state (dg_rand_keep_state): the Dropout2d masks of a hipGraph-recorded step from the device-resident generator,
    one launch - flags 1 / 0 with keep frequency 1 - p, only the requested ones, successive draws differ, and the head takes them
    as `keeps` exactly like masks drawn by torch."""
    from depthg_amd import ops
    from depthg_amd.head import ProjectionHead
    torch.manual_seed(11)
    st = ops.new_perm_state(dev)
    k1, k2, k3 = ops.keep_masks_state(st, 64, 384, 0.1)
    assert k1.shape == (64, 384) and int(st[1]) == 1
    allk = torch.stack([k1, k2, k3])
    assert bool(((allk == 0) | (allk == 1)).all()) and abs(float(allk.mean()) - 0.9) < 0.01
    assert not torch.equal(k1, k2)
    a, b, c = ops.keep_masks_state(st, 64, 384, 0.1, use=(True, False, True))
    assert b is None and not torch.equal(a, k1) and int(st[1]) == 2
    head = ProjectionHead(384, 70).to(dev).train()
    f, fp = torch.randn(32, 384, 28, 28, device=dev), torch.randn(32, 384, 28, 28, device=dev)
    (c1, f1), (c2, f2) = head.forward_pair(f, fp, True, (k1, k2, k3))
    assert torch.isfinite(c1).all() and torch.isfinite(c2).all()
    assert bool((f1.abs().sum((2, 3))[k3[:32] == 0] == 0).all()) and bool((f2.abs().sum((2, 3))[k3[32:] == 0] == 0).all())
