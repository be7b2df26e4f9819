"""d loss / d feats of the reconstruction term on the GPU (k_rec_bwd_code<true> through dg_rec_feats_backward, ops.rec_loss_backward(
want_feats=True), rec_loss.reconstruction_loss(feats_grad=True)), the head's epilogue addend (k_head_dx<MB, true> through
dg_head_backward_input's grad_feats_out, ProjectionHead(input_grad=True, feats_grad=True)) and cfg.dg_rec_feats_grad in training_step.

Parity: d feats against the float64 restatement (tests/rec_feats_reference.py) with the float32 torch chain under autograd on the
GPU as the yardstick, in the measure and under the MARGIN of tests/test_gpu_rec_loss.py: relative L2, at most 2 x the yardstick's.
For `aligned` the true gradient vanishes (1e-17 of a term): there both figures are the ABSOLUTE L2 error - the same ratio, without a
denominator made of float64 rounding residue.  scripts/rec_feats_parity.py runs measure() over the cases and writes
profiles/rec_feats_parity.md.

Head: d image_feat against float64 autograd of oracle.head_oracle.head_forward on inputs of tests/head_margin_inputs.py (they flip no
ReLU mask) with the criterion of tests/test_gpu_head_input_grad.py - every figure within FACTOR x the bf16-operand yardstick's, L2
below CAP_L2 - when the loss reads code, feats, or both.  The addend itself is an fp32 product of the fp32 upstream and the fp32
scale: where the loss reads feats alone the result is held to 2^-23 relative L2 (the scale's rounding and the product's).

Segmenter: the gradient of the depth encoder against a float32 torch-only restatement of the step's reconstruction path within 6e-2
relative L2, the bound tests/test_gpu_depth_featurizer.py holds for the encoder's gradients behind the head.
"""
import copy

import pytest
import torch

import head_input_grad_reference as HR
import head_margin_inputs as H
import rec_feats_reference as F
import rec_loss_reference as R
from oracle import head_oracle as HO

pytestmark = pytest.mark.gpu
MARGIN = 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- the loss term
def kernel_d_feats(shape, kind, dev, params=True):
    """d feats of reconstruction_loss(feats_grad=True); `dropped` goes in as an ops.DeferredDropout, whose maps get the gradient."""
    from depthg_amd import ops, reconstruction_loss
    i = F.inputs(shape, kind)
    code, weight, bias = (i[k].to(dev).requires_grad_(params) for k in ("code", "weight", "bias"))
    raw = i["raw"].to(dev).requires_grad_(True)
    feats = raw if i["keep"] is None else ops.DeferredDropout(raw, i["keep"].to(dev), i["scale"])
    reconstruction_loss(code, feats, weight, bias, feats_grad=True).backward()
    return raw.grad


def measure(shape, kind, dev):
    """{"kernel", "yard": error figures, "ratio"} of one case against the float64 restatement."""
    want = F.truth(shape, kind)
    err = lambda g: float((g.double().cpu() - want).norm()) / (1.0 if kind == "aligned" else float(want.norm()))
    k, y = err(kernel_d_feats(shape, kind, dev)), err(F.torch_d_feats(shape, kind, torch.float32, dev))
    return {"kernel": k, "yard": y, "ratio": k / y if y > 0 else (0.0 if k == 0 else float("inf"))}


@pytest.mark.parametrize("shape,kind", F.CASES)
def test_d_feats_within_the_yardsticks_margin(shape, kind, dev):
    m = measure(shape, kind, dev)
    print(f"{shape}/{kind}: d_feats kernel {m['kernel']:.3e} yardstick {m['yard']:.3e} ratio {m['ratio']:.2f}")
    assert m["kernel"] <= MARGIN * m["yard"], m


@pytest.mark.parametrize("shape,kind", [("ragged", "random"), ("ragged", "dropped"), ("head", "random"), ("head", "dropped")])
def test_the_other_gradients_keep_their_bits_and_two_calls_agree(shape, kind, dev):
    from depthg_amd import ops
    i = F.inputs(shape, kind)
    code, raw, weight, bias = (i[k].to(dev) for k in ("code", "raw", "weight", "bias"))
    kw = {} if i["keep"] is None else dict(keep=i["keep"].to(dev), scale=i["scale"])
    g = torch.tensor(0.75, device=dev)
    loss, ws = ops.rec_loss_forward(code, raw, weight, bias, **kw)
    parent = ops.rec_loss_backward(ws, code, raw, weight, bias, g, **kw)
    runs = [ops.rec_loss_backward(ws, code, raw, weight, bias, g, want_feats=True, **kw) for _ in range(2)]
    assert len(runs[0]) == 4 and runs[0][3].shape == raw.shape
    for a, b in zip(parent, runs[0][:3]):                                     # d code, d W, d b: the launches they always came from
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    alone = ops.rec_loss_backward(ws, code, raw, weight, bias, g, want_feats=True, want_params=False, **kw)
    assert alone[:3] == (None, None, None) and torch.equal(alone[3], runs[0][3])
    once = ops.rec_loss_backward(ws, code, raw, weight, bias, torch.tensor(1.0, device=dev), want_feats=True, **kw)[3]
    assert float((runs[0][3] - once * 0.75).norm() / once.norm()) <= 1e-6     # the upstream gradient is a factor


@pytest.mark.parametrize("shape,kind", [("ragged", "dropped"), ("tiny", "random"), ("ragged", "small_f")])
def test_poisoned_buffers_leave_no_element_unwritten(shape, kind, dev, monkeypatch):
    """ops.POISON (DG_POISON=1): the outputs and the workspace start as 0xFF bytes - NaN in whatever no kernel writes."""
    from depthg_amd import ops
    monkeypatch.setattr(ops, "POISON", False)
    want = kernel_d_feats(shape, kind, dev)
    monkeypatch.setattr(ops, "POISON", True)
    got, alone = kernel_d_feats(shape, kind, dev), kernel_d_feats(shape, kind, dev, params=False)
    assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want) and torch.equal(alone, want)
    keep = F.inputs(shape, kind)["keep"]
    if keep is not None:
        dropped = (keep == 0).to(dev)
        assert bool(dropped.any()) and bool((got[dropped] == 0).all()) and bool((got[~dropped] != 0).any())


def test_without_a_feats_that_asks_the_keyword_changes_no_bit(dev):
    from depthg_amd import reconstruction_loss
    code, feats, weight, bias = (t.to(dev) for t in R.operands("ragged", "random"))
    outs = []
    for kw in ({}, {"feats_grad": True}):
        c, w, b = (t.clone().requires_grad_(True) for t in (code, weight, bias))
        loss = reconstruction_loss(c, feats, w, b, **kw)
        loss.backward()
        outs.append((loss.detach(), c.grad, w.grad, b.grad))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    with pytest.raises(RuntimeError, match="no gradient for `feats`"):
        reconstruction_loss(code, feats.clone().requires_grad_(True), weight, bias)


# ---------------------------------------------------------------------------------------------------------------- the head
def head_inputs(pair, B, C, D, hw, seed):
    """Inputs of tests/head_margin_inputs.py at (B, C, D); hw = (h, w): the first h w positions of the next square map (the margins
    hold per position), and an upstream gradient for the returned feats."""
    h, w = hw
    side = next(s for s in range(1, 64) if s * s >= h * w)
    case = H.Case(f"rec-feats-{C}-{h}x{w}", pair, B, C, D, side, "nonlinear", seed, None, None, None, None, False, None, "")
    inp = H.case_inputs(case)
    cut = lambda t: t.flatten(2)[:, :, :h * w].reshape(t.shape[0], t.shape[1], h, w).contiguous()
    inp = H.Inputs(cut(inp.feat), inp.keeps, *inp[2:8], cut(inp.up))
    upf = torch.randn(inp.feat.shape, generator=torch.Generator().manual_seed(9000 + seed), dtype=torch.float64).float()
    return case, inp, upf


def head_truth(inp, upf, reads, feats_dropout=True):
    """float64 autograd of oracle.head_oracle.head_forward; reads: which of (code, feats) the loss reads."""
    prm = [t.double() for t in (inp.w1, inp.b1, inp.w2a, inp.b2a, inp.w2b, inp.b2b)]
    f = inp.feat.double().requires_grad_(True)
    code, feats = HO.head_forward(f, *prm, keeps=tuple(k.double() for k in inp.keeps), p=H.P_DROP, feats_dropout=feats_dropout)
    ((code * inp.up.double()).sum() * reads[0] + (feats * upf.double()).sum() * reads[1]).backward()
    return f.grad


def head_yardstick(inp, upf, reads, truth):
    """The bf16-operand restatement of the code half (head_input_grad_reference.dx_manual, the truth's ReLU mask) plus the exact
    addend: the error the operand formats force on any kernel."""
    rounded = HR.dx_manual(inp, H.to_bf16, mask=HR.pre_activation(inp) > 0) * reads[0]
    rounded = rounded + reads[1] * (inp.keeps[2].double() * H.SCALE)[:, :, None, None] * upf.double()
    return H.tensor_errors(rounded, truth, "code")


def run_head(case, inp, upf, dev, reads, feats_grad=True, need=(True, True), feats_dropout=True, feats_read=(True, True)):
    import test_gpu_head_input_grad as T
    head = T.make_head(case, inp, dev)
    keeps = tuple(k.to(dev) for k in inp.keeps)
    feat, up, upf = inp.feat.to(dev), inp.up.to(dev), upf.to(dev)
    kw = dict(input_grad=True, feats_grad=True) if feats_grad else dict(input_grad=True)
    term = lambda code, feats, sl: (code * up[sl]).sum() * reads[0] + ((feats * upf[sl]).sum() * reads[1] if reads[1] else 0.0)
    if case.pair:
        B = case.B
        fa, fb = (feat[:B].clone().requires_grad_(need[0]), feat[B:].clone().requires_grad_(need[1]))
        (c1, f1), (c2, f2) = head.forward_pair(fa, fb, feats_dropout, keeps, **kw)
        assert f1.requires_grad == (need[0] and feats_grad) and f2.requires_grad == (need[1] and feats_grad)
        loss = (c1 * up[:B]).sum() * reads[0] + (c2 * up[B:]).sum() * reads[0]
        for f, sl, read in ((f1, slice(0, B), feats_read[0]), (f2, slice(B, 2 * B), feats_read[1])):
            if f.requires_grad and reads[1] and read:
                loss = loss + (f * upf[sl]).sum()
        loss.backward()
        dx = (fa.grad, fb.grad)
    else:
        fa = feat.clone().requires_grad_(True)
        code, feats = head(fa, feats_dropout, keeps, **kw)
        assert feats.requires_grad == feats_grad or not feats_dropout
        term(code, feats, slice(None)).backward()
        dx = (fa.grad,)
    torch.cuda.synchronize()
    return dx, {name: prm.grad for name, prm in head.named_parameters()}


def check_head(case, got, truth, yard, reads):
    assert bool(torch.isfinite(got).all())
    if reads == (0, 1):                      # the addend alone: one fp32 product of the upstream and the fp32 scale
        rel = float((got.double().cpu() - truth).norm() / truth.norm())
        print(f"{case.id} reads feats: d image_feat L2 {rel:.3e} (bound {2.0 ** -23:.3e})")
        assert rel <= 2.0 ** -23
        return
    bad = []
    for fig, (k, where) in H.tensor_errors(got, truth, "code").items():
        y = yard[fig][0]
        print(f"{case.id} reads {reads} d image_feat {fig}: kernel {k:.3e} yardstick {y:.3e} ratio {k / y:.2f} (factor {H.FACTOR[fig]:g})")
        if not k <= H.FACTOR[fig] * y or (fig == "l2" and not k <= H.CAP_L2):
            bad.append((fig, k, y, where))
    assert not bad, bad


@pytest.mark.parametrize("B,C,D,hw,seed", [(2, 384, 70, (8, 8), 31), (3, 128, 27, (5, 7), 32)], ids=["head-8x8", "ragged-5x7"])
def test_head_adds_the_feats_gradient_in_its_input_launch(B, C, D, hw, seed, dev, monkeypatch):
    from depthg_amd import ops
    torch.set_num_threads(16)
    case, inp, upf = head_inputs(False, B, C, D, hw, seed)
    monkeypatch.setattr(ops, "POISON", True)
    base = None
    for reads in ((1, 0), (0, 1), (1, 1)):
        truth = head_truth(inp, upf, reads)
        dx, grads = run_head(case, inp, upf, dev, reads)
        check_head(case, dx[0], truth, head_yardstick(inp, upf, reads, truth), reads)
        dropped = ((inp.keeps[0] == 0) & (inp.keeps[1] == 0) & (inp.keeps[2] == 0)).to(dev)
        assert bool((dx[0][dropped] == 0).all())
        if reads == (1, 0):
            base = (dx[0], grads)
        elif reads == (1, 1):                # the parameters never see the addend; two calls give the same bits
            assert all(torch.equal(grads[n], base[1][n]) for n in grads)
            assert torch.equal(run_head(case, inp, upf, dev, reads)[0][0], dx[0])
    # the keyword off is the route it was: d image_feat and the six parameter gradients, bit for bit
    off_dx, off_grads = run_head(case, inp, upf, dev, (1, 0), feats_grad=False)
    assert torch.equal(off_dx[0], base[0]) and set(off_grads) == set(H.PARAMS)
    assert all(torch.equal(off_grads[n], base[1][n]) for n in off_grads)
    # without feats_dropout the head hands back its input, and autograd adds the two gradients itself
    truth = head_truth(inp, upf, (1, 1), feats_dropout=False)
    dx, _ = run_head(case, inp, upf, dev, (1, 1), feats_dropout=False)
    want = base[0] + upf.to(dev)
    assert torch.equal(dx[0], want) and float((dx[0].double().cpu() - truth).norm() / truth.norm()) <= H.CAP_L2


def test_head_pair_with_one_pass_asking(dev, monkeypatch):
    from depthg_amd import ops
    torch.set_num_threads(16)
    B = 3
    case, inp, upf = head_inputs(True, B, 128, 27, (5, 7), 33)
    monkeypatch.setattr(ops, "POISON", True)
    truth = head_truth(inp, upf, (1, 1))
    dx, grads = run_head(case, inp, upf, dev, (1, 1), need=(False, True))
    assert dx[0] is None and dx[1] is not None
    second = H.Inputs(inp.feat[B:], tuple(k[B:] for k in inp.keeps), *inp[2:8], inp.up[B:])
    check_head(case, dx[1], truth[B:], head_yardstick(second, upf[B:], (1, 1), truth[B:]), (1, 1))
    # both passes asking, the first one's feats unread: its images carry the code half alone, the second's are what they were
    dx2, grads2 = run_head(case, inp, upf, dev, (1, 1), need=(True, True), feats_read=(False, True))
    assert torch.equal(dx2[1], dx[1]) and all(torch.equal(grads[n], grads2[n]) for n in grads)
    first = H.Inputs(inp.feat[:B], tuple(k[:B] for k in inp.keeps), *inp[2:8], inp.up[:B])
    truth_code = head_truth(inp, upf, (1, 0))
    check_head(case, dx2[0], truth_code[:B], head_yardstick(first, upf[:B], (1, 0), truth_code[:B]), (1, 0))
    # both read
    dx3, _ = run_head(case, inp, upf, dev, (1, 1))
    assert torch.equal(dx3[1], dx[1])
    check_head(case, dx3[0], truth[:B], head_yardstick(first, upf[:B], (1, 1), truth[:B]), (1, 1))


# ---------------------------------------------------------------------------------------------------------------- the segmenter
DEPTH_TOPS = ("depth_downscaling", "cross_attn")


def seg_batch(dev, B=2, hw=64, n_classes=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(0, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.rand(B, 1, hw, hw, generator=g).to(dev), "depth_pos": torch.rand(B, 1, hw, hw, generator=g).to(dev)}


def seg_step(dev, **over):
    """One seeded training_step -> (segmenter as it was before the step, logs, {name: gradient} of the trained depth parameters)."""
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(11)
    seg = UnsupervisedSegmenter(5, default_segmenter_cfg(arch="dino_depth", res=64, feature_samples=5, **over)).to(dev).train()
    before = copy.deepcopy(seg)
    grads = {}
    for name, p in seg.net.named_parameters():                                # (the step may clear p.grad: keep what backward hands over)
        if name.split(".")[0] in DEPTH_TOPS and p.requires_grad:
            p.register_hook(lambda g, name=name: grads.__setitem__(name, g.detach().clone()))
    torch.manual_seed(9)
    loss, logs = seg.training_step(seg_batch(dev), 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return before, logs, grads


@pytest.mark.parametrize("guidance,fused", [("sum", {}), ("cross_attn", {}), ("sum", {"dg_fused_depth_encoder": True}),
                                            ("cross_attn", {"dg_fused_cross_attn": True})],
                         ids=["sum", "cross_attn", "sum-fused-encoder", "cross_attn-fused-attention"])
def test_training_step_trains_the_depth_modules_through_feats(guidance, fused, dev):
    _, logs, grads = seg_step(dev, guidance=guidance, rec_weight=0.5, dg_rec_feats_grad=True, **fused)
    _, logs0, grads0 = seg_step(dev, guidance=guidance, rec_weight=0.0, **fused)
    assert "loss/rec" in logs and "loss/rec" not in logs0 and bool(torch.isfinite(logs["loss/rec"]))
    trained = {"sum": 10, "cross_attn": 14}[guidance]
    assert len(grads) == len(grads0) == trained
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())
    assert not torch.equal(grads["depth_downscaling.0.weight"], grads0["depth_downscaling.0.weight"])


def test_sum_guidance_step_matches_a_torch_restatement_of_the_reconstruction_path(dev):
    """correspondence_weight = 0: the step's loss is rec_weight x the reconstruction term, whose gradient reaches the depth encoder
    through code (the head) and through feats (the new path).  The restatement: the frozen backbone's features, the encoder, the add,
    oracle.head_oracle.head_forward with the step's own keep masks (the same seed, the same draw), the float32 torch chain."""
    from depthg_amd.head import draw_keep_masks
    weight = 0.5
    before, logs, grads = seg_step(dev, guidance="sum", rec_weight=weight, dg_rec_feats_grad=True, correspondence_weight=0.0)
    assert len(grads) == 10
    batch = seg_batch(dev)
    net = before.net
    with torch.no_grad():
        image_feat = net._backbone(batch["img"])[0]
    torch.manual_seed(9)
    keeps = draw_keep_masks(2, 384, dev, 0.1)
    x = image_feat + net.depth_downscaling(batch["depth"])
    prm = [p.detach() for m in (net.cluster1, net.cluster2) for p in m.parameters()]
    code, feats = HO.head_forward(x, *prm, keeps=keeps, p=0.1)
    rec = R.torch_chain(code, feats, before.decoder.weight.detach(), before.decoder.bias.detach())
    # (every s is a cosine: it moves by at most the relative error of the head's bf16 code, 6e-3 in L2 in tests/test_gpu_head.py)
    print(f"loss/rec: step {float(logs['loss/rec']):.6e} restatement {float(rec.detach()):.6e}")
    assert abs(float(rec.detach()) - float(logs["loss/rec"])) <= 6e-3
    (weight * rec).backward()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for name, p in net.named_parameters():
        if name.split(".")[0] == "depth_downscaling":
            print(f"d {name}: L2 {rel(grads[name], p.grad):.3e}")
            assert rel(grads[name], p.grad) < 6e-2, (name, rel(grads[name], p.grad))
    # and the path through feats is a real share of it: the same restatement with feats detached is further away than the bound
    for p in net.parameters():
        p.grad = None
    x = image_feat + net.depth_downscaling(batch["depth"])
    code, feats = HO.head_forward(x, *prm, keeps=keeps, p=0.1)
    (weight * R.torch_chain(code, feats.detach(), before.decoder.weight.detach(), before.decoder.bias.detach())).backward()
    assert rel(grads["depth_downscaling.6.weight"], net.depth_downscaling[6].weight.grad) > 6e-2
