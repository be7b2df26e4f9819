"""The reconstruction term on the GPU (dg_rec_loss.hip through ops.rec_loss_forward / rec_loss_backward and
rec_loss.reconstruction_loss): loss and the three gradients against the float64 restatement (tests/rec_loss_reference.py) with the same
chain in float32 torch on the GPU as the yardstick, zero vectors, determinism, the complete write of the gradients, views and deferred
Dropout2d as inputs, and cfg.rec_weight in training_step.

MARGIN: the kernels' errors may be at most MARGIN x the yardstick's - 2, what tests/adam_reference.py and the CRF-loss and
augmentation-alignment tests hold.  A loss error is floored at one float32 spacing of the loss's magnitude (neither route can return a
better scalar than the format holds); gradient figures are relative L2.  scripts/rec_loss_parity.py runs measure() over R.CASES and
writes the ratios to profiles/rec_loss_parity.md.
"""
import pytest
import torch

import rec_loss_reference as R

MARGIN = 2.0
GRADS = ("d_code", "d_weight", "d_bias")


def _run(fn, code, feats, weight, bias, dev):
    c, w, b = (t.detach().clone().to(dev).requires_grad_(True) for t in (code, weight, bias))
    loss = fn(c, feats.to(dev), w, b)
    loss.backward()
    return float(loss.detach().double()), c.grad.double().cpu(), w.grad.double().cpu().reshape(w.shape[0], w.shape[1]), b.grad.double().cpu()


def kernel(code, feats, weight, bias, dev):
    from depthg_amd import reconstruction_loss
    return _run(reconstruction_loss, code, feats, weight, bias, dev)


def yardstick(code, feats, weight, bias, dev):
    """conv2d + the two norms + product + sum + mean + autograd in float32 torch on the GPU."""
    return _run(R.torch_chain, code, feats, weight, bias, dev)


def figures(got, t):
    """(loss error over the mean |s|, floored at one float32 spacing of the loss; relative L2 of d code, d W, d b)."""
    rel = lambda g, want: float((g - want).norm() / want.norm())
    return (max(abs(got[0] - t["loss"]), R.spacing32(t["loss"])) / t["mean_abs_s"],) + tuple(rel(g, t[k]) for g, k in zip(got[1:], GRADS))


def measure(shape, kind, dev):
    """The figures of one case, of the kernels and of the yardstick, against the float64 restatement."""
    ops_, t = R.operands(shape, kind), R.truth(shape, kind)
    k, y = figures(kernel(*ops_, dev), t), figures(yardstick(*ops_, dev), t)
    out = {"loss": t["loss"]}
    for i, name in enumerate(("loss",) + GRADS):
        out[name + "_err_kernel"], out[name + "_err_yard"] = k[i], y[i]
    return out


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", R.CASES)
def test_loss_and_gradients_within_the_yardsticks_margin(shape, kind, dev):
    m = measure(shape, kind, dev)
    print(f"{shape}/{kind}: loss {m['loss']:.9e} | " + " | ".join(
        f"{n} kernel {m[n + '_err_kernel']:.3e} yardstick {m[n + '_err_yard']:.3e}" for n in ("loss",) + GRADS))
    assert m["loss_err_kernel"] <= MARGIN * m["loss_err_yard"], m
    if kind == "aligned":                    # the true gradient vanishes: the loss only
        return
    for n in GRADS:
        assert m[n + "_err_kernel"] <= MARGIN * m[n + "_err_yard"], (n, m)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["tiny", "head"])
def test_aligned_features_give_minus_one(shape, dev):
    """feats = decoder(code): every s is 1 - the loss only."""
    from depthg_amd import ops, reconstruction_loss
    code, feats, weight, bias = (t.to(dev) for t in R.operands(shape, "aligned"))
    assert abs(float(reconstruction_loss(code, feats, weight, bias)) + 1.0) <= 2 * 2.0 ** -23
    loss, ws = ops.rec_loss_forward(code, feats, weight, bias)
    B, _, _, (h, w) = R.SHAPES[shape]
    sec = ops.rec_loss_workspace_sections(ws, B, h, w)
    assert abs(float(loss) + 1.0) <= 2 * 2.0 ** -23 and float((sec["s"] - 1).abs().max()) <= 1e-6
    assert torch.allclose(sec["norm_f"], feats.square().sum(1).sqrt(), rtol=1e-6, atol=0) and torch.allclose(sec["norm_y"], sec["norm_f"], rtol=1e-5, atol=0)


@pytest.mark.gpu
def test_zero_vectors(dev):
    """One position's feats are zero; at another code and the bias are zero, so y = 0 exactly: s = 0 at both and the second hands d code
    the partner's unit vector over eps - about 1e10 / N, finite - as in the reference.  The elements those two positions reach and the
    rest are held against the restatement separately, each within the yardstick's margin (a figure floored at 2^-23)."""
    code, feats, weight, bias = (t.clone() for t in R.operands("ragged", "random"))
    B, D, C, (h, w) = R.SHAPES["ragged"]
    bias.zero_()
    code[0, :, 1, 2] = 0                                                      # y = 0
    feats[1, :, 3, 4] = 0                                                     # f = 0
    t = R.chain(code, feats, weight, bias)
    assert float(t["s"][0, 1, 2]) == 0.0 and float(t["s"][1, 3, 4]) == 0.0 and float(t["norm_y"][0, 1, 2]) == 0.0
    assert float(t["d_code"][0, :, 1, 2].abs().max()) > 1e7
    got, yard = kernel(code, feats, weight, bias, dev), yardstick(code, feats, weight, bias, dev)
    assert got[0] == got[0] and all(bool(torch.isfinite(g).all()) for g in got[1:])
    m_code = torch.zeros(B, D, h, w, dtype=torch.bool)
    m_code[0, :, 1, 2] = True
    m_code[1, :, 3, 4] = True

    def parts(res):
        rel = lambda g, want, m: max(float((g[m] - want[m]).norm() / want[m].norm()), 2.0 ** -23)
        out = {"loss": max(abs(res[0] - t["loss"]), R.spacing32(t["loss"])) / t["mean_abs_s"],
               "d_code/zero": rel(res[1], t["d_code"], m_code), "d_code/rest": rel(res[1], t["d_code"], ~m_code)}
        # (d W and d b sum over every position: the two reach all of their elements)
        for name, g in zip(GRADS[1:], res[2:]):
            out[name] = rel(g, t[name], torch.ones_like(g, dtype=torch.bool))
        return out

    k, y = parts(got), parts(yard)
    print("zero vectors: kernel", {a: f"{v:.3e}" for a, v in k.items()}, "yardstick", {a: f"{v:.3e}" for a, v in y.items()})
    for name in k:
        assert k[name] <= MARGIN * y[name], (name, k, y)


def _nan_outs(shape, dev):
    B, D, C, (h, w) = R.SHAPES[shape]
    return tuple(torch.full(sh, float("nan"), device=dev) for sh in ((B, D, h, w), (C, D), (C,)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", [("head", "random"), ("ragged", "dropped"), ("many", "random")])
def test_two_calls_give_the_same_bits_and_the_gradients_are_written_completely(shape, kind, dev):
    from depthg_amd import ops
    args = tuple(t.to(dev) for t in R.operands(shape, kind))
    runs = []
    for _ in range(2):
        loss, ws = ops.rec_loss_forward(*args)
        out = _nan_outs(shape, dev)
        ops.rec_loss_backward(ws, *args, torch.tensor(0.75, device=dev), out=out)
        runs.append((loss.clone(),) + out)
    assert not any(bool(torch.isnan(g).any()) for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # the upstream gradient is a factor
    once = ops.rec_loss_backward(ws, *args, torch.tensor(1.0, device=dev))
    for got, want in zip(runs[1][1:], once):
        assert float((got - want * 0.75).norm() / want.norm()) <= 1e-6        # (two float32 roundings apart, element by element)


@pytest.mark.gpu
def test_poisoned_buffers_change_nothing(dev, monkeypatch):
    """ops.POISON (DG_POISON=1): workspace and outputs start as 0xFF bytes - a kernel reading what none has written would show NaN."""
    from depthg_amd import ops
    for shape, kind in (("ragged", "scaled"), ("many", "dropped")):
        args = R.operands(shape, kind)
        monkeypatch.setattr(ops, "POISON", False)
        want = kernel(*args, dev)
        monkeypatch.setattr(ops, "POISON", True)
        got = kernel(*args, dev)
        assert want[0] == got[0] and all(torch.equal(a, b) for a, b in zip(want[1:], got[1:]))


def _grads(fn, code, feats, weight, bias):
    c, w, b = (t.detach().requires_grad_(True) for t in (code, weight, bias))
    loss = fn(c, feats, w, b)
    loss.backward()
    return loss.detach(), c.grad, w.grad.reshape(w.shape[0], w.shape[1]), b.grad


@pytest.mark.gpu
def test_views_are_read_as_the_tensors_they_are(dev):
    """Offset and permuted views of larger buffers give the bits of their contiguous copies."""
    from depthg_amd import reconstruction_loss
    code, feats, weight, bias = (t.to(dev) for t in R.operands("ragged", "random"))
    B, D, C, (h, w) = R.SHAPES["ragged"]
    big = torch.randn(B, D + 3, h, w, device=dev)
    big[:, 2:D + 2] = code
    v_code = big[:, 2:D + 2]                                                  # an offset channel slice
    v_feats = feats.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)      # transposed storage
    v_weight = torch.cat([weight[:, :, 0, 0], weight[:, :, 0, 0]], 1)[:, D:]  # a (C, D) view with a row stride of 2 D
    assert not v_code.is_contiguous() and not v_feats.is_contiguous() and not v_weight.is_contiguous()
    want, got = _grads(reconstruction_loss, code, feats, weight, bias), _grads(reconstruction_loss, v_code, v_feats, v_weight, bias)
    assert all(torch.equal(x, y) for x, y in zip(want, got))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["ragged", "head", "many"])
def test_deferred_dropout_gives_the_bits_of_the_materialised_features(shape, dev):
    from depthg_amd import ops, reconstruction_loss
    i = R.inputs(shape, "dropped")
    code, weight, bias, raw, keep = (i[k].to(dev) for k in ("code", "weight", "bias", "raw", "keep"))
    deferred = ops.DeferredDropout(raw, keep, i["scale"])
    feats = deferred.materialize()
    assert torch.equal(feats.cpu(), i["feats"]) and bool((keep == 0).any()) and bool((keep == 1).any())
    want, got = _grads(reconstruction_loss, code, feats, weight, bias), _grads(reconstruction_loss, code, deferred, weight, bias)
    assert all(torch.equal(x, y) for x, y in zip(want, got))
    # the same through ops, flags and scale as arguments
    l0, ws0 = ops.rec_loss_forward(code, feats, weight, bias)
    l1, ws1 = ops.rec_loss_forward(code, raw, weight, bias, keep=keep, scale=i["scale"])
    g = torch.tensor(1.0, device=dev)
    b0, b1 = ops.rec_loss_backward(ws0, code, feats, weight, bias, g), ops.rec_loss_backward(ws1, code, raw, weight, bias, g, keep=keep, scale=i["scale"])
    assert torch.equal(l0, l1) and all(torch.equal(x, y) for x, y in zip(b0, b1))


@pytest.mark.gpu
def test_gpu_refusals(dev):
    from depthg_amd import reconstruction_loss
    code, feats, weight, bias = (t.to(dev) for t in R.operands("tiny", "random"))
    for bad in ((code.double(), feats, weight, bias), (code, feats.half(), weight, bias), (code, feats, weight.double(), bias),
                (code, feats, weight, bias.half())):
        with pytest.raises(ValueError, match="float32"):
            reconstruction_loss(*bad)
    for bad in ((code, feats.cpu(), weight, bias), (code.cpu(), feats, weight, bias), (code, feats, weight.cpu(), bias)):
        with pytest.raises(RuntimeError, match="GPU"):
            reconstruction_loss(*bad)
    with pytest.raises(RuntimeError, match="feats"):
        reconstruction_loss(code, feats.clone().requires_grad_(True), weight, bias)
    with pytest.raises(ValueError, match="128"):
        reconstruction_loss(torch.zeros(1, 129, 2, 2, device=dev), torch.zeros(1, 4, 2, 2, device=dev), torch.zeros(4, 129, device=dev),
                            torch.zeros(4, device=dev))
    with torch.no_grad():                                                     # only the forward runs
        out = reconstruction_loss(code.clone().requires_grad_(True), feats, weight, bias)
    assert not out.requires_grad and out.dim() == 0


def _batch(dev, seed=0, hw=32, n_classes=5, B=2):
    g = torch.Generator().manual_seed(seed)
    return {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
            "label": torch.randint(-1, n_classes, (B, hw, hw), generator=g).to(dev),
            "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
            "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}


def _step(dev, monkeypatch, weight, hw=32, **over):
    """One seeded training_step; returns (model, loss, logs, what reconstruction_loss saw and returned, the decoder's initial weight)."""
    from depthg_amd import ops, rec_loss, segmenter
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    m = UnsupervisedSegmenter(5, default_segmenter_cfg(res=hw, rec_weight=weight, **{"correspondence_weight": 0.0, **over})).to(dev)
    m.train()
    seen = []

    def spy(code, feats, w, b):
        out = rec_loss.reconstruction_loss(code, feats, w, b)
        maps = feats.materialize() if isinstance(feats, ops.DeferredDropout) else feats
        seen.append((code.detach().clone(), maps.detach().clone(), w.detach().clone(), b.detach().clone(), out.detach().clone(),
                     isinstance(feats, ops.DeferredDropout)))
        return out

    monkeypatch.setattr(segmenter, "reconstruction_loss", spy)
    before = m.decoder.weight.detach().clone() if weight > 0 else None
    grads = {}
    if weight > 0:                           # (the step may clear p.grad: keep what backward hands each parameter)
        for name, p in [("decoder.weight", m.decoder.weight), ("decoder.bias", m.decoder.bias)] + [(f"head{k}", p) for k, p in enumerate(m.head_parameters())]:
            p.register_hook(lambda g, name=name: grads.__setitem__(name, g.detach().clone()))
    torch.manual_seed(9)
    loss, logs = m.training_step(_batch(dev, hw=hw), 0)
    torch.cuda.synchronize()
    return m, loss, logs, seen, before, grads


@pytest.mark.gpu
def test_training_step_with_and_without_the_weight(dev, monkeypatch):
    m0, loss0, logs0, seen0, _, _ = _step(dev, monkeypatch, 0.0)
    assert "loss/rec" not in logs0 and not seen0 and not hasattr(m0, "decoder")           # no launch, no log key, no decoder
    weight = 0.5
    m1, loss1, logs1, seen1, before, grads = _step(dev, monkeypatch, weight)
    assert len(seen1) == 1
    code, feats, w, b, out, deferred = seen1[0]
    assert code.shape == (2, 70, 4, 4) and feats.shape == (2, 384, 4, 4) and not deferred
    assert torch.equal(logs1["loss/rec"], out) and torch.equal(w, before)
    t = R.chain(code.cpu(), feats.cpu(), w.cpu(), b.cpu())
    assert abs(float(out) - t["loss"]) <= 1e-5 * t["mean_abs_s"] and float(out) != 0.0
    # the featurizer pass, the probes and their losses are those of the weight-0 step: the total grows by weight x the term
    assert torch.equal(logs1["loss/linear"], logs0["loss/linear"]) and torch.equal(logs1["loss/cluster"], logs0["loss/cluster"])
    want = float(logs0["loss/total"]) + weight * float(out)
    assert abs(float(logs1["loss/total"]) - want) <= 4e-7 * (abs(float(logs0["loss/total"])) + abs(float(out)))
    assert torch.equal(loss1, logs1["loss/total"])
    # the term's gradient reaches the decoder and the head, and the decoder is stepped
    assert len(grads) == 2 + len(m1.head_parameters())
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())
    assert not torch.equal(m1.decoder.weight.detach(), before)
    rel = lambda g, want: float((g.double().cpu() - want).norm() / want.norm())
    assert rel(grads["decoder.weight"].reshape(384, 70), weight * t["d_weight"]) <= 1e-5 and rel(grads["decoder.bias"], weight * t["d_bias"]) <= 1e-5


@pytest.mark.gpu
def test_training_step_feeds_the_term_deferred_dropout_from_the_paired_pass(dev, monkeypatch):
    """correspondence_weight = 1 on the identity grid (feature_samples = the map's side, dg_dense_grid): the paired featurizer pass hands
    the step its feats as ops.DeferredDropout, and the step hands them on as they are."""
    m, loss, logs, seen, before, grads = _step(dev, monkeypatch, 0.5, hw=112, correspondence_weight=1.0, feature_samples=14,
                                               depth_sampling="none", dg_dense_grid=True, dg_outputs="reduced", fps_sample_decay=False)
    assert len(seen) == 1
    code, feats, w, b, out, deferred = seen[0]
    assert deferred                                                           # the paired pass left the Dropout2d to the kernels
    assert bool((feats.flatten(2).abs().sum(2) == 0).any())                   # dropped channels in the materialised maps
    t = R.chain(code.cpu(), feats.cpu(), w.cpu(), b.cpu())
    assert torch.equal(logs["loss/rec"], out) and abs(float(out) - t["loss"]) <= 1e-5 * t["mean_abs_s"]
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values()) and len(grads) == 2 + len(m.head_parameters())
    assert not torch.equal(m.decoder.weight.detach(), before) and bool(torch.isfinite(loss))


@pytest.mark.gpu
def test_training_step_with_the_fused_optimiser_steps_eleven_tensors(dev, monkeypatch):
    m, loss, logs, seen, before, grads = _step(dev, monkeypatch, 0.5, dg_fused_adam=True)
    assert len(m._fused_set().parameters()) == 11 and len(m.all_reduced_parameters()) == 11
    assert len(seen) == 1 and "loss/rec" in logs and bool(torch.isfinite(loss))
    assert not torch.equal(m.decoder.weight.detach(), before) and bool(torch.isfinite(m.decoder.weight).all())
