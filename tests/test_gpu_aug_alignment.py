"""The augmentation-alignment term on the GPU (dg_aug.hip through ops.aug_alignment_forward / aug_alignment_backward and
aug_loss.aug_alignment_loss): loss and both gradients against the float64 restatement (tests/aug_alignment_reference.py) with the same
chain in float32 torch on the GPU as the yardstick, zero vectors, determinism, the complete write of both gradients, views as inputs,
and cfg.aug_alignment_weight in training_step.

MARGIN: the kernels' errors may be at most MARGIN x the yardstick's - 2, what tests/adam_reference.py and the CRF-loss tests hold.  A
loss error is floored at one float32 spacing of the loss's magnitude (neither route can return a better scalar than the format holds).
scripts/aug_alignment_parity.py runs measure() over R.CASES and writes the ratios to profiles/aug_alignment_parity.md.
"""
import pytest
import torch

import aug_alignment_reference as R

MARGIN = 2.0
B = R.B


def _run(fn, code, code_aug, coord, dev):
    a, b = code.to(dev).requires_grad_(True), code_aug.to(dev).requires_grad_(True)
    loss = fn(a, b, coord.to(dev))
    loss.backward()
    return float(loss.detach().double()), a.grad.double().cpu(), b.grad.double().cpu()


def kernel(code, code_aug, coord, dev):
    from depthg_amd import aug_alignment_loss
    return _run(aug_alignment_loss, code, code_aug, coord, dev)


def yardstick(code, code_aug, coord, dev):
    """resize + sample + the two norms + einsum + mean + autograd in float32 torch on the GPU."""
    return _run(R.torch_chain, code, code_aug, coord, dev)


def figures(got, t):
    """(loss error over the mean |s|, floored at one float32 spacing of the loss; relative L2 of d code; of d code_aug)."""
    loss, d_code, d_code_aug = got
    rel = lambda g, want: float((g - want).norm() / want.norm())
    return (max(abs(loss - t["loss"]), R.spacing32(t["loss"])) / t["mean_abs_s"], rel(d_code, t["d_code"]), rel(d_code_aug, t["d_code_aug"]))


def measure(shape, kind, dev):
    """The figures of one case, of the kernels and of the yardstick, against the float64 restatement."""
    code, code_aug, coord = R.inputs(shape, kind)
    t = R.truth(shape, kind)
    k_loss, k_code, k_aug = figures(kernel(code, code_aug, coord, dev), t)
    y_loss, y_code, y_aug = figures(yardstick(code, code_aug, coord, dev), t)
    return {"loss": t["loss"], "loss_err_kernel": k_loss, "loss_err_yard": y_loss, "d_code_err_kernel": k_code, "d_code_err_yard": y_code,
            "d_code_aug_err_kernel": k_aug, "d_code_aug_err_yard": y_aug}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", R.CASES + [R.WRAPS_CASE])
def test_loss_and_gradients_within_the_yardsticks_margin(shape, kind, dev):
    m = measure(shape, kind, dev)
    print(f"{shape}/{kind}: loss {m['loss']:.9e} | loss err kernel {m['loss_err_kernel']:.3e} yardstick {m['loss_err_yard']:.3e} | d code "
          f"rel-L2 kernel {m['d_code_err_kernel']:.3e} yardstick {m['d_code_err_yard']:.3e} | d code_aug rel-L2 kernel "
          f"{m['d_code_aug_err_kernel']:.3e} yardstick {m['d_code_aug_err_yard']:.3e}")
    assert m["loss_err_kernel"] <= MARGIN * m["loss_err_yard"], m
    assert m["d_code_err_kernel"] <= MARGIN * m["d_code_err_yard"], m
    assert m["d_code_aug_err_kernel"] <= MARGIN * m["d_code_aug_err_yard"], m


@pytest.mark.gpu
def test_identity_grid_with_equal_maps_gives_minus_one(dev):
    """code_aug = code on the untransformed grid: u == code, every s is 1 and the true gradient vanishes - the loss only."""
    from depthg_amd import aug_alignment_loss, ops
    code = R.inputs("upsample", "cropflip")[0].to(dev)                       # (2,33,6,6)
    coord = R.dataset_grid(B, 6, 6).to(dev)
    loss, ws = ops.aug_alignment_forward(code, code, coord)
    sec = ops.aug_alignment_workspace_sections(ws, B, 6)
    assert abs(float(loss) + 1.0) <= 2 * 2.0 ** -23
    assert float((sec["s"] - 1).abs().max()) <= 4e-7
    assert torch.equal(sec["ds"], coord)                                     # a coordinate resize that is the identity
    assert torch.allclose(sec["norm_u"], code.square().sum(1).sqrt(), rtol=1e-6, atol=0) and torch.allclose(sec["norm_u"], sec["norm_v"], rtol=1e-6, atol=0)
    assert abs(float(aug_alignment_loss(code, code, coord)) + 1.0) <= 2 * 2.0 ** -23


@pytest.mark.gpu
def test_zero_vectors(dev):
    """One code_aug position and the 2 x 2 patch of code under one sampled position are zero: s = 0 there and the gradients are the
    partner's unit vector over eps - about 1e10 / N, finite - as in the reference.  The elements those reach and the rest are held
    against the restatement separately, each within the yardstick's margin (a figure floored at one float32 spacing, 2^-23)."""
    code, code_aug, coord = (t.clone() for t in R.inputs("nonsquare", "cropflip"))
    D, (h, w), n, _ = R.SHAPES["nonsquare"]
    idx, _ = R.taps(R.downsample_coords(coord, n), h, w)
    pos, pos_v = 2 * n + 3, 4 * n + 1                                        # (i, j) = (2, 3) of u, (4, 1) of code_aug
    patch = torch.zeros(B, h * w, dtype=torch.bool)
    for b in range(B):
        patch[b, idx[b, pos]] = True
    code.flatten(2)[:] = code.flatten(2) * (~patch)[:, None]
    code_aug[:, :, 4, 1] = 0
    t = R.chain(code, code_aug, coord)
    assert not bool(t["u"].flatten(2)[:, :, pos].any()) and not bool(t["s"].flatten(1)[:, pos].any()) and not bool(t["s"].flatten(1)[:, pos_v].any())
    assert float(t["d_code"].flatten(2)[patch[:, None].expand(B, D, h * w)].abs().max()) > 1e7
    got, yard = kernel(code, code_aug, coord, dev), yardstick(code, code_aug, coord, dev)
    assert all(bool(torch.isfinite(g).all()) for g in got[1:]) and got[0] == got[0]
    m_code = patch[:, None].expand(B, D, h * w)
    m_aug = torch.zeros(B, D, n * n, dtype=torch.bool)
    m_aug[:, :, pos_v] = True

    def parts(res):
        loss, d_code, d_code_aug = res
        rel = lambda g, want, m: max(float((g[m] - want[m]).norm() / want[m].norm()), 2.0 ** -23)
        out = {"loss": max(abs(loss - t["loss"]), R.spacing32(t["loss"])) / t["mean_abs_s"]}
        for name, g, want, m in (("d_code", d_code.flatten(2), t["d_code"].flatten(2), m_code),
                                 ("d_code_aug", d_code_aug.flatten(2), t["d_code_aug"].flatten(2), m_aug)):
            out[name + "/zero"], out[name + "/rest"] = rel(g, want, m), rel(g, want, ~m)
        return out

    k, y = parts(got), parts(yard)
    print("zero vectors: kernel", {a: f"{v:.3e}" for a, v in k.items()}, "yardstick", {a: f"{v:.3e}" for a, v in y.items()})
    for name in k:
        assert k[name] <= MARGIN * y[name], (name, k, y)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", [("reference", "cropflip"), ("nonsquare", "equal"), ("upsample", "cropflip")])
def test_two_calls_give_the_same_bits_and_both_gradients_are_written_completely(shape, kind, dev):
    from depthg_amd import ops
    code, code_aug, coord = (t.to(dev) for t in R.inputs(shape, kind))
    runs = []
    for _ in range(2):
        loss, ws = ops.aug_alignment_forward(code, code_aug, coord)
        out = (torch.full_like(code, float("nan")), torch.full_like(code_aug, float("nan")))
        ops.aug_alignment_backward(ws, code, code_aug, torch.tensor(0.75, device=dev), out=out)
        runs.append((loss.clone(), out[0], out[1]))
    assert not bool(torch.isnan(runs[0][1]).any()) and not bool(torch.isnan(runs[0][2]).any())
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # the upstream gradient is a factor
    once = ops.aug_alignment_backward(ws, code, code_aug, torch.tensor(1.0, device=dev))
    for got, want in ((runs[1][1], once[0] * 0.75), (runs[1][2], once[1] * 0.75)):
        assert float((got - want).norm() / want.norm()) <= 1e-6             # (two float32 roundings apart, element by element)


@pytest.mark.gpu
def test_poisoned_buffers_change_nothing(dev, monkeypatch):
    """ops.POISON (DG_POISON=1): workspace and outputs start as 0xFF bytes - a kernel reading what none has written would show NaN."""
    from depthg_amd import aug_alignment_loss, ops
    code, code_aug, coord = R.inputs("nonsquare", "scaled")
    want = kernel(code, code_aug, coord, dev)
    monkeypatch.setattr(ops, "POISON", True)
    got = kernel(code, code_aug, coord, dev)
    assert want[0] == got[0] and torch.equal(want[1], got[1]) and torch.equal(want[2], got[2])


@pytest.mark.gpu
def test_views_are_read_as_the_tensors_they_are(dev):
    """Offset and permuted views of larger buffers give the bits of their contiguous copies."""
    from depthg_amd import aug_alignment_loss
    code, code_aug, coord = (t.to(dev) for t in R.inputs("nonsquare", "cropflip"))
    D = code.shape[1]
    big = torch.randn(B, D + 3, 7, 9 + 2, device=dev)
    big[:, 2:D + 2, :, 1:10] = code
    v_code = big[:, 2:D + 2, :, 1:10]                                        # offset, strided
    v_aug = code_aug.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)    # transposed storage
    v_coord = torch.cat([coord, coord], 3)[..., 2:]                          # offset last axis
    assert not v_code.is_contiguous() and not v_aug.is_contiguous() and not v_coord.is_contiguous()

    def run(a, b, c):
        a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        loss = aug_alignment_loss(a, b, c)
        loss.backward()
        return loss.detach(), a.grad, b.grad

    want, got = run(code, code_aug, coord), run(v_code, v_aug, v_coord)
    assert all(torch.equal(x, y) for x, y in zip(want, got))


@pytest.mark.gpu
def test_gpu_refusals(dev):
    from depthg_amd import aug_alignment_loss
    code, code_aug, coord = (t.to(dev) for t in R.inputs("tiny", "cropflip"))
    for bad in ((code.double(), code_aug, coord), (code, code_aug.half(), coord), (code, code_aug, coord.double())):
        with pytest.raises(ValueError, match="float32"):
            aug_alignment_loss(*bad)
    with pytest.raises(RuntimeError, match="GPU"):
        aug_alignment_loss(code, code_aug.cpu(), coord)
    with pytest.raises(RuntimeError, match="coord_aug"):
        aug_alignment_loss(code, code_aug, coord.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="LDS"):
        aug_alignment_loss(torch.zeros(1, 2, 150, 150, device=dev), torch.zeros(1, 2, 3, 3, device=dev), torch.zeros(1, 4, 4, 2, device=dev))


def _batch(dev, aug, seed=0, hw=32, n_classes=5):
    from depthg_amd import crop_flip_coords
    g = torch.Generator().manual_seed(seed)
    batch = {"img": torch.randn(B, 3, hw, hw, generator=g).to(dev), "img_pos": torch.randn(B, 3, hw, hw, generator=g).to(dev),
             "label": torch.randint(-1, n_classes, (B, hw, hw), generator=g).to(dev),
             "depth": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev),
             "depth_pos": torch.randint(1, 256, (B, 1, hw, hw), generator=g).float().to(dev)}
    if aug:
        batch["img_aug"] = torch.randn(B, 3, hw, hw, generator=g).to(dev)
        batch["coord_aug"] = crop_flip_coords(B, hw, hw, [(2.0, 1.0, 29.0, 30.0), (0.0, 3.0, 30.5, 28.0)], [False, True]).to(dev)
    return batch


def _step(dev, monkeypatch, weight, aug_keys):
    """One seeded training_step; returns (logs, head gradients, featurizer passes, what aug_alignment_loss saw and returned)."""
    from depthg_amd import aug_loss, segmenter
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(4)
    m = UnsupervisedSegmenter(5, default_segmenter_cfg(res=32, correspondence_weight=0.0, aug_alignment_weight=weight)).to(dev)
    m.train()
    passes, seen = [], []
    m.net.register_forward_hook(lambda mod, args, out: passes.append(1))

    def spy(code, code_aug, coord_aug):
        out = aug_loss.aug_alignment_loss(code, code_aug, coord_aug)
        seen.append((code.detach().clone(), code_aug.detach().clone(), coord_aug, out.detach().clone()))
        return out

    monkeypatch.setattr(segmenter, "aug_alignment_loss", spy)
    torch.manual_seed(9)
    loss, logs = m.training_step(_batch(dev, aug_keys), 0)
    torch.cuda.synchronize()
    grads = [None if p.grad is None else p.grad.detach().clone() for p in m.head_parameters()]
    return loss, logs, grads, len(passes), seen, torch.cat([torch.get_rng_state(), torch.cuda.get_rng_state(dev)])


@pytest.mark.gpu
def test_training_step_with_and_without_the_weight(dev, monkeypatch):
    from depthg_amd import aug_alignment_loss
    loss0, logs0, grads0, passes0, seen0, rng0 = _step(dev, monkeypatch, 0.0, False)
    assert "loss/aug_alignment" not in logs0 and passes0 == 1 and not seen0              # no third pass, no launch, no log key
    loss0k, logs0k, _, passes0k, seen0k, rng0k = _step(dev, monkeypatch, 0.0, True)     # the keys are there and nobody reads them
    assert torch.equal(loss0, loss0k) and set(logs0) == set(logs0k) and passes0k == 1 and not seen0k and torch.equal(rng0, rng0k)
    assert all(torch.equal(logs0[k], logs0k[k]) for k in logs0)

    weight = 0.5
    loss1, logs1, grads1, passes1, seen1, rng1 = _step(dev, monkeypatch, weight, True)
    assert passes1 == 2 and len(seen1) == 1 and not torch.equal(rng0, rng1)              # the extra pass drew its own dropout masks
    code, code_aug, coord, out = seen1[0]
    assert code_aug.shape == code.shape == (B, 70, 4, 4)
    assert torch.equal(logs1["loss/aug_alignment"], out) and torch.equal(aug_alignment_loss(code, code_aug, coord), out)
    t = R.chain(code.cpu(), code_aug.cpu(), coord.cpu())
    assert abs(float(out) - t["loss"]) <= 1e-5 * t["mean_abs_s"] and float(out) != 0.0
    # the first pass, the probes and their losses are those of the weight-0 step: the total grows by weight x the term
    assert torch.equal(logs1["loss/linear"], logs0["loss/linear"]) and torch.equal(logs1["loss/cluster"], logs0["loss/cluster"])
    want = float(logs0["loss/total"]) + weight * float(out)
    assert abs(float(logs1["loss/total"]) - want) <= 4e-7 * (abs(float(logs0["loss/total"])) + abs(float(out)))
    assert torch.equal(loss1, logs1["loss/total"])
    # the term's gradient reaches the head
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads1)
    assert any(g0 is None or not torch.equal(g0, g1) for g0, g1 in zip(grads0, grads1)) and any(bool(g.any()) for g in grads1)
