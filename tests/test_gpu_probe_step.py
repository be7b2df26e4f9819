"""The fused probe step on the GPU (dg_probe_step.hip through head.fused_probe_losses): both losses and the three parameter gradients
against the float64 restatement (tests/probe_step_reference.py) with the same chain in float32 torch on the GPU as the yardstick,
determinism, poisoned buffers, the complete write of the gradients, and the refusals.

MARGIN: the kernels' errors may be at most MARGIN x the yardstick's - 2, the bound of the auxiliary loss terms' tests (the cross
entropy's and the cluster probe's gradients are linear reductions of the same kind).  The inputs are margin inputs: no float32 route can
pick another centre at any position."""
import ctypes

import pytest
import torch

import probe_step_reference as R

MARGIN = 2.0
NAMES = ("linear_loss", "cluster_loss") + R.GRADS


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def measure(shape, upstream, dev):
    """{name: (kernel's figure, yardstick's figure)} of one case against the float64 restatement."""
    from depthg_amd.head import fused_probe_losses
    ops, t = R.operands(shape), R.truth(shape, upstream)
    k, y = R.figures(R.run(fused_probe_losses, ops, upstream, dev), t), R.figures(R.run(R.torch_chain, ops, upstream, dev), t)
    return {n: (k[n], y[n]) for n in NAMES}


@pytest.mark.gpu
@pytest.mark.parametrize("upstream", R.UPSTREAM)
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_losses_and_gradients_within_the_yardsticks_margin(shape, upstream, dev):
    m = measure(shape, upstream, dev)
    print(f"{shape} upstream {upstream}: " + " | ".join(f"{n} kernel {k:.3e} yardstick {y:.3e} ratio {k / y:.2f}" for n, (k, y) in m.items()))
    for n, (k, y) in m.items():
        assert k <= MARGIN * y, (n, m)


def _direct(shape, dev, poison_grads=True):
    """One forward and one backward through the C entries themselves -> (out3, d W, d b, d clusters, workspace)."""
    from depthg_amd import _lib
    from depthg_amd.ops import _ptr, _stream
    lib = _lib.load()
    code, label, weight, bias, clusters = (t.to(dev).contiguous() for t in R.operands(shape))
    B, D, n, m, (h, w), (H, W) = R.SHAPES[shape]
    dims = (B, D, n, m, h, w, H, W)
    nb = lib.dg_probe_step_workspace_bytes(*dims)
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
    out3 = torch.full((3,), float("nan"), device=dev)
    _lib.check(lib.dg_probe_step_forward(_ptr(code), _ptr(label), _ptr(weight), _ptr(bias), _ptr(clusters), *dims, _ptr(out3), _ptr(ws), nb,
                                         _stream(dev)), "dg_probe_step_forward")
    gw, gb, gc = (torch.full(s, float("nan"), device=dev) for s in ((n, D), (n,), (m, D)))
    g1, g2 = torch.tensor([0.7], device=dev), torch.tensor([-1.3], device=dev)
    _lib.check(lib.dg_probe_step_backward(_ptr(ws), nb, _ptr(g1), _ptr(g2), *dims, _ptr(gw), _ptr(gb), _ptr(gc), _stream(dev)),
               "dg_probe_step_backward")
    return out3, gw, gb, gc, ws


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_two_calls_give_the_same_bits_and_every_element_is_written(shape, dev):
    """The workspace is pre-filled with 0xFF bytes and the outputs with NaN: a byte read before it is written, or an element left
    unwritten, shows as NaN; the second call's results are the first's, bit for bit."""
    a, b = _direct(shape, dev), _direct(shape, dev)
    B, D, n, m, hw, HW = R.SHAPES[shape]
    for x in a[:4]:
        assert not bool(torch.isnan(x).any())
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    t = R.truth(shape, (0.7, -1.3))
    assert int(a[0][2]) == t["count"]
    assert float((a[1].double().cpu() - t["d_weight"]).norm() / t["d_weight"].norm()) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["tiny", "ragged", "ratios"])
def test_under_poisoned_buffers(shape, dev, monkeypatch):
    """DG_POISON=1's hook: every buffer the Python layer hands to the library is pre-filled with 0xFF bytes."""
    from depthg_amd import ops
    from depthg_amd.head import fused_probe_losses
    monkeypatch.setattr(ops, "POISON", True)
    import depthg_amd.head as head
    assert head._empty is ops._empty
    got, t = R.run(fused_probe_losses, R.operands(shape), (0.7, -1.3), dev), R.truth(shape, (0.7, -1.3))
    f = R.figures(got, t)
    assert all(v == v and v < 1e-4 for v in f.values()), f


@pytest.mark.gpu
def test_no_labelled_pixel_gives_what_probe_cross_entropy_gives(dev):
    from depthg_amd.head import fused_probe_losses, probe_cross_entropy
    code, label, weight, bias, clusters = (t.to(dev) for t in R.operands("tiny"))
    none = torch.full_like(label, -1)
    lin, clu = fused_probe_losses(code, none, weight, bias, clusters)
    old = probe_cross_entropy(torch.nn.functional.conv2d(code, weight, bias), none)
    assert torch.equal(torch.isnan(lin), torch.isnan(old)) and bool(torch.isfinite(clu))
    assert float(clu) == pytest.approx(R.truth("tiny")["cluster_loss"], rel=1e-5)


@pytest.mark.gpu
def test_unsupported_shapes_return_the_error_and_launch_nothing(dev):
    from depthg_amd import _lib
    from depthg_amd.ops import _ptr, _stream
    lib = _lib.load()
    out3 = torch.full((3,), float("nan"), device=dev)
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device=dev)
    x = torch.zeros(1 << 16, device=dev)
    lab = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    for dims, why in (((1, 129, 3, 3, 2, 2, 4, 4), "D <= 128"), ((1, 8, 65, 3, 2, 2, 4, 4), "n_lin <= 64"), ((1, 8, 3, 65, 2, 2, 4, 4), "n_clu <= 64"),
                      ((1, 8, 64, 3, 1, 65, 4, 4), "n_lin * w <= 4096")):
        rc = lib.dg_probe_step_forward(_ptr(x), _ptr(lab), _ptr(x), _ptr(x), _ptr(x), *dims, _ptr(out3), _ptr(ws), ws.numel(), _stream(dev))
        assert rc == -2 and why in lib.dg_last_error().decode(), (dims, rc)
        rc = lib.dg_probe_step_backward(_ptr(ws), ws.numel(), _ptr(x), _ptr(x), *dims, _ptr(out3), _ptr(out3), _ptr(out3), _stream(dev))
        assert rc == -2
    # a workspace that is too small is refused as well
    rc = lib.dg_probe_step_forward(_ptr(x), _ptr(lab), _ptr(x), _ptr(x), _ptr(x), 2, 8, 3, 5, 4, 4, 8, 8, _ptr(out3), _ptr(ws), 64, _stream(dev))
    assert rc == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(out3).all()) and int(ws.min()) == 255
    from depthg_amd.head import fused_probe_losses
    with pytest.raises(RuntimeError, match="n_lin \\* w <= 4096"):
        fused_probe_losses(torch.zeros(1, 8, 1, 65, device=dev), lab[:16].reshape(1, 4, 4), torch.zeros(64, 8, 1, 1, device=dev),
                           torch.zeros(64, device=dev), torch.zeros(3, 8, device=dev))
    with pytest.raises(RuntimeError, match="requires grad"):
        fused_probe_losses(torch.zeros(1, 8, 2, 2, device=dev, requires_grad=True), lab[:16].reshape(1, 4, 4),
                           torch.zeros(3, 8, 1, 1, device=dev), torch.zeros(3, device=dev), torch.zeros(3, 8, device=dev))
