"""The cd histograms on the GPU (k_cd_hist / k_cd_hist_rows behind dg_corr_cd_hist): exact counts, the edge-mass bound against the
reference's own cd tensors, both output modes, untouched gradients, the segmenter's hist_freq switch and the refusals.

The truth is never the library's materialised output: it is the cd tensors a reference fixture stores in full, otherwise
oracle.depthg_oracle on the fixture's inputs.  Bound (tests/cd_hist_reference.py): with C(e) the number of elements below interior
edge e, |C_ours(e) - C_ref(e)| <= #{reference elements within delta of e}; delta is the per-element tolerance the materialised
tensors are held to on the same route - 1e-3 on the blob routes (fp16 code operands), 2e-5 on the rows route (fp32 rows).

Measured on an MI355X (profiles/cd_hist_parity.md): see that file for the largest edge difference and the bound's slack per case.
"""
import functools

import numpy as np
import pytest
import torch

import cd_hist_reference as R
from conftest import cfg_from_fixture, load_golden, load_golden_seeded

pytestmark = pytest.mark.gpu

# fixture -> (seeded inputs, identity grid, delta, what it reaches)
CASES = {
    "c1_none": (False, False, 2e-5, "rows route, P = 121 (not a multiple of 32)"),
    "batch1": (False, False, 2e-5, "rows route, B = 1"),
    "nodepthloss": (False, False, 2e-5, "rows route, 6-tuple"),
    "simple": (False, False, 2e-5, "rows route, DG_LINE_GRID (P = S = 9)"),
    "S14_dim100": (False, False, 1e-3, "general blobs, P = 196 padded to 224, D = 100"),
    "hl28_ident": (True, True, 1e-3, "dense identity grid, k_corr2 with FOLD (stash in place)"),
    "wide1024_ident": (True, True, 1e-3, "channel chunks, shared coordinates with perms"),
}
BINNINGS = [(64, -1.0, 1.0), (7, -0.5, 0.9)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked tests need an MI355X; there is no fallback path")
    return torch.device("cuda:0")


def _forward(fx, ident, dev, mode):
    from depthg_amd import ContrastiveCorrelationLoss
    cfg = cfg_from_fixture(fx, dg_outputs=mode)
    T = lambda a: torch.from_numpy(a).to(dev)
    loss = ContrastiveCorrelationLoss(cfg)
    code, code_pos = T(fx["code"]).requires_grad_(True), T(fx["code_pos"]).requires_grad_(True)       # a gradient forward
    loss.forward_with(T(fx["feats"]), T(fx["feats_pos"]), code, code_pos, T(fx["depth"]), T(fx["coords1"]), T(fx["coords2"]),
                      T(fx["perms"]), shared_coords=ident, identity_grid=ident)
    return loss, code, code_pos


def _reference_cd(fx):
    """{"intra_cd", "inter_cd", "neg_cd"} -> the reference's un-reduced tensors: the fixture's where it stores them in full, else the
    oracle on the fixture's inputs."""
    if bool(fx["store_full"]):
        return {"intra_cd": fx["pos_intra_cd"], "inter_cd": fx["pos_inter_cd"], "neg_cd": fx["neg_inter_cd"]}
    from oracle import depthg_oracle as O
    T = torch.from_numpy
    with torch.no_grad():
        out = O.forward(cfg_from_fixture(fx), T(fx["feats"]), T(fx["feats_pos"]), T(fx["code"]), T(fx["code_pos"]), T(fx["depth"]),
                        T(fx["depth_pos"]), coords1=T(fx["coords1"]), coords2=T(fx["coords2"]), perms=list(T(fx["perms"])))
    sub = int(fx["sub"])          # the oracle run is the one the fixture sampled: pinned by its stored elements
    assert np.abs(out[1].reshape(-1)[::sub].numpy() - fx["pos_intra_cd"]).max() < 1e-5
    return {"intra_cd": out[1].numpy(), "inter_cd": out[3].numpy(), "neg_cd": out[5].numpy()}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the tests of one fixture share, computed once: a gradient forward in `reduced` mode with the histograms of both
    binnings (the first twice) in front of its backward, the same forward + backward without histograms, a `full` forward with
    histograms, and the reference's cd tensors."""
    seeded, ident, delta, _ = CASES[name]
    dev = torch.device("cuda:0")
    fx = (load_golden_seeded if seeded else load_golden)(f"forward_{name}.npz")
    run = {"fx": fx, "delta": delta, "ref": _reference_cd(fx)}
    loss, code, code_pos = _forward(fx, ident, dev, "reduced")
    run["hists"] = {b: loss.cd_histograms(bins=b[0], range=b[1:]) for b in BINNINGS}
    run["again"] = loss.cd_histograms(bins=BINNINGS[0][0], range=BINNINGS[0][1:])
    loss.total.backward()
    run["grads_after_hist"] = (code.grad.clone(), code_pos.grad.clone())
    loss2, code2, code_pos2 = _forward(fx, ident, dev, "reduced")
    loss2.total.backward()
    run["grads_plain"] = (code2.grad.clone(), code_pos2.grad.clone())
    loss3, _, _ = _forward(fx, ident, dev, "full")
    run["hists_full"] = {b: loss3.cd_histograms(bins=b[0], range=b[1:]) for b in BINNINGS}
    run["last_call"] = loss3.last_call
    torch.cuda.synchronize()
    return run


@pytest.mark.parametrize("binning", BINNINGS, ids=["64bins", "7bins_clamped"])
@pytest.mark.parametrize("name", list(CASES))
def test_counts_are_exact_and_reproducible(name, binning, dev):
    run = _case(name)
    fx = run["fx"]
    B, N = int(fx["code"].shape[0]), int(fx["neg_samples"])
    P = int(np.prod(fx["coords1"].shape[1:3]))
    h = run["hists"][binning]
    assert set(h) == {"intra_cd", "inter_cd", "neg_cd"}
    for key, numel in (("intra_cd", B * P * P), ("inter_cd", B * P * P), ("neg_cd", N * B * P * P)):
        t = h[key]
        assert t.dtype == torch.int64 and t.is_cuda and tuple(t.shape) == (binning[0],)
        assert int(t.min()) >= 0 and int(t.sum()) == numel, (key, int(t.sum()), numel)
        assert numel == run["ref"][key].size
    if binning == BINNINGS[0]:
        for key in h:
            assert torch.equal(h[key], run["again"][key]), key


@pytest.mark.parametrize("binning", BINNINGS, ids=["64bins", "7bins_clamped"])
@pytest.mark.parametrize("name", list(CASES))
def test_counts_against_the_reference(name, binning, dev):
    run = _case(name)
    bins, lo, hi = binning
    for key, got in run["hists"][binning].items():
        ref = run["ref"][key]
        c_ours = R.below_edges(got.cpu().numpy())
        c_ref = R.below_edges(R.clamped_histc(ref, bins, lo, hi))
        mass = R.edge_mass(ref, bins, lo, hi, run["delta"])
        diff = np.abs(c_ours - c_ref)
        worst = int(diff.argmax())
        print(f"cd_hist_parity | {name} | {bins} on [{lo}, {hi}] | {key} | elements {ref.size} | largest edge difference {int(diff.max())} "
              f"(bound there {int(mass[worst])}) | smallest slack {int((mass - diff).min())} | edges with no reference mass {int((mass == 0).sum())}")
        assert (diff <= mass).all(), (name, key, binning, int(diff.max()), int((mass - diff).min()))


@pytest.mark.parametrize("name", list(CASES))
def test_modes_agree_and_gradients_are_untouched(name, dev):
    run = _case(name)
    for b in BINNINGS:
        for key in run["hists"][b]:
            assert torch.equal(run["hists"][b][key], run["hists_full"][b][key]), (b, key)
    for a, b in zip(run["grads_after_hist"], run["grads_plain"]):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(a, b)            # the call only reads the workspace


def test_stale_workspace_is_refused(dev):
    from depthg_amd import ops
    fx = load_golden("forward_batch1.npz")
    loss, _, _ = _forward(fx, False, dev, "reduced")
    loss.cd_histograms()
    desc, perms, ws = loss.last_call
    T = lambda a: torch.from_numpy(a).to(dev)
    ops.corr_forward(desc, T(fx["feats"]), T(fx["feats_pos"]), T(fx["code"]), T(fx["code_pos"]), T(fx["depth"]), T(fx["coords1"]),
                     T(fx["coords2"]), perms, ws)          # the same workspace run on again
    with pytest.raises(RuntimeError, match="run on again"):
        loss.cd_histograms()


def test_refusals(dev):
    from depthg_amd import ops
    desc, perms, ws = _case("hl28_ident")["last_call"]
    T = 2 + int(desc.n_neg)
    ok = ops.corr_cd_hist(desc, ws, 1, T - 1, perms=perms, bins=5)          # a sub-range of the pair-sets
    one = ops.corr_cd_hist(desc, ws, 1, 1, bins=5)                          # inter alone: no batch maps needed
    assert tuple(ok.shape) == (T - 1, 5) and torch.equal(ok[0], one[0])
    for kw, text in ((dict(first=-1, count=1), "first=-1"), (dict(first=0, count=T + 1), "outside"), (dict(first=T, count=1), "outside"),
                     (dict(first=0, count=2, bins=0), "nbins=0"), (dict(first=0, count=2, bins=257), "nbins=257"),
                     (dict(first=0, count=2, range=(0.5, 0.5)), "lo < hi"), (dict(first=0, count=2, range=(1.0, -1.0)), "lo < hi"),
                     (dict(first=2, count=1, perms=None), "batch maps")):
        kw = {"perms": perms, **kw}
        with pytest.raises(RuntimeError, match=text):
            ops.corr_cd_hist(desc, ws, kw.pop("first"), kw.pop("count"), **kw)


def test_segmenter_logs_histograms_every_hist_freq_steps(dev):
    """Steps 0 and 1 log no histograms, step 2 (hist_freq = 2) the three of them; with hist_freq = None never; losses and parameters
    after three steps are the same with and without."""
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg

    def three_steps(**over):
        cfg = default_segmenter_cfg(dim=70, dg_outputs="reduced", **over)
        torch.manual_seed(21)
        m = UnsupervisedSegmenter(27, cfg).to(dev)
        m.train()
        g = torch.Generator().manual_seed(22)
        torch.manual_seed(23)
        steps = []
        for step in range(3):
            B = 2
            batch = {"img": torch.randn(B, 3, 112, 112, generator=g).to(dev), "img_pos": torch.randn(B, 3, 112, 112, generator=g).to(dev),
                     "label": torch.randint(-1, 27, (B, 112, 112), generator=g).to(dev),
                     "depth": torch.randint(1, 256, (B, 1, 112, 112), generator=g).float().to(dev),
                     "depth_pos": torch.randint(1, 256, (B, 1, 112, 112), generator=g).float().to(dev)}
            steps.append(m.training_step(batch, step))
        return steps, [p.detach().clone() for p in m.parameters()]

    # (torch's default algorithm for the linear probe's convolution backward adds in an order that changes from run to run - two runs
    #  WITHOUT histograms differ by 1e-8 in linear_probe.* - so the comparison asks torch for its deterministic algorithms; everything
    #  of this library is reproducible as it is)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with_h, params_h = three_steps(hist_freq=2, dg_hist_bins=32)
        without, params_0 = three_steps(hist_freq=None)
        with_d, _ = three_steps(hist_freq=1)
    finally:
        torch.backends.cudnn.deterministic = was
    keys = {"hist/intra_cd", "hist/inter_cd", "hist/neg_cd"}
    for step in (0, 1):
        assert not any(k.startswith("hist/") for k in with_h[step][1])
    logs = with_h[2][1]
    assert keys <= set(logs)
    P = 9 * 9          # feature_samples 11 decays to 9 at step 0 (quirk Q9)
    for k in keys:
        t = logs[k]
        assert t.dtype == torch.int64 and t.is_cuda and tuple(t.shape) == (32,)
        assert int(t.sum()) == (5 if k == "hist/neg_cd" else 1) * 2 * P * P
    for (loss_h, logs_h), (loss_0, logs_0) in zip(with_h, without):
        assert not any(k.startswith("hist/") for k in logs_0)
        assert torch.equal(loss_h, loss_0)
        assert {k for k in logs_h if not k.startswith("hist/")} == set(logs_0)
    for a, b in zip(params_h, params_0):
        assert torch.equal(a, b)
    # the default key: 64 bins
    assert tuple(with_d[1][1]["hist/intra_cd"].shape) == (64,) and "hist/intra_cd" not in with_d[0][1]
