"""depthg_amd/optim.py on the GPU (-m gpu): dg_adam_step against torch.optim.Adam itself (tests/adam_reference.py).

The parity criterion (every comparison with "the truth" below): parameters, exp_avg and exp_avg_sq against the float64 run of
torch.optim.Adam on the same gradient sequence; the kernel's error - relative L2 and max-abs over max-abs, per quantity - must not
exceed 2 x the error of torch's own float32 Adam (the yardstick), computed in the same run.  Both are fp32 evaluations of the same
formula that differ only in rounding order, so their errors are random walks of the same step size; a wrong t, a missed tail or a
skipped segment is off by orders of magnitude.  The figures are printed before each assertion (profiles/adam_parity.md keeps the
ones of the first green run)."""
import pytest
import torch

import adam_reference as AR

DEV = "cuda:0"


def _bucket_offsets(shapes):
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        off += int(torch.Size(s).numel())
    return offs, off


class _GpuRun:
    """The product's side of a comparison: one FusedAdam per group, all in one FusedAdamSet."""

    def __init__(self, params0, groups, capturable=False):
        from depthg_amd.optim import FusedAdam, FusedAdamSet
        self.params = [torch.nn.Parameter(p.to(DEV).clone()) for p in params0]
        self.optims = [FusedAdam([self.params[i] for i in gr["params"]], capturable=capturable,
                                 **{k: v for k, v in gr.items() if k != "params"}) for gr in groups]
        self.order = [i for gr in groups for i in gr["params"]]           # the set's parameter order
        self.owner = {i: o for o, gr in zip(self.optims, groups) for i in gr["params"]}
        self.set = FusedAdamSet(self.optims)

    def step(self, grads, flat_views=False):
        """grads aligned with params0.  flat_views: handed over as views of ONE flat buffer at a GradBucket's offsets."""
        if flat_views:
            offs, total = _bucket_offsets([p.shape for p in self.params])
            flat = torch.zeros(total, device=DEV)
            views = []
            for p, g, o in zip(self.params, grads, offs):
                v = flat[o:o + p.numel()].view_as(p)
                if g is not None:
                    v.copy_(g)
                views.append(v if g is not None else None)
            self.set.step(grads=[views[i] for i in self.order])
        else:
            for p, g in zip(self.params, grads):
                p.grad = None if g is None else g.to(DEV)
            self.set.step()

    def record(self):
        rec = {"param": [p.detach().cpu().clone() for p in self.params], "exp_avg": [], "exp_avg_sq": [], "step": []}
        for i, p in enumerate(self.params):
            st = self.owner[i].state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq"):
                rec[k].append(st[k].detach().cpu().clone() if st else torch.zeros(p.shape))
            rec["step"].append(float(st["step"]) if st else 0.0)
        return rec


DWORD_SHAPES = AR.SEGMENTER_SHAPES + [(1,), (1024 * 16 + 3,)]
DWORD_GROUPS = AR.SEGMENTER_GROUPS + [dict(params=[9, 10], lr=2e-3, betas=(0.8, 0.99), eps=1e-6)]


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True], ids=["host_steps", "device_steps"])
@pytest.mark.parametrize("case", ["segmenter", "bucket_views"])
def test_parity_one_step_and_200(case, capturable):
    """The nine default tensors with their own gradients (128-bit path, tails of 70 / 27 / 1890 elements), and a second set read
    from views of one flat buffer at a GradBucket's offsets (26 950, ...: 4-byte aligned only - the dword path), with a 1-element
    tensor and one of 16 * 1024 + 3 elements over 17 blocks; a fourth group with other betas / eps."""
    shapes, groups = (AR.SEGMENTER_SHAPES, AR.SEGMENTER_GROUPS) if case == "segmenter" else (DWORD_SHAPES, DWORD_GROUPS)
    params0, grad_seq = AR.seeded_problem(shapes, 200, seed=7 if case == "segmenter" else 8)
    truth = AR.run(params0, grad_seq, groups, torch.float64)
    yard = AR.run(params0, grad_seq, groups, torch.float32)
    run = _GpuRun(params0, groups, capturable)
    if case == "bucket_views":
        offs, _ = _bucket_offsets(shapes)
        assert any(o % 4 for o in offs)                                   # some views are not 16-byte aligned
    for t, grads in enumerate(grad_seq):
        run.step(grads, flat_views=case == "bucket_views")
        if t in (0, 199):
            rec = run.record()
            assert rec["step"] == [float(t + 1)] * len(shapes)
            AR.assert_within_2x(rec, yard[t], truth[t], f"{case}/{'device' if capturable else 'host'} step {t + 1}")
    st = run.optims[0].state[run.params[0]]["step"]
    assert st.dtype == torch.float32 and st.dim() == 0 and st.is_cuda == capturable


@pytest.mark.gpu
def test_more_segments_than_one_launch_holds():
    """40 tensors in 3 groups: the table is split into launches of 16; every tensor is stepped exactly once."""
    shapes = [(3 + 5 * i,) for i in range(40)]
    groups = [dict(params=list(range(0, 15)), lr=1e-3), dict(params=list(range(15, 33)), lr=4e-3), dict(params=list(range(33, 40)), lr=2e-2)]
    params0, grad_seq = AR.seeded_problem(shapes, 3, seed=5)
    truth, yard = AR.run(params0, grad_seq, groups, torch.float64), AR.run(params0, grad_seq, groups, torch.float32)
    for capturable in (False, True):
        run = _GpuRun(params0, groups, capturable)
        for grads in grad_seq:
            run.step(grads)
        rec = run.record()
        assert rec["step"] == [3.0] * 40
        AR.assert_within_2x(rec, yard[-1], truth[-1], f"40 segments/{'device' if capturable else 'host'}")


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True], ids=["host_steps", "device_steps"])
def test_missing_gradient_skips_the_parameter(capturable):
    """torch skips parameters whose .grad is None: tensor 1 has no gradient at steps 2 and 3 (its weights, moments and step stay
    as they are, bit for bit), tensor 2 none until step 3 (no state until then, and it starts at t = 1)."""
    shapes = [(33, 7), (2050,), (70,)]
    groups = [dict(params=[0, 1], lr=5e-3), dict(params=[2], lr=1e-2)]
    params0, grad_seq = AR.seeded_problem(shapes, 4, seed=2, skip={0: [2], 1: [1, 2], 2: [1]})
    truth, yard = AR.run(params0, grad_seq, groups, torch.float64), AR.run(params0, grad_seq, groups, torch.float32)
    run = _GpuRun(params0, groups, capturable)
    recs = []
    for t, grads in enumerate(grad_seq):
        run.step(grads)
        recs.append(run.record())
        assert recs[t]["step"] == truth[t]["step"], (t, recs[t]["step"])
        AR.assert_within_2x(recs[t], yard[t], truth[t], f"skip/{'device' if capturable else 'host'} step {t + 1}")
    assert truth[-1]["step"] == [4.0, 2.0, 2.0]
    for q in AR.QUANTITIES:                                               # tensor 1 over its two skipped steps
        assert torch.equal(recs[0][q][1], recs[1][q][1]) and torch.equal(recs[1][q][1], recs[2][q][1])
        assert not torch.equal(recs[2][q][1], recs[3][q][1]) and not torch.equal(recs[0][q][0], recs[1][q][0])
    assert torch.equal(recs[1]["param"][2], params0[2]) and recs[1]["step"][2] == 0.0       # tensor 2: untouched, no state yet,
    assert recs[2]["step"][2] == 1.0 and recs[3]["step"][2] == 2.0                          # then t = 1, 2


@pytest.mark.gpu
def test_graph_replay_advances_the_device_step():
    """FusedAdamSet over capturable members: one warm-up step, then a step captured with torch.cuda.graph (a capture records the
    launch, it does not run it) and replayed five times with the gradients rewritten in place in between - six Adam steps in
    all, t = 6 on the device; nothing the host computed at capture time may be baked in."""
    shapes, groups = AR.SEGMENTER_SHAPES, AR.SEGMENTER_GROUPS
    params0, grad_seq = AR.seeded_problem(shapes, 6, seed=9)
    truth, yard = AR.run(params0, grad_seq, groups, torch.float64), AR.run(params0, grad_seq, groups, torch.float32)
    run = _GpuRun(params0, groups, capturable=True)
    static = [g.to(DEV).clone() for g in grad_seq[0]]
    for p, g in zip(run.params, static):
        p.grad = g
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run.set.step()                                                    # warm-up: state and ticket words are allocated here
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            run.set.step()
        torch.cuda.synchronize()
        assert run.record()["step"] == [1.0] * 9                          # (the capture ran nothing)
        for t in range(1, 6):
            for g, new in zip(static, grad_seq[t]):
                g.copy_(new)
            graph.replay()
        torch.cuda.synchronize()
    rec = run.record()
    assert rec["step"] == [6.0] * 9
    assert int(run.set._tickets.abs().sum()) == 0                         # every launch leaves its tickets at zero
    AR.assert_within_2x(rec, yard[5], truth[5], "graph replay, step 6")


def _batch(B, g, hw_img=112, n_classes=27):
    return {"img": torch.randn(B, 3, hw_img, hw_img, generator=g).to(DEV),
            "img_pos": torch.randn(B, 3, hw_img, hw_img, generator=g).to(DEV),
            "label": torch.randint(-1, n_classes, (B, hw_img, hw_img), generator=g).to(DEV),
            "depth": torch.randint(1, 256, (B, 1, hw_img, hw_img), generator=g).float().to(DEV),
            "depth_pos": torch.randint(1, 256, (B, 1, hw_img, hw_img), generator=g).float().to(DEV)}


@pytest.mark.gpu
def test_training_step_is_one_adam_launch(monkeypatch):
    from depthg_amd import ops
    from depthg_amd.optim import FusedAdam
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    calls = []
    real = ops.adam_step
    monkeypatch.setattr(ops, "adam_step", lambda segs, *a, **k: (calls.append(len(segs)), real(segs, *a, **k))[1])
    g = torch.Generator().manual_seed(21)
    for flag in (True, False):
        torch.manual_seed(6)
        m = UnsupervisedSegmenter(27, default_segmenter_cfg(dim=70, dg_outputs="reduced", dg_fused_adam=flag)).to(DEV)
        m.train()
        w0 = [p.detach().clone() for p in m.all_reduced_parameters()]
        del calls[:]
        loss, _ = m.training_step(_batch(2, g), 0)
        assert torch.isfinite(loss)
        assert calls == ([9] if flag else []), calls
        assert all(type(o) is (FusedAdam if flag else torch.optim.Adam) for o in m.optimizers())
        assert all(not torch.equal(a, b.detach()) for a, b in zip(w0, m.all_reduced_parameters()))


def _model_record(m, params):
    rec = {"param": [p.detach().cpu().clone() for p in params], "exp_avg": [], "exp_avg_sq": [], "step": []}
    state = {}
    for o in m.optimizers():
        state.update({id(p): o.state.get(p, {}) for gr in o.param_groups for p in gr["params"]})
    for p in params:
        st = state[id(p)]
        for k in ("exp_avg", "exp_avg_sq"):
            rec[k].append(st[k].detach().cpu().clone() if st else torch.zeros(p.shape))
        rec["step"].append(float(st["step"]) if st else 0.0)
    return rec


def _pick(rec, idx):
    return {k: [v[i] for i in idx] for k, v in rec.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "reset_probe_steps", "no_correspondence"])
def test_training_steps_end_to_end(case):
    """Three training_steps under cfg.dg_fused_adam; a grad_sync hook records every step's gradients (and the weights they meet);
    torch.optim.Adam on the CPU, fed those gradients from the same weights, gives the expected weights and moments after each
    step.  reset_probe_steps = 1: after the second step the probes get new weights and new optimisers (their Adam restarts at
    t = 1 in the third step), the head's state continues.  correspondence_weight = 0: the head receives no gradient and is skipped."""
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    over = {"reset_probe_steps": dict(reset_probe_steps=1), "no_correspondence": dict(correspondence_weight=0.0)}.get(case, {})
    cfg = default_segmenter_cfg(dim=70, dg_outputs="reduced", dg_fused_adam=True, **over)
    torch.manual_seed(8)
    m = UnsupervisedSegmenter(27, cfg).to(DEV)
    m.train()
    g = torch.Generator().manual_seed(31)
    head, probes = list(range(6)), [6, 7, 8]
    groups = [dict(params=head, lr=cfg.lr), dict(params=[6, 7], lr=5e-3), dict(params=[8], lr=5e-3)]
    seen, after = [], []
    for step in range(3):
        def hook():
            ps = m.all_reduced_parameters()
            seen.append(([p.detach().cpu().clone() for p in ps], [None if p.grad is None else p.grad.detach().cpu().clone() for p in ps]))
        loss, _ = m.training_step(_batch(2, g), step, grad_sync=hook)
        assert torch.isfinite(loss)
        after.append(_model_record(m, m.all_reduced_parameters()))
    weights0, grad_seq = seen[0][0], [s[1] for s in seen]
    if case == "no_correspondence":
        assert all(gr[i] is None for gr in grad_seq for i in head) and all(gr[i] is not None for gr in grad_seq for i in probes)
    else:
        assert all(x is not None for gr in grad_seq for x in gr)
    truth, yard = AR.run(weights0, grad_seq, groups, torch.float64), AR.run(weights0, grad_seq, groups, torch.float32)
    if case != "reset_probe_steps":
        for t in range(3):
            assert after[t]["step"] == truth[t]["step"]
            AR.assert_within_2x(after[t], yard[t], truth[t], f"training_step/{case} step {t + 1}")
        if case == "no_correspondence":
            assert all(torch.equal(after[2]["param"][i], weights0[i]) for i in head) and after[2]["step"][:6] == [0.0] * 6
        return
    # reset_probe_steps = 1: the head runs through; the probes' first two steps end in the reset (their weights after step 2 are
    # the new draw, their optimisers are new), their third step is a first step from the weights it met
    for t in range(3):
        AR.assert_within_2x(_pick(after[t], head), _pick(yard[t], head), _pick(truth[t], head), f"training_step/{case} head step {t + 1}")
    AR.assert_within_2x(_pick(after[0], probes), _pick(yard[0], probes), _pick(truth[0], probes), f"training_step/{case} probes step 1")
    assert after[1]["step"] == [2.0] * 6 + [0.0] * 3                       # fresh optimisers for the probes
    assert all(torch.equal(after[1]["param"][i], seen[2][0][i]) for i in probes)
    assert not any(torch.equal(after[1]["param"][i], truth[1]["param"][i].float()) for i in probes)     # ... and new weights
    g2 = [dict(params=[0, 1], lr=5e-3), dict(params=[2], lr=5e-3)]
    w2, gr2 = [seen[2][0][i] for i in probes], [[seen[2][1][i] for i in probes]]
    t2, y2 = AR.run(w2, gr2, g2, torch.float64), AR.run(w2, gr2, g2, torch.float32)
    assert after[2]["step"] == [3.0] * 6 + [1.0] * 3
    AR.assert_within_2x(_pick(after[2], probes), y2[0], t2[0], f"training_step/{case} probes step 3 (t = 1 again)")


@pytest.mark.gpu
def test_step_from_the_bucket_views():
    """Data-parallel hand-over on one GPU: pack the GradBucket, allreduce_mean_ (alone: the buffer as it is), and step from
    grad_views() - against the same library stepping from p.grad after unpack().  Which comparison applies: a view that starts on
    a 16-byte boundary takes the same 128-bit path as p.grad does - those tensors must agree BIT FOR BIT; the others (offsets
    26 950, 174 790, ...) take the dword path, and the whole set is held to the parity criterion against the truth instead.
    training_step(grad_sync=...) returning the bucket does the same hand-over (spied: the gradients are the views)."""
    from depthg_amd import ops
    from depthg_amd.parallel import GradBucket
    shapes, groups = AR.SEGMENTER_SHAPES, AR.SEGMENTER_GROUPS
    params0, grad_seq = AR.seeded_problem(shapes, 3, seed=4)
    truth, yard = AR.run(params0, grad_seq, groups, torch.float64), AR.run(params0, grad_seq, groups, torch.float32)
    a, b = _GpuRun(params0, groups), _GpuRun(params0, groups)
    bucket = GradBucket.for_parameters(a.params)
    bucket_b = GradBucket.for_parameters(b.params)
    views = bucket.grad_views()
    assert [v.shape for v in views] == [p.shape for p in a.params] and views[0].data_ptr() == bucket.flat.data_ptr()
    aligned = [i for i, v in enumerate(views) if v.data_ptr() % 16 == 0]
    assert 0 < len(aligned) < len(views)
    for grads in grad_seq:
        for run, bk in ((a, bucket), (b, bucket_b)):
            for p, g in zip(run.params, grads):
                p.grad = g.to(DEV)
            bk.pack()
            bk.allreduce_mean_(even_if_alone=False)
        a.set.step(grads=[views[i] for i in a.order])
        bucket_b.unpack()
        b.set.step()
    ra, rb = a.record(), b.record()
    for q in AR.QUANTITIES:
        for i in aligned:
            assert torch.equal(ra[q][i], rb[q][i]), (q, i)
    print("dword path equals the 128-bit path bit for bit:", all(torch.equal(ra[q][i], rb[q][i]) for q in AR.QUANTITIES for i in range(9)))
    AR.assert_within_2x(ra, yard[-1], truth[-1], "bucket views, step 3")
    AR.assert_within_2x(rb, yard[-1], truth[-1], "unpacked p.grad, step 3")

    # the same hand-over through training_step
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    torch.manual_seed(2)
    m = UnsupervisedSegmenter(27, default_segmenter_cfg(dim=70, dg_outputs="reduced", dg_fused_adam=True)).to(DEV)
    m.train()
    mb = GradBucket.for_parameters(m.all_reduced_parameters())
    got = []
    real = ops.adam_step
    ops.adam_step = lambda segs, *x, **k: (got.append([s[1].data_ptr() for s in segs]), real(segs, *x, **k))[1]
    try:
        m.training_step(_batch(2, torch.Generator().manual_seed(1)), 0, grad_sync=lambda: [mb.pack(), mb.allreduce_mean_(), mb][-1])
    finally:
        ops.adam_step = real
    assert got == [[v.data_ptr() for v in mb.grad_views()]]
    assert all(torch.isfinite(p).all() for p in m.all_reduced_parameters())
