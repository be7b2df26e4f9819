"""depthg_amd/optim.py without a GPU: the symbol, the refusals, the segmenter's flag, state-dict compatibility with
torch.optim.Adam in both directions, and the restatement tests/adam_reference.py against itself."""
import copy

import pytest
import torch

import adam_reference as AR


def test_adam_symbol_and_public_names():
    import depthg_amd
    from depthg_amd import _lib
    assert "dg_adam_step" in _lib.EXPORTS and hasattr(_lib.load(), "dg_adam_step")
    from depthg_amd.optim import FusedAdam, FusedAdamSet
    assert depthg_amd.FusedAdam is FusedAdam and depthg_amd.FusedAdamSet is FusedAdamSet
    assert issubclass(FusedAdam, torch.optim.Optimizer)


def test_c_entry_point_refuses_bad_tables():
    import ctypes
    from depthg_amd import _lib
    lib = _lib.load()
    seg, grp = (_lib.AdamSeg * 1)(), (_lib.AdamGroup * 1)()
    grp[0].lr, grp[0].beta1, grp[0].beta2, grp[0].eps = 1e-3, 0.9, 0.999, 1e-8
    assert ctypes.sizeof(_lib.AdamSeg) == 64 and ctypes.sizeof(_lib.AdamGroup) == 32         # include/depthg_corr.h
    assert lib.dg_adam_step(seg, 1, grp, 1, 0, None, None) == -1 and b"null parameter" in lib.dg_last_error()
    assert lib.dg_adam_step(seg, 0, grp, 1, 0, None, None) == -1 and b"positive" in lib.dg_last_error()
    assert lib.dg_adam_step(None, 1, grp, 1, 0, None, None) == -1
    seg[0].param = seg[0].exp_avg = seg[0].exp_avg_sq = seg[0].grad = 4096                   # (never dereferenced: refused first)
    seg[0].numel = 0
    assert lib.dg_adam_step(seg, 1, grp, 1, 0, None, None) == -1 and b"numel" in lib.dg_last_error()
    seg[0].numel, seg[0].group = 8, 1
    assert lib.dg_adam_step(seg, 1, grp, 1, 0, None, None) == -1 and b"group" in lib.dg_last_error()
    seg[0].group, seg[0].step_host = 0, 0.0
    assert lib.dg_adam_step(seg, 1, grp, 1, 0, None, None) == -1 and b"step_host" in lib.dg_last_error()
    assert lib.dg_adam_step(seg, 1, grp, 1, 1, None, None) == -1 and b"step_dev" in lib.dg_last_error()
    seg[0].step_dev, seg[0].numel = 8192, 5000
    assert lib.dg_adam_step(seg, 1, grp, 1, 1, None, None) == -1 and b"tickets" in lib.dg_last_error()
    grp[0].beta1 = 1.0
    assert lib.dg_adam_step(seg, 1, grp, 1, 0, None, None) == -1 and b"betas" in lib.dg_last_error()


def test_fused_adam_refuses_what_the_kernel_does_not_do():
    from depthg_amd import ops
    from depthg_amd.optim import FusedAdam, FusedAdamSet
    p = torch.nn.Parameter(torch.randn(5, 3))
    p.grad = torch.randn(5, 3)
    opt = FusedAdam([p], lr=1e-2)
    with pytest.raises(RuntimeError, match="GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="GPU"):
        FusedAdamSet([opt]).step()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.adam_step([(p.data, p.grad, torch.zeros(5, 3), torch.zeros(5, 3), 1.0, 0)], [(1e-3, 0.9, 0.999, 1e-8)])
    assert len(opt.state) == 0 and torch.equal(p.grad, p.grad)          # nothing was stepped, no state was made
    for kw in (dict(weight_decay=1e-2), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            FusedAdam([p], **kw)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(ValueError, match="float32"):
            FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=dt))])
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError):
        FusedAdam([p], betas=(1.0, 0.999))
    with pytest.raises(TypeError):
        FusedAdamSet([torch.optim.Adam([p])])
    # a group edited after construction is checked again at step()
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()


def test_segmenter_flag_selects_the_fused_triple():
    from depthg_amd.optim import FusedAdam
    from depthg_amd.segmenter import UnsupervisedSegmenter, default_segmenter_cfg
    assert default_segmenter_cfg().dg_fused_adam is False
    torch.manual_seed(0)
    m = UnsupervisedSegmenter(27, default_segmenter_cfg(dim=70, extra_clusters=2, lr=3e-4))
    plain = m.configure_optimizers()
    assert all(type(o) is torch.optim.Adam for o in plain)
    m.cfg.dg_fused_adam = True
    fused = m.configure_optimizers()
    assert len(fused) == 3 and all(type(o) is FusedAdam for o in fused)
    for a, b in zip(plain, fused):
        assert len(a.param_groups) == len(b.param_groups) == 1
        ga, gb = a.param_groups[0], b.param_groups[0]
        assert [id(p) for p in ga["params"]] == [id(p) for p in gb["params"]]
        assert ga["lr"] == gb["lr"] and ga["betas"] == gb["betas"] and ga["eps"] == gb["eps"]
        assert set(ga) == set(gb)                                        # the same keys: either class reads the other's state_dict
    assert fused[0].param_groups[0]["lr"] == 3e-4 and fused[1].param_groups[0]["lr"] == 5e-3 and fused[2].param_groups[0]["lr"] == 5e-3
    assert [id(p) for p in m._fused_set().parameters()] == [id(p) for p in m.all_reduced_parameters()]
    # handing gradients over needs the fused step
    m.cfg.dg_fused_adam = False
    with pytest.raises(RuntimeError, match="dg_fused_adam"):
        m._handed_over_grads([None] * 9, None)
    assert m._handed_over_grads((None, None), None) is None and m._handed_over_grads(None, None) is None


def _equal_state_dicts(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for q, va in a["state"][k].items():
            vb = b["state"][k][q]
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.device == vb.device and torch.equal(va, vb), (k, q)


def test_state_dict_round_trip_with_torch_adam():
    from depthg_amd.optim import FusedAdam
    shapes = [(7, 5), (5,), (3, 4, 1, 1)]
    params0, grad_seq = AR.seeded_problem(shapes, 7, seed=3)

    def fresh():
        return [torch.nn.Parameter(p.clone()) for p in params0]

    def step(opt, ps, grads):
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
    # an uninterrupted torch run
    pu = fresh()
    ou = torch.optim.Adam(pu, lr=5e-3)
    for grads in grad_seq:
        step(ou, pu, grads)
    # torch (4 steps) -> FusedAdam -> state_dict equal key by key
    pa = fresh()
    oa = torch.optim.Adam(pa, lr=5e-3)
    for grads in grad_seq[:4]:
        step(oa, pa, grads)
    sd = copy.deepcopy(oa.state_dict())
    pf = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    of = FusedAdam(pf, lr=1.0, betas=(0.5, 0.5), eps=1.0)              # (everything comes from the checkpoint)
    of.load_state_dict(sd)
    _equal_state_dicts(of.state_dict(), sd)
    assert all(of.state[p]["step"].device.type == "cpu" and of.state[p]["step"].dtype == torch.float32 for p in pf)
    # ... -> a fresh torch Adam, which continues on the CPU and ends where the uninterrupted run ends, bit for bit
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pf]
    ob = torch.optim.Adam(pb, lr=1.0)
    ob.load_state_dict(copy.deepcopy(of.state_dict()))
    for grads in grad_seq[4:]:
        step(ob, pb, grads)
    for a, b in zip(pu, pb):
        assert torch.equal(a, b)
    _equal_state_dicts(ob.state_dict(), ou.state_dict())
    # a FusedAdam that never stepped writes a state_dict a torch Adam accepts (same group keys)
    fresh_sd = FusedAdam(fresh(), lr=5e-3).state_dict()
    assert fresh_sd["state"] == {} and fresh_sd["param_groups"] == torch.optim.Adam(fresh(), lr=5e-3).state_dict()["param_groups"]


def test_adam_reference_agrees_with_itself():
    """float32 yardstick against float64 truth on the segmenter's nine shapes, 200 steps, gradients randn * 10**k.  The bounds are
    the formula's own: one step moves a weight by <= lr, computed with a few fp32 roundings (relative 2^-24 each), on weights of
    size 0.05 - about 1e-3 * 6e-8 / 5e-2 ~ 1e-9 per step before the weight's own rounding (6e-8); 200 steps of a random walk of
    that rounding stay far below 200 * 6e-8 = 1.2e-5.  (torch 2.10 measures 2.5e-8 after one step and 3.6e-7 after 200.)"""
    params0, grad_seq = AR.seeded_problem(AR.SEGMENTER_SHAPES, 200, seed=0)
    assert sum(p.numel() for p in params0) == 205_547
    truth = AR.run(params0, grad_seq, AR.SEGMENTER_GROUPS, torch.float64)
    yard = AR.run(params0, grad_seq, AR.SEGMENTER_GROUPS, torch.float32)
    assert truth[0]["param"][0].dtype == torch.float64 and yard[0]["param"][0].dtype == torch.float32
    first, last = AR.errors(yard[0]["param"], truth[0]["param"]), AR.errors(yard[-1]["param"], truth[-1]["param"])
    print("yardstick vs truth, parameters: step 1", first, "step 200", last)
    assert 0 < first[0] < 1.2e-7 and 0 < last[0] < 1.2e-5
    for q in ("exp_avg", "exp_avg_sq"):
        e = AR.errors(yard[-1][q], truth[-1][q])
        assert 0 < e[0] < 1e-5, (q, e)
    assert truth[-1]["step"] == [200.0] * 9
    # skipped gradients: the parameter, its moments and its step stay; a later gradient starts it at t = 1
    p0, gs = AR.seeded_problem([(4, 3), (6,)], 3, seed=1, skip={0: [1], 1: [1]})
    rec = AR.run(p0, gs, [dict(params=[0, 1], lr=1e-2)], torch.float64)
    assert torch.equal(rec[1]["param"][1], p0[1].double()) and rec[1]["step"] == [2.0, 0.0] and rec[2]["step"] == [3.0, 1.0]
    assert float(rec[1]["exp_avg"][1].abs().sum()) == 0.0 and float(rec[2]["exp_avg"][1].abs().sum()) > 0.0
