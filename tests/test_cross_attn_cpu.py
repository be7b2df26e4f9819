"""The fused cross-attention (cfg.dg_fused_cross_attn) without a GPU: the C ABI's declarations and refusals, the float64 restatement
of tests/xattn_reference.py against nn.MultiheadAttention, the CPU route of depthg_amd.cross_attn, the flag's build-side contract, and
the error ratios of the prescribed arithmetic (the bounds tests/test_gpu_cross_attn.py holds the kernels to)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import xattn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dg_xattn_workspace_bytes", "dg_xattn_forward", "dg_xattn_backward", "dg_xattn_keep_mask")
A, MIS = 0x10000, 0x10004                 # an aligned and a misaligned address: never dereferenced, every call below is refused first


def lib():
    from depthg_amd import _lib
    return _lib.load()


def fwd(q=A, k=A, v=A, B=2, heads=8, nq=33, nk=31, hd=48, scale=0.1, p=0.1, out=A, lse=A, ws=A, nbytes=1 << 40):
    P = ctypes.c_void_p
    return lib().dg_xattn_forward(P(q), P(k), P(v), B, heads, nq, nk, hd, scale, p, 7, P(out), P(lse), P(ws), nbytes, None)


def bwd(q=A, k=A, v=A, o=A, lse=A, g=A, B=2, heads=8, nq=33, nk=31, hd=48, scale=0.1, p=0.1, dq=A, dk=A, dv=A, ws=A, nbytes=1 << 40):
    P = ctypes.c_void_p
    return lib().dg_xattn_backward(P(q), P(k), P(v), P(o), P(lse), P(g), B, heads, nq, nk, hd, scale, p, 7, P(dq), P(dk), P(dv), P(ws), nbytes, None)


def test_exports_are_declared_and_the_version_stays():
    from depthg_amd import _lib
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    names = re.findall(r"\b(dg_[a-z0-9_]+)\s*\(", header)
    order = [n for n in _lib.EXPORTS if n in NEW]
    assert tuple(order) == NEW and [n for n in names if n in NEW][-4:] == list(NEW)
    for n in NEW:
        assert hasattr(lib(), n), n
    assert _lib.DG_VERSION == 119 and lib().dg_version() == 119 and re.search(r"#define\s+DG_VERSION\s+119\b", header)


def test_workspace_bytes_is_zero_exactly_for_the_refused_shapes():
    w = lib().dg_xattn_workspace_bytes
    assert w(32, 8, 784, 784, 0) == 2 * 256 * 25 * 7168
    assert w(32, 8, 784, 784, 1) == 4 * 256 * 25 * 7168 + 2 * 256 * 25 * 32 * 4
    assert w(1, 1, 1, 1, 0) == 2 * 7168 and w(1, 1, 1, 1, 1) == 4 * 7168 + 2 * 256
    assert w(2, 8, 33, 65, 1) > w(2, 8, 33, 65, 0) > 0
    assert w(8191, 8, 5, 5, 0) > 0 and w(8192, 8, 5, 5, 0) == 0            # B * heads = 65528 / 65536
    for bad in ((0, 8, 5, 5), (1, 0, 5, 5), (1, 8, 0, 5), (1, 8, 5, 0), (-1, 8, 5, 5), (1, 8, (1 << 24) + 1, 5)):
        assert w(*bad, 0) == 0 and w(*bad, 1) == 0, bad


@pytest.mark.parametrize("call", [fwd, bwd], ids=["forward", "backward"])
def test_refusals_need_no_device(call):
    err = lambda: lib().dg_last_error()                                      # noqa: E731
    assert call(hd=64) == -2 and b"head_dim=64" in err()
    assert call(hd=32) == -2
    for p in (1.0, 1.5, -0.1, float("nan")):
        assert call(p=p) == -1 and b"dropout" in err(), p
    for s in (float("inf"), float("-inf"), float("nan")):
        assert call(scale=s) == -1 and b"scale" in err(), s
    for z in (dict(B=0), dict(heads=0), dict(nq=0), dict(nk=0), dict(nq=-3)):
        assert call(**z) == -1, z
    assert call(B=8192, heads=8) == -2 and b"65535" in err()
    for name in ("q", "k", "v", "ws") + (("out",) if call is fwd else ("o", "lse", "g")):
        assert call(**{name: 0}) == -1 and b"null" in err(), name
    for name in ("q", "k", "v", "ws") + (("out",) if call is fwd else ("o", "g", "dq", "dk", "dv")):
        assert call(**{name: MIS}) == -1 and b"aligned" in err(), name
    assert call(lse=A + 2) == -1 and b"aligned" in err()
    need = lib().dg_xattn_workspace_bytes(2, 8, 33, 31, int(call is bwd))
    assert call(nbytes=need - 1) == -3 and b"dg_xattn_workspace_bytes" in err()
    assert call(nbytes=0) == -3


def test_backward_refuses_half_a_key_value_pair():
    assert bwd(dk=0) == -1 and bwd(dv=0) == -1 and bwd(dq=0, dk=0, dv=0) == -1


def test_keep_mask_refusals():
    P = ctypes.c_void_p
    m = lib().dg_xattn_keep_mask
    assert m(1, 2, 8, 5, 5, 0.1, P(0), None) == -1
    assert m(1, 2, 8, 5, 5, 1.0, P(A), None) == -1 and m(1, 0, 8, 5, 5, 0.1, P(A), None) == -1
    assert m(1, 8192, 8, 5, 5, 0.1, P(A), None) == -2


def test_ops_refuse_in_order():
    """Shape, dtype and contiguity first, then the device (CPU tensors never get further)."""
    from depthg_amd import ops
    q, k = torch.zeros(2, 5, 96), torch.zeros(2, 7, 96)
    with pytest.raises(ValueError, match="heads"):
        ops.xattn_forward(torch.zeros(2, 5, 100), k, k, 2)
    with pytest.raises(ValueError, match="k and v"):
        ops.xattn_forward(q, k, torch.zeros(2, 8, 96), 2)
    with pytest.raises(ValueError, match="float32"):
        ops.xattn_forward(q.double(), k, k, 2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.xattn_forward(torch.zeros(2, 96, 5).transpose(1, 2), k, k, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.xattn_forward(q, k, k, 2)
    with pytest.raises(ValueError, match="grad_out"):
        ops.xattn_backward(q, k, k, q, torch.zeros(2, 2, 5), torch.zeros(2, 5, 48), 2)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        ops.xattn_keep_mask(0, 1, 1, 1, 1, 1.0, "cpu")


def _mha_case(dtype, seed=0, L=9, S=11, B=2, C=96, H=2):
    torch.manual_seed(seed)
    mha = torch.nn.MultiheadAttention(C, H, dropout=0.0).to(dtype)
    with torch.no_grad():
        mha.in_proj_bias.normal_(0, 0.1)
        mha.out_proj.bias.normal_(0, 0.1)
    g = torch.Generator().manual_seed(seed + 1)
    return mha, torch.randn(L, B, C, generator=g, dtype=torch.float64), torch.randn(S, B, C, generator=g, dtype=torch.float64), \
        torch.randn(L, B, C, generator=g, dtype=torch.float64)


def _grads(mha, out, query, up):
    mha.zero_grad()
    query.grad = None
    (out * up).sum().backward()
    return {"out": out.detach().double(), "query": query.grad.double(), **{n: p.grad.double() for n, p in mha.named_parameters()}}


def test_float64_restatement_equals_the_module():
    mha, query, kv, up = _mha_case(torch.float64)
    query.requires_grad_(True)
    want = _grads(mha, mha(query, kv, kv)[0], query, up)
    got = _grads(mha, R.mha_reference(mha, query, kv, torch.ones(2, 2, 9, 11), 0.0), query, up)
    assert set(want) >= {"out", "query", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"}
    for n in want:
        assert float((got[n] - want[n]).norm() / want[n].norm()) <= 1e-12, n
    # ... and the per-head restatement with explicit gradients equals autograd through the same formula
    q, k, v, g = R.make_inputs((33, 31, 2, 8, 0.5, 1.0))
    mask = R.random_mask((33, 31, 2, 8, 0.5, 1.0))
    t = R.attention_f64(q, k, v, g, 8, mask, 0.5)
    qd, kd, vd = (x.double().requires_grad_(True) for x in (q, k, v))
    P = torch.softmax(R.heads_first(qd, 8) @ R.heads_first(kd, 8).transpose(-1, -2) * 48 ** -0.5, -1) * mask.double() / 0.5
    o = R.tokens_first(P @ R.heads_first(vd, 8))
    o.backward(g.double())
    for n, x in (("o", o.detach()), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert float((t[n] - x).norm() / x.norm()) <= 1e-12, n


def test_cpu_route_matches_within_twice_the_float32_modules_error():
    from depthg_amd.cross_attn import multihead_cross_attention
    # the module's CPU route takes maps: (B, C, h, w) with h * w = S keys; the queries as a map of the same grid
    ref2, _, kv2, up2 = _mha_case(torch.float64, L=12, S=12)
    g = torch.Generator().manual_seed(3)
    qmap = torch.randn(2, 96, 3, 4, generator=g, dtype=torch.float64)
    fmap = kv2.permute(1, 2, 0).reshape(2, 96, 3, 4).contiguous()
    outs = {}
    for dtype in (torch.float64, torch.float32):
        m, _, _, _ = _mha_case(dtype, L=12, S=12)
        qm = qmap.detach().to(dtype).clone().requires_grad_(True)
        seq = qm.reshape(2, 96, -1).permute(2, 0, 1)
        direct = m(seq, fmap.to(dtype).reshape(2, 96, -1).permute(2, 0, 1), fmap.to(dtype).reshape(2, 96, -1).permute(2, 0, 1))[0]
        d = _grads(m, direct.permute(1, 2, 0).reshape(2, 96, 3, 4), qm, up2.permute(1, 2, 0).reshape(2, 96, 3, 4).to(dtype))
        r = _grads(m, multihead_cross_attention(m, qm, fmap.to(dtype), False), qm, up2.permute(1, 2, 0).reshape(2, 96, 3, 4).to(dtype))
        outs[dtype] = (d, r)
    t64, r64 = outs[torch.float64]
    d32, r32 = outs[torch.float32]
    rel = lambda a, b: float((a - b).norm() / b.norm())                      # noqa: E731
    for n in t64:
        assert rel(r64[n], t64[n]) <= 1e-12, n
        assert rel(r32[n], t64[n]) <= 2 * rel(d32[n], t64[n]), (n, rel(r32[n], t64[n]), rel(d32[n], t64[n]))
    # the evaluation branch's single query, expanded
    m, _, _, _ = _mha_case(torch.float64, L=12, S=12)
    one = torch.randn(1, 96, generator=g, dtype=torch.float64)
    want = m(one.reshape(1, 1, -1).expand(12, 2, -1), fmap.reshape(2, 96, -1).permute(2, 0, 1), fmap.reshape(2, 96, -1).permute(2, 0, 1))[0]
    got = multihead_cross_attention(m, one, fmap, False)
    assert rel(got, want.permute(1, 2, 0).reshape(2, 96, 3, 4)) <= 1e-12


def _stand_in(**over):
    from depthg_amd.segmenter import StandInFeaturizerWithDepth, default_segmenter_cfg
    cfg = default_segmenter_cfg(arch="dino_depth", guidance="cross_attn", dim=16)
    delattr(cfg, "dg_fused_cross_attn")
    for k, v in over.items():
        setattr(cfg, k, v)
    torch.manual_seed(0)
    return StandInFeaturizerWithDepth(16, cfg)


def test_flag_off_is_the_featurizer_without_the_key():
    a, b = _stand_in(), _stand_in(dg_fused_cross_attn=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[n], sb[n]) for n in sa)
    assert not a.fused_cross_attn and not b.fused_cross_attn and type(a.cross_attn) is torch.nn.MultiheadAttention
    g = torch.Generator().manual_seed(1)
    query, feat = torch.randn(16, 2, 384, generator=g), torch.randn(2, 384, 4, 4, generator=g)
    for train in (True, False):
        outs = []
        for net in (a, b):
            net.train(train)
            torch.manual_seed(3)
            outs.append(net._cross_attend(query, feat))
        assert torch.equal(outs[0], outs[1])
    on = _stand_in(dg_fused_cross_attn=True)
    assert on.fused_cross_attn and list(on.state_dict()) == list(sa) and all(torch.equal(on.state_dict()[n], sa[n]) for n in sa)


def test_flag_is_refused_where_the_kernels_do_not_fit():
    from depthg_amd.cross_attn import check_module, multihead_cross_attention
    with pytest.raises(ValueError, match="n_feats = 768"):
        _stand_in(dg_fused_cross_attn=True, model_type="vit_base")
    MHA = torch.nn.MultiheadAttention
    for bad, word in ((MHA(384, 6), "head dimension"), (MHA(384, 8, batch_first=True), "batch_first"), (MHA(384, 8, kdim=100), "kdim"),
                      (MHA(384, 8, vdim=100), "vdim"), (MHA(384, 8, bias=False), "bias"), (MHA(384, 8, add_bias_kv=True), "add_bias_kv"),
                      (torch.nn.Linear(4, 4), "MultiheadAttention")):
        with pytest.raises(ValueError, match=word):
            check_module(bad)
    with pytest.raises(ValueError, match="batch_first"):
        multihead_cross_attention(MHA(384, 8, batch_first=True), torch.zeros(1, 384, 2, 2), torch.zeros(1, 384, 2, 2), False)
    check_module(MHA(384, 8, dropout=0.1))
    check_module(MHA(96, 2))


def test_emulated_ratios_stay_under_the_gpu_tests_bounds(tmp_path):
    """scripts/cross_attn_parity.py computes the ratios of the prescribed arithmetic over the GPU test's grid and writes the table;
    they are what xattn_reference records (EMULATED_*), O stays at or under 1.2, and every gradient under its bound."""
    out = tmp_path / "parity.md"
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cross_attn_parity.py"), "--out", str(out)], check=True, cwd=ROOT)
    line = next(ln for ln in out.read_text().splitlines() if ln.startswith("worst over the grid"))
    worst = {n: float(x) for n, x in re.findall(r"(o|dq|dk|dv) ([0-9.]+)", line)}
    print(worst)
    assert worst["o"] <= R.EMULATED_O <= 1.2 and R.FACTOR_O == 1.5
    for n in ("dq", "dk", "dv"):
        assert worst[n] <= R.EMULATED_GRAD[n] and R.FACTOR_GRAD[n] == 1.25 * R.EMULATED_GRAD[n]
