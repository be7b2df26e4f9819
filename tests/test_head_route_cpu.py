"""The head's route to the C ABI without a GPU: _HeadFunction calls dg_head_forward, dg_head_backward and - where an input gradient is
asked for - dg_head_backward_input, once each, with the argument lists _lib.SIGNATURES declares; a single pass leaves the second
pass's slots NULL, a pair fills them with the second tensors.  The ctypes functions are replaced by recorders; the tensors live on the
CPU.  Below: what the built library's one-entry-per-operation forms of the head, the FPS sampler and super_perms refuse before any
launch."""
import ctypes

import pytest
import torch

from depthg_amd import _lib, head

B, C, D, HW = 2, 8, 4, 3
SIZERS = ("dg_head_weights_bytes", "dg_head_workspace_bytes", "dg_head_input_workspace_bytes")
# positions in the argument lists of include/depthg_corr.h: (first pass, second pass)
FWD = dict(feat=(4, 5), keeps=(12, 13, 14), code=(16, 17), feats_out=(18, 19), hidden=20)
BWD = dict(feat=(4, 5), grad_code=(11, 12), workspace=19)
DX = dict(keep3=8, grad_code=(11, 12), grad_feats_out=(13, 14), workspace=15, grad_feat=(17, 18))


class Recorder:
    """Stands in for the loaded library: every function records its call; a sizer answers 64 bytes, anything else DG_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 64 if name in SIZERS else 0
        return fn

    def entries(self):
        return [(name, args) for name, args in self.calls if name not in SIZERS]


@pytest.fixture
def rec(monkeypatch):
    """The recorder in place of the library, and inside `head` a null stream and an _f32c without the GPU requirement that notes
    what it was handed under each name (the upstream gradients are seen nowhere else)."""
    r = Recorder()
    r.seen = {}

    def f32c(t, name):
        if t is None:
            return None
        t = t.detach().to(torch.float32).contiguous()
        r.seen.setdefault(name, []).append(t)
        return t
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(head, "_stream", lambda device: ctypes.c_void_p(0))
    monkeypatch.setattr(head, "_f32c", f32c)
    return r


def ptr(a):
    return a.value or 0


def check_declared(name, args):
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes), name
    for a, t in zip(args, argtypes):
        t.from_param(a)                       # (what ctypes does with the declared argtypes: raises on a mismatch)


def run(proj, pair, input_grad, feats_grad, use_feats, need=(True, True)):
    """One training-mode forward and backward of a ProjectionHead; returns (feature maps, outputs per pass)."""
    torch.manual_seed(0)
    net = head.ProjectionHead(C, D, proj).train()
    feats = [torch.randn(B, C, HW, HW).requires_grad_(input_grad and n) for n in (need if pair else need[:1])]
    kw = dict(input_grad=input_grad, feats_grad=feats_grad)
    outs = net.forward_pair(*feats, **kw) if pair else (net(feats[0], **kw),)
    loss = sum(code.sum() for code, _ in outs)
    if use_feats:
        loss = loss + sum(fo.sum() for _, fo in outs)
    loss.backward()
    return feats, outs


@pytest.mark.parametrize("mode", ["params", "input", "input+feats"])
@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("proj", ["linear", "nonlinear"])
def test_each_pass_count_reaches_the_one_entry_with_the_declared_arguments(proj, pair, mode, rec):
    input_grad, feats_grad = mode != "params", mode == "input+feats"
    feats, outs = run(proj, pair, input_grad, feats_grad, use_feats=feats_grad)
    n = len(feats)
    calls = rec.entries()
    assert [name for name, _ in calls] == ["dg_head_forward", "dg_head_backward"] + ["dg_head_backward_input"] * input_grad
    for name, args in calls:
        check_declared(name, args)
        assert args[:4] == (B, C, D, HW * HW)                   # B is the images of ONE pass, with one pass and with two
    second = lambda tensors: tensors[1].data_ptr() if pair else 0
    fwd, bwd = calls[0][1], calls[1][1]
    # forward: the features, the codes and the dropped feats of each pass; the second pass's slots NULL on a single pass
    assert [ptr(fwd[i]) for i in FWD["feat"]] == [feats[0].data_ptr(), second(feats)]
    assert [ptr(fwd[i]) for i in FWD["code"]] == [outs[0][0].data_ptr(), second([c for c, _ in outs])]
    assert [ptr(fwd[i]) for i in FWD["feats_out"]] == [outs[0][1].data_ptr(), second([f for _, f in outs])]
    keeps = [ptr(fwd[i]) for i in FWD["keeps"]]
    assert keeps[0] and keeps[2] and bool(keeps[1]) == (proj == "nonlinear")
    assert bool(ptr(fwd[FWD["hidden"]])) == (proj == "nonlinear")
    # backward: the same features, the upstream gradient of each pass's code
    gc, gcp = rec.seen["grad_code"][0], rec.seen.get("grad_code_pos", [None])[0]
    assert (gcp is not None) == pair
    assert [ptr(bwd[i]) for i in BWD["feat"]] == [feats[0].data_ptr(), second(feats)]
    assert [ptr(bwd[i]) for i in BWD["grad_code"]] == [gc.data_ptr(), gcp.data_ptr() if pair else 0]
    assert bwd[BWD["workspace"] + 1] == 64
    if not input_grad:
        assert all(f.grad is None for f in feats)
        return
    dx = calls[2][1]
    assert [ptr(dx[i]) for i in DX["grad_code"]] == [ptr(bwd[i]) for i in BWD["grad_code"]]
    assert ptr(dx[DX["workspace"]]) == ptr(bwd[BWD["workspace"]]) and dx[DX["workspace"] + 1] == 64
    gf = [ptr(dx[i]) for i in DX["grad_feat"]]
    assert gf[0] and bool(gf[1]) == pair
    assert all(f.grad is not None and f.grad.shape == f.shape for f in feats)
    # keep3 and the gradients of the returned feats: NULL unless feats_grad carried them here
    gfo = [ptr(dx[i]) for i in DX["grad_feats_out"]]
    if feats_grad:
        seen = rec.seen["grad_feats"]
        assert len(seen) == n and gfo == [seen[0].data_ptr(), seen[1].data_ptr() if pair else 0]
        assert ptr(dx[DX["keep3"]]) == keeps[2]
    else:
        assert gfo == [0, 0] and ptr(dx[DX["keep3"]]) == 0 and "grad_feats" not in rec.seen


def test_a_pass_that_asks_for_nothing_gets_null_slots(rec):
    """Only the second pass's features require grad: its grad_feat and grad_feats_out slots are filled, the first pass's are NULL;
    feats_grad without a gradient reaching the returned feats hands no grad_feats_out at all."""
    feats, _ = run("nonlinear", True, True, True, use_feats=True, need=(False, True))
    dx = rec.entries()[2][1]
    check_declared("dg_head_backward_input", dx)
    assert [bool(ptr(dx[i])) for i in DX["grad_feat"]] == [False, True]
    assert [ptr(dx[i]) for i in DX["grad_feats_out"]] == [0, rec.seen["grad_feats"][0].data_ptr()] and ptr(dx[DX["keep3"]])
    assert feats[0].grad is None and feats[1].grad is not None
    del rec.calls[:]
    rec.seen.clear()
    run("nonlinear", True, True, True, use_feats=False)
    dx = rec.entries()[2][1]
    assert [ptr(dx[i]) for i in DX["grad_feats_out"]] == [0, 0] and all(ptr(dx[i]) for i in DX["grad_feat"])


# ---- the built library: refusals that return before any launch (the addresses are never dereferenced)
INVALID, UNSUPPORTED = -1, -2
X, NULL = ctypes.c_void_p(4096), ctypes.c_void_p(0)


def test_a_second_pass_pointer_without_its_pass_is_refused():
    lib = _lib.load()
    Bh, Ch, Dh, Ph = 2, 64, 16, 9

    def forward(feat_pos=NULL, code_pos=NULL, feats_out_pos=NULL):
        return lib.dg_head_forward(Bh, Ch, Dh, Ph, X, feat_pos, X, X, X, X, X, X, X, X, X, 1.0, X, code_pos, X, feats_out_pos, X, X, NULL)

    def backward(grad_code_pos):
        return lib.dg_head_backward(Bh, Ch, Dh, Ph, X, NULL, X, X, 1.0, X, X, X, grad_code_pos, X, X, X, X, X, X, X, 1 << 30, NULL)

    def backward_input(grad_feats_out_pos=NULL, grad_feat_pos=NULL):
        return lib.dg_head_backward_input(Bh, Ch, Dh, Ph, X, X, X, X, X, 1.0, X, X, NULL, X, grad_feats_out_pos, X, 1 << 30, X,
                                          grad_feat_pos, X, 1 << 30, NULL)

    for call in (lambda: forward(code_pos=X), lambda: forward(feats_out_pos=X), lambda: backward(X),
                 lambda: backward_input(grad_feat_pos=X), lambda: backward_input(grad_feats_out_pos=X)):
        assert call() == INVALID
        assert b"second pass" in lib.dg_last_error()
    # with its pass, a missing partner is the refusal it always was
    assert forward(feat_pos=X) == INVALID and b"null pointer of the second pass" in lib.dg_last_error()


def test_super_perms_takes_one_source_of_keys():
    lib = _lib.load()
    assert lib.dg_super_perms(X, 0, X, 3, 4, X, NULL) == INVALID
    assert b"keys" in lib.dg_last_error() and b"state" in lib.dg_last_error()
    assert lib.dg_super_perms(NULL, 0, NULL, 0, 4, NULL, NULL) == 0                    # count == 0: no pointer is looked at
    for count, Bp in ((-1, 4), (1, 0), (1, 8193)):
        assert lib.dg_super_perms(X, 0, NULL, count, Bp, X, NULL) == INVALID
        assert f"count={count} B={Bp}".encode() in lib.dg_last_error()


@pytest.mark.parametrize("depth_pos", [NULL, X], ids=["single", "pair"])
def test_fps_refusals_hold_with_and_without_depth_pos(depth_pos):
    lib = _lib.load()

    def fps(h, w, S, Bf=2):
        return lib.dg_fps_coords(X, depth_pos, Bf, 224, 224, h, w, S, X, NULL, NULL, 0, NULL)

    assert fps(8, 8, 9) == INVALID and b"cannot sample 81 points" in lib.dg_last_error()
    assert fps(65, 64, 4) == UNSUPPORTED and b"too large" in lib.dg_last_error()
    assert fps(8, 8, 2, Bf=0) == INVALID and b"bad FPS dimensions" in lib.dg_last_error()
