"""ops.corr_forward without a GPU: which C entry each extra selects, with the argument list _lib.SIGNATURES declares for it, and the
combinations it refuses before the library is touched.  The ctypes functions are replaced by recorders; the tensors live on the CPU."""
import ctypes

import pytest
import torch

from depthg_amd import _lib, ops

B, C, D, HW, S, N = 2, 8, 4, 6, 3, 2
SIZERS = ("dg_corr_workspace_bytes", "dg_corr_workspace_bytes_intra_feats")


class Recorder:
    """Stands in for the loaded library: every function records its call; a sizer answers 64 bytes, anything else DG_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 64 if name in SIZERS else 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda device: ctypes.c_void_p(0))
    return r


def _operands():
    desc = ops.make_desc(B, C, D, HW, HW, S, N, pointwise=True, zero_clamp=True, stabalize=False, depth_term=False, need_grad=True,
                         shared_coords=False, shifts=(0.1, 0.1, 0.4, 0.0))
    f, c, xy = torch.zeros(B, C, HW, HW), torch.zeros(B, D, HW, HW), torch.zeros(B, S, S, 2)
    return desc, (f, f.clone(), c, c.clone(), None, xy, xy.clone())


EXTRAS = {
    "keep": lambda: (torch.ones(B, C), None, 1.25),
    "feat_inv": lambda: torch.ones(2 + N, B, S * S),
    "intra_feats": lambda: torch.zeros(B, C, HW, HW),
}


@pytest.mark.parametrize("pair", [("keep", "feat_inv"), ("keep", "intra_feats"), ("feat_inv", "intra_feats")])
def test_two_extras_are_refused_by_name_before_the_library_is_touched(pair, monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    desc, maps = _operands()
    with pytest.raises(ValueError) as e:
        ops.corr_forward(desc, *maps, torch.zeros(N, B, dtype=torch.long), **{k: EXTRAS[k]() for k in pair})
    assert all(f"`{k}`" in str(e.value) for k in pair)


def test_feat_inv_without_perms_is_refused_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    desc, maps = _operands()
    with pytest.raises(ValueError) as e:
        ops.corr_forward(desc, *maps, None, feat_inv=EXTRAS["feat_inv"]())
    assert "`feat_inv`" in str(e.value) and "perms" in str(e.value)


@pytest.mark.parametrize("extra, draw, entry", [
    (None, False, "dg_corr_forward"), (None, True, "dg_corr_forward_draw"),
    ("keep", False, "dg_corr_forward_masked"), ("keep", True, "dg_corr_forward_masked"),
    ("feat_inv", False, "dg_corr_forward_extnorm"),
    ("intra_feats", False, "dg_corr_forward_intra_feats"), ("intra_feats", True, "dg_corr_forward_intra_feats"),
])
def test_each_selection_reaches_its_entry_with_the_declared_arguments(extra, draw, entry, rec, monkeypatch):
    monkeypatch.setattr(ops, "_cpu_seed", lambda: 4242)
    desc, maps = _operands()
    perms = None if draw else torch.zeros(N, B, dtype=torch.long)
    kw = {extra: EXTRAS[extra]()} if extra else {}
    out, used, ws = ops.corr_forward(desc, *maps, perms, **kw)
    # the sizer of the entry, then the entry itself - once each, nothing else
    sizer = SIZERS[extra == "intra_feats"]
    assert [name for name, _ in rec.calls] == [sizer, entry]
    args = rec.calls[1][1]
    argtypes = _lib.SIGNATURES[entry][1]
    assert len(args) == len(argtypes)
    for a, t in zip(args, argtypes):
        t.from_param(a)                       # (what ctypes does with the declared argtypes: raises on a mismatch)
    ptr = lambda a: a.value or 0
    assert [ptr(a) for a in args[1:5]] == [t.data_ptr() for t in maps[:4]] and ptr(args[5]) == 0       # depth: null here
    assert ptr(args[8]) == used.data_ptr() and (used is perms or draw)
    assert tuple(used.shape) == (N, B) and used.dtype == torch.long
    assert ws.numel() == 64 and ptr(args[-3]) == ws.data_ptr() and args[-2] == 64
    assert ptr(args[-4]) == out.data_ptr() and out.numel() == _lib.DG_OUT_COUNT
    mid = args[9:-4]
    if extra in ("keep", "intra_feats"):
        assert mid[:2] == ((1, 4242) if draw else (0, 0))
    if entry == "dg_corr_forward_draw":
        assert mid[0] == 4242
    if extra == "keep":
        assert ptr(mid[3]) == kw["keep"][0].data_ptr() and ptr(mid[4]) == 0 and mid[5] == 1.25
    elif extra:
        assert ptr(mid[-1]) == kw[extra].data_ptr()
    # a workspace handed in is used as given: no sizer call
    del rec.calls[:]
    mine = torch.zeros(96, dtype=torch.uint8)
    ws = ops.corr_forward(desc, *maps, perms, mine, **kw)[2]
    assert [name for name, _ in rec.calls] == [entry] and ws is mine and rec.calls[0][1][-2] == 96


def test_the_intra_entry_never_sees_depth(rec):
    desc, maps = _operands()
    maps = maps[:4] + (torch.zeros(B, 1, 8, 8),) + maps[5:]
    ops.corr_forward(desc, *maps, torch.zeros(N, B, dtype=torch.long), intra_feats=EXTRAS["intra_feats"]())
    assert rec.calls[1][0] == "dg_corr_forward_intra_feats" and not rec.calls[1][1][5].value


def test_alloc_workspace_picks_the_sizer(rec):
    desc, _ = _operands()
    ops.alloc_workspace(desc, "cpu")
    ops.alloc_workspace(desc, "cpu", intra_feats=True)
    assert [name for name, _ in rec.calls] == list(SIZERS)
