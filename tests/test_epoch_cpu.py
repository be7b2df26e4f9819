"""The device-side batch draw without a GPU: the export, ops.epoch_draw's CPU route against the restatement of the stated function,
DeviceEpoch's epoch on CPU tensors, and every refusal of GraphedTrainStep."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from epoch_draw_reference import case, epoch_draw, philox_word0

CASES = [(5, 3, 2, 1), (33, 8, 32, 7), (1000, 8, 7, 7), (1025, 31, 1024, 30)]          # (n_images, K, B, num_neighbors)


def test_export_is_declared_and_bound():
    from depthg_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "depthg_corr.h")).read()
    assert "int dg_epoch_draw(uint64_t* state, const int64_t* order, const int64_t* nns, int32_t B, int32_t num_neighbors, int64_t n_images, int32_t K," in header
    assert "src/data.py:1073-1080" in header
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _lib.SIGNATURES["dg_epoch_draw"] == (ctypes.c_int, [vp, vp, vp, i32, i32, i64, i32, vp, vp, vp])
    lib = _lib.load()
    assert hasattr(lib, "dg_epoch_draw") and callable(ops.epoch_draw)
    assert _lib.EXPORTS.index("dg_epoch_draw") == _lib.EXPORTS.index("dg_samplecache_gather") + 1
    assert "dg_epoch.hip" in open(os.path.join(ROOT, "depthg_amd", "csrc", "Makefile")).read()
    # the host entry's refusals come before any launch: no GPU is touched
    p = ctypes.c_void_p(4096)
    for args, word in (((p, p, p, 4, 0, 10, 8, p, p, None), b"num_neighbors"), ((p, p, p, 4, 8, 10, 8, p, p, None), b"num_neighbors"),
                       ((p, p, p, 1025, 3, 2000, 8, p, p, None), b"above 1024"), ((p, p, p, 0, 3, 10, 8, p, p, None), b"positive"),
                       ((None, p, p, 4, 3, 10, 8, p, p, None), b"null"), ((ctypes.c_void_p(4100), p, p, 4, 3, 10, 8, p, p, None), b"aligned")):
        assert lib.dg_epoch_draw(*args) < 0 and word in lib.dg_last_error(), (args, lib.dg_last_error())


def test_philox_word_is_the_published_function():
    """Random123's known-answer vectors for philox4x32_10: counter 0 / key 0, and all ones."""
    assert philox_word0(0, 0) == 0x6627E8D5
    # (counter (ff.., ff.., 0, 0) is not a published vector; the all-ones one has four counter words - the device function's word 0 at
    #  counter (c, 0) with the upper counter words zero is pinned by the first vector and by the kernel test)
    from depthg_amd.ops import _philox_word0
    import numpy as np
    ctrs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345, 2 ** 64 - 1]
    for seed in (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1):
        got = _philox_word0(seed, np.array(ctrs, dtype=np.uint64)).tolist()
        assert got == [philox_word0(seed, c) for c in ctrs]


@pytest.mark.parametrize("n,K,B,nn", CASES, ids=[f"n{c[0]}-K{c[1]}-B{c[2]}-nn{c[3]}" for c in CASES])
def test_cpu_route_matches_the_restatement(n, K, B, nn):
    from depthg_amd import ops
    order, nns = case(n, K)
    state = torch.tensor([0x1234567887654321, 2 ** 32 - 3, 0], dtype=torch.int64)
    want_state = state.tolist()
    for _ in range(3):                                           # (the largest case runs past the end: the held position)
        ind = torch.full((B,), -7, dtype=torch.int64)
        ind_pos = torch.full((B,), -7, dtype=torch.int64)
        a, b = ops.epoch_draw(state, order, nns, B, nn, ind, ind_pos)
        assert a is ind and b is ind_pos
        want_ind, want_pos, want_state = epoch_draw(want_state, order.tolist(), nns.tolist(), B, nn)
        assert ind.tolist() == want_ind and ind_pos.tolist() == want_pos and state.tolist() == want_state
        # every positive is one of its image's neighbours 1 .. num_neighbors
        for i, p in zip(want_ind, want_pos):
            assert p in nns[i, 1:nn + 1].tolist()
    # a cursor past the end repeats the last entry instead of reading past the buffer; a negative seed word is the same 64 bits
    state = torch.tensor([-5, 0, n + 3], dtype=torch.int64)
    ind, ind_pos = ops.epoch_draw(state, order, nns, B, nn)
    want_ind, want_pos, want_state = epoch_draw([-5, 0, n + 3], order.tolist(), nns.tolist(), B, nn)
    assert ind.tolist() == want_ind == [int(order[-1])] * B and ind_pos.tolist() == want_pos and state.tolist() == want_state


def test_positives_cover_the_neighbours_evenly():
    from depthg_amd import ops
    order, nns = case(64, 8)
    nns[:, 1:] = torch.arange(1, 8)                              # (the column drawn is the value read)
    state = torch.tensor([99, 0, 0], dtype=torch.int64)
    counts = torch.zeros(8, dtype=torch.int64)
    for _ in range(200):
        state[2] = 0
        counts += torch.bincount(ops.epoch_draw(state, order, nns, 64, 7)[1], minlength=8)
    assert counts[0] == 0 and counts.sum() == 12800
    # 12800 draws over 7 columns: mean 1828.6, standard deviation 39.6; six of them is a bound no fair draw misses in practice
    assert (counts[1:].float() - 12800 / 7).abs().max() < 6 * 39.6, counts.tolist()


def test_refusals_of_the_python_entry():
    from depthg_amd import ops
    order, nns = case(10, 4)
    st = torch.tensor([1, 0, 0], dtype=torch.int64)
    for kw, word in ((dict(B=0), "B=0"), (dict(B=1025), "B=1025"), (dict(num_neighbors=0), "num_neighbors=0"), (dict(num_neighbors=4), "num_neighbors=4"),
                     (dict(order=order[:5]), "order"), (dict(nns=nns.to(torch.int32)), "nns"), (dict(state=st[:2]), "state"),
                     (dict(ind=torch.zeros(3, dtype=torch.int64)), "`ind`")):
        args = {**dict(state=st, order=order, nns=nns, B=2, num_neighbors=3), **kw}
        with pytest.raises(ValueError, match=word):
            ops.epoch_draw(**args)


def test_one_epoch_visits_the_order_once():
    from depthg_amd.epoch import DeviceEpoch
    _, nns = case(23, 6)
    torch.manual_seed(11)
    ep = DeviceEpoch(nns.numpy(), 4, 3, "cpu", shuffle=True, generator=torch.Generator().manual_seed(5))
    assert ep.steps_per_epoch == len(ep) == 5
    with pytest.raises(RuntimeError, match="begin_epoch"):
        ep.draw()
    for epoch in range(2):
        ep.begin_epoch()
        seen, pos = [], []
        for _ in range(ep.steps_per_epoch):
            ind, ind_pos = ep.draw()
            assert ind is ep.ind and ind_pos is ep.ind_pos
            seen += ind.tolist()
            pos += ind_pos.tolist()
        assert seen == ep.order[:20].tolist() and len(set(seen)) == 20           # the first (n // B) * B entries, once each
        assert all(p in nns[i, 1:4].tolist() for i, p in zip(seen, pos))
        assert ep.state.tolist()[1:] == [20 * (epoch + 1), 20]
        with pytest.raises(RuntimeError, match="begin_epoch"):                    # the short last batch is dropped, not drawn
            ep.draw()


def test_begin_epoch_is_the_generators_randperm():
    from depthg_amd.epoch import DeviceEpoch
    _, nns = case(17, 5)
    ep = DeviceEpoch(nns, 4, 2, "cpu", shuffle=True, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        ep.begin_epoch()
        assert ep.order.tolist() == torch.randperm(17, generator=g).tolist() and int(ep.state[2]) == 0
    plain = DeviceEpoch(nns, 4, 2, "cpu", shuffle=False)
    ptr = plain.order.data_ptr()
    plain.begin_epoch()
    assert plain.order.tolist() == list(range(17)) and plain.order.data_ptr() == ptr
    # the global generator without one: what ContrastiveBatches.__iter__ draws
    ep = DeviceEpoch(nns, 4, 2, "cpu", shuffle=True)
    torch.manual_seed(4)
    ep.begin_epoch()
    torch.manual_seed(4)
    assert ep.order.tolist() == torch.randperm(17).tolist()


def test_device_epoch_refusals():
    from depthg_amd.epoch import DeviceEpoch
    _, nns = case(10, 4)
    for args, err, word in (((nns, 0, 2), ValueError, "batch_size=0"), ((nns, 1025, 2), ValueError, "batch_size=1025"),
                            ((nns, 11, 2), ValueError, "no batch"), ((nns, 2, 4), ValueError, "num_neighbors=4"),
                            ((nns, 2, 0), ValueError, "num_neighbors=0"), ((nns.float(), 2, 2), ValueError, "integer"),
                            ((nns + 1, 2, 2), IndexError, "outside")):
        with pytest.raises(err, match=word):
            DeviceEpoch(*args, "cpu")
    # a cache with a row never put, of another size, or elsewhere: asked once, by batch()
    ep = DeviceEpoch(nns, 2, 2, "cpu")
    ep.begin_epoch()
    import numpy as np
    full = SimpleNamespace(n_images=10, device=torch.device("cpu"), filled=np.ones(10, dtype=bool))
    holed = SimpleNamespace(n_images=10, device=torch.device("cpu"), filled=np.arange(10) != 6)
    with pytest.raises(ValueError, match="row 6 of the sample cache was never put"):
        ep.batch(holed, None)
    with pytest.raises(ValueError, match="row 6 of the feature cache was never put"):
        ep.batch(full, holed)
    with pytest.raises(ValueError, match="holds 9 images"):
        ep.batch(SimpleNamespace(n_images=9, device=torch.device("cpu"), filled=np.ones(9, dtype=bool)), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ep.batch(full, full)
    assert ep.drawn == 0                                         # nothing was drawn by a refused call


# ---------------------------------------------------------------------------------------------------------------- GraphedTrainStep
def _stub(**over):
    from depthg_amd.segmenter import default_segmenter_cfg
    cfg = default_segmenter_cfg(**{**dict(dg_feature_cache="float32", dg_graph_safe=True, dg_fused_adam=True, dg_graph_step=True), **over})
    return SimpleNamespace(cfg=cfg)


REFUSALS = [(dict(), dict(sample_cache=None), "no sample cache"), (dict(), dict(feature_cache=None), "no feature cache"),
            (dict(dg_feature_cache=None), {}, "cfg.dg_feature_cache"), (dict(dg_graph_safe=False), {}, "cfg.dg_graph_safe = True"),
            (dict(dg_fused_adam=False), {}, "cfg.dg_fused_adam = True"), (dict(arch="dino_depth"), {}, "dino_depth"),
            (dict(lhp=True), {}, "cfg.lhp = False"), (dict(crf_weight=0.1), {}, "cfg.crf_weight = 0"),
            (dict(aug_alignment_weight=0.5), {}, "cfg.aug_alignment_weight = 0"),
            (dict(use_depth_only_intra=True), {}, "cfg.use_depth_only_intra = False"),
            (dict(), dict(grad_sync=lambda: None), "grad_sync")]


@pytest.mark.parametrize("over,kw,word", REFUSALS, ids=[r[2].replace(" ", "_") for r in REFUSALS])
def test_graphed_step_refuses_at_construction(over, kw, word):
    """Each refusal fires on a stub model before anything touches a GPU, and names the way out."""
    from depthg_amd.graph_step import GraphedTrainStep
    args = {**dict(sample_cache=object(), feature_cache=object()), **kw}
    with pytest.raises(ValueError) as e:
        GraphedTrainStep(_stub(**over), None, args.pop("sample_cache"), args.pop("feature_cache"), **args)
    assert word in str(e.value) and ("set cfg." in str(e.value) or "build a" in str(e.value) or "without dg_graph_step" in str(e.value)
                                     or "eagerly" in str(e.value)), str(e.value)


def test_capture_key_lists_what_the_decays_change():
    from depthg_amd.graph_step import CAPTURE_KEY
    for key in ("depth_feat_weight", "depth_feat_shift", "feature_samples", "depth_sampling", "pos_intra_weight", "pos_inter_weight",
                "neg_inter_weight", "correspondence_weight"):
        assert key in CAPTURE_KEY
    assert len(set(CAPTURE_KEY)) == len(CAPTURE_KEY)


def test_train_command_wants_both_caches_for_the_graph_step(capsys):
    from depthg_amd import train
    for argv in (["--data-dir", "d", "--out", "o", "--graph-step"], ["--data-dir", "d", "--out", "o", "--graph-step", "--sample-cache"],
                 ["--data-dir", "d", "--out", "o", "--graph-step", "--feature-cache", "float32"]):
        with pytest.raises(SystemExit):
            train.main(argv)
        assert "--feature-cache" in capsys.readouterr().err
