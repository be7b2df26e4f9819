"""Decision table of training.step_plan and its two step-number predicates: host logic on SimpleNamespace configurations and a stub
net - no GPU, no library."""
from types import SimpleNamespace

import pytest

from depthg_amd import graph_step, training
from depthg_amd.training import histogram_step, reset_probe_step, step_plan

# the keys the reference always has (read as attributes) and nothing else: every optional key is absent
REQUIRED = dict(correspondence_weight=1.0, use_salience=False, depth_feat_correlation_loss=True, reset_probe_steps=None)
# today's absent-key defaults of the optional keys the plan reads
DEFAULTS = dict(lhp=False, hist_freq=None, dg_hist_bins=64, rec_weight=0, aug_alignment_weight=0, crf_weight=0, dg_rec_feats_grad=False,
                dg_gpu_augment=False, dg_fused_adam=False, dg_feature_cache=None)
FEATS = {"img": 0, "img_pos": 0, "image_feat": 0, "image_feat_pos": 0}


def cfg(**over):
    return SimpleNamespace(**{**REQUIRED, **over})


def net(pair=True, features=True, training=True):
    n = SimpleNamespace(training=training)
    if pair:
        n.forward_pair = None
    if features:
        n.forward_pair_features = None
    return n


def plan(c, n=None, batch=FEATS, depth_arch=False, depth_only_intra=False, global_step=0):
    return step_plan(c, net=n or net(), batch=batch, depth_arch=depth_arch, depth_only_intra=depth_only_intra, global_step=global_step)


@pytest.mark.parametrize("over,net_kw,depth_arch,route", [
    ({}, {}, False, "pair"),
    ({"lhp": True}, {}, False, "single"),                       # the LHP module draws between the passes
    ({"correspondence_weight": 0.0}, {}, False, "single"),      # no positive pass at all
    ({}, {"pair": False}, False, "single"),                     # the featurizer does not offer both passes at once
    ({}, {"training": False}, False, "single"),
    ({}, {}, True, "depth"),
    ({"lhp": True}, {}, True, "depth"),
    ({"correspondence_weight": 0.0}, {"pair": False, "training": False}, True, "depth"),
])
def test_route(over, net_kw, depth_arch, route):
    p = plan(cfg(**over), net(**net_kw), depth_arch=depth_arch)
    assert p.route == route and p.route in ("pair", "depth", "single")
    assert p.correspondence == (over.get("correspondence_weight", 1.0) > 0) and p.lhp == over.get("lhp", False)


@pytest.mark.parametrize("key,batch,net_kw,depth_arch,cached", [
    ("float32", FEATS, {}, False, True),
    (None, FEATS, {}, False, False),
    ("absent", FEATS, {}, False, False),
    ("float16", {"img": 0, "image_feat": 0}, {}, False, False),            # one of the two batch keys is not enough
    ("float16", {"img": 0, "image_feat_pos": 0}, {}, False, False),
    ("float32", FEATS, {"features": False}, False, False),                 # the featurizer cannot start behind its backbone
    ("float32", FEATS, {}, True, False),                                   # the depth-guided featurizer has no feature cache
])
def test_cached(key, batch, net_kw, depth_arch, cached):
    c = cfg() if key == "absent" else cfg(dg_feature_cache=key)
    for lhp in (False, True):                                               # both the pair and the single route start from the cache
        c.lhp = lhp
        assert plan(c, net(**net_kw), batch=batch, depth_arch=depth_arch).cached is cached


def test_absent_keys_give_the_plan_of_todays_defaults():
    for over in ({}, {"correspondence_weight": 0.0}, {"reset_probe_steps": 3}):
        for depth_arch in (False, True):
            for step in (0, 3):
                assert plan(cfg(**over), depth_arch=depth_arch, global_step=step) == \
                    plan(cfg(**DEFAULTS, **over), depth_arch=depth_arch, global_step=step)
    p = plan(cfg())
    assert (p.hist_bins, p.rec, p.aug, p.crf, p.rec_feats_grad, p.gpu_augment, p.fused_adam, p.histograms, p.reset_probes) == \
        (64, False, False, False, False, None, False, False, False)
    assert p.depth_term is True and p.use_salience is False and p.depth_only_intra is False
    assert p._fields == training.StepPlan._fields and len(p) == 16


def test_switches_follow_their_keys():
    p = plan(cfg(rec_weight=0.5, aug_alignment_weight=0.1, crf_weight=2, dg_rec_feats_grad=True, dg_fused_adam=True, dg_hist_bins=32,
                 use_salience=True, depth_feat_correlation_loss=False), depth_only_intra=True)
    assert (p.rec, p.aug, p.crf, p.rec_feats_grad, p.fused_adam, p.hist_bins, p.use_salience, p.depth_term, p.depth_only_intra) == \
        (True, True, True, True, True, 32, True, False, True)
    assert [plan(cfg(dg_gpu_augment=v)).gpu_augment for v in (False, None, 0, True, "unit", "given", "anything", 1)] == \
        [None, None, None, "given", "unit", "given", "given", "given"]
    # under correspondence_weight = 0 nothing reads the salience masks or the depth term
    off = plan(cfg(correspondence_weight=0.0, use_salience=True))
    assert off.use_salience is False and off.depth_term is False


def test_histogram_step():
    f = 4
    assert [histogram_step(cfg(hist_freq=f), s) for s in (0, f, f + 1, 2 * f)] == [False, True, False, True]
    assert not any(histogram_step(cfg(hist_freq=None), s) for s in (0, f, f + 1))
    assert not any(histogram_step(cfg(), s) for s in (0, f, f + 1))                                       # the key is absent
    assert not any(histogram_step(cfg(hist_freq=f, correspondence_weight=0.0), s) for s in (0, f, f + 1))
    assert [histogram_step(cfg(hist_freq=1), s) for s in (0, 1, 2)] == [False, True, True]
    assert [plan(cfg(hist_freq=f), global_step=s).histograms for s in (0, f, f + 1)] == [False, True, False]


def test_reset_probe_step():
    assert [reset_probe_step(cfg(reset_probe_steps=5), s) for s in (4, 5, 6)] == [False, True, False]
    assert not any(reset_probe_step(cfg(reset_probe_steps=None), s) for s in (0, 4, 5))
    assert reset_probe_step(cfg(reset_probe_steps=0), 0)
    assert [plan(cfg(reset_probe_steps=5), global_step=s).reset_probes for s in (4, 5, 6)] == [False, True, False]


def test_graph_step_imports_the_predicates():
    assert graph_step.histogram_step is training.histogram_step and graph_step.reset_probe_step is training.reset_probe_step
    stepper = SimpleNamespace(model=SimpleNamespace(cfg=cfg(hist_freq=4, reset_probe_steps=5)))
    stepper._reset_step = lambda s: graph_step.GraphedTrainStep._reset_step(stepper, s)
    assert [graph_step.GraphedTrainStep._forced_eager(stepper, s) for s in (0, 3, 4, 5, 6, 8)] == [False, False, True, True, False, True]
