"""GraphedTrainStep (cfg.dg_graph_step): the cached training step recorded once in a hipGraph and replayed.

With both caches on the card (feature_cache.FeatureCache, sample_cache.SampleCache) a training step is about a hundred short launches
and the host that issues them is the limit.  Every piece of the step that drew on the host has a device-resident form - the batch and
its positives (epoch.DeviceEpoch), the loss's coordinates and permutations (cfg.dg_graph_safe), the three Adams' step counts
(optim.FusedAdam with `capturable`), torch's own generator for the Dropout2d masks (torch.cuda.graph registers it: a replay advances
its offset as the eager calls would) - so `DeviceEpoch.batch` + `UnsupervisedSegmenter.training_step` is recorded with torch.cuda.graph
and one replay is one step.

What a replay cannot do is the step's HOST bookkeeping - depth_decay.legacy_decay_step, which mutates cfg, and global_step += 1: the
wrapper does both behind every replay, once (an eager step does them itself, inside training_step).  The scalars a recorded step
holds as launch arguments are the cfg fields of CAPTURE_KEY; when the bookkeeping changes one of them - the reference's decays do -
the recording is dropped and made again.  Steps that cannot be a replay run eagerly through the same objects, on the same device state:
    - the first step, and the first step behind any dropped recording: it is the warm-up of the recording that follows it (every
      lazily made buffer - workspaces, optimiser state, generator states - exists before anything is recorded);
    - a cfg.hist_freq step (it launches the histogram kernel and returns three more logs);
    - the cfg.reset_probe_steps step, and the step behind it (the probes' optimisers are new: their state is made by an eager step).
`captures` counts the recordings.  A recording that fails is reported once on stderr and every later step runs eagerly; with
`strict=True` it raises.

The tensors `step()` returns behind a replay are the recording's own: the next `step()` overwrites them (clone what must be kept).
"""
import sys

import torch

from .depth_decay import legacy_decay_step
from .optim import FusedAdam
from .training import histogram_step, reset_probe_step

# The cfg fields a recorded step holds as launch arguments, shapes or branches: a change of any of them drops the recording.
CAPTURE_KEY = (
    # the loss weights and shifts (correspondence_total, the correlation loss's descriptor)
    "correspondence_weight", "pos_intra_weight", "pos_inter_weight", "neg_inter_weight", "depth_feat_weight",
    "pos_intra_shift", "pos_inter_shift", "neg_inter_shift", "depth_feat_shift", "rec_weight",
    # the sample grid and how it is drawn (legacy_decay_step changes the first two)
    "feature_samples", "depth_sampling", "dg_fps_feats", "neg_samples", "use_salience", "depth_feat_correlation_loss",
    # the loss's form
    "pointwise", "zero_clamp", "stabalize", "dropout", "dg_dense_grid", "dg_outputs", "dg_exact_masks", "dg_small_identity_blobs",
    # what the constructor refuses (set later, they are refused in front of the next recording)
    "dg_feature_cache", "dg_graph_safe", "dg_fused_adam", "arch", "lhp", "crf_weight", "aug_alignment_weight", "use_depth_only_intra")


def refuse(cfg, sample_cache, feature_cache, grad_sync=None):
    """What GraphedTrainStep cannot record, each with the way out."""
    who = "depthg_amd: GraphedTrainStep (cfg.dg_graph_step)"
    if sample_cache is None or feature_cache is None:
        missing = "a sample cache" if sample_cache is None else "a feature cache"
        raise ValueError(f"{who} needs both caches on the device and got no {missing[2:]}: build {missing} (data.build_sample_cache / "
                         "data.build_feature_cache; `--sample-cache --feature-cache float32` on the train command) or train without dg_graph_step")
    for key, how in (("dg_feature_cache", "set cfg.dg_feature_cache to the cache's storage type: a recorded step starts behind the backbone"),
                     ("dg_graph_safe", "set cfg.dg_graph_safe = True: the loss's coordinates and permutations must come from the device-resident generator"),
                     ("dg_fused_adam", "set cfg.dg_fused_adam = True: torch.optim.Adam's step counts live on the host")):
        if not getattr(cfg, key, None):
            raise ValueError(f"{who} needs cfg.{key}: {how}")
    if getattr(cfg, "arch", "dino") == "dino_depth":
        raise ValueError(f"{who} serves cfg.arch = 'dino': the depth-guided featurizer (arch 'dino_depth') has no feature cache; train it "
                         "without dg_graph_step")
    if getattr(cfg, "lhp", False):
        raise ValueError(f"{who} cannot record cfg.lhp: the LHP module's draws are torch's own on the host's schedule; set cfg.lhp = False or train "
                         "without dg_graph_step")
    for key in ("crf_weight", "aug_alignment_weight"):
        if getattr(cfg, key, 0) > 0:
            raise ValueError(f"{who} cannot record cfg.{key} > 0: the term's draws are made on the host (a replay would repeat them); set "
                             f"cfg.{key} = 0 or train without dg_graph_step")
    if getattr(cfg, "use_depth_only_intra", False):
        raise ValueError(f"{who} cannot record cfg.use_depth_only_intra (DepthContrastiveCorrelationLoss does not run under cfg.dg_graph_safe); set "
                         "cfg.use_depth_only_intra = False or train without dg_graph_step")
    if getattr(cfg, "use_true_labels", False):
        raise ValueError(f"{who} cannot record cfg.use_true_labels: the one-hot label signal is a diagnostic route the recorded step does not "
                         "carry; set cfg.use_true_labels = False or train without dg_graph_step")
    if grad_sync is not None:
        raise ValueError(f"{who} records one GPU's step: a `grad_sync` (data parallelism) is out of scope; call training_step(batch, grad_sync=...) "
                         "eagerly instead")


def make_capturable(model):
    """The step counts of the model's three FusedAdam onto the device (`capturable`, the torch idiom): a recorded step advances them at
    every replay.  Also what an eager run needs to be compared bit for bit with a replayed one."""
    for optim in model.optimizers():
        if not isinstance(optim, FusedAdam):
            raise ValueError("depthg_amd: GraphedTrainStep needs the model's optimisers to be optim.FusedAdam (cfg.dg_fused_adam), got "
                             f"{type(optim).__name__}")
        for group in optim.param_groups:
            group["capturable"] = True


class GraphedTrainStep:
    """GraphedTrainStep(model, epoch, sample_cache, feature_cache, strict=False)
        model           an UnsupervisedSegmenter in training mode, on the caches' device
        epoch           an epoch.DeviceEpoch over the train split's table (the caller calls its begin_epoch() per epoch)
        step()          one training step: (loss, logs) as training_step returns them
        captures        recordings made so far
        graphed         whether the last step() was a replay
    label_dims: the dataset's (4: label and mask carry a channel axis).  Refusals: `refuse`."""

    def __init__(self, model, epoch, sample_cache, feature_cache, strict=False, grad_sync=None, label_dims=3):
        refuse(model.cfg, sample_cache, feature_cache, grad_sync)
        self.model, self.epoch, self.sample_cache, self.feature_cache = model, epoch, sample_cache, feature_cache
        self.strict, self.label_dims = bool(strict), int(label_dims)
        if getattr(model, "use_depth", False) and not sample_cache.with_depth:
            raise ValueError("depthg_amd: GraphedTrainStep: the model reads depth (cfg.use_depth) but the sample cache has no depth plane: "
                             "build it with want_depth=True")
        if epoch.device.type != "cuda":
            raise RuntimeError("depthg_amd: GraphedTrainStep records a GPU step; the epoch lives on " + str(epoch.device))
        make_capturable(model)
        self.captures, self.graphed = 0, False
        self._graph = self._out = self._key = None
        self._warm = self._failed = False
        self._side = torch.cuda.Stream(device=epoch.device)

    # ---- what decides between a replay and an eager step
    def _cfgs(self):
        cfg, loss_cfg = self.model.cfg, self.model.contrastive_corr_loss_fn.cfg
        return (cfg,) if loss_cfg is cfg else (cfg, loss_cfg)

    def capture_key(self):
        # (cfg.dg_fused_probes decides launches too, but the segmenter reads it once, at construction: its attribute is the key)
        return tuple(getattr(c, k, None) for c in self._cfgs() for k in CAPTURE_KEY) + \
            (bool(self.model.training), bool(self.model.net.training), bool(getattr(self.model, "fused_probes", False)))

    def _forced_eager(self, global_step):
        return histogram_step(self.model.cfg, global_step) or self._reset_step(global_step)

    def _reset_step(self, global_step):
        return reset_probe_step(self.model.cfg, global_step)

    # ---- the step itself, as both routes run it
    def _run(self):
        m = self.model
        batch = self.epoch.batch(self.sample_cache, self.feature_cache, label_dims=self.label_dims, return_depth=bool(m.use_depth))
        return m.training_step(batch, 0)

    def _eager(self):
        cur = torch.cuda.current_stream(self.epoch.device)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            out = self._run()
        cur.wait_stream(self._side)
        return out

    def _capture(self):
        """Record `_run` for the cfg now in force.  Recording executes nothing on the device but runs the step's Python: the host state
        it moves - global_step, the cfg fields the decays mutate, the epoch's count - is put back."""
        m = self.model
        refuse(m.cfg, self.sample_cache, self.feature_cache)
        key = self.capture_key()
        saved = [(c, dict(vars(c))) for c in self._cfgs()]
        step0, drawn0 = m.global_step, self.epoch.drawn
        self.epoch.drawn = 0                                     # (the recording itself draws nothing)
        torch.cuda.synchronize(self.epoch.device)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                out = self._run()
        except RuntimeError as e:
            self._graph = self._out = self._key = None
            self._failed = True
            torch.cuda.synchronize(self.epoch.device)
            if self.strict:
                raise
            print(f"depthg_amd: GraphedTrainStep: recording the step failed ({str(e).splitlines()[0] if str(e) else type(e).__name__}); "
                  "every step runs eagerly from here on", file=sys.stderr)
            return
        finally:
            for c, fields in saved:
                vars(c).clear()
                vars(c).update(fields)
            m.global_step, self.epoch.drawn = step0, drawn0
        self._graph, self._out, self._key = graph, out, key
        self.captures += 1

    def _valid(self):
        return self._graph is not None and self._key == self.capture_key()

    def step(self):
        m = self.model
        if self._failed or not self._valid() or self._forced_eager(m.global_step):
            reset = self._reset_step(m.global_step)
            out = self._eager()                                  # (training_step does the step's bookkeeping itself)
            self.graphed = False
            if reset:                                            # new probe optimisers: their state is made by the next eager step
                make_capturable(m)
                self._graph = self._out = self._key = None
            self._warm = not reset
            if not self._failed and self._warm and not self._valid() and not self._forced_eager(m.global_step):
                self._graph = self._out = self._key = None       # (a recording for other scalars is dropped before the new one is made)
                self._capture()
            return out
        self.epoch.replayed()
        self._graph.replay()
        self.graphed = True
        # the host bookkeeping the replay skipped, once: src/train_segmentation.py:356-375 (mutates cfg), then the step count
        legacy_decay_step(m.cfg, m.contrastive_corr_loss_fn.cfg, m.global_step)
        m.global_step += 1
        return self._out
