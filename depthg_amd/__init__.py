"""depthg_amd - MI355X (gfx950) implementation of DepthG's feature-correlation loss hot path.

Public surface (mirrors the reference's Python operator surface for this path):
    ContrastiveCorrelationLoss   drop-in for src/modules.py:1221-1367; .cd_histograms(): the cd histograms of its last call without
                                 the un-reduced tensors (ops.corr_cd_hist; cfg.hist_freq / cfg.dg_hist_bins in the segmenter)
    DepthContrastiveCorrelationLoss  src/modules.py:1370-1463: the same loss with the intra pair-set's feature correlation taken from the
                                 depth-augmented features (cfg.use_depth_only_intra in the segmenter); one launch set (dg_corr_forward_intra_feats)
    ContrastiveCRFLoss           src/modules.py:1510-1542: forward() the reference's (B,n,n) tensor in plain torch, mean_loss() the training
                                 step's `crf_loss_fn(resize(img, 56), norm(resize(code, 56))).mean()` as fused HIP kernels (cfg.crf_weight)
    aug_alignment_loss           src/train_segmentation.py:400-411: the augmentation-alignment term as fused HIP kernels (cfg.aug_alignment_weight);
                                 aug_loss.crop_flip_coords makes a valid coord_aug (the crop-and-flip of the dataset's grid)
    augment_batch                src/data.py:1082-1139: img_aug and coord_aug of a batch from two fused HIP kernels (augment.py,
                                 draw_augment_params; cfg.dg_gpu_augment in the segmenter)
    reconstruction_loss          src/train_segmentation.py:391-398: the reconstruction term - the 1 x 1 decoder and both norms - as fused HIP
                                 kernels (cfg.rec_weight); no (B, n_feats, h, w) tensor is written in either direction
    depth_decay                  scalar decay schedules (src/depth_decay_modules.py) + the live legacy decay
    training                     the caller arithmetic around the loss (means, weighted total, log keys;
                                 src/train_segmentation.py:240-350)
    metrics                      UnsupervisedMetrics (src/utils.py:202-319): confusion matrix on the GPU, summed over DP ranks
    evaluation                   predict_and_score: the probes' predictions at label resolution and their confusion counts
                                 (src/train_segmentation.py:471-499, src/eval_segmentation.py:146-170, run_crf for the CRF);
                                 segment: label-free inference (src/demo_segmentation.py:59-78) - byte label maps and painted
                                 images of every image from one fused HIP launch pair; `python -m depthg_amd.demo` is its command line
    crf                          dense_crf / batched_crf (src/crf.py, src/eval_segmentation.py:55-60): mean-field dense CRF in HIP
    knn                          image-level nearest-neighbour table: search, file format, online pick (src/precompute_knns.py)
    lhp                          LocalHiddenPositiveProjection with depth propagation (src/modules.py:140-339)
    segmenter                    the producers and the caller: projection head, stand-in featurizer, cluster probe, one optimisation
                                 step of LitUnsupervisedSegmenter (src/modules.py:19-137,647-675; src/train_segmentation.py:71-462)
    optim                        FusedAdam / FusedAdamSet: the step's three torch.optim.Adam (src/train_segmentation.py:447-455,537-547)
                                 as one HIP launch, torch's state layout (cfg.dg_fused_adam in the segmenter)
    vit                          the DINO vision transformer (src/dino/vision_transformer.py:68-280) on torch, checkpoint-compatible;
                                 its attention optionally through the fused HIP kernel k_attn_fwd (cfg.dg_fused_attention)
                                 and its blocks' linear layers, LayerNorms, GELU and residual adds through the bf16 MFMA kernel
                                 k_lin_fwd (cfg.dg_fused_linear)
    featurizer / DinoFeaturizer  src/modules.py:19-137: frozen ViT + the fused projection head (cfg.dg_dino_backbone in the segmenter);
                                 DinoFeaturizerWithDepth (:490-631, cfg.arch "dino_depth"): depth-guided features in front of the head
    cross_attn                   the depth guidance's nn.MultiheadAttention core (src/modules.py:524, :566-585) as a fused HIP forward
                                 and backward with Philox dropout (cfg.dg_fused_cross_attn)
    data                         the training data path (src/data.py:87-132, 815-912, 1073-1141; src/utils.py:164-182): CroppedFolder /
                                 DirectoryFolder, loader_index_tables, ContrastiveBatches - the loader transform of a batch and its kNN
                                 positives as ONE fused HIP launch (ops.batch_prep, k_batch_prep) - and precompute_knns
    feature_cache / FeatureCache the frozen backbone's image_feat of every train image (src/modules.py:90-137), stored once as float32,
                                 float16 or bfloat16 and gathered per batch and positives in ONE HIP launch (k_fc_put / k_fc_gather);
                                 data.build_feature_cache fills it, cfg.dg_feature_cache makes the step start from it
                                 (src/train_segmentation.py:194-212 without the two backbone passes)
    sample_cache / SampleCache   the loader transform's output bytes of every image, label and depth map of a split on the device; a batch
                                 and its positives come back as img / label / mask / depth from ONE launch (k_sc_gather), no decoding:
                                 data.build_sample_cache fills it, ContrastiveBatches(sample_cache=...) reads it
    epoch / DeviceEpoch          the batches of a cached epoch chosen on the device (src/data.py:1073-1080): indices from the epoch's order,
                                 kNN positives from Philox, ONE launch (ops.epoch_draw, k_epoch_draw), then the two caches' gathers
    graph_step / GraphedTrainStep  cfg.dg_graph_step: DeviceEpoch.batch + training_step recorded once in a hipGraph and replayed; the
                                 host bookkeeping (legacy decay, step count) behind every replay, a new recording when it changes a scalar
    train                        fit(model, train_batches, val_batches, cfg, out_dir): the loop of src/train_segmentation.py:551-714 without
                                 Lightning; `python -m depthg_amd.train` is its command line
    ops                          thin ctypes binding of the C ABI in include/depthg_corr.h; ops.corr_forward is the one route to its five
                                 forward entries (keep / feat_inv / intra_feats select one; perms=None draws the batch maps)
"""
from .loss import ContrastiveCorrelationLoss, DepthContrastiveCorrelationLoss  # noqa: F401
from . import crf_loss  # noqa: F401
from .crf_loss import ContrastiveCRFLoss  # noqa: F401
from . import aug_loss  # noqa: F401
from .aug_loss import aug_alignment_loss, crop_flip_coords  # noqa: F401
from . import augment  # noqa: F401
from .augment import AugmentParams, augment_batch, draw_augment_params  # noqa: F401
from . import rec_loss  # noqa: F401
from .rec_loss import reconstruction_loss  # noqa: F401
from .depth_encoder import depth_encoder  # noqa: F401
from . import cross_attn  # noqa: F401
from .cross_attn import cross_attention, multihead_cross_attention  # noqa: F401
from . import depth_decay  # noqa: F401
from . import training  # noqa: F401
from . import metrics  # noqa: F401
from . import evaluation  # noqa: F401
from .evaluation import predict_and_score, segment  # noqa: F401
from . import crf  # noqa: F401
from .crf import batched_crf, dense_crf  # noqa: F401
from . import knn  # noqa: F401
from . import lhp  # noqa: F401
from . import optim  # noqa: F401
from .optim import FusedAdam, FusedAdamSet  # noqa: F401
from . import vit  # noqa: F401
from . import featurizer  # noqa: F401
from .featurizer import DinoFeaturizer, DinoFeaturizerWithDepth  # noqa: F401
from . import segmenter  # noqa: F401
from . import data  # noqa: F401
from .data import ContrastiveBatches, CroppedFolder, DirectoryFolder, loader_index_tables, precompute_knns  # noqa: F401
from . import feature_cache  # noqa: F401
from .feature_cache import FeatureCache  # noqa: F401
from .data import build_feature_cache  # noqa: F401
from . import sample_cache  # noqa: F401
from .sample_cache import SampleCache  # noqa: F401
from .data import build_sample_cache  # noqa: F401
from . import epoch  # noqa: F401
from .epoch import DeviceEpoch  # noqa: F401
from . import graph_step  # noqa: F401
from .graph_step import GraphedTrainStep  # noqa: F401

__all__ = ["ContrastiveCorrelationLoss", "DepthContrastiveCorrelationLoss", "ContrastiveCRFLoss", "crf_loss", "aug_loss", "aug_alignment_loss", "crop_flip_coords", "augment", "AugmentParams", "augment_batch", "draw_augment_params", "rec_loss", "reconstruction_loss", "depth_encoder", "cross_attn", "cross_attention", "multihead_cross_attention", "depth_decay", "training", "metrics", "evaluation", "predict_and_score", "segment", "crf", "dense_crf",
           "batched_crf", "knn", "lhp", "optim", "FusedAdam", "FusedAdamSet", "segmenter", "vit", "featurizer",
           "DinoFeaturizer", "DinoFeaturizerWithDepth", "data", "ContrastiveBatches", "CroppedFolder", "DirectoryFolder",
           "loader_index_tables", "precompute_knns", "feature_cache", "FeatureCache", "build_feature_cache",
           "sample_cache", "SampleCache", "build_sample_cache", "epoch", "DeviceEpoch", "graph_step", "GraphedTrainStep"]
