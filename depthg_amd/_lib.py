"""ctypes loader for libdepthg_hip.so (C ABI: include/depthg_corr.h).  Fails loudly when the
library is missing: there is no CPU or eager fallback for the product path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEPTHG_LIB") or os.path.join(_HERE, "lib", "libdepthg_hip.so")   # DEPTHG_LIB: developer A/B builds

DG_OUT_COUNT = 9
DG_OUT_TOTAL = 8
DG_VERSION = 119                     # must match include/depthg_corr.h: a stale library is refused
DG_POINTWISE, DG_ZERO_CLAMP, DG_STABALIZE, DG_DEPTH_TERM, DG_NEED_GRAD, DG_SHARED_COORDS, DG_IDENTITY_GRID, DG_LINE_GRID, \
    DG_EXACT_MASKS, DG_FEATS_UNIT = (1 << i for i in range(10))
DG_LIN_LAYERNORM, DG_LIN_GELU, DG_LIN_IN_BF16, DG_LIN_OUT_BF16 = 1, 2, 4, 8      # dg_vit_linear_forward flags
DG_FC_F32, DG_FC_F16, DG_FC_BF16 = 0, 1, 2                                        # dg_featcache_put / _gather storage types

class CorrDesc(ctypes.Structure):
    """struct dg_corr_desc"""
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("D", ctypes.c_int32), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("S", ctypes.c_int32), ("n_neg", ctypes.c_int32),
                ("depth_h", ctypes.c_int32), ("depth_w", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("shift_intra", ctypes.c_float), ("shift_inter", ctypes.c_float), ("shift_neg", ctypes.c_float),
                ("shift_depth", ctypes.c_float),
                ("w_intra", ctypes.c_float), ("w_inter", ctypes.c_float), ("w_neg", ctypes.c_float),
                ("w_depth", ctypes.c_float), ("code_h", ctypes.c_int32), ("code_w", ctypes.c_int32)]


class AdamSeg(ctypes.Structure):
    """struct dg_adam_seg"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step_dev", ctypes.c_void_p), ("numel", ctypes.c_int64), ("step_host", ctypes.c_double), ("group", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class AdamGroup(ctypes.Structure):
    """struct dg_adam_group"""
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double)]


_I, _SZ, _STR = ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p
vp, cp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.POINTER(CorrDesc), ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float

# name -> (restype, argtypes): every prototype of include/depthg_corr.h, in the header's order (tests/test_host_cpu.py holds the two
# against each other, parameter by parameter).  vp: any pointer and dg_stream_t; the last vp of most entries is the stream.
SIGNATURES = {
    "dg_version": (_I, []),
    "dg_last_error": (_STR, []),
    # correlation loss
    "dg_corr_workspace_bytes": (_SZ, [cp]),
    "dg_corr_forward": (_I, [cp] + [vp] * 9 + [vp, _SZ, vp]),
    "dg_corr_forward_draw": (_I, [cp] + [vp] * 8 + [u64, vp, vp, vp, _SZ, vp]),
    "dg_corr_forward_masked": (_I, [cp] + [vp] * 8 + [i32, u64, vp, vp, vp, f32, vp, vp, _SZ, vp]),
    "dg_corr_workspace_bytes_intra_feats": (_SZ, [cp]),
    "dg_corr_forward_intra_feats": (_I, [cp] + [vp] * 8 + [i32, u64, vp, vp, vp, vp, _SZ, vp]),
    "dg_corr_backward": (_I, [cp] + [vp] * 6 + [vp, _SZ, vp]),
    "dg_corr_backward_total": (_I, [cp] + [vp] * 6 + [vp, _SZ, vp]),
    "dg_corr_materialize": (_I, [cp, i32, vp, vp, vp, _SZ, vp]),
    "dg_corr_materialize_shared": (_I, [cp, i32, vp, vp, vp, vp, _SZ, vp]),
    "dg_corr_cd_hist": (_I, [cp, i32, i32, vp, i32, f32, f32, vp, vp, _SZ, vp]),
    # samplers
    "dg_fps_workspace_bytes": (_SZ, [i32] * 3),
    "dg_fps_coords": (_I, [vp, vp] + [i32] * 6 + [vp, vp, vp, _SZ, vp]),
    "dg_fps_feats_workspace_bytes": (_SZ, [i32] * 3),
    "dg_fps_feats_coords": (_I, [vp] * 4 + [i32] * 7 + [vp, vp, vp, _SZ, vp]),
    "dg_fps_large_workspace_bytes": (_SZ, [i32] * 3),
    "dg_fps_coords_large": (_I, [vp, vp] + [i32] * 6 + [vp, vp, vp, _SZ, vp]),
    "dg_label_onehot": (_I, [vp, vp] + [i32] * 4 + [vp, vp]),
    "dg_sample_rows": (_I, [vp] * 3 + [i32] * 8 + [vp, vp]),
    "dg_salience_coords": (_I, [vp] + [i32] * 4 + [vp] * 4),
    "dg_simple_depth_coords": (_I, [vp] + [i32] * 6 + [vp] * 4),
    # metrics, LHP, nearest neighbours
    "dg_confusion_update": (_I, [vp, vp, i64, i32, i32, vp, vp]),
    "dg_lhp_forward": (_I, [vp, vp] + [i32] * 6 + [vp] * 4),
    "dg_lhp_backward": (_I, [vp] * 3 + [i32] * 4 + [vp, vp]),
    "dg_lhp_map_forward": (_I, [i32] + [vp] * 4 + [i32] * 7 + [vp] * 4),
    "dg_lhp_map_backward": (_I, [i32] + [vp] * 3 + [i32] * 4 + [vp, vp]),
    "dg_knn_similarities": (_I, [vp, vp, i64, i64, i32, i64, i64, vp, i64, vp]),
    "dg_topk_rows": (_I, [vp, i64, i64, i64, i32, vp, vp, vp]),
    # random draws
    "dg_super_perms": (_I, [vp, u64, vp, i32, i32, vp, vp]),
    "dg_rand_coords_state": (_I, [vp, i64, vp, vp]),
    "dg_rand_keep_state": (_I, [vp, i64, f32, vp, vp]),
    # wide feature maps
    "dg_normalize_split": (_I, [i32] * 4 + [vp, i32, i32, ctypes.POINTER(vp), vp]),
    "dg_sampled_sumsq": (_I, [i32] * 6 + [vp, vp, vp, i32, vp, vp]),
    "dg_corr_forward_extnorm": (_I, [cp] + [vp] * 10 + [vp, _SZ, vp]),
    # head and probes
    "dg_head_weights_bytes": (_SZ, [i32] * 2),
    "dg_head_forward": (_I, [i32] * 4 + [vp] * 11 + [f32] + [vp] * 7),
    "dg_head_workspace_bytes": (_SZ, [i32] * 4),
    "dg_head_backward": (_I, [i32] * 4 + [vp] * 4 + [f32] + [vp] * 11 + [_SZ, vp]),
    "dg_head_input_workspace_bytes": (_SZ, [i32] * 2),
    "dg_head_backward_input": (_I, [i32] * 4 + [vp] * 5 + [f32] + [vp] * 6 + [_SZ, vp, vp, vp, _SZ, vp]),
    "dg_head_plan_describe": (_I, [i32] * 4 + [vp]),
    "dg_cluster_lookup_forward": (_I, [vp, vp, f32] + [i32] * 4 + [vp] * 6),
    "dg_cluster_lookup_backward": (_I, [vp, vp, vp, f32, vp] + [i32] * 4 + [vp] * 4),
    "dg_probe_ce_forward": (_I, [vp, vp] + [i32] * 6 + [vp] * 3),
    "dg_probe_ce_backward": (_I, [vp] * 4 + [i32] * 6 + [vp] * 2),
    "dg_probe_step_workspace_bytes": (_SZ, [i32] * 8),
    "dg_probe_step_forward": (_I, [vp] * 5 + [i32] * 8 + [vp, vp, _SZ, vp]),
    "dg_probe_step_backward": (_I, [vp, _SZ, vp, vp] + [i32] * 8 + [vp] * 4),
    # evaluation and dense CRF
    "dg_segment_predict": (_I, [vp, vp] + [i32] * 4 + [vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, _SZ, vp]),
    "dg_segment_labels": (_I, [vp, vp] + [i32] * 4 + [vp, vp, i32, vp] + [i32] * 3 + [vp] * 5 + [i32, i32] + [vp] * 4 + [vp, _SZ, vp]),
    "dg_label_paint": (_I, [vp] + [i32] * 5 + [vp] * 5 + [i32, i32] + [vp] * 4 + [vp]),
    "dg_crf_workspace_bytes": (_SZ, [i32] * 5),
    "dg_crf_unary": (_I, [vp] + [i32] * 6 + [vp, i32, vp, vp]),
    "dg_segment_unary": (_I, [vp, vp] + [i32] * 4 + [vp, vp, i32, vp, i32, i32, i32, f32, vp, vp, _SZ, vp]),
    "dg_crf_filter": (_I, [vp, vp] + [i32] * 5 + [f32, f32, vp, vp, _SZ, vp]),
    "dg_dense_crf": (_I, [vp, vp] + [i32] * 3 + [vp, i32, i32] + [f32] * 5 + [vp, vp, vp, _SZ, vp]),
    # contrastive CRF loss term
    "dg_crfloss_workspace_bytes": (_SZ, [i32] * 3),
    "dg_crfloss_forward": (_I, [vp, vp] + [i32] * 7 + [vp, i32] + [f32] * 6 + [vp, _SZ, vp, vp]),
    "dg_crfloss_backward": (_I, [vp, _SZ, vp] + [i32] * 6 + [vp, vp, vp]),
    # augmentation-alignment loss term
    "dg_augalign_workspace_bytes": (_SZ, [i32] * 5),
    "dg_augalign_forward": (_I, [vp] * 3 + [i32] * 7 + [vp, _SZ, vp, vp]),
    "dg_augalign_backward": (_I, [vp, vp, vp, _SZ] + [i32] * 5 + [vp] * 4),
    # reconstruction loss term
    "dg_recloss_workspace_bytes": (_SZ, [i32] * 5),
    "dg_recloss_forward": (_I, [vp] * 5 + [f32] + [i32] * 5 + [vp, _SZ, vp, vp]),
    "dg_recloss_backward": (_I, [vp] * 5 + [f32, vp, _SZ] + [i32] * 5 + [vp] * 5),
    "dg_rec_feats_backward": (_I, [vp] * 5 + [f32, vp, _SZ] + [i32] * 5 + [vp] * 6),
    # optimiser
    "dg_adam_step": (_I, [ctypes.POINTER(AdamSeg), i32, ctypes.POINTER(AdamGroup), i32, i32, vp, vp]),
    # frozen ViT
    "dg_attention_workspace_bytes": (_SZ, [i32] * 3),
    "dg_attention_forward": (_I, [vp] + [i32] * 4 + [f32, vp, vp, _SZ, vp]),
    "dg_vit_linear_packed_bytes": (_SZ, [i32] * 2),
    "dg_vit_linear_pack": (_I, [vp, i32, i32, vp, vp]),
    "dg_vit_linear_forward": (_I, [vp, vp, vp, f32, vp, vp, vp, vp] + [i32] * 4 + [vp]),
    # depth encoder
    "dg_depthenc_workspace_bytes": (_SZ, [i32] * 5),
    "dg_depthenc_forward": (_I, [vp] * 12 + [i32] * 8 + [vp, vp, _SZ, vp]),
    "dg_depthenc_backward": (_I, [vp] * 12 + [i32] * 6 + [vp] * 11 + [_SZ, vp]),
    # depth guidance: fused cross-attention
    "dg_xattn_workspace_bytes": (_SZ, [i32] * 5),
    "dg_xattn_forward": (_I, [vp] * 3 + [i32] * 5 + [f32, f32, u64, vp, vp, vp, _SZ, vp]),
    "dg_xattn_backward": (_I, [vp] * 6 + [i32] * 5 + [f32, f32, u64, vp, vp, vp, vp, _SZ, vp]),
    "dg_xattn_keep_mask": (_I, [u64] + [i32] * 4 + [f32, vp, vp]),
    # GPU batch augmentation
    "dg_augment_workspace_bytes": (_SZ, [i32] * 3),
    "dg_augment_forward": (_I, [vp] + [i64] * 4 + [vp] * 4 + [i32] * 6 + [vp, vp, vp, _SZ, vp]),
    # batch preparation
    "dg_batch_prep": (_I, [vp, _SZ, vp, vp, vp] + [i32] * 4 + [vp] * 7),
    # frozen-backbone feature cache
    "dg_featcache_put": (_I, [vp, i32, i64, i64, vp, vp, i64, vp]),
    "dg_featcache_gather": (_I, [vp, i32, i64, i64, vp, vp, i64, vp, vp]),
    # device-resident sample cache
    "dg_samplecache_put": (_I, [vp, i64] + [i32] * 4 + [vp, i32, vp, _SZ, vp, vp, vp, i32, vp]),
    "dg_samplecache_gather": (_I, [vp, i64] + [i32] * 4 + [vp, vp, i32, vp, vp] + [i32] * 3 + [vp] * 5),
    # the batch draw of a cached step
    "dg_epoch_draw": (_I, [vp, vp, vp, i32, i32, i64, i32, vp, vp, vp]),
    # measurement aids
    "dg_corr_main_kernel_name": (_STR, [cp]),
    "dg_corr_intra_folded": (_I, [cp]),
    "dg_prof_main_span": (_I, [vp]),
    "dg_corr_relaunch_main": (_I, [cp, vp, vp, _SZ, vp]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"depthg_amd: {LIB_PATH} not found. Build it with `make -C depthg_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.dg_version.restype = _I
    if lib.dg_version() != DG_VERSION:
        raise RuntimeError(f"depthg_amd: {LIB_PATH} is version {lib.dg_version()}, the Python layer expects {DG_VERSION}; "
                           "rebuild it with `make -C depthg_amd/csrc`")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().dg_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"depthg_amd: {what} failed ({rc}): {msg}")
