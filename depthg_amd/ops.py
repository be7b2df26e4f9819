"""Tensor-level wrappers over the C ABI (raw device pointers + the current HIP stream).
torch is used for device memory and streams only."""
import collections
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import CorrDesc


# Test hook (tests/test_gpu_poison.py, DG_POISON=1): every buffer this layer hands to the library - the workspace and all
# outputs - is pre-filled with 0xFF bytes (a NaN pattern for fp32/fp16, -1 for integers), so that a kernel that reads a
# byte it (or an earlier kernel of the call) has not written shows up as NaN instead of depending on recycled memory.
POISON = os.environ.get("DG_POISON", "") not in ("", "0")


def _empty(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    if POISON and t.numel():
        t.reshape(-1).view(torch.uint8).fill_(0xFF)
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    """Current stream of `device`, as the C ABI wants it.  The library launches on the CURRENT HIP device and keys its
    kernel-attribute cache on it: a call with tensors of another device would run on a foreign stream - refuse it."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"depthg_amd: tensors must live on the GPU (got {device}); there is no CPU path")
    cur = torch.cuda.current_device()
    if device.index is not None and device.index != cur:
        raise RuntimeError(f"depthg_amd: tensors live on cuda:{device.index} but the current device is cuda:{cur}; "
                           f"call under `with torch.cuda.device({device.index}):` (one process per GPU sets it once)")
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _on_gpu(t, name):
    """The product path has no CPU route: a tensor anywhere else is refused by name."""
    if not t.is_cuda:
        raise RuntimeError(f"depthg_amd: `{name}` must live on the GPU (got {t.device}); there is no CPU path")
    return t


def _f32c(t, name):
    """`t` as the library reads it - detached, fp32, contiguous, on the GPU (None stays None)."""
    return None if t is None else _on_gpu(t, name).detach().to(torch.float32).contiguous()


def _check_state(state, who, device=None):
    """`state` must be new_perm_state's int64[3] generator words, on `device` when one is named, else on any GPU."""
    placed = state.is_cuda if device is None else state.device == device
    if state.dtype != torch.int64 or state.numel() != 3 or not placed:
        raise ValueError(f"{who}: state must be the int64[3] tensor of new_perm_state on " + ("the same device" if device is not None else "the GPU"))


def _cpu_seed():
    """A 62-bit seed from torch's CPU generator: torch.manual_seed fixes every draw keyed by it, and no device RNG launch is needed."""
    return int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())


def make_desc(B, C, D, h, w, S, n_neg, *, pointwise, zero_clamp, stabalize, depth_term, need_grad, shared_coords,
              shifts, depth_hw=(0, 0), identity_grid=False, weights=(0.0, 0.0, 0.0, 0.0), line_grid=False, code_hw=None,
              exact_masks=False, feats_unit=False):
    """dg_corr_desc.  (h, w): the feature maps; code_hw: the code maps' size when it differs (None: the same)."""
    flags = 0
    flags |= _lib.DG_POINTWISE if pointwise else 0
    flags |= _lib.DG_ZERO_CLAMP if zero_clamp else 0
    flags |= _lib.DG_STABALIZE if stabalize else 0
    flags |= _lib.DG_DEPTH_TERM if depth_term else 0
    flags |= _lib.DG_NEED_GRAD if need_grad else 0
    flags |= _lib.DG_SHARED_COORDS if shared_coords else 0
    flags |= _lib.DG_IDENTITY_GRID if identity_grid else 0
    flags |= _lib.DG_LINE_GRID if line_grid else 0
    flags |= _lib.DG_EXACT_MASKS if exact_masks else 0
    flags |= _lib.DG_FEATS_UNIT if feats_unit else 0
    ch, cw = (int(code_hw[0]), int(code_hw[1])) if code_hw is not None and tuple(code_hw) != (h, w) else (0, 0)
    return CorrDesc(B, C, D, h, w, S, n_neg, int(depth_hw[0]), int(depth_hw[1]), flags,
                    float(shifts[0]), float(shifts[1]), float(shifts[2]), float(shifts[3]),
                    float(weights[0]), float(weights[1]), float(weights[2]), float(weights[3]), ch, cw)


BLOB_MAX_C = 768          # feature channels the blob kernels (grids above 160 positions, the identity grid) hold per call


def normalize_split(feats, chunk_c):
    """norm() of the reference over all channels of (B,C,h,w), returned as contiguous channel chunks of `chunk_c` (the last: the
    rest) - the operands of DG_FEATS_UNIT calls (dg_normalize_split)."""
    feats = _f32c(feats, "feats")
    B, C, h, w = feats.shape
    n = (C + chunk_c - 1) // chunk_c
    outs = [_empty((B, min(chunk_c, C - k * chunk_c), h, w), torch.float32, feats.device) for k in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    _lib.check(_lib.load().dg_normalize_split(B, C, h, w, _ptr(feats), n, chunk_c, ptrs, _stream(feats.device)), "dg_normalize_split")
    return outs


def sampled_sumsq(feats_chunk, coords, srcidx, out, accumulate):
    """out[n][p] (+)= sum over the chunk's channels of sample(feats_chunk[srcidx[n]], coords[n])^2 (dg_sampled_sumsq)."""
    B, C, h, w = feats_chunk.shape
    S, line = coords.shape[1], coords.shape[2] == 1 and coords.shape[1] != 1
    _lib.check(_lib.load().dg_sampled_sumsq(B, C, h, w, S, 1 if line else 0, _ptr(feats_chunk), _ptr(coords), _ptr(srcidx),
                                            1 if accumulate else 0, _ptr(out), _stream(feats_chunk.device)), "dg_sampled_sumsq")


def workspace_bytes(desc, intra_feats=False):
    """Bytes of workspace a forward on `desc` needs; intra_feats: the plain call's regions, then the intra feature operand's (the
    backward, cd_hist and materialize take that workspace as they take the plain one)."""
    entry = "dg_corr_workspace_bytes_intra_feats" if intra_feats else "dg_corr_workspace_bytes"
    n = getattr(_lib.load(), entry)(ctypes.byref(desc))
    if n == 0:
        _lib.check(-1, entry)
    return n


def alloc_workspace(desc, device, intra_feats=False):
    return _empty(workspace_bytes(desc, intra_feats), torch.uint8, device)


_forward_count = 0        # forwards run so far: every forward stamps its workspace tensor (`_dg_forward`), so that a reader of the
                          # operands it left there (ContrastiveCorrelationLoss.cd_histograms) can tell a workspace that was run on again


def corr_forward(desc, feats, feats_pos, code, code_pos, depth, coords1, coords2, perms, workspace=None, *,
                 draw_state=None, keep=None, feat_inv=None, intra_feats=None):
    """The forward, through the one C entry its extras select.  -> (out, perms, workspace): out fp32 [DG_OUT_COUNT] on the device
    (order: DG_OUT_* of include/depthg_corr.h); perms (n_neg, B) int64 and workspace are what backward / materialize need.
      perms None    drawn by the forward itself (on the identity grid inside its first launch): dg_corr_forward_draw, or the masked /
                    intra entry's own draw.  `draw_state` (new_perm_state) = device-resident generator (hipGraph-safe); without it the
                    seed comes from torch's CPU generator, as in super_perms().
      keep          (keep, keep_pos, scale): dg_corr_forward_masked - UN-dropped feature maps + their Dropout2d keep flags (B,C), either
                    may be None (identity grid).
      feat_inv      dg_corr_forward_extnorm - ONE channel chunk of wider feature maps, normalised by `feat_inv` (nops, B, P): 1 / the
                    norm of the whole sampled vector (sampled coordinates above 160 positions; see include/depthg_corr.h).
      intra_feats   dg_corr_forward_intra_feats - the intra pair-set correlates `intra_feats` (the shape of `feats`, sampled at coords1)
                    instead of `feats` (DepthContrastiveCorrelationLoss, src/modules.py:1427-1438); `depth` is not read.
      workspace     None: allocated here by the sizer of the entry; else alloc_workspace(desc, device, intra_feats=...)'s.
    The C ABI has one entry per extra, so two extras at once are refused, and so is `feat_inv` without `perms` (that entry has no draw).
    (Messages about an operand name its entry without the dg_ prefix, as they always have: entry[3:].)"""
    global _forward_count
    if (keep is not None) + (feat_inv is not None) + (intra_feats is not None) > 1:
        given = [f"`{n}`" for n, v in (("keep", keep), ("feat_inv", feat_inv), ("intra_feats", intra_feats)) if v is not None]
        raise ValueError(f"corr_forward: {' and '.join(given)} cannot ride in one call (the C ABI has one entry for each)")
    draw, seed, dev = perms is None, 0, feats.device
    if draw and feat_inv is not None:
        raise ValueError("corr_forward: `feat_inv` needs `perms`: perms=None asks for a draw, and dg_corr_forward_extnorm has none")
    entry = ("dg_corr_forward_masked" if keep is not None else "dg_corr_forward_extnorm" if feat_inv is not None else
             "dg_corr_forward_intra_feats" if intra_feats is not None else "dg_corr_forward_draw" if draw else "dg_corr_forward")
    if workspace is None:
        workspace = alloc_workspace(desc, dev, intra_feats is not None)
    if intra_feats is not None and (intra_feats.dtype != torch.float32 or not intra_feats.is_contiguous() or intra_feats.device != dev
                                    or tuple(intra_feats.shape) != tuple(feats.shape)):
        raise ValueError(f"{entry[3:]}: intra_feats must be contiguous fp32 {tuple(feats.shape)} on {dev}, got "
                         f"{intra_feats.dtype} {tuple(intra_feats.shape)} on {intra_feats.device}")
    if draw:
        perms = _empty((int(desc.n_neg), int(desc.B)), torch.long, dev)
        if draw_state is None:
            seed = _cpu_seed()
        else:
            _check_state(draw_state, entry[3:], dev)      # (keys the draw on the device: seed 0)
    state = _ptr(draw_state) if draw else None
    if keep is not None:
        for k in keep[:2]:
            if k is not None and (k.dtype != torch.float32 or not k.is_contiguous() or k.device != dev or tuple(k.shape) != (int(desc.B), int(desc.C))):
                raise ValueError(f"{entry[3:]}: keep flags must be contiguous fp32 (B,C) = ({desc.B},{desc.C}) on {dev}")
        mid = (int(draw), seed, state, _ptr(keep[0]), _ptr(keep[1]), float(keep[2]))
    elif feat_inv is not None:
        mid = (_ptr(feat_inv),)
    elif intra_feats is not None:
        mid, depth = (int(draw), seed, state, _ptr(intra_feats)), None
    else:
        mid = (seed, state) if draw else ()
    _forward_count += 1
    workspace._dg_forward = _forward_count
    out = _empty(_lib.DG_OUT_COUNT, torch.float32, dev)
    rc = getattr(_lib.load(), entry)(ctypes.byref(desc), _ptr(feats), _ptr(feats_pos), _ptr(code), _ptr(code_pos), _ptr(depth), _ptr(coords1),
                                     _ptr(coords2), _ptr(perms), *mid, _ptr(out), _ptr(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, entry)
    return out, perms, workspace


class DeferredDropout:
    """Feature maps whose Dropout2d (`feats = self.dropout(image_feat)`, src/modules.py:122-137) has been DRAWN but not applied:
    `feats` (B,C,h,w) un-dropped, `keep` (B,C) flags 1 / 0, `scale` = 1/(1-p).  ContrastiveCorrelationLoss takes one in place of
    orig_feats / orig_feats_pos and applies the mask inside its operand preparation on the identity grid (dg_corr_forward_masked:
    the same bits, without the dropped tensor's round trip through HBM); anything else calls materialize()."""

    def __init__(self, feats, keep, scale):
        if keep.dim() != 2 or tuple(keep.shape) != tuple(feats.shape[:2]) or keep.device != feats.device:
            raise ValueError(f"depthg_amd: keep flags {tuple(keep.shape)} on {keep.device} do not match feature maps "
                             f"{tuple(feats.shape)} on {feats.device}")
        if not scale > 0:
            raise ValueError(f"depthg_amd: keep scale must be positive, got {scale}")
        self.feats, self.keep, self.scale = feats, keep, float(scale)

    shape = property(lambda self: self.feats.shape)
    device = property(lambda self: self.feats.device)
    dtype = property(lambda self: self.feats.dtype)
    is_cuda = property(lambda self: self.feats.is_cuda)

    def dim(self):
        return self.feats.dim()

    def materialize(self):
        return self.feats * (self.keep.to(torch.float32) * self.scale)[:, :, None, None]


def _corr_backward(entry, desc, grad, coords1, coords2, perms, workspace, shape_code):
    dev = grad.device
    g_code = _empty(shape_code, torch.float32, dev)
    g_code_pos = _empty(shape_code, torch.float32, dev)
    rc = getattr(_lib.load(), entry)(ctypes.byref(desc), _ptr(grad), _ptr(coords1), _ptr(coords2), _ptr(perms),
                                     _ptr(g_code), _ptr(g_code_pos), _ptr(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, entry)
    return g_code, g_code_pos


def corr_backward(desc, grad_scalars, coords1, coords2, perms, workspace, shape_code):
    """Backward for the upstream gradient of the whole out vector: grad_scalars fp32 [DG_OUT_COUNT] on the device."""
    return _corr_backward("dg_corr_backward", desc, grad_scalars, coords1, coords2, perms, workspace, shape_code)


def corr_backward_total(desc, grad_total, coords1, coords2, perms, workspace, shape_code):
    """Backward for an upstream gradient of out[DG_OUT_TOTAL] alone (`total.backward()`): grad_total is a device scalar."""
    return _corr_backward("dg_corr_backward_total", desc, grad_total, coords1, coords2, perms, workspace, shape_code)


def corr_materialize(desc, which, workspace, want_cd=True, want_loss=False, perms=None):
    """The un-reduced (B,S,S,S,S) tensors of pair-set `which` (-1: the depth term's dd) from the operands the forward left in
    `workspace`.  `perms`: the forward's (n_neg, B) batch maps - needed for the negatives of a shared-coordinates (dense grid) call."""
    lib = _lib.load()
    dev = workspace.device
    sh = 1 if (desc.flags & _lib.DG_LINE_GRID) else desc.S
    shape = (desc.B, sh, desc.S, sh, desc.S)
    cd = _empty(shape, torch.float32, dev) if want_cd else None
    loss = _empty(shape, torch.float32, dev) if want_loss else None
    rc = lib.dg_corr_materialize_shared(ctypes.byref(desc), int(which), _ptr(perms), _ptr(cd), _ptr(loss), _ptr(workspace),
                                        workspace.numel(), _stream(dev))
    _lib.check(rc, "dg_corr_materialize_shared")
    return cd, loss


def corr_cd_hist(desc, workspace, first, count, perms=None, bins=64, range=(-1.0, 1.0)):
    """int64 (count, bins) histograms of the un-reduced code correlations cd of pair-sets first .. first + count - 1 (0 intra, 1
    inter, 2 + k negative k) over `range`, from the operands the forward left in `workspace` - nothing of size (B,P,P) is written
    (dg_corr_cd_hist).  torch.histc's bins, except that values outside the range count in the end bins.  `perms`: the forward's
    (n_neg, B) batch maps - needed for the negatives of a shared-coordinates (dense grid) call."""
    dev = _on_gpu(workspace, "workspace").device
    if perms is not None:
        _on_gpu(perms, "perms")
    out = _empty((max(int(count), 0), max(int(bins), 0)), torch.int64, dev)
    rc = _lib.load().dg_corr_cd_hist(ctypes.byref(desc), int(first), int(count), _ptr(perms), int(bins), float(range[0]), float(range[1]),
                                     _ptr(out), _ptr(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, "dg_corr_cd_hist")
    return out


# ---- what the three auxiliary loss terms share (dg_api_loss.hip)
def _gpu_float32(tensors, text, also_gpu=()):
    """The fused routes' gate: every (tensor, name) of both lists on the GPU, those of `tensors` float32 as well (the kernels read
    and write fp32: a cast here would hand back gradients of another dtype).  text: the complaint, with {name} and {dtype}."""
    for t, name in (*tensors, *also_gpu):
        _on_gpu(t, name)
    for t, name in tensors:
        if t.dtype != torch.float32:
            raise ValueError("depthg_amd: " + text.format(name=name, dtype=t.dtype))


def _plan_bytes(need, term, dims, limits):
    """A sizer's answer, or the refusal it stands for: 0 bytes means the library has no plan for these sizes."""
    if need == 0:
        raise ValueError(f"depthg_amd: no {term} plan for {dims} ({limits})")
    return need


def _workspace_views(workspace, specs):
    """Views of a workspace's leading sections, specs = (name, shape, dtype) in the layout's order (include/depthg_corr.h: every
    section starts at a multiple of 256 bytes)."""
    off, out = 0, {}
    for name, shape, dtype in specs:
        nbytes = math.prod(shape) * dtype.itemsize
        out[name] = workspace[off:off + nbytes].view(dtype).view(shape)
        off += (nbytes + 255) // 256 * 256
    return out


def _forward_workspace(workspace, maker, dev, need):
    """A backward's `workspace`: the contiguous uint8 tensor `maker` returned on `dev`, of at least `need` bytes."""
    if _on_gpu(workspace, "workspace").device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"depthg_amd: workspace must be the contiguous uint8 tensor of {maker} on {dev}")
    return workspace


def _grad_out_scalar(grad_out, dev):
    """The upstream gradient of a scalar loss as the library reads it: one fp32 element on `dev`."""
    grad_out = _f32c(grad_out, "grad_out")
    if grad_out.numel() != 1 or grad_out.device != dev:
        raise ValueError(f"depthg_amd: grad_out must be one element on {dev}, got {tuple(grad_out.shape)} on {grad_out.device}")
    return grad_out


def _out_buffers(out, shapes, names, dev):
    """A backward's result buffers: fresh ones, or the caller's `out`, each a contiguous float32 tensor of its shape on `dev`."""
    if out is None:
        return tuple(_empty(sh, torch.float32, dev) for sh in shapes)
    for o, sh, name in zip(out, shapes, names):
        if not (o.device == dev and o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == tuple(sh)):
            raise ValueError(f"depthg_amd: the `out` buffer of {name} must be a contiguous float32 {tuple(sh)} tensor on {dev}")
    return tuple(out)


def _crf_loss_coords(coords, n, dev):
    if coords.dim() != 2 or coords.shape[0] != 2 or coords.shape[1] < 1:
        raise ValueError(f"depthg_amd: coords must be (2, n) - the y row, then the x row - got {tuple(coords.shape)}")
    if coords.dtype not in (torch.int32, torch.int64) or (n is not None and coords.shape[1] != n):
        raise ValueError(f"depthg_amd: coords must be integer (2, {n if n is not None else 'n'}), got {coords.dtype} {tuple(coords.shape)}")
    if _on_gpu(coords, "coords").device != dev:
        raise RuntimeError(f"depthg_amd: coords live on {coords.device}, the maps on {dev}")
    return coords.detach().to(torch.int32).contiguous()


def crf_loss_workspace_sections(workspace, B, D, n):
    """Views of what crf_loss_forward left in its workspace (the layout of include/depthg_corr.h: sections at multiples of 256
    bytes): S (B,n,Dp) the normalised resized code vectors (Dp = D rounded up to 4, zero columns above D), G (B,n,Dp) = K S without
    the rows' own terms, g (B,n,4) the resized image colours (a zero fourth column), norm (B,n), q (B,n) fp64 = S_a . G_a / |S_a|^2."""
    Dp = (D + 3) // 4 * 4
    return _workspace_views(workspace, (("S", (B, n, Dp), torch.float32), ("G", (B, n, Dp), torch.float32), ("g", (B, n, 4), torch.float32),
                                        ("norm", (B, n), torch.float32), ("q", (B, n), torch.float64)))


def crf_loss_forward(code, img, coords, size, alpha, beta, gamma, w1, w2, shift):
    """mean(ContrastiveCRFLoss(resize(img, size), norm(resize(code, size)))) at the samples `coords` (dg_crfloss_forward;
    src/modules.py:1510-1542, src/train_segmentation.py:413-419): code (B,D,h,w), img (B,3,H,W) on the GPU, coords integer (2,n)
    (y row, x row) on the size x size grid.  Returns (loss, workspace): a 0-dim fp32 device tensor and what crf_loss_backward needs."""
    lib = _lib.load()
    if code.dim() != 4 or img.dim() != 4 or img.shape[0] != code.shape[0] or img.shape[1] != 3:
        raise ValueError(f"depthg_amd: code must be (B, D, h, w) and img (B, 3, H, W), got {tuple(code.shape)} and {tuple(img.shape)}")
    code, img = _f32c(code, "code"), _f32c(img, "img")
    dev = code.device
    if img.device != dev:
        raise RuntimeError(f"depthg_amd: code lives on {dev}, img on {img.device}")
    coords = _crf_loss_coords(coords, None, dev)
    B, D, h, w = code.shape
    n = coords.shape[1]
    need = _plan_bytes(lib.dg_crfloss_workspace_bytes(B, D, n), "CRF-loss", f"B={B}, D={D}, n={n}", "B <= 65535, D <= 128, n <= 4096")
    ws = _empty((need,), torch.uint8, dev)
    loss = _empty((), torch.float32, dev)
    rc = lib.dg_crfloss_forward(_ptr(code), _ptr(img), B, D, h, w, img.shape[2], img.shape[3], int(size), _ptr(coords), n, float(alpha),
                                float(beta), float(gamma), float(w1), float(w2), float(shift), _ptr(ws), ws.numel(), _ptr(loss),
                                _stream(dev))
    _lib.check(rc, "dg_crfloss_forward")
    return loss, ws


def crf_loss_backward(workspace, coords, shape_code, size, grad_out, out=None):
    """d loss / d code (B,D,h,w) of the crf_loss_forward whose workspace this is, times the 0-dim device tensor `grad_out`
    (dg_crfloss_backward); every element is written.  out: optional result buffer."""
    lib = _lib.load()
    B, D, h, w = (int(v) for v in shape_code)
    dev = _on_gpu(workspace, "workspace").device
    coords = _crf_loss_coords(coords, None, dev)
    # (sizes without a plan - 0 bytes - are the library's to refuse, by name)
    _forward_workspace(workspace, "crf_loss_forward", dev, lib.dg_crfloss_workspace_bytes(B, D, coords.shape[1]))
    grad_out = _grad_out_scalar(grad_out, dev)
    out, = _out_buffers(None if out is None else (out,), ((B, D, h, w),), ("code",), dev)
    rc = lib.dg_crfloss_backward(_ptr(workspace), workspace.numel(), _ptr(coords), B, D, h, w, int(size), coords.shape[1], _ptr(grad_out),
                                 _ptr(out), _stream(dev))
    _lib.check(rc, "dg_crfloss_backward")
    return out


def _aug_alignment_maps(code, code_aug):
    if code.dim() != 4 or code_aug.dim() != 4:
        raise ValueError(f"depthg_amd: code must be (B, D, h, w) and code_aug (B, D, n, n), got {tuple(code.shape)} and {tuple(code_aug.shape)}")
    if code.shape[:2] != code_aug.shape[:2]:
        raise ValueError(f"depthg_amd: code {tuple(code.shape)} and code_aug {tuple(code_aug.shape)} must share the batch size and D")
    if code_aug.shape[2] != code_aug.shape[3]:
        raise ValueError(f"depthg_amd: code_aug must be square (the reference resizes the coordinates to (n, n)), got {tuple(code_aug.shape)}")
    code, code_aug = _f32c(code, "code"), _f32c(code_aug, "code_aug")
    if code_aug.device != code.device:
        raise RuntimeError(f"depthg_amd: code lives on {code.device}, code_aug on {code_aug.device}")
    return code, code_aug


def _aug_alignment_workspace_bytes(lib, B, D, h, w, n):
    return _plan_bytes(lib.dg_augalign_workspace_bytes(B, D, h, w, n), "augmentation-alignment", f"B={B}, D={D}, code map {h}x{w}, n={n}",
                       "B <= 65535, n <= 255, 8 h w + 24 n^2 + 4 <= 163776: the inverse tap records are built in LDS")


def aug_alignment_workspace_sections(workspace, B, n):
    """Views of what aug_alignment_forward left in its workspace (the layout of include/depthg_corr.h: sections at multiples of 256
    bytes): ds (B,n,n,2) the resized coordinates, norm_u (B,n,n) and norm_v (B,n,n) the norms in front of the eps clamp, s (B,n,n)."""
    return _workspace_views(workspace, (("ds", (B, n, n, 2), torch.float32),) + tuple((name, (B, n, n), torch.float32) for name in ("norm_u", "norm_v", "s")))


def aug_alignment_forward(code, code_aug, coord_aug):
    """-mean <norm(sample(code, resize(coord_aug, n))), norm(code_aug)> (dg_augalign_forward; src/train_segmentation.py:400-411):
    code (B,D,h,w), code_aug (B,D,n,n), coord_aug (B,H,W,2) on the GPU.  Returns (loss, workspace): a 0-dim fp32 device tensor and
    what aug_alignment_backward needs."""
    lib = _lib.load()
    code, code_aug = _aug_alignment_maps(code, code_aug)
    if coord_aug.dim() != 4 or coord_aug.shape[3] != 2 or coord_aug.shape[0] != code.shape[0]:
        raise ValueError(f"depthg_amd: coord_aug must be (B, H, W, 2) with code's batch size, got {tuple(coord_aug.shape)} beside {tuple(code.shape)}")
    coord_aug = _f32c(coord_aug, "coord_aug")
    dev = code.device
    if coord_aug.device != dev:
        raise RuntimeError(f"depthg_amd: code lives on {dev}, coord_aug on {coord_aug.device}")
    B, D, h, w = code.shape
    n = code_aug.shape[2]
    ws = _empty((_aug_alignment_workspace_bytes(lib, B, D, h, w, n),), torch.uint8, dev)
    loss = _empty((), torch.float32, dev)
    rc = lib.dg_augalign_forward(_ptr(code), _ptr(code_aug), _ptr(coord_aug), B, D, h, w, n, coord_aug.shape[1], coord_aug.shape[2], _ptr(ws),
                                 ws.numel(), _ptr(loss), _stream(dev))
    _lib.check(rc, "dg_augalign_forward")
    return loss, ws


def aug_alignment_backward(workspace, code, code_aug, grad_out, out=None):
    """(d loss / d code (B,D,h,w), d loss / d code_aug (B,D,n,n)) of the aug_alignment_forward whose workspace this is - same code and
    code_aug - times the 0-dim device tensor `grad_out` (dg_augalign_backward); every element of both is written.  out: optional
    pair of result buffers."""
    lib = _lib.load()
    code, code_aug = _aug_alignment_maps(code, code_aug)
    dev = code.device
    B, D, h, w = code.shape
    n = code_aug.shape[2]
    _forward_workspace(workspace, "aug_alignment_forward", dev, _aug_alignment_workspace_bytes(lib, B, D, h, w, n))
    grad_out = _grad_out_scalar(grad_out, dev)
    out = _out_buffers(out, (code.shape, code_aug.shape), ("code", "code_aug"), dev)
    rc = lib.dg_augalign_backward(_ptr(code), _ptr(code_aug), _ptr(workspace), workspace.numel(), B, D, h, w, n, _ptr(grad_out), _ptr(out[0]),
                                  _ptr(out[1]), _stream(dev))
    _lib.check(rc, "dg_augalign_backward")
    return out[0], out[1]


def augment_forward(img, packed, out_size, mean=None, std=None):
    """(img_aug (B,3,h,w), coord_aug (B,h,w,2)) of img (B,3,H,W) on the GPU under the records of `packed` - augment.pack_params's CPU
    int32 tensor, uploaded here once - in two launches for the whole batch (dg_augment_forward, dg_augment.hip); every element of
    both results is written.  mean / std: three floats each, or None (the ops act on the tensor as given)."""
    lib = _lib.load()
    img = _f32c(img, "img")                       # (a non-contiguous img is copied once, here)
    dev = img.device
    B, C, H, W = img.shape
    h, w = int(out_size[0]), int(out_size[1])
    if packed.dtype != torch.int32 or packed.is_cuda or packed.numel() != B * 16 + H + W or not packed.is_contiguous():
        raise ValueError(f"depthg_amd: augment_forward wants augment.pack_params's CPU int32 tensor of {B} x 16 + {H} + {W} words")
    ws = _empty((_plan_bytes(lib.dg_augment_workspace_bytes(B, h, w), "batch augmentation", f"B={B}, output {h}x{w}",
                             "B <= 65535, sides from 3 to 16384"),), torch.uint8, dev)
    img_aug, coord_aug = _empty((B, 3, h, w), torch.float32, dev), _empty((B, h, w, 2), torch.float32, dev)
    params = packed.to(dev)
    space = [None, None] if mean is None else [(ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)]
    rc = lib.dg_augment_forward(_ptr(img), *img.stride(), ctypes.c_void_p(packed.data_ptr()), _ptr(params), space[0], space[1], B, C, H, W,
                                h, w, _ptr(img_aug), _ptr(coord_aug), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "dg_augment_forward")
    return img_aug, coord_aug


BATCH_IMAGE, BATCH_LABEL, BATCH_DEPTH, BATCH_DEPTH_PLANE, BATCH_LABEL_FILL = range(5)      # dg_batch_prep's record kinds
BATCH_MASK_BOOL_IGNORED, BATCH_MASK_FLOAT_POSITIVE = 0, 1                                   # and its mask rules
BATCH_REC_WORDS = 8


def _packed_source(who, packed, records, tables, H, W, device, rows=None, params=None):
    """What data.pack_batch makes, as dg_batch_prep and dg_samplecache_put take it: records CPU int32 (k, 8), tables CPU int32 of W + H
    columns - and `rows` rows, if given - and packed a flat uint8 tensor.  Returns (src, params, device, stream): packed on `device`
    (None: where packed or `params` lives, else the current GPU) and the device copy of [records, tables] - `params`, or uploaded
    here, once."""
    for t, name in ((records, "records"), (tables, "tables")):
        if t.dtype != torch.int32 or t.is_cuda or not t.is_contiguous():
            raise ValueError(f"depthg_amd: {who} wants `{name}` as a contiguous CPU int32 tensor")
    if (records.dim() != 2 or records.shape[1] != BATCH_REC_WORDS or tables.dim() != 2 or tables.shape[1] != W + H or
            (rows is not None and tables.shape[0] != rows)):
        k, N = ("n", "N") if rows is None else ("k", rows)
        raise ValueError(f"depthg_amd: {who} wants records ({k}, {BATCH_REC_WORDS}) and tables ({N}, {W} + {H}), got {tuple(records.shape)} and "
                         f"{tuple(tables.shape)}")
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError(f"depthg_amd: {who} wants `packed` as a flat contiguous uint8 tensor")
    if device is None:
        device = packed.device if packed.is_cuda else (params.device if params is not None else torch.device("cuda", torch.cuda.current_device()))
    dev = torch.device(device)
    stream = _stream(dev)
    src = _on_gpu(packed.to(dev, non_blocking=True), "packed")
    if params is None:
        params = torch.cat([records.reshape(-1), tables.reshape(-1)]).to(dev, non_blocking=True)
    elif not params.is_cuda or params.dtype != torch.int32 or params.numel() != records.numel() + tables.numel():
        raise ValueError(f"depthg_amd: {who} wants `params` as the GPU int32 copy of [records, tables]")
    return src, params, dev, stream


def _loader_outputs(rows, H, W, names, mask_rule, dev):
    """The loader's outputs `names` of `rows` samples, unwritten: img fp32 (rows,3,H,W), label int64, mask fp32 or bool by `mask_rule`,
    depth fp32 (rows,H,W) each."""
    kinds = {"img": ((rows, 3, H, W), torch.float32), "label": ((rows, H, W), torch.int64),
             "mask": ((rows, H, W), torch.float32 if mask_rule == BATCH_MASK_FLOAT_POSITIVE else torch.bool), "depth": ((rows, H, W), torch.float32)}
    return {k: _empty(*kinds[k], dev) for k in kinds if k in names}


def _index_lists(who, cache, idx_a, idx_b=None, names=("idx_a", "idx_b")):
    """The index lists of a cache entry: each a contiguous int64 tensor on the cache's device (the kernels read them there; the caller
    has checked the values on the host), both of one length.  Returns (n, the rows of both lists together)."""
    _on_gpu(cache, "cache")
    for name, idx in zip(names, (idx_a,) if idx_b is None else (idx_a, idx_b)):
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != cache.device or not idx.is_contiguous():
            raise ValueError(f"depthg_amd: {who} wants `{name}` as a contiguous 1-d int64 tensor on {cache.device} (the kernel reads it there)")
    n = idx_a.numel()
    if idx_b is not None and idx_b.numel() != n:
        raise ValueError(f"depthg_amd: {who}: {n} indices and {idx_b.numel()} positives")
    return n, (2 * n if idx_b is not None else n)


def batch_prep(packed, records, tables, out_size, device=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), params=None):
    """The loader transform of a whole batch in one launch (dg_batch_prep, dg_batch.hip).  packed: uint8 tensor of the decoded source
    planes - on the CPU (pinned memory makes the one upload asynchronous) or already on the GPU; records: CPU int32 (n_records, 8);
    tables: CPU int32 (N, W + H), per sample xs[W] then ys[H] (data.pack_batch makes all three); out_size: (H, W).  `params`: the
    device copy of [records, tables] when the caller has uploaded it already, else it is uploaded here, once.  Returns a dict of the
    outputs the records write - img fp32 (N,3,H,W), label int64 (N,H,W), mask bool or fp32 (N,H,W), depth fp32 (N,H,W) - every
    element written."""
    lib = _lib.load()
    H, W = int(out_size[0]), int(out_size[1])
    src, params, dev, stream = _packed_source("batch_prep", packed, records, tables, H, W, device, params=params)
    n_records, N = records.shape[0], tables.shape[0]
    kinds = set(records[:, 0].tolist())
    rules = set(records[:, 7][(records[:, 0] == BATCH_LABEL) | (records[:, 0] == BATCH_LABEL_FILL)].tolist())
    names = ((("img",) if BATCH_IMAGE in kinds else ()) + (("label", "mask") if kinds & {BATCH_LABEL, BATCH_LABEL_FILL} else ()) +
             (("depth",) if kinds & {BATCH_DEPTH, BATCH_DEPTH_PLANE} else ()))
    out = _loader_outputs(N, H, W, names, BATCH_MASK_FLOAT_POSITIVE if rules == {BATCH_MASK_FLOAT_POSITIVE} else BATCH_MASK_BOOL_IGNORED, dev)
    rc = lib.dg_batch_prep(_ptr(src), src.numel(), ctypes.c_void_p(records.data_ptr()), ctypes.c_void_p(tables.data_ptr()), _ptr(params),
                           n_records, N, H, W, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), _ptr(out.get("img")),
                           _ptr(out.get("label")), _ptr(out.get("mask")), _ptr(out.get("depth")), stream)
    _lib.check(rc, "dg_batch_prep")
    return out


FEATURE_CACHE_DTYPES = {torch.float32: _lib.DG_FC_F32, torch.float16: _lib.DG_FC_F16, torch.bfloat16: _lib.DG_FC_BF16}
FEATURE_CACHE_MAX_ROWS = 65535      # rows one dg_featcache_* call moves (gather: the two lists together)


def _feature_cache_operands(who, cache, idx_a, idx_b=None, names=("idx_a", "idx_b")):
    """The cache as the two entries take it - a contiguous (N, L) GPU tensor of a storage type - and its index lists (_index_lists).
    Returns (the storage type's id, n, rows)."""
    if cache.dim() != 2 or cache.dtype not in FEATURE_CACHE_DTYPES or not cache.is_contiguous():
        raise ValueError(f"depthg_amd: {who} wants the cache as a contiguous (N, L) tensor of float32, float16 or bfloat16, got "
                         f"{tuple(cache.shape)} {cache.dtype}")
    return (FEATURE_CACHE_DTYPES[cache.dtype],) + _index_lists(who, cache, idx_a, idx_b, names)


def feature_cache_put(cache, idx, src):
    """Rows idx[0..n) of `cache` (N, L) = src (n, L) - or (n, C, h, w) with C h w = L - converted to the cache's dtype with torch's
    rounding (dg_featcache_put, k_fc_put of dg_feat_cache.hip): one launch.  `idx`: int64 on the cache's device, each row once."""
    lib = _lib.load()
    dt, n, _ = _feature_cache_operands("feature_cache_put", cache, idx, names=("idx",))
    N, L = cache.shape
    src = _f32c(src, "src")
    if src.device != cache.device or src.numel() != n * L or src.shape[0] != n:
        raise ValueError(f"depthg_amd: feature_cache_put: src {tuple(src.shape)} on {src.device} is not {n} rows of {L} elements on {cache.device}")
    rc = lib.dg_featcache_put(_ptr(cache), dt, N, L, _ptr(src), _ptr(idx), n, _stream(cache.device))
    _lib.check(rc, "dg_featcache_put")


def feature_cache_gather(cache, idx_a, idx_b=None, out=None):
    """(2n, L) fp32: the cache rows idx_a[0..n), then the rows idx_b[0..n) - or (n, L) without idx_b - from ONE launch into one
    allocation (dg_featcache_gather, k_fc_gather of dg_feat_cache.hip): the layout the head's paired pass takes its two maps in.
    Indices: int64 on the cache's device; they may repeat.  `out`: a buffer to write instead of a new one; every element is written."""
    lib = _lib.load()
    dt, n, rows = _feature_cache_operands("feature_cache_gather", cache, idx_a, idx_b)
    N, L = cache.shape
    if out is None:
        out = _empty((rows, L), torch.float32, cache.device)
    elif out.dtype != torch.float32 or out.device != cache.device or tuple(out.shape) != (rows, L) or not out.is_contiguous():
        raise ValueError(f"depthg_amd: feature_cache_gather: `out` must be a contiguous float32 ({rows}, {L}) tensor on {cache.device}")
    rc = lib.dg_featcache_gather(_ptr(cache), dt, N, L, _ptr(idx_a), _ptr(idx_b), n, _ptr(out), _stream(cache.device))
    _lib.check(rc, "dg_featcache_gather")
    return out


SAMPLE_CACHE_MAX_ROWS = 65535       # rows one dg_samplecache_gather call forms (the two lists together)


def _sample_cache_operands(who, cache, has_labels, with_depth, idx_a, idx_b=None, names=("idx_a", "idx_b")):
    """The cache as the two entries take it - a contiguous uint8 (n_images, planes, H, W) GPU tensor with planes = 3 + has_labels +
    with_depth - and its index lists (_index_lists).  Returns (n, rows)."""
    planes = 3 + int(bool(has_labels)) + int(bool(with_depth))
    if cache.dim() != 4 or cache.dtype != torch.uint8 or not cache.is_contiguous() or cache.shape[1] != planes:
        raise ValueError(f"depthg_amd: {who} wants the cache as a contiguous uint8 (n_images, {planes}, H, W) tensor, got "
                         f"{tuple(cache.shape)} {cache.dtype}")
    return _index_lists(who, cache, idx_a, idx_b, names)


def sample_cache_put(cache, has_labels, with_depth, idx, packed, records, tables):
    """Rows idx[0..n) of `cache` - uint8 (n_images, planes, H, W), planes R, G, B, label (has_labels), depth (with_depth) - = the bytes
    the loader's nearest resize and crop select from the decoded planes of n samples (dg_samplecache_put, k_sc_put of
    dg_sample_cache.hip): one launch.  packed / records / tables: what data.pack_batch makes and ops.batch_prep takes; `idx`: int64
    on the cache's device, each row once."""
    lib = _lib.load()
    n, _ = _sample_cache_operands("sample_cache_put", cache, has_labels, with_depth, idx, names=("idx",))
    N, _, H, W = cache.shape
    src, params, _, stream = _packed_source("sample_cache_put", packed, records, tables, H, W, cache.device, rows=n)
    rc = lib.dg_samplecache_put(_ptr(cache), N, int(bool(has_labels)), int(bool(with_depth)), H, W, _ptr(idx), n, _ptr(src), src.numel(),
                                ctypes.c_void_p(records.data_ptr()), ctypes.c_void_p(tables.data_ptr()), _ptr(params), records.shape[0], stream)
    _lib.check(rc, "dg_samplecache_put")


def sample_cache_gather(cache, has_labels, with_depth, idx_a, idx_b=None, label_offset=0, fill=-1, mask_rule=BATCH_MASK_BOOL_IGNORED,
                        mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), want=None):
    """The rows idx_a[0..n), then the rows idx_b[0..n) (None: n rows), of a sample cache in the step's dtypes from ONE launch
    (dg_samplecache_gather, k_sc_gather of dg_sample_cache.hip): a dict of img fp32 (rows,3,H,W) normalised with `mean` / `std`, label
    int64 (rows,H,W) = byte + label_offset (or `fill` without a label plane), mask (rows,H,W) bool label == -1 or fp32 label > 0 by
    `mask_rule`, depth fp32 (rows,H,W) - those of them `want` names (None: all the cache can form), every element written.  Indices:
    int64 on the cache's device; they may repeat."""
    lib = _lib.load()
    n, rows = _sample_cache_operands("sample_cache_gather", cache, has_labels, with_depth, idx_a, idx_b)
    N, _, H, W = cache.shape
    can = ("img", "label", "mask") + (("depth",) if with_depth else ())
    want = can if want is None else tuple(want)
    if not want or set(want) - set(can):
        raise ValueError(f"depthg_amd: sample_cache_gather: `want` = {want!r}, this cache forms {can!r}")
    dev = cache.device
    out = _loader_outputs(rows, H, W, want, mask_rule, dev)
    rc = lib.dg_samplecache_gather(_ptr(cache), N, int(bool(has_labels)), int(bool(with_depth)), H, W, _ptr(idx_a), _ptr(idx_b), n,
                                   (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), int(label_offset), int(fill), int(mask_rule),
                                   _ptr(out.get("img")), _ptr(out.get("label")), _ptr(out.get("mask")), _ptr(out.get("depth")), _stream(dev))
    _lib.check(rc, "dg_samplecache_gather")
    return out


EPOCH_DRAW_MAX_B = 1024             # one block of k_epoch_draw draws the batch


def _philox_word0(seed, counters):
    """Word 0 of Philox4x32-10 (dg_philox4 of csrc/dg_device.h) keyed by the 64-bit `seed` at the 128-bit counters (c, 0): numpy
    uint64 in, numpy uint64 (32-bit values) out.  The host statement of what k_epoch_draw draws."""
    import numpy as np
    u, M = np.uint64, np.uint64(0xFFFFFFFF)
    c = np.asarray(counters, dtype=np.uint64)
    c0, c1, c2, c3 = c & M, c >> u(32), np.zeros_like(c), np.zeros_like(c)
    k0, k1 = u(seed & 0xFFFFFFFF), u((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ k0, p1 & M, (p0 >> u(32)) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + u(0x9E3779B9)) & M, (k1 + u(0xBB67AE85)) & M
    return c0


def epoch_draw(state, order, nns, B, num_neighbors, ind=None, ind_pos=None):
    """The next batch of a cached epoch and its kNN positives (src/data.py:1073-1080) from operands that all live on one device, ONE
    launch (dg_epoch_draw, k_epoch_draw of dg_epoch.hip).  state: int64 {seed, draws, cursor} - the words of new_perm_state, the
    third used as the cursor: a state of its own, not one super_perms or rand_coords_state also advance; order: int64 (n_images,);
    nns: int64 (n_images, K), the table knn.load_nns returns.  Slot j: ind[j] = order[cursor + j], ind_pos[j] =
    nns[ind[j]][1 + u % num_neighbors] with u = word 0 of Philox4x32-10 keyed by the seed at counter draws + j; then cursor and draws
    advance by B.  Nothing about the draw is an argument of the launch: recorded in a hipGraph it draws anew at every replay.
    The positives are uniform over columns 1 .. num_neighbors as the reference's are, but they are this generator's stream, NOT
    torch.randint's.  `ind` / `ind_pos`: int64 (B,) buffers to write instead of new ones; every element is written.  The caller keeps
    cursor + B <= n_images (the cursor is not read on the host); the position in `order` is held at n_images - 1 all the same.
    On CPU tensors the same arithmetic runs in numpy: the statement the kernel is tested against."""
    B, num_neighbors = int(B), int(num_neighbors)
    dev = state.device
    if state.dtype != torch.int64 or state.numel() != 3 or not state.is_contiguous():
        raise ValueError("depthg_amd: epoch_draw: state must be the contiguous int64[3] tensor {seed, draws, cursor}")
    if order.dtype != torch.int64 or order.dim() != 1 or nns.dtype != torch.int64 or nns.dim() != 2 or nns.shape[0] != order.shape[0] \
            or not order.is_contiguous() or not nns.is_contiguous() or order.device != dev or nns.device != dev:
        raise ValueError(f"depthg_amd: epoch_draw wants order as a contiguous int64 (n_images,) tensor and nns as a contiguous int64 "
                         f"(n_images, K) tensor on {dev}, got {tuple(order.shape)} {order.dtype} on {order.device} and "
                         f"{tuple(nns.shape)} {nns.dtype} on {nns.device}")
    n_images, K = int(nns.shape[0]), int(nns.shape[1])
    if B < 1 or B > EPOCH_DRAW_MAX_B or n_images < 1:
        raise ValueError(f"depthg_amd: epoch_draw: B={B} outside [1, {EPOCH_DRAW_MAX_B}] (one block draws the batch), or an empty table")
    if num_neighbors < 1 or num_neighbors >= K:
        raise ValueError(f"depthg_amd: epoch_draw: num_neighbors={num_neighbors} outside [1, {K - 1}] of a table with {K} columns "
                         "(column 0 is the image itself)")
    outs = []
    for name, t in (("ind", ind), ("ind_pos", ind_pos)):
        if t is None:
            t = _empty((B,), torch.int64, dev)
        elif t.dtype != torch.int64 or tuple(t.shape) != (B,) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"depthg_amd: epoch_draw: `{name}` must be a contiguous int64 ({B},) tensor on {dev}")
        outs.append(t)
    ind, ind_pos = outs
    if dev.type == "cuda":
        rc = _lib.load().dg_epoch_draw(_ptr(state), _ptr(order), _ptr(nns), B, num_neighbors, n_images, K, _ptr(ind), _ptr(ind_pos), _stream(dev))
        _lib.check(rc, "dg_epoch_draw")
        return ind, ind_pos
    import numpy as np
    mask = (1 << 64) - 1
    seed, draws, cursor = (int(v) & mask for v in state.tolist())
    j = np.arange(B, dtype=np.uint64)
    at = np.minimum((np.uint64(cursor) + j) & np.uint64(mask), np.uint64(n_images - 1)).astype(np.int64)
    image = order.numpy()[at]
    r = 1 + (_philox_word0(seed, np.uint64(draws) + j) % np.uint64(num_neighbors)).astype(np.int64)
    ind.copy_(torch.from_numpy(image))
    ind_pos.copy_(torch.from_numpy(nns.numpy()[np.clip(image, 0, n_images - 1), r]))
    for k, v in ((1, draws + B), (2, cursor + B)):
        v &= mask
        state[k] = v - (1 << 64) if v >= (1 << 63) else v
    return ind, ind_pos


def rec_loss_shapes(code, feats, weight, bias):
    """The reconstruction term's shape rules, on any device: code (B,D,h,w), feats (B,C,h,w) on the same grid, the decoder's weight
    (C,D,1,1) or (C,D) and bias (C,).  Returns (weight as (C,D), (B, D, C, h, w))."""
    if code.dim() != 4 or feats.dim() != 4:
        raise ValueError(f"depthg_amd: code must be (B, D, h, w) and feats (B, C, h, w), got {tuple(code.shape)} and {tuple(feats.shape)}")
    if code.shape[0] != feats.shape[0] or code.shape[2:] != feats.shape[2:]:
        raise ValueError(f"depthg_amd: code {tuple(code.shape)} and feats {tuple(feats.shape)} must share the batch size and the grid")
    B, D, h, w = code.shape
    C = feats.shape[1]
    if tuple(weight.shape) not in ((C, D, 1, 1), (C, D)) or tuple(bias.shape) != (C,):
        raise ValueError(f"depthg_amd: the decoder maps code's {D} channels to feats' {C}: weight must be ({C}, {D}, 1, 1) or ({C}, {D}) and "
                         f"bias ({C},), got {tuple(weight.shape)} and {tuple(bias.shape)}")
    return (weight[:, :, 0, 0] if weight.dim() == 4 else weight), (B, D, C, h, w)


def _rec_loss_operands(code, feats, weight, bias, keep, scale):
    """The reconstruction term's tensors as the library reads them (contiguous fp32 on one GPU; nothing is copied that already is)
    and its sizes; `feats` may be a DeferredDropout, whose flags and scale then stand for keep / scale."""
    if isinstance(feats, DeferredDropout):
        if keep is not None:
            raise ValueError("depthg_amd: keep flags given twice (feats is a DeferredDropout)")
        feats, keep, scale = feats.feats, feats.keep, feats.scale
    weight, (B, D, C, h, w) = rec_loss_shapes(code, feats, weight, bias)
    if D > 128:
        raise ValueError(f"depthg_amd: the reconstruction term takes code of at most 128 channels on the GPU (the head's limit), got D={D}")
    code, feats, weight, bias = _f32c(code, "code"), _f32c(feats, "feats"), _f32c(weight, "weight"), _f32c(bias, "bias")
    dev = code.device
    for t, name in ((feats, "feats"), (weight, "weight"), (bias, "bias")):
        if t.device != dev:
            raise RuntimeError(f"depthg_amd: code lives on {dev}, {name} on {t.device}")
    if keep is not None:
        if tuple(keep.shape) != (B, C) or not scale > 0:
            raise ValueError(f"depthg_amd: keep flags must be (B, C) = ({B}, {C}) with a positive scale, got {tuple(keep.shape)} and scale {scale}")
        keep = _f32c(keep, "keep")
        if keep.device != dev:
            raise RuntimeError(f"depthg_amd: code lives on {dev}, keep on {keep.device}")
    return code, feats, weight, bias, keep, float(scale), (B, D, C, h, w)


def _rec_loss_workspace_bytes(lib, B, D, C, h, w):
    return _plan_bytes(lib.dg_recloss_workspace_bytes(B, D, C, h, w), "reconstruction-loss", f"B={B}, D={D}, C={C}, map {h}x{w}",
                       "D <= 128, every tensor below 2^31 elements")


def rec_loss_workspace_sections(workspace, B, h, w):
    """Views of what rec_loss_forward left in its workspace (the layout of include/depthg_corr.h: sections at multiples of 256
    bytes): norm_y (B,h,w) and norm_f (B,h,w) the norms in front of the eps clamp, s (B,h,w)."""
    return _workspace_views(workspace, tuple((name, (B, h, w), torch.float32) for name in ("norm_y", "norm_f", "s")))


def rec_loss_forward(code, feats, weight, bias, keep=None, scale=1.0):
    """-mean <norm(decoder(code)), norm(feats)> (dg_recloss_forward; src/train_segmentation.py:391-398): code (B,D,h,w), feats
    (B,C,h,w) - a tensor or a DeferredDropout - the decoder's weight (C,D,1,1) or (C,D) and bias (C,), on the GPU; keep / scale:
    Dropout2d flags (B,C) still to be applied to feats.  Returns (loss, workspace): a 0-dim fp32 device tensor and what
    rec_loss_backward needs."""
    lib = _lib.load()
    code, feats, weight, bias, keep, scale, (B, D, C, h, w) = _rec_loss_operands(code, feats, weight, bias, keep, scale)
    dev = code.device
    ws = _empty((_rec_loss_workspace_bytes(lib, B, D, C, h, w),), torch.uint8, dev)
    loss = _empty((), torch.float32, dev)
    rc = lib.dg_recloss_forward(_ptr(code), _ptr(feats), _ptr(weight), _ptr(bias), _ptr(keep), scale, B, D, C, h, w, _ptr(ws), ws.numel(),
                                _ptr(loss), _stream(dev))
    _lib.check(rc, "dg_recloss_forward")
    return loss, ws


def rec_loss_backward(workspace, code, feats, weight, bias, grad_out, keep=None, scale=1.0, out=None, want_feats=False, want_params=True):
    """(d loss / d code (B,D,h,w), d loss / d weight (C,D), d loss / d bias (C,)) of the rec_loss_forward whose workspace this is -
    same tensors - times the 0-dim device tensor `grad_out` (dg_recloss_backward); every element of the three is written.  out:
    optional triple of result buffers.
    want_feats: a fourth value, d loss / d feats (B,C,h,w) - of the un-dropped maps when keep flags are given, dropped channels an
    exact 0 - from the same launches (dg_rec_feats_backward; the first three keep their bits; `out` may then name four buffers);
    with want_params=False on top the first three are None and one launch forms d feats alone."""
    lib = _lib.load()
    code, feats, weight, bias, keep, scale, (B, D, C, h, w) = _rec_loss_operands(code, feats, weight, bias, keep, scale)
    dev = code.device
    _forward_workspace(workspace, "rec_loss_forward", dev, _rec_loss_workspace_bytes(lib, B, D, C, h, w))
    grad_out = _grad_out_scalar(grad_out, dev)
    if not want_feats:
        if not want_params:
            raise ValueError("depthg_amd: rec_loss_backward(want_params=False) leaves nothing to compute without want_feats=True")
        out = _out_buffers(out, ((B, D, h, w), (C, D), (C,)), ("code", "weight", "bias"), dev)
        rc = lib.dg_recloss_backward(_ptr(code), _ptr(feats), _ptr(weight), _ptr(bias), _ptr(keep), scale, _ptr(workspace), workspace.numel(),
                                     B, D, C, h, w, _ptr(grad_out), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream(dev))
        _lib.check(rc, "dg_recloss_backward")
        return out[0], out[1], out[2]
    if want_params:
        if out is not None and len(out) != 4:
            raise ValueError(f"depthg_amd: rec_loss_backward(want_feats=True) fills four `out` buffers, got {len(out)}")
        out = _out_buffers(out, ((B, D, h, w), (C, D), (C,), (B, C, h, w)), ("code", "weight", "bias", "feats"), dev)
    else:
        if out is not None:
            raise ValueError("depthg_amd: rec_loss_backward(want_params=False) allocates its one result itself")
        out = (None, None, None, _empty((B, C, h, w), torch.float32, dev))
    rc = lib.dg_rec_feats_backward(_ptr(code), _ptr(feats), _ptr(weight), _ptr(bias), _ptr(keep), scale, _ptr(workspace), workspace.numel(),
                                   B, D, C, h, w, _ptr(grad_out), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _stream(dev))
    _lib.check(rc, "dg_rec_feats_backward")
    return out[0], out[1], out[2], out[3]


def depth_encoder_shapes(depth, params, residual=None):
    """The fused depth encoder's shape rules, on any device: depth (B, 1, 8h, 8w) or (B, 8h, 8w); params the ten tensors of the
    three-stage stack in module order (w1, b1, gamma1, beta1, w2, b2, gamma2, beta2, w3, b3); residual None or (B, C, h, w).
    Returns (B, C, h, w)."""
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depthg_amd: the depth map must be (B, 1, H, W) or (B, H, W), got {tuple(depth.shape)}")
    B, H, W = depth.shape
    if B < 1 or H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"depthg_amd: the three-stage depth encoder shrinks by 8: the depth map's {H}x{W} must be positive multiples of 8")
    if len(params) != 10:
        raise ValueError(f"depthg_amd: the three-stage depth encoder has ten parameters, got {len(params)}")
    C = params[8].shape[0]
    want = ((64, 1, 2, 2), (64,), (64,), (64,), (128, 64, 2, 2), (128,), (128,), (128,), (C, 128, 2, 2), (C,))
    names = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")
    for t, sh, name in zip(params, want, names):
        if tuple(t.shape) != sh:
            raise ValueError(f"depthg_amd: depth encoder parameter {name} must be {sh}, got {tuple(t.shape)}")
    if C % 64 or not 64 <= C <= 768:
        raise ValueError(f"depthg_amd: the fused depth encoder takes a last width that is a multiple of 64 up to 768, got C={C}")
    h, w = H // 8, W // 8
    if residual is not None and tuple(residual.shape) != (B, C, h, w):
        raise ValueError(f"depthg_amd: residual must be (B, C, h, w) = {(B, C, h, w)}, the encoder's result, got {tuple(residual.shape)}")
    return B, C, h, w


def _depth_encoder_operands(depth, params, extra, extra_name):
    """The encoder's tensors as the library reads them: fp32 (refused otherwise), on one GPU, contiguous (a strided depth map is
    copied here, once); depth as (B, 8h, 8w).  extra: the residual (or None) / the upstream gradient, shaped (B, C, h, w)."""
    B, C, h, w = depth_encoder_shapes(depth, params, extra)
    names = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")
    tensors = [(depth, "depth"), *zip(params, names)] + ([(extra, extra_name)] if extra is not None else [])
    _gpu_float32(tensors, "the fused depth encoder wants float32 tensors on the GPU, got {name} as {dtype}")
    dev = depth.device
    for t, name in tensors:
        if t.device != dev:
            raise RuntimeError(f"depthg_amd: depth lives on {dev}, {name} on {t.device}")
    depth = depth.detach().reshape(B, 8 * h, 8 * w).contiguous()
    params = [p.detach().contiguous() for p in params]
    extra = extra.detach().contiguous() if extra is not None else None
    return depth, params, extra, (B, C, h, w)


def depth_encoder_workspace_bytes(B, C, h, w, backward):
    return _plan_bytes(_lib.load().dg_depthenc_workspace_bytes(B, C, h, w, 1 if backward else 0), "depth-encoder", f"B={B}, C={C}, grid {h}x{w}",
                       "C a multiple of 64 up to 768, B h w <= 2^24")


def depth_encoder_forward(depth, params, residual=None):
    """The three-stage depth encoder (dg_depthenc_forward; src/modules.py:497-506, :557): depth (B, 1, 8h, 8w) or (B, 8h, 8w), the
    stack's ten parameters in module order, optionally `residual` (B, C, h, w) added in the epilogue (:562-563) -> (B, C, h, w)."""
    lib = _lib.load()
    depth, params, residual, (B, C, h, w) = _depth_encoder_operands(depth, params, residual, "residual")
    dev = depth.device
    ws = _empty((depth_encoder_workspace_bytes(B, C, h, w, False),), torch.uint8, dev)
    out = _empty((B, C, h, w), torch.float32, dev)
    rc = lib.dg_depthenc_forward(_ptr(depth), *[_ptr(p) for p in params], _ptr(residual), h, w, B, C, h, w, 8 * h, 8 * w, _ptr(out), _ptr(ws),
                                 ws.numel(), _stream(dev))
    _lib.check(rc, "dg_depthenc_forward")
    return out


def depth_encoder_backward(depth, params, grad_out, out=None):
    """The gradients of depth_encoder_forward's ten parameters for the upstream gradient `grad_out` (B, C, h, w), in the parameters'
    order and shapes (dg_depthenc_backward); every element written.  out: optional tuple of ten result buffers."""
    lib = _lib.load()
    depth, params, grad_out, (B, C, h, w) = _depth_encoder_operands(depth, params, grad_out, "grad_out")
    dev = depth.device
    names = ("w1", "b1", "gamma1", "beta1", "w2", "b2", "gamma2", "beta2", "w3", "b3")
    out = _out_buffers(out, [tuple(p.shape) for p in params], names, dev)
    ws = _empty((depth_encoder_workspace_bytes(B, C, h, w, True),), torch.uint8, dev)
    rc = lib.dg_depthenc_backward(_ptr(depth), *[_ptr(p) for p in params], _ptr(grad_out), B, C, h, w, 8 * h, 8 * w, *[_ptr(o) for o in out],
                                  _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "dg_depthenc_backward")
    return out


def _fps(depth, depth_pos, feat_hw, n_samples, return_inds):
    """dg_fps_coords on the B maps of `depth` and - not None - on the B of `depth_pos` behind them."""
    lib = _lib.load()
    B, _, H, W = depth.shape
    nB = B if depth_pos is None else 2 * B
    h, w = int(feat_hw[0]), int(feat_hw[1])
    S = int(n_samples)
    coords = _empty((nB, S, S, 2), torch.float32, depth.device)
    inds = _empty((nB, S * S), torch.int32, depth.device) if return_inds else None
    ws = _empty((lib.dg_fps_workspace_bytes(nB, h, w)), torch.uint8, depth.device)         # the pooled depth maps
    rc = lib.dg_fps_coords(_ptr(depth), _ptr(depth_pos), B, H, W, h, w, S, _ptr(coords), _ptr(inds), _ptr(ws), ws.numel(),
                           _stream(depth.device))
    _lib.check(rc, "dg_fps_coords")
    return (coords, inds) if return_inds else coords


def fps_coords(depth, feat_hw, n_samples, return_inds=False):
    """depth (B,1,H,W) on GPU -> coords (B,S,S,2) in [-1,1) (already *2-1)."""
    return _fps(_f32c(depth, "depth"), None, feat_hw, n_samples, return_inds)


def fps_coords_pair(depth, depth_pos, feat_hw, n_samples):
    """The two FPS calls of one step in one launch (dg_fps_coords with depth_pos): depth, depth_pos (B,1,H,W) -> coords (2B,S,S,2),
    rows [0,B) the anchors', [B,2B) the positives'."""
    depth, depth_pos = _f32c(depth, "depth"), _f32c(depth_pos, "depth_pos")
    if depth.shape != depth_pos.shape or depth.device != depth_pos.device:
        raise ValueError(f"depthg_amd: depth {tuple(depth.shape)} on {depth.device} and depth_pos {tuple(depth_pos.shape)} on "
                         f"{depth_pos.device} must match for the paired sampler")
    return _fps(depth, depth_pos, feat_hw, n_samples, False)


FPS_MAX_POSITIONS = 4096             # pooled grids up to here: dg_fps_coords (and the 'simple' / feature-aware samplers' limit)
FPS_LARGE_MAX_POSITIONS = 65536      # ... up to here: dg_fps_coords_large


def _fps_large(depth, depth_pos, feat_hw, n_samples, return_inds):
    """dg_fps_coords_large on the B maps of `depth` and - not None - on the B of `depth_pos` behind them."""
    lib = _lib.load()
    B, _, H, W = depth.shape
    nB = B if depth_pos is None else 2 * B
    h, w = int(feat_hw[0]), int(feat_hw[1])
    S = int(n_samples)
    coords = _empty((nB, S, S, 2), torch.float32, depth.device)
    inds = _empty((nB, S * S), torch.int32, depth.device) if return_inds else None
    # (the pooled depth maps; depth maps of the grid's own size are read in place)
    ws = _empty((lib.dg_fps_large_workspace_bytes(nB, h, w)), torch.uint8, depth.device) if (H, W) != (h, w) else None
    rc = lib.dg_fps_coords_large(_ptr(depth), _ptr(depth_pos), B, H, W, h, w, S, _ptr(coords), _ptr(inds), _ptr(ws),
                                 ws.numel() if ws is not None else 0, _stream(depth.device))
    _lib.check(rc, "dg_fps_coords_large")
    return (coords, inds) if return_inds else coords


def fps_coords_large(depth, feat_hw, n_samples, return_inds=False):
    """fps_coords on pooled grids of up to 65536 positions (dg_fps_coords_large; the grid of the loss under cfg.use_true_labels is
    the labels'): depth (B,1,H,W) on GPU -> coords (B,S,S,2) in [-1,1).  Equal to fps_coords, bit for bit, on every grid both take."""
    return _fps_large(_f32c(depth, "depth"), None, feat_hw, n_samples, return_inds)


def fps_coords_large_pair(depth, depth_pos, feat_hw, n_samples):
    """The two calls of one step in one launch: -> coords (2B,S,S,2), rows [0,B) the anchors', [B,2B) the positives'."""
    depth, depth_pos = _f32c(depth, "depth"), _f32c(depth_pos, "depth_pos")
    if depth.shape != depth_pos.shape or depth.device != depth_pos.device:
        raise ValueError(f"depthg_amd: depth {tuple(depth.shape)} on {depth.device} and depth_pos {tuple(depth_pos.shape)} on "
                         f"{depth_pos.device} must match for the paired sampler")
    return _fps_large(depth, depth_pos, feat_hw, n_samples, False)


LABEL_ONEHOT_MAX_CHANNELS = 256


def _label_map(label, name, n_classes, check):
    """One label tensor as dg_label_onehot reads it: int64 (B,H,W) - or (B,1,H,W) -, contiguous; check: its range, on the host."""
    if not isinstance(label, torch.Tensor) or label.dtype != torch.int64 or label.dim() not in (3, 4) or (label.dim() == 4 and label.shape[1] != 1):
        raise ValueError(f"depthg_amd: `{name}` must be an int64 (B,H,W) or (B,1,H,W) tensor, got "
                         f"{(label.dtype, tuple(label.shape)) if isinstance(label, torch.Tensor) else type(label).__name__}")
    label = label.detach()
    label = (label.squeeze(1) if label.dim() == 4 else label).contiguous()
    if check and label.numel():
        lo, hi = (int(v) for v in torch.aminmax(label))          # (one host sync; check=False launches without it)
        if lo < -1 or hi > n_classes - 1:
            bad = lo if lo < -1 else hi
            raise ValueError(f"depthg_amd: `{name}` holds the value {bad}, outside [-1, {n_classes - 1}] (n_classes = {n_classes}): "
                             "the reference's F.one_hot(label + 1, n_classes + 1) raises on it")
    return label


def label_onehot(label, n_classes, label_pos=None, check=True):
    """one_hot_feats(label + 1, n_classes + 1) of the reference (src/train_segmentation.py:219-225; src/utils.py:64-65) - the
    correlation loss's signal under cfg.use_true_labels: int64 labels (B,H,W) or (B,1,H,W) with values in [-1, n_classes - 1] ->
    fp32 (B, n_classes + 1, H, W), channel label + 1 of a pixel 1.0 and every other 0.0.  With `label_pos` (the same shape): the pair
    (signal, signal_pos), two views of ONE (2B, ...) tensor written by ONE launch (dg_label_onehot: the labels are read in place, no
    int64 one-hot tensor and no permuted copy exist).  On CPU tensors: the reference's torch chain.
    check=True reads the labels' range on the host first (one sync) and raises ValueError naming the offending value, where the
    reference's F.one_hot would raise.  check=False launches without that read (a step recorded in a graph): THE CALLER then vouches
    for the range - the kernel writes an all-zero pixel for a label outside it, where the reference would have raised."""
    n_classes = int(n_classes)
    if n_classes < 0 or n_classes + 1 > LABEL_ONEHOT_MAX_CHANNELS:
        raise ValueError(f"depthg_amd: label_onehot serves 1 <= n_classes + 1 <= {LABEL_ONEHOT_MAX_CHANNELS}, got n_classes = {n_classes}")
    label = _label_map(label, "label", n_classes, check)
    if label_pos is not None:
        label_pos = _label_map(label_pos, "label_pos", n_classes, check)
        if label_pos.shape != label.shape or label_pos.device != label.device:
            raise ValueError(f"depthg_amd: label {tuple(label.shape)} on {label.device} and label_pos {tuple(label_pos.shape)} on "
                             f"{label_pos.device} must match")
    B, H, W = label.shape
    if not label.is_cuda:
        chain = lambda t: torch.nn.functional.one_hot(t + 1, n_classes + 1).permute(0, 3, 1, 2).to(torch.float32)
        if not check:          # (F.one_hot raises on an out-of-range value; the kernel's contract is an all-zero pixel)
            chain = lambda t: (t.unsqueeze(1) + 1 == torch.arange(n_classes + 1).view(1, -1, 1, 1)).to(torch.float32)
        return chain(label) if label_pos is None else (chain(label), chain(label_pos))
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"depthg_amd: label_onehot needs a non-empty label map, got {tuple(label.shape)}")
    nB = B if label_pos is None else 2 * B
    out = _empty((nB, n_classes + 1, H, W), torch.float32, label.device)
    rc = _lib.load().dg_label_onehot(_ptr(label), _ptr(label_pos), B, n_classes, H, W, _ptr(out), _stream(label.device))
    _lib.check(rc, "dg_label_onehot")
    return out if label_pos is None else (out[:B], out[B:])


def sample_rows(t, coords, srcidx=None, bf16=False):
    """sample() of the reference (src/modules.py:822-825) as rows: t (B,K,h,w) fp32, coords (B,S,Sh,2) in [-1,1] -> (B, Sh*S, Kout),
    row p = i*S + j of image n = t[srcidx[n]] (srcidx None: t[n]) sampled at coords[n, j, i], channels K..Kout-1 zero.  fp32 rows with
    Kout = K rounded up to 4, or (bf16=True) bfloat16 rows with Kout = K rounded up to 128 - what the loss's kernels read.  On the GPU
    dg_sample_rows: the four taps of every element read in place from the NCHW map (maps of up to 65536 positions; no copy of the map
    is made).  On CPU tensors: F.grid_sample with the reference's arguments, permuted to rows."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or not isinstance(coords, torch.Tensor) or coords.dim() != 4 or coords.shape[-1] != 2 \
            or coords.shape[0] != t.shape[0]:
        raise ValueError(f"depthg_amd: sample_rows takes a (B,K,h,w) map and (B,S,Sh,2) coordinates, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} and "
                         f"{tuple(coords.shape) if isinstance(coords, torch.Tensor) else type(coords).__name__}")
    B, K, h, w = t.shape
    S, Sh = int(coords.shape[1]), int(coords.shape[2])
    if min(B, K, h, w, S, Sh) < 1:
        raise ValueError(f"depthg_amd: sample_rows needs non-empty operands, got a map {tuple(t.shape)} and coordinates {tuple(coords.shape)}")
    if srcidx is not None and (srcidx.dtype != torch.int64 or tuple(srcidx.shape) != (B,) or srcidx.device != t.device):
        raise ValueError(f"depthg_amd: `srcidx` must be an int64 ({B},) tensor on {t.device}, got {srcidx.dtype} {tuple(srcidx.shape)} on {srcidx.device}")
    if coords.device != t.device:
        raise ValueError(f"depthg_amd: `coords` lives on {coords.device}, the map on {t.device}")
    Kout = (K + 127) // 128 * 128 if bf16 else (K + 3) // 4 * 4
    if not t.is_cuda:
        src = t.detach().to(torch.float32)
        src = src if srcidx is None else src[srcidx]
        rows = torch.nn.functional.grid_sample(src, coords.detach().to(torch.float32).permute(0, 2, 1, 3), padding_mode="border",
                                               align_corners=True).permute(0, 2, 3, 1).reshape(B, Sh * S, K)
        rows = torch.nn.functional.pad(rows, (0, Kout - K))
        return rows.to(torch.bfloat16) if bf16 else rows
    t, coords = _f32c(t, "t"), _f32c(coords, "coords")
    srcidx = srcidx.contiguous() if srcidx is not None else None
    out = _empty((B, Sh * S, Kout), torch.bfloat16 if bf16 else torch.float32, t.device)
    rc = _lib.load().dg_sample_rows(_ptr(t), _ptr(coords), _ptr(srcidx), B, K, h, w, S, Sh, Kout, 1 if bf16 else 0, _ptr(out), _stream(t.device))
    _lib.check(rc, "dg_sample_rows")
    return out


def _fps_feats_operand(t, name):
    """The feature-aware sampler reads its maps in place: a contiguous fp32 GPU tensor, or a refusal by name."""
    _on_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"depthg_amd: `{name}` must be a contiguous 4-D float32 tensor (the sampler reads it in place), got "
                         f"{t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ', not contiguous'}")
    return t.detach()


def _fps_feats(depth, depth_pos, feats, feats_pos, feat_hw, n_samples, return_inds):
    """dg_fps_feats_coords on the B maps of `depth` / `feats` and - not None - on the B of `depth_pos` / `feats_pos` behind them."""
    lib = _lib.load()
    B, _, H, W = depth.shape
    h, w = int(feat_hw[0]), int(feat_hw[1])
    C = feats.shape[1]
    for name, d, f in (("depth", depth, feats),) + ((("depth_pos", depth_pos, feats_pos),) if depth_pos is not None else ()):
        if d.shape[1] != 1 or tuple(f.shape) != (d.shape[0], C, h, w) or f.device != d.device:
            raise ValueError(f"depthg_amd: `{name}` {tuple(d.shape)} on {d.device} needs features ({d.shape[0]}, C, {h}, {w}) on the same device, "
                             f"got {tuple(f.shape)} on {f.device}")
    nB = B if depth_pos is None else 2 * B
    S = int(n_samples)
    coords = _empty((nB, S, S, 2), torch.float32, depth.device)
    inds = _empty((nB, S * S), torch.int32, depth.device) if return_inds else None
    ws = _empty((lib.dg_fps_feats_workspace_bytes(nB, h, w)), torch.uint8, depth.device)         # the pooled depth maps
    rc = lib.dg_fps_feats_coords(_ptr(depth), _ptr(depth_pos), _ptr(feats), _ptr(feats_pos), B, C, H, W, h, w, S, _ptr(coords), _ptr(inds),
                                 _ptr(ws), ws.numel(), _stream(depth.device))
    _lib.check(rc, "dg_fps_feats_coords")
    return (coords, inds) if return_inds else coords


def fps_feats_coords(depth, feats, feat_hw, n_samples, return_inds=False):
    """Farthest point sampling over depth AND features (dg_fps_feats_coords; the reference's fps_depth_feats, src/modules.py:1124-1180,
    inside farthest_point_sampling_depth): depth (B,1,H,W), feats (B,C,h,w) with (h,w) = feat_hw, both contiguous float32 on the GPU
    -> coords (B,S,S,2) in [-1,1) (already *2-1), and the selection order int32 (B,S*S) with return_inds."""
    return _fps_feats(_fps_feats_operand(depth, "depth"), None, _fps_feats_operand(feats, "feats"), None, feat_hw, n_samples, return_inds)


def fps_feats_coords_pair(depth, depth_pos, feats, feats_pos, feat_hw, n_samples):
    """The two calls of one step in one launch over 2B blocks: -> coords (2B,S,S,2), rows [0,B) the anchors', [B,2B) the positives'."""
    depth, depth_pos = _fps_feats_operand(depth, "depth"), _fps_feats_operand(depth_pos, "depth_pos")
    feats, feats_pos = _fps_feats_operand(feats, "feats"), _fps_feats_operand(feats_pos, "feats_pos")
    if depth.shape != depth_pos.shape or depth.device != depth_pos.device or feats.shape != feats_pos.shape:
        raise ValueError(f"depthg_amd: depth {tuple(depth.shape)} on {depth.device} / feats {tuple(feats.shape)} and depth_pos "
                         f"{tuple(depth_pos.shape)} on {depth_pos.device} / feats_pos {tuple(feats_pos.shape)} must match for the paired sampler")
    return _fps_feats(depth, depth_pos, feats, feats_pos, feat_hw, n_samples, False)


def salience_coords(salience, n_side, u_sel=None, u_fallback=None):
    """sample_nonzero_locations (src/modules.py:1191-1204) on the GPU: salience (B,H,W) -> (B,S,S,2), flipped and *2-1 like
    the reference.  u_sel (B,S*S) / u_fallback (B,S*S,2): iid uniforms in [0,1), drawn here unless given (tests)."""
    lib = _lib.load()
    sal = _f32c(salience, "salience")
    if sal.dim() != 3:
        raise ValueError(f"depthg_amd: salience must be (B,H,W) like the reference's batch['mask'].squeeze(1), got {tuple(sal.shape)}")
    B, H, W = sal.shape
    S = int(n_side)
    n = S * S
    dev = sal.device
    u_sel = torch.rand(B, n, device=dev) if u_sel is None else _f32c(u_sel, "u_sel")
    u_fallback = torch.rand(B, n, 2, device=dev) if u_fallback is None else _f32c(u_fallback, "u_fallback")
    assert tuple(u_sel.shape) == (B, n) and tuple(u_fallback.shape) == (B, n, 2)
    coords = _empty((B, S, S, 2), torch.float32, dev)
    rc = lib.dg_salience_coords(_ptr(sal), B, H, W, n, _ptr(u_sel), _ptr(u_fallback), _ptr(coords), _stream(dev))
    _lib.check(rc, "dg_salience_coords")
    return coords


def simple_depth_coords(depth, feat_hw, n_samples, u_value=None, u_pick=None):
    """simple_depth_informed_sampling (src/modules.py:828-883) on the GPU: depth (B,1,H,W) -> coords (B,n,1,2), already
    *2-1 (the caller's step at modules.py:1300).  u_value / u_pick (B,n): iid uniforms, drawn here unless given."""
    lib = _lib.load()
    depth = _f32c(depth, "depth")
    B, _, H, W = depth.shape
    h, w = int(feat_hw[0]), int(feat_hw[1])
    n = int(n_samples)
    dev = depth.device
    u_value = torch.rand(B, n, device=dev) if u_value is None else _f32c(u_value, "u_value")
    u_pick = torch.rand(B, n, device=dev) if u_pick is None else _f32c(u_pick, "u_pick")
    assert tuple(u_value.shape) == (B, n) and tuple(u_pick.shape) == (B, n)
    coords = _empty((B, n, 1, 2), torch.float32, dev)
    rc = lib.dg_simple_depth_coords(_ptr(depth), B, H, W, h, w, n, _ptr(u_value), _ptr(u_pick), _ptr(coords), _stream(dev))
    _lib.check(rc, "dg_simple_depth_coords")
    return coords


def confusion_update(stats, preds, target, n_classes, extra_clusters):
    """stats (n_classes + extra, n_classes) int64 on the GPU += confusion counts of (preds, target) (src/utils.py:222-232)."""
    lib = _lib.load()
    for name, t in (("stats", stats), ("preds", preds), ("target", target)):
        _on_gpu(t, name)
    if stats.dtype != torch.int64 or not stats.is_contiguous() or tuple(stats.shape) != (n_classes + extra_clusters, n_classes):
        raise ValueError("depthg_amd: stats must be a contiguous int64 (n_classes + extra_clusters, n_classes) tensor")
    p = preds.detach().reshape(-1).to(torch.int64).contiguous()
    a = target.detach().reshape(-1).to(torch.int64).contiguous()
    if p.numel() != a.numel():
        raise ValueError(f"depthg_amd: preds and target differ in size ({p.numel()} vs {a.numel()})")
    rc = lib.dg_confusion_update(_ptr(p), _ptr(a), p.numel(), int(n_classes), int(extra_clusters), _ptr(stats), _stream(stats.device))
    _lib.check(rc, "dg_confusion_update")
    return stats


def _probe_args(code, code_flip, lin_w, lin_b, clusters):
    """The probes' arguments of segment_predict / segment_unary, checked: code, code_flip (B,D,h,w); lin_w (n,D) or the 1x1
    convolution's (n,D,1,1); lin_b (n) or None; clusters (m,D).  -> (lin_w as (n,D), (B, D, h, w), n, m)."""
    if code.dim() != 4:
        raise ValueError(f"depthg_amd: code must be (B, D, h, w), got {tuple(code.shape)}")
    D = code.shape[1]
    if code_flip is not None and tuple(code_flip.shape) != tuple(code.shape):
        raise ValueError(f"depthg_amd: code_flip {tuple(code_flip.shape)} differs from code {tuple(code.shape)}")
    if lin_w.dim() == 4 and tuple(lin_w.shape[2:]) == (1, 1):
        lin_w = lin_w.reshape(lin_w.shape[0], lin_w.shape[1])
    if lin_w.dim() != 2 or lin_w.shape[1] != D:
        raise ValueError(f"depthg_amd: lin_w must be (n, {D}) (a 1x1 convolution's weight), got {tuple(lin_w.shape)}")
    n = lin_w.shape[0]
    if lin_b is not None and tuple(lin_b.shape) != (n,):
        raise ValueError(f"depthg_amd: lin_b must be ({n},), got {tuple(lin_b.shape)}")
    if clusters.dim() != 2 or clusters.shape[1] != D:
        raise ValueError(f"depthg_amd: clusters must be (m, {D}), got {tuple(clusters.shape)}")
    return lin_w, tuple(code.shape), n, clusters.shape[0]


def _probe_operands(code, code_flip, lin_w, lin_b, clusters, n, m):
    """The five as the library reads them, and the scratch of the projection at feature resolution (n, m rounded up to 4)."""
    B, _, h, w = code.shape
    named = (("code", code), ("code_flip", code_flip), ("lin_w", lin_w), ("lin_b", lin_b), ("clusters", clusters))
    scratch = _empty((B * h * w * ((n + 3) // 4 * 4 + (m + 3) // 4 * 4) * 4,), torch.uint8, code.device)
    return tuple(_f32c(t, name) for name, t in named) + (scratch,)


def segment_predict(code, label, lin_w, lin_b, clusters, code_flip=None, stats_lin=None, stats_clu=None, n_store=0):
    """The probes' arg-max predictions at the label resolution and their confusion counts (dg_segment_predict; the chain of
    src/train_segmentation.py:471-499 and, with `code_flip`, src/eval_segmentation.py:146-170 without the CRF).
    code, code_flip (B,D,h,w); lin_w (n,D) or (n,D,1,1); lin_b (n) or None; clusters (m,D); label (B,H,W) (or any shape ending in
    (H,W) with B*H*W elements).  stats_lin / stats_clu: int64 (rows, n) on the GPU, += the counts [pred][label] in place (rows >= n
    are never touched), or None.  Returns (preds_lin, preds_clu), int64 (n_store,H,W), or (None, None) when n_store is 0."""
    lib = _lib.load()
    lin_w, (B, D, h, w), n, m = _probe_args(code, code_flip, lin_w, lin_b, clusters)
    if label.dim() < 2 or label.numel() != B * label.shape[-2] * label.shape[-1]:
        raise ValueError(f"depthg_amd: label must hold (B={B}, H, W) elements, got {tuple(label.shape)}")
    H, W = label.shape[-2:]
    for name, st, rows in (("stats_lin", stats_lin, n), ("stats_clu", stats_clu, min(n, m))):
        if st is not None and (st.dtype != torch.int64 or not st.is_contiguous() or st.dim() != 2 or st.shape[1] != n
                               or st.shape[0] < rows):
            raise ValueError(f"depthg_amd: {name} must be a contiguous int64 (rows >= {rows}, {n}) tensor, got "
                             f"{st.dtype} {tuple(st.shape)}")
    n_store = int(n_store)
    if n_store < 0:
        raise ValueError(f"depthg_amd: n_store must be >= 0, got {n_store}")
    n_store = min(n_store, B)
    tensors = (("code", code), ("label", label), ("lin_w", lin_w), ("lin_b", lin_b), ("clusters", clusters),
               ("code_flip", code_flip), ("stats_lin", stats_lin), ("stats_clu", stats_clu))
    for name, t in tensors:
        if t is not None:
            _on_gpu(t, name)
    dev = code.device
    code, code_flip, lin_w, lin_b, clusters, scratch = _probe_operands(code, code_flip, lin_w, lin_b, clusters, n, m)
    lab = label.detach().to(torch.int64).reshape(B, H, W).contiguous()
    preds_lin = _empty((n_store, H, W), torch.int64, dev) if n_store else None
    preds_clu = _empty((n_store, H, W), torch.int64, dev) if n_store else None
    rc = lib.dg_segment_predict(_ptr(code), _ptr(code_flip), B, D, h, w, _ptr(lin_w), _ptr(lin_b), n, _ptr(clusters), m, _ptr(lab),
                                H, W, _ptr(stats_lin), _ptr(stats_clu), n_store, _ptr(preds_lin), _ptr(preds_clu), _ptr(scratch),
                                scratch.numel(), _stream(dev))
    _lib.check(rc, "dg_segment_predict")
    return preds_lin, preds_clu


IMAGENET_MEAN = (0.485, 0.456, 0.406)          # the loader's T.Normalize (src/utils.py:139)
IMAGENET_STD = (0.229, 0.224, 0.225)
SEGMENT_OUTPUTS = ("lin", "clu", "lin_rgb", "clu_rgb")


def pascal_colormap(rows=256):
    """The PASCAL VOC colour map, uint8 (rows, 3), by its public rule: the bits of the class id go, three at a time from the lowest,
    to red, green and blue, filling each channel from its highest bit down."""
    cmap = torch.zeros(rows, 3, dtype=torch.uint8)
    for i in range(rows):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for k in range(3):
                rgb[k] |= ((c >> k) & 1) << (7 - j)
            c >>= 3
        cmap[i] = torch.tensor(rgb, dtype=torch.uint8)
    return cmap


_default_cmaps = {}


def _paint_operands(dev, B, H, W, m, remap, img, cmap, alpha, want, mean, std, out):
    """What dg_segment_labels and dg_label_paint share, checked and as the library reads it: (remap, img, mean, std, cmap, cmap_rows,
    alpha256, outputs) - outputs a dict over SEGMENT_OUTPUTS of uint8 tensors or None (taken from `out` where it has the key)."""
    want = tuple(want)
    if not want or any(k not in SEGMENT_OUTPUTS for k in want):
        raise ValueError(f"depthg_amd: want must name some of {SEGMENT_OUTPUTS}, got {want}")
    if remap is not None:
        remap = torch.as_tensor(remap)
        if remap.dim() != 1 or remap.numel() != m or remap.dtype.is_floating_point:
            raise ValueError(f"depthg_amd: remap must be an integer table of the m={m} cluster ids, got {remap.dtype} {tuple(remap.shape)}")
        # (the table is device data to the library, which stores any entry it cannot put in a byte as 255: refuse it here, by name)
        if remap.numel() and (int(remap.min()) < -1 or int(remap.max()) > 254):
            raise ValueError(f"depthg_amd: remap entries must lie in [-1, 254] (-1: no class, stored as 255), got "
                             f"[{int(remap.min())}, {int(remap.max())}]")
        remap = remap.detach().to(device=dev, dtype=torch.int32).contiguous()
    colour = any(k.endswith("rgb") for k in want)
    alpha256 = int(round(float(alpha) * 256))
    if not 0 <= alpha256 <= 256:
        raise ValueError(f"depthg_amd: alpha must lie in [0, 1], got {alpha}")
    cmean = cstd = None
    if colour:
        if alpha256 < 256 and img is None:
            raise ValueError(f"depthg_amd: alpha = {alpha} < 1 blends the colours with the image: img is needed")
        if cmap is None:
            if dev not in _default_cmaps:
                _default_cmaps[dev] = pascal_colormap().to(dev)
            cmap = _default_cmaps[dev]
        if cmap.dtype != torch.uint8 or cmap.dim() != 2 or cmap.shape[1] != 3 or not 1 <= cmap.shape[0] <= 256:
            raise ValueError(f"depthg_amd: cmap must be uint8 (rows <= 256, 3), got {cmap.dtype} {tuple(cmap.shape)}")
        cmap = _on_gpu(cmap, "cmap").contiguous()
        if alpha256 < 256:
            img = _crf_image(img, B, H, W)
            if len(mean) != 3 or len(std) != 3:
                raise ValueError("depthg_amd: mean and std must have three entries")
            cmean, cstd = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
        else:
            img = None
    else:
        cmap = img = None
    shapes = {"lin": (B, H, W), "clu": (B, H, W), "lin_rgb": (B, H, W, 3), "clu_rgb": (B, H, W, 3)}
    outs = {k: None for k in SEGMENT_OUTPUTS}
    for k in want:
        t = out.get(k) if out else None
        if t is None:
            t = _empty(shapes[k], torch.uint8, dev)
        elif t.dtype != torch.uint8 or tuple(t.shape) != shapes[k] or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"depthg_amd: out[{k!r}] must be a contiguous uint8 {shapes[k]} tensor on {dev}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
        outs[k] = t
    return remap, img, cmean, cstd, cmap, (cmap.shape[0] if cmap is not None else 0), alpha256, outs


def segment_labels(code, lin_w, lin_b, clusters, H, W, code_flip=None, remap=None, img=None, cmap=None, alpha=1.0,
                   want=("lin", "clu"), mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """Label-free inference (dg_segment_labels; src/demo_segmentation.py:59-78 without the CRF): both probes' arg-max label maps of
    every image at (H, W) as bytes - ops.segment_predict's predictions bit for bit - and their painted images.
    code, code_flip, lin_w, lin_b, clusters: as segment_predict (n, m <= 255).  remap: integer (m) table cluster id -> class id
    (UnsupervisedMetrics.map_clusters; -1 is stored as 255) or None (the raw cluster id).  want: which of "lin", "clu" (uint8
    (B,H,W)) and "lin_rgb", "clu_rgb" (uint8 (B,H,W,3)) to write.  A colour is (a cmap[label] + (256 - a) pix + 128) >> 8 with
    a = round(256 alpha) and pix the de-normalised byte of img (B,3,H,W) (needed when alpha < 1); cmap: uint8 (rows <= 256, 3) on the
    GPU, default the PASCAL map; a label past the map (255 among them) paints its last row.  out: a dict of tensors to write
    into instead of new ones (keys of `want`; other keys are ignored and never touched).  Returns a dict over `want`."""
    lib = _lib.load()
    lin_w, (B, D, h, w), n, m = _probe_args(code, code_flip, lin_w, lin_b, clusters)
    H, W = int(H), int(W)
    dev = code.device
    code, code_flip, lin_w, lin_b, clusters, scratch = _probe_operands(code, code_flip, lin_w, lin_b, clusters, n, m)
    remap, img, cmean, cstd, cmap, rows, alpha256, outs = _paint_operands(dev, B, H, W, m, remap, img, cmap, alpha, want, mean, std, out)
    rc = lib.dg_segment_labels(_ptr(code), _ptr(code_flip), B, D, h, w, _ptr(lin_w), _ptr(lin_b), n, _ptr(clusters), m, H, W, _ptr(remap),
                               _ptr(img), cmean, cstd, _ptr(cmap), rows, alpha256, _ptr(outs["lin"]), _ptr(outs["clu"]),
                               _ptr(outs["lin_rgb"]), _ptr(outs["clu_rgb"]), _ptr(scratch), scratch.numel(), _stream(dev))
    _lib.check(rc, "dg_segment_labels")
    return {k: v for k, v in outs.items() if v is not None}


def label_paint(preds, m=None, remap=None, img=None, cmap=None, alpha=1.0, want=("lin", "clu"), mean=IMAGENET_MEAN, std=IMAGENET_STD,
                out=None):
    """The remap and paint of segment_labels on the dense CRF's predictions (dg_label_paint): preds int64 (G,B,H,W) on the GPU as
    ops.dense_crf(..., return_preds=True) returns them, preds[0] the linear probe's map and preds[1] the cluster probe's.  m: the
    number of clusters (default: remap's length, else 255).  A value no byte label holds (outside [0, 254]) is stored as 255."""
    lib = _lib.load()
    if preds.dim() != 4 or preds.dtype != torch.int64:
        raise ValueError(f"depthg_amd: preds must be int64 (G, B, H, W), got {preds.dtype} {tuple(preds.shape)}")
    preds = _on_gpu(preds, "preds").contiguous()
    G, B, H, W = preds.shape
    if m is None:
        m = len(remap) if remap is not None else 255
    dev = preds.device
    remap, img, cmean, cstd, cmap, rows, alpha256, outs = _paint_operands(dev, B, H, W, int(m), remap, img, cmap, alpha, want, mean, std, out)
    rc = lib.dg_label_paint(_ptr(preds), G, B, H, W, int(m), _ptr(remap), _ptr(img), cmean, cstd, _ptr(cmap), rows, alpha256,
                            _ptr(outs["lin"]), _ptr(outs["clu"]), _ptr(outs["lin_rgb"]), _ptr(outs["clu_rgb"]), _stream(dev))
    _lib.check(rc, "dg_label_paint")
    return {k: v for k, v in outs.items() if v is not None}


def _crf_groups(group_ends, C=None):
    ends = [int(e) for e in group_ends]
    if not ends or any(b <= a for a, b in zip([0] + ends, ends)) or (C is not None and ends[-1] != C):
        raise ValueError(f"depthg_amd: group ends must rise strictly from above 0 to the channel count ({C}), got {ends}")
    kp = sum((b - a + 3) // 4 * 4 for a, b in zip([0] + ends, ends))
    return ends, (ctypes.c_int32 * len(ends))(*ends), kp


CRF_WORKSPACE_BUDGET = 1 << 30        # bytes dense_crf / crf_filter allocate at most beyond one image's need (images go in chunks)


def _crf_workspace(lib, B, H, W, kp, dev, budget, lattices):
    """The workspace of the largest chunk of images that fits `budget` (at least one image); lattices: 1 Gaussian, 2 bilateral,
    3 both."""
    one = lib.dg_crf_workspace_bytes(1, H, W, kp, lattices)
    if one == 0:
        raise ValueError(f"depthg_amd: no CRF workspace plan for {H}x{W} pixels and {kp} padded channels")
    c = max(1, min(B, int(budget) // one))
    while c > 1 and not 0 < lib.dg_crf_workspace_bytes(c, H, W, kp, lattices) <= budget:     # 0: the chunk is refused
        c -= 1
    return _empty((lib.dg_crf_workspace_bytes(c, H, W, kp, lattices),), torch.uint8, dev)


def _crf_image(img, B, H, W):
    if img.dim() != 4 or tuple(img.shape) != (B, 3, H, W):
        raise ValueError(f"depthg_amd: img must be ({B}, 3, {H}, {W}), got {tuple(img.shape)}")
    return _f32c(img, "img")


def crf_unary(logits, H, W, group_ends=None):
    """U = -log(clip(softmax(interp(logits)), 1e-5, 1)) (dg_crf_unary; src/crf.py:27-35): logits (B,C,h,w) fp32 on the GPU resized
    to (H,W) (bilinear, align_corners=False), one softmax per channel group (group_ends; None: one group).  Returns (B,C,H,W)."""
    lib = _lib.load()
    if logits.dim() != 4:
        raise ValueError(f"depthg_amd: logits must be (B, C, h, w), got {tuple(logits.shape)}")
    B, C, h, w = logits.shape
    _, ends, _ = _crf_groups([C] if group_ends is None else group_ends, C)
    logits = _f32c(logits, "logits")
    U = _empty((B, C, int(H), int(W)), torch.float32, logits.device)
    rc = lib.dg_crf_unary(_ptr(logits), B, C, h, w, int(H), int(W), ends, len(ends), _ptr(U), _stream(logits.device))
    _lib.check(rc, "dg_crf_unary")
    return U


def segment_unary(code, lin_w, lin_b, clusters, H, W, code_flip=None, alpha=2.0):
    """The evaluation's CRF unary (dg_segment_unary; src/eval_segmentation.py:150-167): code (B,D,h,w) (averaged with
    code_flip.flip(3) when given) resized to (H,W), linear probe lin_w (n,D) / lin_b -> channels [0, n), cluster probe (clusters
    (m,D), alpha) -> channels [n, n + m), U per probe.  Returns (B, n + m, H, W) fp32."""
    lib = _lib.load()
    lin_w, (B, D, h, w), n, m = _probe_args(code, code_flip, lin_w, lin_b, clusters)
    dev = code.device
    code, code_flip, lin_w, lin_b, clusters, scratch = _probe_operands(code, code_flip, lin_w, lin_b, clusters, n, m)
    U = _empty((B, n + m, int(H), int(W)), torch.float32, dev)
    rc = lib.dg_segment_unary(_ptr(code), _ptr(code_flip), B, D, h, w, _ptr(lin_w), _ptr(lin_b), n, _ptr(clusters), m, int(H), int(W),
                              float(alpha), _ptr(U), _ptr(scratch), scratch.numel(), _stream(dev))
    _lib.check(rc, "dg_segment_unary")
    return U


def crf_filter(values, img=None, bilateral=False, sxy=1.0, srgb=3.0, workspace_budget=CRF_WORKSPACE_BUDGET):
    """One normalised dense-CRF message K~(values) = norm * K(norm * values) (dg_crf_filter; densecrf's DenseKernel with
    NORMALIZE_SYMMETRIC): the Gaussian kernel over (x, y) / sxy, or (bilateral) over ((x, y) / sxy, (B, G, R) / srgb) of the
    normalised image img (B,3,H,W).  values (B,C,H,W) fp32 on the GPU; returns (B,C,H,W)."""
    lib = _lib.load()
    if values.dim() != 4:
        raise ValueError(f"depthg_amd: values must be (B, C, H, W), got {tuple(values.shape)}")
    B, C, H, W = values.shape
    values = _f32c(values, "values")
    if bilateral:
        if img is None:
            raise ValueError("depthg_amd: the bilateral kernel needs the image")
        img = _crf_image(img, B, H, W)
    elif img is not None:
        img = _crf_image(img, B, H, W)
    dev = values.device
    kp = (C + 3) // 4 * 4
    ws = _crf_workspace(lib, B, H, W, kp, dev, workspace_budget, 2 if bilateral else 1)
    out = _empty((B, C, H, W), torch.float32, dev)
    rc = lib.dg_crf_filter(_ptr(img), _ptr(values), B, C, H, W, int(bool(bilateral)), float(sxy), float(srgb), _ptr(out), _ptr(ws),
                           ws.numel(), _stream(dev))
    _lib.check(rc, "dg_crf_filter")
    return out


def dense_crf(img, unary, group_ends=None, n_iter=10, pos_w=3.0, pos_xy_std=1.0, bi_w=4.0, bi_xy_std=67.0, bi_rgb_std=3.0,
              return_q=True, return_preds=False, workspace_budget=CRF_WORKSPACE_BUDGET):
    """Mean-field dense CRF (dg_dense_crf; src/crf.py dense_crf): img (B,3,H,W) normalised, unary U (B,C,H,W) fp32 on the GPU, one
    softmax per channel group (group_ends; None: one group).  Returns (Q (B,C,H,W) fp32 or None, preds (G,B,H,W) int64 or None):
    preds[g] is the arg-max of Q within group g, counted from the group's first channel."""
    lib = _lib.load()
    if unary.dim() != 4:
        raise ValueError(f"depthg_amd: unary must be (B, C, H, W), got {tuple(unary.shape)}")
    B, C, H, W = unary.shape
    ends, cends, kp = _crf_groups([C] if group_ends is None else group_ends, C)
    if not (return_q or return_preds):
        raise ValueError("depthg_amd: dense_crf needs return_q or return_preds")
    unary = _f32c(unary, "unary")
    img = _crf_image(img, B, H, W)
    dev = unary.device
    ws = _crf_workspace(lib, B, H, W, kp, dev, workspace_budget, 3)
    q = _empty((B, C, H, W), torch.float32, dev) if return_q else None
    preds = _empty((len(ends), B, H, W), torch.int64, dev) if return_preds else None
    rc = lib.dg_dense_crf(_ptr(img), _ptr(unary), B, H, W, cends, len(ends), int(n_iter), float(pos_w), float(pos_xy_std), float(bi_w),
                          float(bi_xy_std), float(bi_rgb_std), _ptr(q), _ptr(preds), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "dg_dense_crf")
    return q, preds


def adam_step(segs, groups, device_steps=False, tickets=None):
    """torch.optim.Adam's default update of every listed tensor in ONE launch (dg_adam_step; src/train_segmentation.py:447-449).
    segs   : sequence of (param, grad, exp_avg, exp_avg_sq, step, group) - fp32 contiguous tensors on the GPU; grad None = the
             segment is skipped (state and step untouched); step = the count AFTER this step as a Python number (host mode), or
             the float32 0-dim device tensor the kernel reads and advances (device_steps); group indexes `groups`
    groups : sequence of (lr, beta1, beta2, eps)
    tickets: device_steps only - int32 zeros (len(segs),) on the GPU, left zero by every call."""
    lib = _lib.load()
    n = len(segs)
    table = (_lib.AdamSeg * max(n, 1))()
    dev = None
    for k, (p, g, m, v, step, gi) in enumerate(segs):
        for name, t in (("param", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v)):
            if t is None and name == "grad":
                continue
            _on_gpu(t, name)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != p.device:
                raise ValueError(f"depthg_amd: adam_step segment {k}: `{name}` must be a contiguous fp32 tensor of the parameter's size and device "
                                 f"(got {t.dtype}, {tuple(t.shape)}, {t.device})")
        if dev is None:
            dev = p.device
        elif p.device != dev:
            raise RuntimeError(f"depthg_amd: adam_step: parameters on {dev} and {p.device} in one call")
        e = table[k]
        e.param, e.exp_avg, e.exp_avg_sq = p.data_ptr(), m.data_ptr(), v.data_ptr()
        e.grad = g.data_ptr() if g is not None else None
        e.numel, e.group = p.numel(), int(gi)
        if device_steps:
            if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32 and step.numel() == 1):
                raise ValueError(f"depthg_amd: adam_step segment {k}: the device step must be a float32 scalar on the GPU")
            e.step_dev = step.data_ptr()
        else:
            e.step_host = float(step)
    if n == 0:
        return
    gt = (_lib.AdamGroup * len(groups))()
    for k, (lr, b1, b2, eps) in enumerate(groups):
        gt[k].lr, gt[k].beta1, gt[k].beta2, gt[k].eps = float(lr), float(b1), float(b2), float(eps)
    if tickets is not None and not (tickets.is_cuda and tickets.dtype == torch.int32 and tickets.numel() >= n and tickets.is_contiguous()):
        raise ValueError("depthg_amd: adam_step: `tickets` must be int32 (len(segs),) on the GPU")
    rc = lib.dg_adam_step(table, n, gt, len(groups), 1 if device_steps else 0, _ptr(tickets if device_steps else None), _stream(dev))
    _lib.check(rc, "dg_adam_step")


def topk_rows(vals, k, return_values=False):
    """Column indices of the k largest entries of every row of `vals` (rows, cols) fp32 on the GPU: value descending, ties by
    ascending column (src/precompute_knns.py:110 `torch.topk(pairwise_sims, 30)[1]`)."""
    lib = _lib.load()
    _on_gpu(vals, "vals")
    if vals.dim() != 2 or vals.dtype != torch.float32 or vals.stride(1) != 1:
        raise ValueError("depthg_amd: topk_rows wants a 2-D fp32 tensor with contiguous rows")
    rows, cols = vals.shape
    idx = _empty((rows, int(k)), torch.int64, vals.device)
    val = _empty((rows, int(k)), torch.float32, vals.device) if return_values else None
    rc = lib.dg_topk_rows(_ptr(vals), rows, cols, vals.stride(0) if rows > 1 else cols, int(k), _ptr(idx), _ptr(val), _stream(vals.device))
    _lib.check(rc, "dg_topk_rows")
    return (idx, val) if return_values else idx


def knn_similarities(queries, feats):
    """queries (m, F), feats (n, F) fp32 on the GPU (rows contiguous) -> (m, n) fp32 similarities, `einsum("nf,mf->nm")` of
    src/precompute_knns.py:106-108 on the fp32 MFMA."""
    lib = _lib.load()
    for name, t in (("queries", queries), ("feats", feats)):
        _on_gpu(t, name)
        if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
            raise ValueError(f"depthg_amd: `{name}` must be a 2-D fp32 tensor with contiguous rows")
    if queries.shape[1] != feats.shape[1] or queries.device != feats.device:
        raise RuntimeError(f"depthg_amd: queries {tuple(queries.shape)} on {queries.device} and feats {tuple(feats.shape)} on {feats.device} do not match")
    m, F = queries.shape
    n = feats.shape[0]
    out = _empty((m, n), torch.float32, feats.device)
    rc = lib.dg_knn_similarities(_ptr(queries), _ptr(feats), m, n, F, queries.stride(0) if m > 1 else F, feats.stride(0) if n > 1 else F,
                                 _ptr(out), n, _stream(feats.device))
    _lib.check(rc, "dg_knn_similarities")
    return out


def lhp_forward(code, depth):
    """code (B,D,h,w), depth (B,1,H,W) on the GPU -> (code_mixed, points, stats) of dg_lhp_forward."""
    lib = _lib.load()
    code = _f32c(code, "code")
    depth = _f32c(depth, "depth")
    B, D, h, w = code.shape
    out = _empty(tuple(code.shape), torch.float32, code.device)
    points = _empty((B, 3, h * w), torch.float32, code.device)
    stats = _empty((B, h * w, 3), torch.float32, code.device)
    rc = lib.dg_lhp_forward(_ptr(code), _ptr(depth), B, D, h, w, depth.shape[-2], depth.shape[-1], _ptr(out), _ptr(points),
                            _ptr(stats), _stream(code.device))
    _lib.check(rc, "dg_lhp_forward")
    return out, points, stats


def lhp_backward(grad_out, points, stats):
    lib = _lib.load()
    g = _f32c(grad_out, "grad_out")
    B, D, h, w = g.shape
    grad_code = _empty(tuple(g.shape), torch.float32, g.device)
    rc = lib.dg_lhp_backward(_ptr(g), _ptr(points), _ptr(stats), B, D, h, w, _ptr(grad_code), _stream(g.device))
    _lib.check(rc, "dg_lhp_backward")
    return grad_code


LHP_ATTN, LHP_ORIG_DEPTH, LHP_ORIG_ATTN = 0, 1, 2          # enum of include/depthg_corr.h


def lhp_map_forward(mode, code, attn=None, depth=None, divide=None):
    """dg_lhp_map_forward: code (B,D,h,w) with attn (B,heads,h*w+1,h*w+1) or depth (B,1,H,W) -> (code_mixed, map).
    `map` is what dg_lhp_map_backward needs: (B,P,P) for LHP_ATTN, (B,P,9) for the Original variants."""
    lib = _lib.load()
    code = _f32c(code, "code")
    B, D, h, w = code.shape
    P = h * w
    heads, dh, dw, points = 0, 0, 0, None
    if mode == LHP_ORIG_DEPTH:
        depth = _f32c(depth, "depth")
        dh, dw = depth.shape[-2], depth.shape[-1]
        points = _empty((B, 3, P), torch.float32, code.device)
    else:
        attn = _f32c(attn, "attn")
        if attn.dim() != 4 or attn.shape[0] != B or attn.shape[2] != P + 1 or attn.shape[3] != P + 1:
            raise ValueError(f"attn must be (B, heads, {P + 1}, {P + 1}) for a {h}x{w} code map, got {tuple(attn.shape)}")
        heads = attn.shape[1]
    if mode != LHP_ATTN:
        divide = _f32c(divide, "divide")
        if divide.numel() != P:
            raise ValueError(f"divide must hold {P} divisors, got {divide.numel()}")
    out = _empty(tuple(code.shape), torch.float32, code.device)
    wmap = _empty((B, P, P if mode == LHP_ATTN else 9), torch.float32, code.device)
    rc = lib.dg_lhp_map_forward(mode, _ptr(code), _ptr(attn) if mode != LHP_ORIG_DEPTH else None,
                                _ptr(depth) if mode == LHP_ORIG_DEPTH else None, _ptr(divide) if mode != LHP_ATTN else None,
                                B, D, h, w, heads, dh, dw, _ptr(out), _ptr(wmap), _ptr(points), _stream(code.device))
    _lib.check(rc, "dg_lhp_map_forward")
    return out, wmap


def lhp_map_backward(mode, grad_out, wmap, divide=None):
    lib = _lib.load()
    g = _f32c(grad_out, "grad_out")
    B, D, h, w = g.shape
    grad_code = _empty(tuple(g.shape), torch.float32, g.device)
    rc = lib.dg_lhp_map_backward(mode, _ptr(g), _ptr(wmap), _ptr(divide) if mode != LHP_ATTN else None, B, D, h, w,
                                 _ptr(grad_code), _stream(g.device))
    _lib.check(rc, "dg_lhp_map_backward")
    return grad_code


def new_perm_state(device):
    """Device-resident generator state for super_perms(state=...): int64 {seed, draws so far, 0}; the seed comes from torch's
    CPU generator, so torch.manual_seed before the first use fixes the whole sequence."""
    return torch.tensor([_cpu_seed(), 0, 0], dtype=torch.int64, device=device)


def rand_coords_state(state, shape):
    """Two coordinate tensors of `shape` (B, S, S2, 2), uniform in [-1, 1), from the device-resident generator `state`
    (new_perm_state) in ONE launch - for steps recorded in a hipGraph (dg_rand_coords_state); advances the state."""
    lib = _lib.load()
    _check_state(state, "rand_coords_state")
    both = _empty((2,) + tuple(int(v) for v in shape), torch.float32, state.device)
    rc = lib.dg_rand_coords_state(_ptr(state), both.numel(), _ptr(both), _stream(state.device))
    _lib.check(rc, "dg_rand_coords_state")
    return both[0], both[1]


def keep_masks_state(state, rows, C, p=0.1, use=(True, True, True)):
    """The Dropout2d keep masks of a graph-recorded step from the device-resident generator, ONE launch: a tuple of three (rows, C)
    tensors of 1 / 0 (keep with probability 1 - p), None where `use` is False - what ProjectionHead.forward(_pair) takes as `keeps`
    (rows = B, or 2B for forward_pair).  Advances the state; not torch's random stream."""
    lib = _lib.load()
    _check_state(state, "keep_masks_state")
    k = sum(1 for u in use if u)
    if k == 0:
        return (None, None, None)
    buf = _empty((k, int(rows), int(C)), torch.float32, state.device)
    rc = lib.dg_rand_keep_state(_ptr(state), buf.numel(), float(1.0 - p), _ptr(buf), _stream(state.device))
    _lib.check(rc, "dg_rand_keep_state")
    it = iter(range(k))
    return tuple(buf[next(it)] if u else None for u in use)


def super_perms(count, size, device, keys=None, state=None):
    """(count, size) int64: independent super_perm draws (src/modules.py:1184-1188), one kernel.  `state` (new_perm_state):
    the draw is keyed by device memory and advances it - safe to record in a hipGraph (every replay draws anew)."""
    lib = _lib.load()
    out = _empty((count, size), torch.long, device)
    if count == 0:
        return out
    if state is not None:
        _check_state(state, "super_perms", out.device)
        keys = None                              # (the state decides, as ever)
    # neither: the keys are drawn inside the kernel (Philox) from a seed of torch's CPU generator, still one launch
    seed = _cpu_seed() if state is None and keys is None else 0
    rc = lib.dg_super_perms(_ptr(keys), seed, _ptr(state), int(count), int(size), _ptr(out), _stream(out.device))
    _lib.check(rc, "dg_super_perms")
    return out


def corr_relaunch_main(desc, perms, workspace):
    """Measurement aid: launch only the fused correlation kernel again (operands already in `workspace`)."""
    lib = _lib.load()
    rc = lib.dg_corr_relaunch_main(ctypes.byref(desc), _ptr(perms), _ptr(workspace), workspace.numel(),
                                   _stream(workspace.device))
    _lib.check(rc, "dg_corr_relaunch_main")


class MainKernelTimer:
    """Measurement aid (bench.py): the execution span of the fused correlation launch INSIDE the step, hipGraph replays included
    (dg_prof_main_span): while armed, every workgroup of that kernel stamps its entry / exit time (the GPU's constant 100-MHz
    clock) into two device words with atomic min / max and adds its lifetime in shader cycles / wall ticks to two more.
    `reset()` in front of a step (an asynchronous copy on the current stream), `last_ms()` / `last()` behind it: the interval a
    kernel trace reports for the launch, minus the dispatch ramp, and the clock the kernel's CUs held.  A hipGraph captured while
    the timer is armed keeps writing to `span` at every replay: keep the timer alive as long as such a graph."""

    def __init__(self, device):
        self.span = torch.zeros(4, dtype=torch.int64, device=device)
        self._init = torch.tensor([-1, 0, 0, 0], dtype=torch.int64, device=device)       # {UINT64_MAX, 0, 0, 0}

    def arm(self, on=True):
        _lib.check(_lib.load().dg_prof_main_span(_ptr(self.span) if on else None), "dg_prof_main_span")

    def reset(self):
        self.span.copy_(self._init, non_blocking=True)

    def last(self):
        """(span in ms, held shader clock in GHz) of the launches since the last reset; (nan, nan) when nothing was stamped."""
        torch.cuda.synchronize()
        t0, t1, cyc, ticks = (int(v) for v in self.span.tolist())
        if t0 < 0 or t1 <= 0:                      # nothing stamped
            return float("nan"), float("nan")
        ghz = cyc / ticks * 0.1 if ticks > 0 else float("nan")      # cycles per 10-ns tick
        return (t1 - t0) * 1e-5, ghz               # 10-ns ticks -> ms

    def last_ms(self):
        return self.last()[0]


def corr_intra_folded(desc):
    """True when the fused correlation launch of `desc` also forms the intra pair-set's streamed-side gradient (k_corr2's FOLD)."""
    rc = _lib.load().dg_corr_intra_folded(ctypes.byref(desc))
    if rc < 0:
        _lib.check(-1, "dg_corr_intra_folded")
    return rc == 1


def corr_main_kernel_name(desc):
    """Which kernel the fused correlation launch of `desc` runs ("k_corr2" / "k_corr_main"), from the library's own predicate."""
    name = _lib.load().dg_corr_main_kernel_name(ctypes.byref(desc))
    if name is None:
        _lib.check(-1, "dg_corr_main_kernel_name")
    return name.decode()


HeadPlan = collections.namedtuple("HeadPlan", "dh_route dh_blocks tiles wgrad_pair wgrad_single s2a s1 s2b step_major")
_HEAD_DH_ROUTES = ("TILES", "FUSED")
_HEAD_WGRAD_FORMS = ("DIRECT", "GROUPED", "ONE_PASS")


def head_plan(B, C, D, P):
    """The routes dg_head_backward takes for B images (both passes of a pair call: 2 B) of C channels, D code channels and P
    positions, from the library's own plan (dg_head_plan_describe): dh_route "TILES" (k_head_dh) / "FUSED" (k_head_dh2 on
    dh_blocks persistent blocks, d W2b inside), tiles per image, wgrad_pair (the d W2a + d W1 launch, s2a splits) and wgrad_single
    (a product alone, s1 splits) "DIRECT" / "GROUPED" / "ONE_PASS", s2b partial sums of d W2b, step_major.  Touches no GPU."""
    out = (ctypes.c_int32 * 9)()
    _lib.check(_lib.load().dg_head_plan_describe(int(B), int(C), int(D), int(P), out), "dg_head_plan_describe")
    v = list(out)
    return HeadPlan(_HEAD_DH_ROUTES[v[0]], v[1], v[2], _HEAD_WGRAD_FORMS[v[3]], _HEAD_WGRAD_FORMS[v[4]], v[5], v[6], v[7], bool(v[8]))


def attention_forward(qkv, heads, scale=None, out=None):
    """softmax(q k^T * scale) v of one ViT block (dg_attention_forward; src/dino/vision_transformer.py:80-92) without the
    (B, heads, N, N) matrix: qkv (B, N, 3 * heads * 64) fp32 contiguous on the GPU - the output of the block's qkv linear as it
    stands - -> (B, N, heads * 64) fp32, the input of its proj linear.  scale: None = 64 ** -0.5.  out: optional result buffer.
    Forward only (the backbone is frozen); bf16 MFMA operands, fp32 softmax.  Runs on the caller's current stream."""
    heads = int(heads)
    if qkv.dim() != 3 or heads < 1 or qkv.shape[2] % (3 * heads):
        raise ValueError(f"depthg_amd: qkv must be (B, N, 3 * heads * 64) with heads={heads}, got {tuple(qkv.shape)}")
    B, N, C3 = qkv.shape
    hd = C3 // (3 * heads)
    if hd != 64:
        raise ValueError(f"depthg_amd: attention_forward is built for head dimension 64 (every DINO ViT), got {hd}")
    if qkv.dtype != torch.float32:
        raise ValueError(f"depthg_amd: qkv must be float32, got {qkv.dtype}")
    if not qkv.is_contiguous():
        raise ValueError(f"depthg_amd: qkv must be contiguous (strides {qkv.stride()})")
    _on_gpu(qkv, "qkv")          # (shape, head dimension and dtype are refused first: those hold on any device)
    if B < 1 or N < 1:
        raise ValueError(f"depthg_amd: qkv must hold at least one token, got {tuple(qkv.shape)}")
    if qkv.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("depthg_amd: attention_forward has no backward (the ViT is frozen); call it under torch.no_grad()")
    dev = qkv.device
    if out is None:
        out = _empty((B, N, heads * hd), torch.float32, dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (B, N, heads * hd)):
        raise ValueError(f"depthg_amd: `out` must be a contiguous float32 ({B}, {N}, {heads * hd}) tensor on {dev}")
    if (qkv.data_ptr() | out.data_ptr()) & 15:       # (a slice of a larger buffer can start anywhere; the kernels use 128-bit accesses)
        raise ValueError("depthg_amd: attention_forward needs qkv and out to start at 16-byte aligned addresses")
    lib = _lib.load()
    need = lib.dg_attention_workspace_bytes(B, heads, N)
    if need == 0:
        raise ValueError(f"depthg_amd: no attention plan for B={B}, heads={heads}, N={N} (B * heads <= 65535)")
    ws = _empty((need,), torch.uint8, dev)
    rc = lib.dg_attention_forward(_ptr(qkv.detach()), B, N, heads, hd, float(hd ** -0.5 if scale is None else scale), _ptr(out),
                                  _ptr(ws), need, _stream(dev))
    _lib.check(rc, "dg_attention_forward")
    return out


VIT_LINEAR_MAX = 3072     # K and Nout of the fused linear kernel: multiples of 64 up to this


def vit_linear_supported(K, Nout):
    """Whether dg_vit_linear_forward has a plan for an nn.Linear(K, Nout): both multiples of 64 up to 3072.  (No library call: the
    constructor of vit.VisionTransformer asks before anything is built.)"""
    return all(64 <= int(v) <= VIT_LINEAR_MAX and int(v) % 64 == 0 for v in (K, Nout))


def vit_linear_pack(weight):
    """dg_vit_linear_pack: an nn.Linear weight (Nout, K) fp32 contiguous on the GPU -> uint8 (K * Nout * 2) tensor: the weight
    rounded to bf16 in the MFMA fragment order k_lin_fwd reads.  Once per weight (the backbone is frozen)."""
    if weight.dim() != 2:
        raise ValueError(f"depthg_amd: weight must be (Nout, K), got {tuple(weight.shape)}")
    Nout, K = weight.shape
    if weight.dtype != torch.float32:
        raise ValueError(f"depthg_amd: weight must be float32, got {weight.dtype}")
    if not weight.is_contiguous():
        raise ValueError(f"depthg_amd: weight must be contiguous (strides {weight.stride()})")
    if not vit_linear_supported(K, Nout):
        raise ValueError(f"depthg_amd: vit_linear_pack is built for K and Nout that are multiples of 64 up to {VIT_LINEAR_MAX}, "
                         f"got K={K}, Nout={Nout}")
    _on_gpu(weight, "weight")
    if weight.data_ptr() & 15:
        raise ValueError("depthg_amd: vit_linear_pack needs weight to start at a 16-byte aligned address")
    lib = _lib.load()
    packed = _empty((lib.dg_vit_linear_packed_bytes(K, Nout),), torch.uint8, weight.device)
    _lib.check(lib.dg_vit_linear_pack(_ptr(weight.detach()), K, Nout, _ptr(packed), _stream(weight.device)), "dg_vit_linear_pack")
    return packed


def vit_linear_forward(x, packed, n_out, bias=None, *, ln_weight=None, ln_bias=None, eps=1e-6, gelu=False, residual=None,
                       out=None, out_bf16=False):
    """epilogue(prologue(x) W^T + bias) of one ViT linear layer as ONE launch (dg_vit_linear_forward;
    src/dino/vision_transformer.py:49-65, 68-92, 95-115).
        x          (..., K) contiguous on the GPU: float32, or bfloat16 (the fc1 -> fc2 hand-over)
        packed     vit_linear_pack(weight) of the (n_out, K) weight;  bias: (n_out) float32 or None
        ln_weight, ln_bias, eps   LayerNorm over the row first (float32 x, K <= 768)
        gelu       exact GELU on accumulator + bias
        residual   (..., n_out) float32: out = residual + (acc + bias); `out` may be `residual` itself
        out        optional result buffer; out_bf16: a bfloat16 result (no residual then)
    -> (..., n_out).  Forward only (the backbone is frozen); bf16 MFMA operands, fp32 accumulation and epilogue.  Runs on the caller's
    current stream."""
    n_out = int(n_out)
    if x.dim() < 1:
        raise ValueError(f"depthg_amd: x must be (..., K), got {tuple(x.shape)}")
    K = x.shape[-1]
    lead = tuple(x.shape[:-1])
    M = 1
    for d in lead:
        M *= d
    if not vit_linear_supported(K, n_out):
        raise ValueError(f"depthg_amd: vit_linear_forward is built for K and Nout that are multiples of 64 up to {VIT_LINEAR_MAX}, "
                         f"got K={K}, Nout={n_out}")
    ln = ln_weight is not None or ln_bias is not None
    if x.dtype not in (torch.float32, torch.bfloat16) or (ln and x.dtype != torch.float32):
        raise ValueError(f"depthg_amd: x must be float32{'' if ln else ' or bfloat16'}, got {x.dtype}")
    if not x.is_contiguous():
        raise ValueError(f"depthg_amd: x must be contiguous (strides {x.stride()})")
    if ln and (ln_weight is None or ln_bias is None):
        raise ValueError("depthg_amd: the LayerNorm prologue needs both ln_weight and ln_bias")
    if ln and K > 768:
        raise ValueError(f"depthg_amd: the LayerNorm prologue is built for K <= 768, got {K}")
    if residual is not None and out_bf16:
        raise ValueError("depthg_amd: the residual stream is float32; a bfloat16 output takes no residual")
    small = [("bias", bias, n_out), ("ln_weight", ln_weight, K), ("ln_bias", ln_bias, K)]
    for name, t, n in small:
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n,)):
            raise ValueError(f"depthg_amd: `{name}` must be a contiguous float32 ({n},) tensor")
    if residual is not None and not (residual.dtype == torch.float32 and residual.is_contiguous()
                                     and tuple(residual.shape) == lead + (n_out,)):
        raise ValueError(f"depthg_amd: `residual` must be a contiguous float32 {lead + (n_out,)} tensor")
    tensors = [x, bias, ln_weight, ln_bias, residual]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("depthg_amd: vit_linear_forward has no backward (the ViT is frozen); call it under torch.no_grad()")
    _on_gpu(x, "x")              # (shape, dtype and autograd are refused first: those hold on any device)
    if M < 1:
        raise ValueError(f"depthg_amd: x must hold at least one row, got {tuple(x.shape)}")
    dev = x.device
    odt = torch.bfloat16 if out_bf16 else torch.float32
    if out is None:
        out = _empty(lead + (n_out,), odt, dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == odt and out.is_contiguous()
              and tuple(out.shape) == lead + (n_out,)):
        raise ValueError(f"depthg_amd: `out` must be a contiguous {odt} {lead + (n_out,)} tensor on {dev}")
    lib = _lib.load()
    if not (isinstance(packed, torch.Tensor) and packed.device == dev and packed.dtype == torch.uint8 and packed.is_contiguous()
            and packed.numel() == lib.dg_vit_linear_packed_bytes(K, n_out)):
        raise ValueError(f"depthg_amd: `packed` must be vit_linear_pack(weight) of a ({n_out}, {K}) weight on {dev}")
    ptrs = 0
    for t in tensors + [packed, out]:
        if t is not None:
            if t.device != dev:
                raise RuntimeError(f"depthg_amd: every tensor must live on {dev} (got {t.device})")
            ptrs |= t.data_ptr()
    if ptrs & 15:                # (a slice of a larger buffer can start anywhere; the kernel uses 128-bit accesses)
        raise ValueError("depthg_amd: vit_linear_forward needs every tensor to start at a 16-byte aligned address")
    if out.data_ptr() == x.data_ptr():
        raise ValueError("depthg_amd: `out` may alias `residual`, not `x`")
    flags = (_lib.DG_LIN_LAYERNORM if ln else 0) | (_lib.DG_LIN_GELU if gelu else 0) \
        | (_lib.DG_LIN_IN_BF16 if x.dtype == torch.bfloat16 else 0) | (_lib.DG_LIN_OUT_BF16 if out_bf16 else 0)
    det = lambda t: _ptr(t.detach()) if t is not None else _ptr(None)
    rc = lib.dg_vit_linear_forward(det(x), det(ln_weight), det(ln_bias), float(eps), _ptr(packed), det(bias), det(residual), _ptr(out),
                                   M, K, n_out, flags, _stream(dev))
    _lib.check(rc, "dg_vit_linear_forward")
    return out


XATTN_HEAD_DIM = 48       # head dimension of the fused cross-attention (384 / 8: the depth guidance's nn.MultiheadAttention)


def _xattn_operands(who, q, k, v, heads, extra=()):
    """Shapes, dtype and contiguity first (they hold on any device), then the device, then the alignment -> (B, Nq, Nk)."""
    heads = int(heads)
    if q.dim() != 3 or k.dim() != 3 or heads < 1 or q.shape[2] != heads * XATTN_HEAD_DIM:
        raise ValueError(f"depthg_amd: {who}: q must be (B, Nq, heads * {XATTN_HEAD_DIM}) with heads={heads}, got {tuple(q.shape)}")
    if k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2] or v.shape != k.shape:
        raise ValueError(f"depthg_amd: {who}: k and v must be (B, Nk, heads * {XATTN_HEAD_DIM}) like q {tuple(q.shape)}, got {tuple(k.shape)} "
                         f"and {tuple(v.shape)}")
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    if B < 1 or Nq < 1 or Nk < 1:
        raise ValueError(f"depthg_amd: {who}: needs at least one query and one key, got q {tuple(q.shape)}, k {tuple(k.shape)}")
    named = [("q", q, q.shape), ("k", k, k.shape), ("v", v, k.shape)] + list(extra)
    for name, t, shape in named:
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"depthg_amd: {who}: `{name}` must be {tuple(shape)}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"depthg_amd: {who}: `{name}` must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"depthg_amd: {who}: `{name}` must be contiguous (strides {t.stride()})")
    for name, t, _ in named:
        _on_gpu(t, name)
        if t.device != q.device:
            raise RuntimeError(f"depthg_amd: {who}: `{name}` lives on {t.device}, q on {q.device}")
    for name, t, _ in named:
        if t.data_ptr() & (3 if name == "lse" else 15):       # (a slice of a larger buffer can start anywhere; the kernels use 128-bit accesses)
            raise ValueError(f"depthg_amd: {who}: `{name}` must start at a 16-byte aligned address")
    return B, Nq, Nk


def _xattn_p(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"depthg_amd: the attention dropout probability must be in [0, 1), got {p}")
    return p


def _xattn_workspace(lib, B, heads, Nq, Nk, backward, dev):
    need = lib.dg_xattn_workspace_bytes(B, heads, Nq, Nk, int(backward))
    if need == 0:
        raise ValueError(f"depthg_amd: no cross-attention plan for B={B}, heads={heads}, Nq={Nq}, Nk={Nk} (B * heads <= 65535, "
                         "Nq and Nk up to 2^24)")
    return _empty((need,), torch.uint8, dev), need


def xattn_forward(q, k, v, heads, p=0.0, seed=0, scale=None, want_lse=False):
    """dropout_p(softmax(q k^T * scale)) v per (batch, head) without the (B, heads, Nq, Nk) matrix (dg_xattn_forward): q (B, Nq,
    heads * 48), k and v (B, Nk, heads * 48), fp32 contiguous on the GPU -> (out (B, Nq, heads * 48), lse (B, heads, Nq) or None).
    scale: None = 48 ** -0.5.  p: dropout probability in [0, 1), the mask a Philox function of (seed, b, head, query, key) -
    xattn_keep_mask shows it.  want_lse: also write the per-row log-sum-exp, all xattn_backward needs beside `out`.  bf16 MFMA
    operands, fp32 softmax.  Runs on the caller's current stream."""
    B, Nq, Nk = _xattn_operands("xattn_forward", q, k, v, heads)
    heads, p, dev = int(heads), _xattn_p(p), q.device
    out = _empty((B, Nq, heads * XATTN_HEAD_DIM), torch.float32, dev)
    lse = _empty((B, heads, Nq), torch.float32, dev) if want_lse else None
    lib = _lib.load()
    ws, need = _xattn_workspace(lib, B, heads, Nq, Nk, False, dev)
    rc = lib.dg_xattn_forward(_ptr(q.detach()), _ptr(k.detach()), _ptr(v.detach()), B, heads, Nq, Nk, XATTN_HEAD_DIM,
                              float(XATTN_HEAD_DIM ** -0.5 if scale is None else scale), p, int(seed) & (2 ** 64 - 1), _ptr(out), _ptr(lse),
                              _ptr(ws), need, _stream(dev))
    _lib.check(rc, "dg_xattn_forward")
    return out, lse


def xattn_backward(q, k, v, out, lse, grad_out, heads, p=0.0, seed=0, scale=None, need=(True, True, True)):
    """The gradients of xattn_forward (dg_xattn_backward) from its results `out` and `lse` and the same p, seed and scale ->
    (grad_q, grad_k, grad_v); `need` says which are wanted (None for the rest: grad_q has a kernel of its own, grad_k and grad_v
    share one).  No atomics: two calls give the same bits; every element of a returned gradient is written."""
    heads = int(heads)
    B, Nq, Nk = _xattn_operands("xattn_backward", q, k, v, heads,
                                [("out", out, q.shape), ("grad_out", grad_out, q.shape), ("lse", lse, (q.shape[0], heads, q.shape[1]))])
    p, dev = _xattn_p(p), q.device
    need = tuple(bool(n) for n in need)
    if not any(need):
        return None, None, None
    gq = _empty(tuple(q.shape), torch.float32, dev) if need[0] else None
    gk = _empty(tuple(k.shape), torch.float32, dev) if need[1] or need[2] else None
    gv = _empty(tuple(k.shape), torch.float32, dev) if need[1] or need[2] else None
    lib = _lib.load()
    ws, nbytes = _xattn_workspace(lib, B, heads, Nq, Nk, True, dev)
    rc = lib.dg_xattn_backward(_ptr(q.detach()), _ptr(k.detach()), _ptr(v.detach()), _ptr(out.detach()), _ptr(lse), _ptr(grad_out.detach()),
                               B, heads, Nq, Nk, XATTN_HEAD_DIM, float(XATTN_HEAD_DIM ** -0.5 if scale is None else scale), p,
                               int(seed) & (2 ** 64 - 1), _ptr(gq), _ptr(gk), _ptr(gv), _ptr(ws), nbytes, _stream(dev))
    _lib.check(rc, "dg_xattn_backward")
    return gq, gk if need[1] else None, gv if need[2] else None


def xattn_keep_mask(seed, B, heads, Nq, Nk, p, device):
    """The keep decisions of xattn_forward / xattn_backward for (seed, p) as a uint8 (B, heads, Nq, Nk) tensor (1 = kept): element
    (b, head, i, j) depends on the seed and its four indices only (include/depthg_corr.h), so a slice does not change with the
    shape around it."""
    B, heads, Nq, Nk, p = int(B), int(heads), int(Nq), int(Nk), _xattn_p(p)
    if min(B, heads, Nq, Nk) < 1:
        raise ValueError(f"depthg_amd: xattn_keep_mask: B={B}, heads={heads}, Nq={Nq}, Nk={Nk} must be positive")
    dev = torch.device(device)
    stream = _stream(dev)
    out = _empty((B, heads, Nq, Nk), torch.uint8, dev)
    _lib.check(_lib.load().dg_xattn_keep_mask(int(seed) & (2 ** 64 - 1), B, heads, Nq, Nk, p, _ptr(out), stream), "dg_xattn_keep_mask")
    return out
