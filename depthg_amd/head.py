"""The segmentation head and the probes around the correlation loss, on the HIP library.

    ProjectionHead      DinoFeaturizer's trainable part (src/modules.py:75-88, 122-132): `cluster1` (1x1 conv C -> dim) and, for
                        projection_type "nonlinear", `cluster2` (1x1 conv C -> C, ReLU, 1x1 conv C -> dim), each fed by its own
                        Dropout2d(p=.1) draw of the backbone features, plus the third draw the features themselves get when
                        cfg.dropout.  One fused launch (dg_head_forward): the fp32 features are read once; parameters keep the
                        reference's names (`cluster1.0.weight`, `cluster2.2.bias`, ...), so its checkpoints load unchanged.
    ClusterLookup       src/modules.py:647-675 (dg_cluster_lookup_forward / _backward)
    probe_cross_entropy the linear probe's loss, src/train_segmentation.py:427-434: resize of the probe's logits to the label
                        resolution + cross entropy over the labelled pixels in one kernel (dg_probe_ce_forward / _backward)
    fused_probe_losses  both probes of the training step on the detached code as ONE operation (cfg.dg_fused_probes;
                        src/train_segmentation.py:421-444): the two losses and, already in the forward, the gradients of the
                        three probe parameters (dg_probe_step_forward / _backward).  On CPU tensors: the plain torch chain.
All arithmetic runs in the library; CPU tensors raise (there is no eager path) - fused_probe_losses apart.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .ops import DeferredDropout, _empty, _f32c, _on_gpu, _ptr, _stream


def _check_keeps(keeps, rows, C, device, what):
    """The library receives the keep flags as raw pointers and indexes keep[b * C + k] for b < rows: a mask of another shape
    (the (B, C) per-pass masks handed to the (2B, C) pair call), dtype, device or stride would be read out of bounds or as
    garbage.  Refuse it here.  Returns the 3-tuple (None entries stay None)."""
    if keeps is None:
        return (None, None, None)
    if not isinstance(keeps, (tuple, list)) or len(keeps) != 3:
        raise ValueError(f"depthg_amd: `keeps` of {what} must be a 3-tuple (cluster1's, cluster2's, the returned feats' Dropout2d "
                         f"keep flags; None where that draw does not exist), got {type(keeps).__name__}")
    for i, k in enumerate(keeps):
        if k is None:
            continue
        if not isinstance(k, torch.Tensor):
            raise ValueError(f"depthg_amd: keeps[{i}] of {what} must be a tensor or None, got {type(k).__name__}")
        if tuple(k.shape) != (rows, C):
            raise ValueError(f"depthg_amd: keeps[{i}] of {what} must have shape ({rows}, {C}) - one flag per (image, channel) - "
                             f"got {tuple(k.shape)}")
        if k.dtype != torch.float32:
            raise ValueError(f"depthg_amd: keeps[{i}] of {what} must be float32 0/1 flags, got {k.dtype}")
        if k.device != device:
            raise ValueError(f"depthg_amd: keeps[{i}] of {what} lives on {k.device}, the features on {device}")
        if not k.is_contiguous():
            raise ValueError(f"depthg_amd: keeps[{i}] of {what} must be contiguous (strides {k.stride()})")
    return tuple(keeps)


def _ptr2(ts):
    """The pointers of a per-pass tensor of the one or two passes in `ts`: the second slot of a single pass is NULL."""
    return _ptr(ts[0]), _ptr(ts[1] if len(ts) == 2 else None)


class _HeadFunction(torch.autograd.Function):
    """The head (dg_head_forward / dg_head_backward) on one featurizer pass or on both passes of a step (img, img_pos) through ONE
    set of launches (the second pass's tensors in the entries' *_pos slots, NULL on a single pass): the same numbers as two single
    calls whose weight gradients autograd adds up - without the six additions, with half the launches, and with no concatenated
    copy of the features.
    `feats`: the one or two (B,C,h,w) maps; keeps: (rows, C) each, rows = B per pass, the first pass's first.
    `input_grad`: features that require grad are accepted, and backward returns d loss / d image_feat for each pass that asks
    (dg_head_backward_input, one more launch behind the parameter gradients, on their workspace); a pass that does not ask
    gets None and is not walked.  False: such features are refused, as ever.
    `feats_grad` (with input_grad): the returned feats_out = Dropout2d(image_feat) of a pass whose features require grad stays
    differentiable, and what reaches it is added - times keep3 scale - to that pass's d image_feat in the d image_feat launch's
    epilogue (dg_head_backward_input's grad_feats_out slots).  False: feats_out is marked non-differentiable, as ever.
    -> (code per pass ..., feats_out per pass ... (None unless want_feats))."""

    @staticmethod
    def forward(ctx, keeps, scale, want_feats, input_grad, feats_grad, w1, b1, w2a, b2a, w2b, b2b, *feats):
        lib = _lib.load()
        n = len(feats)
        fs = [_f32c(t, name) for t, name in zip(feats, ("image_feat", "image_feat_pos"))]
        f = fs[0]
        if n == 2 and (f.shape != fs[1].shape or f.device != fs[1].device):
            raise ValueError(f"depthg_amd: the two passes' features must match: {tuple(f.shape)} on {f.device} and {tuple(fs[1].shape)} on {fs[1].device}")
        if any(ctx.needs_input_grad[11:]) and not input_grad:
            # (the backbone is frozen in the reference - DinoFeaturizer runs it under no_grad, src/modules.py:96 - and the
            #  d/d image_feat launch is opt-in: refuse rather than drop that gradient silently)
            raise RuntimeError("depthg_amd: ProjectionHead received features that require grad; the head has no gradient with "
                               "respect to its input (frozen backbone) - detach them, or pass input_grad=True")
        B, C, h, w = f.shape
        D, P, dev = w1.shape[0], h * w, f.device
        nonlinear = w2a is not None
        # grad mode and requires_grad of the six parameters, as autograd sees them: under torch.no_grad() / eval inference the
        # bf16 hidden tile (19 MB at the headline shape) is neither written nor kept
        need_grad = any(ctx.needs_input_grad[5:])
        codes = [_empty((B, D, h, w), torch.float32, dev) for _ in fs]
        fouts = [_empty((B, C, h, w), torch.float32, dev) if want_feats else None for _ in fs]
        hidden = _empty((n * B, C, P), torch.bfloat16, dev) if (nonlinear and need_grad) else None
        k1, k2, k3 = _check_keeps(keeps, n * B, C, dev, "ProjectionHead.forward" + ("_pair" if n == 2 else ""))
        # (weights as (out, in) matrices; None stays None, which the library takes as NULL: projection_type "linear")
        w1c, b1c, w2ac, b2ac, w2bc, b2bc = (_f32c(t, "head parameter") for t in (w1, b1, w2a, b2a, w2b, b2b))
        w1c, w2ac, w2bc = (t.reshape(t.shape[0], -1) if t is not None else None for t in (w1c, w2ac, w2bc))
        wscratch = _empty((lib.dg_head_weights_bytes(C, D),), torch.uint8, dev)     # bf16 copies of the weights (first launch)
        rc = lib.dg_head_forward(B, C, D, P, *_ptr2(fs), _ptr(w1c), _ptr(b1c), _ptr(w2ac), _ptr(b2ac), _ptr(w2bc), _ptr(b2bc),
                                 _ptr(k1), _ptr(k2), _ptr(k3), float(scale), *_ptr2(codes), *_ptr2(fouts), _ptr(hidden),
                                 _ptr(wscratch), _stream(dev))
        _lib.check(rc, "dg_head_forward")
        ctx.dims, ctx.scale, ctx.nonlinear = (B, C, D, P), float(scale), nonlinear
        ctx.shapes = tuple(t.shape if t is not None else None for t in (w1, b1, w2a, b2a, w2b, b2b))
        ctx.hw = (h, w)
        # (the fp32 weight matrices: what the d image_feat launch makes its transposed copies from)
        ctx.want_dx = bool(input_grad) and any(ctx.needs_input_grad[11:])
        # the passes whose feats_out carries a gradient back: the third mask is then needed in backward
        ctx.feats_diff = tuple(bool(want_feats and input_grad and feats_grad and need) for need in ctx.needs_input_grad[11:])
        ctx.save_for_backward(k1, k2, hidden, wscratch, w1c if ctx.want_dx else None, w2ac if ctx.want_dx else None,
                              k3 if any(ctx.feats_diff) else None, *fs)
        ctx.set_materialize_grads(False)
        if want_feats:
            frozen = [fo for fo, diff in zip(fouts, ctx.feats_diff) if not diff]
            if frozen:
                ctx.mark_non_differentiable(*frozen)
        return (*codes, *fouts)

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib.load()
        k1, k2, hidden, wscratch, w1c, w2ac, k3, *fs = ctx.saved_tensors
        B, C, D, P = ctx.dims
        n, dev = len(fs), fs[0].device
        if ctx.nonlinear and hidden is None:
            raise RuntimeError("depthg_amd: head backward without the saved hidden activations")
        # (a pass whose code took no part in the loss contributes nothing: a zero upstream)
        gs = [_f32c(g, name) if g is not None else torch.zeros((B, D, P), dtype=torch.float32, device=dev)
              for g, name in zip(grads[:n], ("grad_code", "grad_code_pos"))]
        nb = lib.dg_head_workspace_bytes(n * B, C, D, P)
        ws = _empty(nb, torch.uint8, dev)
        gw1, gb1 = _empty((D, C), torch.float32, dev), _empty((D,), torch.float32, dev)
        gw2a = gb2a = gw2b = gb2b = None
        if ctx.nonlinear:
            gw2a, gb2a = _empty((C, C), torch.float32, dev), _empty((C,), torch.float32, dev)
            gw2b, gb2b = _empty((D, C), torch.float32, dev), _empty((D,), torch.float32, dev)
        rc = lib.dg_head_backward(B, C, D, P, *_ptr2(fs), _ptr(k1), _ptr(k2), ctx.scale, _ptr(hidden), _ptr(wscratch),
                                  *_ptr2(gs), _ptr(gw1), _ptr(gb1), _ptr(gw2a), _ptr(gb2a), _ptr(gw2b), _ptr(gb2b), _ptr(ws), nb,
                                  _stream(dev))
        _lib.check(rc, "dg_head_backward")
        gparams = (gw1, gb1, gw2a, gb2a, gw2b, gb2b)
        gfs = [None] * n
        if ctx.want_dx:
            # d image_feat of the passes that ask: one launch behind the parameter gradients, d hidden read from their workspace
            gfs = [_empty((B, C) + ctx.hw, torch.float32, dev) if need else None for need in ctx.needs_input_grad[11:]]
            nbi = lib.dg_head_input_workspace_bytes(C, D)
            iws = _empty(nbi, torch.uint8, dev)
            # what reached each pass's feats_out (None: nothing, or that output was not differentiable)
            gfo = [_f32c(g, "grad_feats") if (g is not None and diff) else None for g, diff in zip(grads[n:2 * n], ctx.feats_diff)]
            rc = lib.dg_head_backward_input(B, C, D, P, _ptr(w1c), _ptr(w2ac), _ptr(k1), _ptr(k2), _ptr(k3), ctx.scale, _ptr(hidden),
                                            *_ptr2(gs), *_ptr2(gfo), _ptr(ws), nb, *_ptr2(gfs), _ptr(iws), nbi, _stream(dev))
            _lib.check(rc, "dg_head_backward_input")
        return (None, None, None, None, None) + tuple(g.reshape(sh) if g is not None else None for g, sh in zip(gparams, ctx.shapes)) + tuple(gfs)


def draw_keep_masks_pair(B, C, device, p=0.1, use=(True, True, True)):
    """The six Dropout2d draws of a step's two featurizer passes in the reference's order - those of pass 1 (cluster1's input,
    cluster2's input, the returned feats), then those of pass 2 - as THREE (2B, C) tensors whose halves are drawn in place: the
    torch generator advances exactly as it does for two draw_keep_masks calls, and nothing is concatenated."""
    ks = [torch.empty(2 * B, C, device=device, dtype=torch.float32) if u else None for u in use]
    for half in (slice(0, B), slice(B, 2 * B)):
        for k in ks:
            if k is not None:
                k[half].bernoulli_(1.0 - p)
    return tuple(ks)


def draw_keep_masks(B, C, device, p=0.1, use=(True, True, True)):
    """The Dropout2d draws of one featurizer pass, in the reference's order (cluster1's input, cluster2's input, the returned
    feats; src/modules.py:122-132): (B, C) keep flags, one bernoulli_(1 - p) each, as F.dropout2d draws its (B, C, 1, 1) noise.
    Only the uses that exist draw (`use`: cluster1, cluster2 = projection_type "nonlinear", feats = cfg.dropout) - the reference
    calls Dropout2d exactly there, so the torch generator advances as it does there; the others are None."""
    return tuple(torch.empty(B, C, device=device, dtype=torch.float32).bernoulli_(1.0 - p) if u else None for u in use)


def _run_head(cluster1, cluster2, feats, training, feats_dropout, p, keeps, draw, defer=False, input_grad=False, feats_grad=False):
    """What run_head and run_head_pair share: the keep masks that exist (given, or drawn with `draw`), the head's parameters, one
    _HeadFunction call on the one or two maps of `feats`, and ((code, feats), ...) per pass."""
    if feats_grad and not input_grad:
        raise ValueError("depthg_amd: feats_grad=True carries the returned feats' gradient into the head's input: it needs input_grad=True")
    B, C = feats[0].shape[:2]
    nl = cluster2 is not None
    scale = 1.0 / (1.0 - p)
    if training:
        if keeps is None:
            keeps = draw(B, C, feats[0].device, p, use=(True, nl, bool(feats_dropout)))
        k1, k2, k3 = keeps
        keeps = (k1, k2 if nl else None, k3 if feats_dropout else None)
    else:
        keeps = None                                                                                  # eval: Dropout2d is the identity
    want_feats = bool(training and feats_dropout)
    deferred = None
    if want_feats and defer:
        deferred, want_feats = keeps[2], False
        keeps = (keeps[0], keeps[1], None)
    convs = (cluster1[0], cluster2[0], cluster2[2]) if nl else (cluster1[0],)
    params = [t for conv in convs for t in (conv.weight, conv.bias)] + [None] * (6 - 2 * len(convs))
    out = _HeadFunction.apply(keeps, scale, want_feats, bool(input_grad), bool(feats_grad), *params, *feats)
    codes, fouts = out[:len(feats)], out[len(feats):]
    if deferred is not None:
        return tuple((c, DeferredDropout(f, deferred[i * B:(i + 1) * B], scale)) for i, (c, f) in enumerate(zip(codes, feats)))
    return tuple((c, fo if want_feats else f) for c, f, fo in zip(codes, feats, fouts))


def run_head(cluster1, cluster2, image_feat, training, feats_dropout, p=0.1, keeps=None, input_grad=False, feats_grad=False):
    """(code, feats) of one featurizer pass (src/modules.py:122-137) from the reference's modules: `cluster1` = Sequential(Conv2d),
    `cluster2` = Sequential(Conv2d, ReLU, Conv2d) or None (projection_type "linear").  Training: three Dropout2d draws (`keeps`
    or drawn here), feats = Dropout2d(image_feat) when `feats_dropout` (cfg.dropout); eval: no dropout, feats = image_feat.
    `input_grad`: an image_feat that requires grad is accepted and receives its gradient through `code` (the returned feats stay
    non-differentiable: the loss reads them under no_grad, src/modules.py:1232-1234); False refuses such features.
    `feats_grad` (only with input_grad): the returned feats stay attached - the reconstruction term reads them with a graph,
    src/train_segmentation.py:391-398 - and their gradient, times the third mask, joins image_feat's inside the d image_feat launch.
    (Without feats_dropout, or in eval mode, feats is image_feat itself and autograd needs no help.)"""
    return _run_head(cluster1, cluster2, (image_feat,), training, feats_dropout, p, keeps, draw_keep_masks, False, input_grad, feats_grad)[0]


def run_head_pair(cluster1, cluster2, image_feat, image_feat_pos, training, feats_dropout, p=0.1, keeps=None, defer_feats_dropout=False,
                  input_grad=False, feats_grad=False):
    """run_head for the two passes of a training step at once: ((code, feats), (code_pos, feats_pos)).  `keeps`: three (2B, C)
    tensors (draw_keep_masks_pair) or None (drawn here, in the order two run_head calls would draw).  `defer_feats_dropout`: the
    Dropout2d of the returned feats is drawn as always but NOT applied - `feats` / `feats_pos` come back as ops.DeferredDropout
    (the input maps + their keep flags), which ContrastiveCorrelationLoss applies inside its operand preparation: the dropped
    tensors (38.5 MB each at the headline shape) are neither written here nor read there.  `input_grad`: as run_head, per pass - a
    pass whose features do not require grad gets no gradient and is not walked by the launch.  `feats_grad`: as run_head, per pass
    (deferred feats are the input maps themselves: whoever applies the mask hands them their gradient)."""
    return _run_head(cluster1, cluster2, (image_feat, image_feat_pos), training, feats_dropout, p, keeps, draw_keep_masks_pair,
                     defer_feats_dropout, input_grad, feats_grad)


class ProjectionHead(nn.Module):
    """cluster1 / cluster2 of DinoFeaturizer with the reference's module and parameter names; forward(image_feat, feats_dropout,
    keeps) -> (code, feats): feats = Dropout2d(image_feat) when `feats_dropout` (cfg.dropout) and the module trains, else
    image_feat itself."""

    def __init__(self, n_feats: int, dim: int, projection_type="nonlinear", p: float = 0.1):
        super().__init__()
        self.n_feats, self.dim, self.proj_type, self.p = n_feats, dim, projection_type, p
        self.cluster1 = nn.Sequential(nn.Conv2d(n_feats, dim, (1, 1)))                                   # make_clusterer, :75-77
        if projection_type == "nonlinear":                                                                # make_nonlinear_clusterer, :79-83
            self.cluster2 = nn.Sequential(nn.Conv2d(n_feats, n_feats, (1, 1)), nn.ReLU(), nn.Conv2d(n_feats, dim, (1, 1)))

    def forward(self, image_feat, feats_dropout=True, keeps=None, input_grad=False, feats_grad=False):
        if self.proj_type is None:                                                                        # :125-126: code = image_feat
            feats = image_feat
            if self.training and feats_dropout:                                                           # :127-129: feats = Dropout2d(image_feat)
                if keeps is not None:
                    _check_keeps(keeps, image_feat.shape[0], image_feat.shape[1], image_feat.device, "ProjectionHead.forward")
                k3 = keeps[2] if keeps is not None and keeps[2] is not None else draw_keep_masks(image_feat.shape[0], image_feat.shape[1], image_feat.device,
                                                                         self.p, use=(False, False, True))[2]
                feats = image_feat * (k3 * (1.0 / (1.0 - self.p)))[:, :, None, None]
            return image_feat, feats
        return run_head(self.cluster1, getattr(self, "cluster2", None) if self.proj_type == "nonlinear" else None, image_feat,
                        self.training, feats_dropout, self.p, keeps, input_grad, feats_grad)

    def forward_pair(self, image_feat, image_feat_pos, feats_dropout=True, keeps=None, defer_feats_dropout=False, input_grad=False,
                     feats_grad=False):
        """forward(image_feat) and forward(image_feat_pos) of one training step (src/train_segmentation.py:303-306) as one set of
        launches: ((code, feats), (code_pos, feats_pos)), the same values and - after backward - the same parameter gradients.
        `defer_feats_dropout`: see run_head_pair (feats / feats_pos as ops.DeferredDropout for the loss to apply); `input_grad`:
        features that require grad receive their gradient (see run_head)."""
        if self.proj_type is None:
            ka = kb = None
            if keeps is not None:
                B = image_feat.shape[0]
                _check_keeps(keeps, 2 * B, image_feat.shape[1], image_feat.device, "ProjectionHead.forward_pair")
                if keeps[2] is not None:
                    ka, kb = (None, None, keeps[2][:B]), (None, None, keeps[2][B:])
            return self.forward(image_feat, feats_dropout, ka), self.forward(image_feat_pos, feats_dropout, kb)
        return run_head_pair(self.cluster1, getattr(self, "cluster2", None) if self.proj_type == "nonlinear" else None, image_feat,
                             image_feat_pos, self.training, feats_dropout, self.p, keeps, defer_feats_dropout, input_grad, feats_grad)


class _ClusterFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, clusters, alpha, want_logp):
        lib = _lib.load()
        xx, cc = _f32c(x, "x"), _f32c(clusters, "clusters")
        B, D, h, w = xx.shape
        n, P, dev = cc.shape[0], h * w, xx.device
        inner = _empty((B, n, h, w), torch.float32, dev)
        probs = _empty((B, n, h, w), torch.float32, dev)
        logp = _empty((B, n, h, w), torch.float32, dev) if want_logp else None
        loss = _empty((1,), torch.float32, dev)
        scratch = _empty((B * ((P + 255) // 256),), torch.float32, dev)
        a = float("nan") if alpha is None else float(alpha)
        rc = lib.dg_cluster_lookup_forward(_ptr(xx), _ptr(cc), a, B, D, n, P, _ptr(inner), _ptr(probs), _ptr(logp), _ptr(loss),
                                           _ptr(scratch), _stream(dev))
        _lib.check(rc, "dg_cluster_lookup_forward")
        ctx.alpha, ctx.dims, ctx.x_grad = a, (B, D, n, P), x.requires_grad
        ctx.save_for_backward(xx, cc, inner)
        ctx.mark_non_differentiable(probs)
        if logp is not None:
            return loss[0], probs, logp
        return loss[0], probs, None

    @staticmethod
    def backward(ctx, gloss, _gprobs, glogp):
        if glogp is not None:
            raise RuntimeError("depthg_amd: ClusterLookup(log_probs=True) is an evaluation output and carries no gradient")
        lib = _lib.load()
        xx, cc, inner = ctx.saved_tensors
        B, D, n, P = ctx.dims
        dev = xx.device
        g = _f32c(gloss, "grad_loss").reshape(1)
        gc = _empty((n, D), torch.float32, dev)
        gx = _empty(tuple(xx.shape), torch.float32, dev) if ctx.x_grad else None
        scratch = _empty((B * n * P + B * ((P + 63) // 64) * n * D,), torch.float32, dev)
        rc = lib.dg_cluster_lookup_backward(_ptr(xx), _ptr(cc), _ptr(inner), ctx.alpha, _ptr(g), B, D, n, P, _ptr(gc), _ptr(gx),
                                            _ptr(scratch), _stream(dev))
        _lib.check(rc, "dg_cluster_lookup_backward")
        return gx, gc, None, None


class ClusterLookup(nn.Module):
    """Cosine cluster probe (src/modules.py:647-675): `clusters` (n_classes, dim) centres; forward(x, alpha, log_probs=False)
    returns (cluster_loss, cluster_probs) - hard one-hot assignment when alpha is None, softmax(alpha * similarity) otherwise -
    or the log-probabilities alone."""

    def __init__(self, dim: int, n_classes: int):
        super().__init__()
        self.n_classes, self.dim = n_classes, dim
        self.clusters = nn.Parameter(torch.randn(n_classes, dim))

    def reset_parameters(self):
        with torch.no_grad():
            self.clusters.copy_(torch.randn(self.n_classes, self.dim))

    def forward(self, x, alpha, log_probs=False):
        if log_probs:
            if alpha is None:
                raise TypeError("log_probs=True needs alpha (the reference multiplies by it)")
            return _ClusterFunction.apply(x, self.clusters, alpha, True)[2]
        loss, probs, _ = _ClusterFunction.apply(x, self.clusters, alpha, False)
        return loss, probs


class _ProbeCeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label):
        lib = _lib.load()
        lg = _f32c(logits, "linear_logits")
        lab = _on_gpu(label, "label").detach().to(torch.int64).contiguous()
        B, n, h, w = lg.shape
        H, W = lab.shape[-2:]
        lab = lab.reshape(B, H, W)
        dev = lg.device
        out3 = _empty((3,), torch.float32, dev)
        scratch = _empty((2 * B * H,), torch.float32, dev)
        rc = lib.dg_probe_ce_forward(_ptr(lg), _ptr(lab), B, n, h, w, H, W, _ptr(out3), _ptr(scratch), _stream(dev))
        _lib.check(rc, "dg_probe_ce_forward")
        ctx.dims = (B, n, h, w, H, W)
        ctx.save_for_backward(lg, lab, out3)
        return out3[2]

    @staticmethod
    def backward(ctx, gloss):
        lib = _lib.load()
        lg, lab, out3 = ctx.saved_tensors
        B, n, h, w, H, W = ctx.dims
        g = _f32c(gloss, "grad_loss").reshape(1)
        gl = _empty((B, n, h, w), torch.float32, lg.device)
        rc = lib.dg_probe_ce_backward(_ptr(lg), _ptr(lab), _ptr(out3), _ptr(g), B, n, h, w, H, W, _ptr(gl), _stream(lg.device))
        _lib.check(rc, "dg_probe_ce_backward")
        return gl, None


def probe_cross_entropy(linear_logits, label):
    """`CrossEntropyLoss()(interpolate(linear_logits, label.shape[-2:], 'bilinear', align_corners=False)[mask], label[mask])`
    with mask = (label >= 0) & (label < n_classes)  (src/train_segmentation.py:421-434), without the label-resolution logits."""
    return _ProbeCeFunction.apply(linear_logits, label)


PROBE_STEP_MAX_D, PROBE_STEP_MAX_N = 128, 64          # dg_probe_step_forward's limits (include/depthg_corr.h)


def _probe_step_args(code, label, weight, bias, clusters):
    """The arguments of fused_probe_losses, checked -> (label as (B,H,W), (B, D, n_lin, n_clu, h, w, H, W): the C entries' order)."""
    if code.requires_grad:
        raise RuntimeError("depthg_amd: fused_probe_losses received a code that requires grad: the fused probe step has no gradient "
                           "with respect to the code (the probes train on code.detach(), src/train_segmentation.py:421) - detach it, "
                           "or take the unfused route: probe_cross_entropy(linear_probe(code), label) and ClusterLookup(code, None)")
    if code.dim() != 4:
        raise ValueError(f"depthg_amd: fused_probe_losses: code must be (B, D, h, w), got {tuple(code.shape)}")
    B, D, h, w = code.shape
    if weight.dim() not in (2, 4) or weight.shape[1] != D or weight.numel() != weight.shape[0] * D:
        raise ValueError(f"depthg_amd: fused_probe_losses: weight must be (n_lin, {D}) or (n_lin, {D}, 1, 1), got {tuple(weight.shape)}")
    n = weight.shape[0]
    if bias is None or tuple(bias.shape) != (n,):
        raise ValueError(f"depthg_amd: fused_probe_losses: bias must be ({n},), got {None if bias is None else tuple(bias.shape)}")
    if clusters.dim() != 2 or clusters.shape[1] != D:
        raise ValueError(f"depthg_amd: fused_probe_losses: clusters must be (n_clu, {D}), got {tuple(clusters.shape)}")
    m = clusters.shape[0]
    if label.dim() == 4 and label.shape[1] == 1:
        label = label[:, 0]
    if label.dim() != 3:
        raise ValueError(f"depthg_amd: fused_probe_losses: label must be (B, H, W) or (B, 1, H, W), got {tuple(label.shape)}")
    if label.shape[0] != B:
        raise ValueError(f"depthg_amd: fused_probe_losses: label holds {label.shape[0]} images, code {B}")
    if D > PROBE_STEP_MAX_D:
        raise RuntimeError(f"depthg_amd: fused_probe_losses serves D <= {PROBE_STEP_MAX_D} (got {D}); take the unfused route")
    if n > PROBE_STEP_MAX_N or m > PROBE_STEP_MAX_N:
        raise RuntimeError(f"depthg_amd: fused_probe_losses serves n_lin <= {PROBE_STEP_MAX_N} and n_clu <= {PROBE_STEP_MAX_N} "
                           f"(got {n} and {m}); take the unfused route")
    H, W = label.shape[-2:]
    return label, (B, D, n, m, h, w, H, W)


def _probe_losses_torch(code, label, weight, bias, clusters):
    """The reference's chain (src/train_segmentation.py:421-444, src/modules.py:664-675 with alpha None) in plain torch."""
    n, D = weight.shape[0], code.shape[1]
    logits = F.interpolate(F.conv2d(code, weight.reshape(n, D, 1, 1), bias), label.shape[-2:], mode="bilinear", align_corners=False)
    flat, lab = logits.permute(0, 2, 3, 1).reshape(-1, n), label.reshape(-1)
    mask = (lab >= 0) & (lab < n)
    linear_loss = F.cross_entropy(flat[mask], lab[mask])
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(code, dim=1), F.normalize(clusters, dim=1))
    probs = F.one_hot(torch.argmax(inner, dim=1), clusters.shape[0]).permute(0, 3, 1, 2).to(torch.float32)
    return linear_loss, -(probs * inner).sum(1).mean()


class _ProbeStepFunction(torch.autograd.Function):
    """dg_probe_step_forward / _backward: the code is detached, so the forward leaves the three parameter gradients - for upstream
    gradients of 1 - in its workspace and the backward is one launch that scales them by the two scalars autograd hands it."""

    @staticmethod
    def forward(ctx, code, label, weight, bias, clusters):
        lib = _lib.load()
        label, dims = _probe_step_args(code, label, weight, bias, clusters)
        B, D, n, m, h, w, H, W = dims
        cc, ww, bb, cl = (_f32c(t, name) for t, name in ((code, "code"), (weight, "weight"), (bias, "bias"), (clusters, "clusters")))
        lab = _on_gpu(label, "label").detach().to(torch.int64).contiguous()
        dev = cc.device
        nb = lib.dg_probe_step_workspace_bytes(*dims)
        if nb == 0:
            _lib.check(-2, "dg_probe_step_workspace_bytes")
        ws = _empty(nb, torch.uint8, dev)
        out3 = _empty((3,), torch.float32, dev)
        rc = lib.dg_probe_step_forward(_ptr(cc), _ptr(lab), _ptr(ww), _ptr(bb), _ptr(cl), *dims, _ptr(out3), _ptr(ws), nb, _stream(dev))
        _lib.check(rc, "dg_probe_step_forward")
        ctx.dims, ctx.shapes = dims, (weight.shape, bias.shape, clusters.shape)
        ctx.save_for_backward(ws)
        return out3[0], out3[1]

    @staticmethod
    def backward(ctx, g_lin, g_clu):
        lib = _lib.load()
        ws, = ctx.saved_tensors
        B, D, n, m, h, w, H, W = ctx.dims
        dev = ws.device
        gl, gc = _f32c(g_lin, "grad_linear_loss").reshape(1), _f32c(g_clu, "grad_cluster_loss").reshape(1)
        gw, gb, gk = _empty((n, D), torch.float32, dev), _empty((n,), torch.float32, dev), _empty((m, D), torch.float32, dev)
        rc = lib.dg_probe_step_backward(_ptr(ws), ws.numel(), _ptr(gl), _ptr(gc), *ctx.dims, _ptr(gw), _ptr(gb), _ptr(gk), _stream(dev))
        _lib.check(rc, "dg_probe_step_backward")
        return None, None, gw.reshape(ctx.shapes[0]), gb, gk


def fused_probe_losses(code, label, weight, bias, clusters):
    """(linear_loss, cluster_loss) of the two probes the training step trains on the detached code (src/train_segmentation.py:421-444):
    `CrossEntropyLoss()(interpolate(conv2d(code, weight, bias), label.shape[-2:], 'bilinear', align_corners=False)[mask], label[mask])`
    with mask = (label >= 0) & (label < n_lin), and ClusterLookup(code, None)'s loss for the centres `clusters` (n_clu, D) - one
    operation whose backward hands `weight`, `bias` and `clusters` their gradients and the code none.  A code that requires grad is
    refused.  GPU tensors: dg_probe_step_forward / _backward (D <= 128, n_lin and n_clu <= 64); CPU tensors: the torch chain."""
    if not code.is_cuda:
        label, _ = _probe_step_args(code, label, weight, bias, clusters)
        return _probe_losses_torch(code.to(torch.float32), label.to(torch.int64), weight, bias, clusters)
    return _ProbeStepFunction.apply(code, label, weight, bias, clusters)
