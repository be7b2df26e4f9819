"""Float64 restatement of the reference's DepthContrastiveCorrelationLoss.forward (src/modules.py:1370-1463) behind its random
draws: the coordinates and the negatives' batch maps are arguments.  Not imported by the product; the tests hold it to the
recorded outputs of the reference class (tests/golden/depth_intra.npz) and, with depth_aug_feats = orig_feats, to
oracle/depthg_oracle.py's plain loss.

What the class does that ContrastiveCorrelationLoss does not (:1433-1438): depth_aug_feats is sampled at coords1 and the
self-correlation (intra) helper call takes it as both feature arguments; depth_aug_feats_pos is sampled at coords2 and the result is
never read (it is not an argument here).  The inter pair-set and the negatives use orig_feats / orig_feats_pos.
"""
import torch
import torch.nn.functional as F


def _norm(t):                                   # :789-790
    return F.normalize(t, dim=1, eps=1e-10)


def _corr(a, b):                                # :797-809
    return torch.einsum("nchw,ncij->nhwij", a, b)


def _sample(t, coords):                         # :822-825
    return F.grid_sample(t, coords.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)


def _helper(cfg, f1, f2, c1, c2, shift):        # :1380-1403
    with torch.no_grad():
        fd = _corr(_norm(f1), _norm(f2))
        if cfg.pointwise:
            old_mean = fd.mean()
            fd = fd - fd.mean([3, 4], keepdim=True)
            fd = fd - fd.mean() + old_mean
    cd = _corr(_norm(c1), _norm(c2))
    lo = 0.0 if cfg.zero_clamp else -9999.0
    clamped = cd.clamp(lo, .8) if cfg.stabalize else cd.clamp(lo)
    return -clamped * (fd - shift), cd


def forward(cfg, orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth_aug_feats, coords1, coords2, perms):
    """The 6-tuple of :1458-1463.  Tensors of any float dtype are computed in float64; orig_code / orig_code_pos may require grad
    (pass them as float64 leaves to read .grad).  perms: sequence of n_neg int64 (B,) batch maps."""
    d = lambda t: t if t.dtype == torch.float64 else t.double()
    c1, c2 = d(coords1), d(coords2)
    feats, code = _sample(d(orig_feats), c1), _sample(d(orig_code), c1)                   # :1427-1428
    feats_pos, code_pos = _sample(d(orig_feats_pos), c2), _sample(d(orig_code_pos), c2)   # :1430-1431
    aug = _sample(d(depth_aug_feats), c1)                                                 # :1433
    intra_loss, intra_cd = _helper(cfg, aug, aug, code, code, cfg.pos_intra_shift)        # :1437-1438
    inter_loss, inter_cd = _helper(cfg, feats, feats_pos, code, code_pos, cfg.pos_inter_shift)
    neg_losses, neg_cds = [], []
    for k in range(int(cfg.neg_samples)):                                                 # :1447-1454
        perm = torch.as_tensor(perms[k], dtype=torch.long)
        l, c = _helper(cfg, feats, _sample(d(orig_feats)[perm], c2), code, _sample(d(orig_code)[perm], c2), cfg.neg_inter_shift)
        neg_losses.append(l)
        neg_cds.append(c)
    return (intra_loss.mean(), intra_cd, inter_loss.mean(), inter_cd, torch.cat(neg_losses, 0), torch.cat(neg_cds, 0))


def total(cfg, out):
    """The six-tuple branch of the caller (src/train_segmentation.py:347-350)."""
    return (cfg.pos_inter_weight * out[2].mean() + cfg.pos_intra_weight * out[0].mean() +
            cfg.neg_inter_weight * out[4].mean()) * cfg.correspondence_weight


def forward_backward_f64(cfg, f, fp, c, cp, aug, c1, c2, perms):
    """-> (tuple, total, d total / d code, d total / d code_pos), float64, detached."""
    cr, cpr = c.double().clone().requires_grad_(True), cp.double().clone().requires_grad_(True)
    out = forward(cfg, f, fp, cr, cpr, aug, c1, c2, perms)
    t = total(cfg, out)
    t.backward()
    return tuple(o.detach() for o in out), t.detach(), cr.grad, cpr.grad
