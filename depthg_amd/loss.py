"""Host-side mirror of the reference's operator surface for the correlation loss.

`ContrastiveCorrelationLoss(cfg)` is a drop-in for the reference class of the same name
(src/modules.py:1221-1367): same constructor, a mutable `.cfg` that is re-read on every call
(the caller rewrites `cfg.depth_sampling`, `cfg.feature_samples`, `cfg.depth_feat_shift` between
steps, src/train_segmentation.py:356-375), no parameters, same positional/keyword call signature
and the same 6- / 8-tuple.  All arithmetic runs in the HIP library behind include/depthg_corr.h;
there is no eager/CPU fallback (a missing library or a CPU tensor raises).

Extra, build-side cfg keys (all optional, read with getattr):
    dg_outputs      "full" (default): tuple elements 1,3,4,5,7 are the reference's un-reduced
                    (.., S,S,S,S) tensors, written by dg_corr_materialize;
                    "reduced": they are 1-element tensors holding the mean (so the caller's
                    `.mean()` / logging keeps working) and nothing of size (B,P,P) ever reaches HBM.
    dg_dense_grid   True: with feature_samples == h == w use the identity grid for coords1 and
                    coords2 (SURVEY.md section 8(d) dense runs) instead of torch.rand.
After a call, `.scalars` is the fused fp32 output vector (DG_OUT_* order: the four loss means, the four cd means, the
weighted total) with its grad_fn and `.total` its last element = the term `training_step` adds to its loss
(src/train_segmentation.py:330-349, weights read from cfg), so `loss_fn.total.backward()` needs no further torch ops.
`.cd_histograms()` gives the histograms of the three un-reduced cd tensors of that call (what the reference logs every cfg.hist_freq
steps) in either dg_outputs mode, from the operands the forward left in its workspace.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops


SMALL_GRID_POSITIONS = 160      # sample grids up to here run the fused small-grid kernel (dg_small.hip), identity coordinates included


def super_perm(size: int, device) -> torch.Tensor:
    """randperm with fixed points bumped by one, modulo size (src/modules.py:1184-1188; quirk Q6)."""
    perm = torch.randperm(size, device=device, dtype=torch.long)
    perm = torch.where(perm == torch.arange(size, device=device), perm + 1, perm)
    return perm % size


def super_perms(count: int, size: int, device) -> torch.Tensor:
    """`count` independent super_perm draws as one (count, size) tensor with ONE sort launch: argsort of iid uniforms
    is a uniform random permutation, like randperm; then the same fixed-point bump (src/modules.py:1186-1188)."""
    if count == 0:
        return torch.zeros(0, size, dtype=torch.long, device=device)
    perm = torch.argsort(torch.rand(count, size, device=device), dim=1)
    ar = torch.arange(size, device=device).unsqueeze(0)
    return torch.where(perm == ar, perm + 1, perm) % size


def identity_coords(b: int, s: int, device) -> torch.Tensor:
    """coords such that sample() reads every pixel of an s x s map exactly once (transposed, quirk Q3)."""
    lin = torch.linspace(-1.0, 1.0, s, device=device)
    c = torch.empty(b, s, s, 2, device=device)
    c[..., 0] = lin.view(1, 1, s)
    c[..., 1] = lin.view(1, s, 1)
    return c


class _Launched:
    """What a forward hands back beside its autograd outputs: the batch maps it ran on (its own draw included) and its workspace."""
    __slots__ = ("perms", "workspace")


class _CorrLossFunction(torch.autograd.Function):
    """out[DG_OUT_COUNT] = fused loss scalars (+ weighted total); backward = dg_corr_backward with the upstream of that vector."""

    @staticmethod
    def forward(ctx, orig_code, orig_code_pos, orig_feats, orig_feats_pos, depth, coords1, coords2, perms, desc, draw_state, keep,
                feat_inv, intra_feats, launched):
        # perms None: the forward draws the negatives itself (draw_state: device generator or None); keep: Dropout2d of the feature maps
        # applied inside the operand preparation (identity grid); feat_inv: one channel chunk of wider maps on sampled coordinates
        # (forward_with: `wide`); intra_feats: the intra pair-set correlates a second feature map (DepthContrastiveCorrelationLoss)
        out, perms, ws = ops.corr_forward(desc, orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms,
                                          draw_state=draw_state, keep=keep, feat_inv=feat_inv, intra_feats=intra_feats)
        launched.perms, launched.workspace = perms, ws
        ctx.desc, ctx.ws, ctx.shape = desc, ws, tuple(orig_code.shape)
        ctx.save_for_backward(coords1, coords2, perms)
        # second output: the weighted total as its own autograd output (a view of element DG_OUT_TOTAL), so that
        # `total.backward()` reaches backward() with a scalar instead of going through a select-backward (zeros + copy)
        ctx.set_materialize_grads(False)
        return out, out[ops._lib.DG_OUT_TOTAL]

    @staticmethod
    def backward(ctx, gout, gtotal):
        nothing = (None,) * 14
        if gout is None and gtotal is None:
            return nothing
        coords1, coords2, perms = ctx.saved_tensors
        if not (ctx.desc.flags & ops._lib.DG_NEED_GRAD):
            raise RuntimeError("depthg_amd: backward called on a forward that ran without gradient pieces")
        if gout is None:
            gt = gtotal.to(torch.float32).contiguous()
            g_code, g_code_pos = ops.corr_backward_total(ctx.desc, gt, coords1, coords2, perms, ctx.ws, ctx.shape)
        else:
            gs = gout.to(torch.float32).contiguous()      # [DG_OUT_COUNT]: entries 0..3 and DG_OUT_TOTAL are used
            if gtotal is not None:
                gs = gs.clone()
                gs[ops._lib.DG_OUT_TOTAL] += gtotal.to(torch.float32)
            g_code, g_code_pos = ops.corr_backward(ctx.desc, gs, coords1, coords2, perms, ctx.ws, ctx.shape)
        return (g_code, g_code_pos) + nothing[2:]


def _rand_coords(shape, device):
    """`torch.rand(shape) * 2 - 1` of the reference (src/modules.py:1310-1321) as ONE launch: `uniform_(-1, 1)` consumes the same
    Philox draws and forms u * 2 + (-1) - bit-identical on the GPU (scripts/rand_eq.py), two 5-us elementwise launches less per
    coordinate set."""
    return torch.empty(shape, device=device).uniform_(-1, 1)


class ContrastiveCorrelationLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self._ident_cache = (None, None)
        self._perm_state = None            # device generator state of the negatives' permutations (cfg.dg_graph_safe)

    def _total_weights(self, depth_term):
        """Weights of (intra, inter, neg, depth) loss means in the caller's total, src/train_segmentation.py:325-349."""
        cfg = self.cfg
        g = lambda k: float(getattr(cfg, k, 0.0))
        balance = g("lhp_weight") if (depth_term and getattr(cfg, "lhp", False) and getattr(cfg, "lhp_weight_balance", False)) else 0.0
        scale = g("correspondence_weight") - balance
        return (g("pos_intra_weight") * scale, g("pos_inter_weight") * scale, g("neg_inter_weight") * scale,
                g("depth_feat_weight") * scale if depth_term else 0.0)

    def takes_deferred_dropout(self, feat_hw, code_hw=None) -> bool:
        """True when a call with feature maps of size `feat_hw` runs the identity grid (_draw_coords), i.e. when the Dropout2d of the
        feature maps can be applied inside the operand preparation (ops.DeferredDropout) instead of by the featurizer."""
        cfg = self.cfg
        if getattr(cfg, "use_salience", False) or cfg.depth_sampling in ("simple", "fps", "fps_depth_feat"):
            return False
        S = int(cfg.feature_samples)
        return bool(getattr(cfg, "dg_dense_grid", False)) and (code_hw is None or tuple(code_hw) == tuple(feat_hw)) and \
            S == feat_hw[0] == feat_hw[1]

    # -- coordinate selection, src/modules.py:1287-1321 -------------------------------------------
    def _draw_coords(self, orig_feats, orig_feats_pos, orig_salience, orig_salience_pos, depth, depth_pos, same_maps=True):
        cfg = self.cfg
        B, S = orig_feats.shape[0], int(cfg.feature_samples)
        dev = orig_feats.device
        coord_shape = [B, S, S, 2]
        if getattr(cfg, "use_salience", False):          # src/modules.py:1290-1297
            c1_nonzero = ops.salience_coords(orig_salience, S)
            c2_nonzero = ops.salience_coords(orig_salience_pos, S)
            c1_reg = _rand_coords(coord_shape, dev)
            c2_reg = _rand_coords(coord_shape, dev)
            mask = (torch.rand(coord_shape[:-1], device=dev) > .1).unsqueeze(-1).to(torch.float32)
            return c1_nonzero * mask + c1_reg * (1 - mask), c2_nonzero * mask + c2_reg * (1 - mask), False
        mode = cfg.depth_sampling
        if mode == "simple":                             # src/modules.py:1299-1302: S x 1 grids, (B,S,1,2)
            if depth is None or depth_pos is None:
                raise AttributeError("depth_sampling='simple' needs depth and depth_pos")
            self._refuse_large_grid(orig_feats, "depth_sampling = 'simple'")
            c1 = ops.simple_depth_coords(depth, orig_feats.shape[-2:], S)
            c2 = ops.simple_depth_coords(depth_pos, orig_feats_pos.shape[-2:], S)
            return c1, c2, False
        # 'fps_depth_feat' == 'fps' in the reference (quirk Q13: farthest_point_sampling_depth drops the feature rows it forms and
        # calls the depth-only fps).  cfg.dg_fps_feats = True gives that mode the sampler its name promises - the reference's
        # uncalled fps_depth_feats (src/modules.py:1124-1180) on the feature maps as handed in; 'fps' never reads the key.
        if mode in ("fps", "fps_depth_feat"):
            if depth is None or depth_pos is None:
                raise AttributeError("depth_sampling='fps' needs depth and depth_pos (the reference fails on None too, quirk Q8)")
            # a signal above 4096 positions (cfg.use_true_labels: the one-hot maps have the labels' resolution, and the reference pools
            # the depth to the signal's, src/modules.py:1003): the large sampler, the same selection bit for bit where both serve
            large = orig_feats.shape[-2] * orig_feats.shape[-1] > ops.FPS_MAX_POSITIONS
            fps_one, fps_pair = (ops.fps_coords_large, ops.fps_coords_large_pair) if large else (ops.fps_coords, ops.fps_coords_pair)
            if mode == "fps_depth_feat" and getattr(cfg, "dg_fps_feats", False):
                self._refuse_large_grid(orig_feats, "depth_sampling = 'fps_depth_feat' with cfg.dg_fps_feats")
                as_read = lambda t: t.to(torch.float32).contiguous()         # (the sampler reads its maps in place)
                d1, d2, f1, f2 = as_read(depth), as_read(depth_pos), as_read(orig_feats), as_read(orig_feats_pos)
                if d1.shape == d2.shape and f1.shape == f2.shape:
                    both = ops.fps_feats_coords_pair(d1, d2, f1, f2, f1.shape[-2:], S)
                    c1, c2 = both[:B], both[B:]
                else:
                    c1 = ops.fps_feats_coords(d1, f1, f1.shape[-2:], S)
                    c2 = ops.fps_feats_coords(d2, f2, f2.shape[-2:], S)
            elif depth.shape == depth_pos.shape and orig_feats.shape[-2:] == orig_feats_pos.shape[-2:]:
                # one launch for both maps: the sampler is a sequential per-image loop (one block per image), so the two
                # calls of the reference (src/modules.py:1304-1308) simply run side by side on twice as many CUs
                both = fps_pair(depth, depth_pos, orig_feats.shape[-2:], S)
                c1, c2 = both[:B], both[B:]
            else:
                c1 = fps_one(depth, orig_feats.shape[-2:], S)
                c2 = fps_one(depth_pos, orig_feats_pos.shape[-2:], S)
            assert tuple(c1.shape) == tuple(c2.shape) == tuple(coord_shape), f"{c1.shape} != {c2.shape} != {coord_shape}"
            return c1, c2, False
        if getattr(cfg, "dg_dense_grid", False) and same_maps and S == orig_feats.shape[-2] == orig_feats.shape[-1]:
            key = (B, S, str(dev))
            if self._ident_cache[0] != key:          # constant tensor: built once per (B, S, device)
                self._ident_cache = (key, identity_coords(B, S, dev))
            c = self._ident_cache[1]
            return c, c, True
        if getattr(cfg, "dg_graph_safe", False):
            # the step is recorded in a hipGraph: both coordinate sets from the device-resident generator the negatives' batch maps
            # use, one launch (torch's generator inside a graph: one launch per tensor and two 64-bit fills per replay)
            c1, c2 = ops.rand_coords_state(self._graph_state(dev), coord_shape)
            return c1, c2, False
        c1 = _rand_coords(coord_shape, dev)
        c2 = _rand_coords(coord_shape, dev)
        return c1, c2, False

    @staticmethod
    def _refuse_large_grid(orig_feats, what):
        """The samplers that stay at 4096 positions, asked in front of their launch: the way out by name."""
        h, w = orig_feats.shape[-2:]
        if h * w > ops.FPS_MAX_POSITIONS:
            raise ValueError(f"depthg_amd: {what} samples on the signal's own grid and serves at most {ops.FPS_MAX_POSITIONS} positions, "
                             f"got {h}x{w}.  Under cfg.use_true_labels the signal has the labels' resolution: set cfg.depth_sampling = "
                             f"'fps' (its sampler serves up to {ops.FPS_LARGE_MAX_POSITIONS} positions) or 'none'")

    def _graph_state(self, dev):
        """Generator state on the device (hipGraph-capturable step: nothing about a draw is baked into a launch)."""
        if self._perm_state is None or self._perm_state.device != dev:
            self._perm_state = ops.new_perm_state(dev)
        return self._perm_state

    @staticmethod
    def _check_maps(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth):
        """The C side receives raw pointers: everything it assumes about the four maps is checked here.  The reference's
        `sample()` (src/modules.py:822-825) takes normalised coordinates, so the code maps may have another resolution than the
        feature maps (FeaturePyramidNet: low_res_feats (B,2048,7,7), code (B,dim,56,56), src/modules.py:732-766); what torch
        itself would refuse there - another batch size (grid_sample), another channel count between the two operands of a
        correlation (einsum), tensors on different devices - raises RuntimeError here as well."""
        maps = (("orig_feats", orig_feats), ("orig_feats_pos", orig_feats_pos), ("orig_code", orig_code),
                ("orig_code_pos", orig_code_pos))
        for name, t in maps:
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"depthg_amd: `{name}` must be a 4-D (B,K,h,w) tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if not t.is_floating_point():
                raise ValueError(f"depthg_amd: `{name}` must be a floating-point tensor, got {t.dtype}")
        dev, B = orig_feats.device, orig_feats.shape[0]
        for name, t in maps[1:] + ((("depth", depth),) if depth is not None else ()):
            if t.device != dev:
                raise RuntimeError(f"depthg_amd: `{name}` lives on {t.device}, `orig_feats` on {dev}: all inputs of one call must "
                                   f"share a device")
            if t.shape[0] != B:
                raise RuntimeError(f"depthg_amd: `{name}` has batch size {t.shape[0]}, `orig_feats` has {B} (the reference's "
                                   f"grid_sample / einsum refuse that too)")
        if tuple(orig_feats_pos.shape) != tuple(orig_feats.shape):
            raise RuntimeError(f"depthg_amd: orig_feats_pos {tuple(orig_feats_pos.shape)} must have the shape of orig_feats "
                               f"{tuple(orig_feats.shape)} (one featurizer produces both)")
        if tuple(orig_code_pos.shape) != tuple(orig_code.shape):
            raise RuntimeError(f"depthg_amd: orig_code_pos {tuple(orig_code_pos.shape)} must have the shape of orig_code "
                               f"{tuple(orig_code.shape)} (one head produces both)")
        if depth is not None and (depth.dim() != 4 or depth.shape[1] != 1):
            raise ValueError(f"depthg_amd: `depth` must be (B,1,H,W), got {tuple(depth.shape)}")

    def forward(self, orig_feats, orig_feats_pos, orig_salience, orig_salience_pos, orig_code, orig_code_pos,
                depth=None, depth_pos=None):
        orig_feats, orig_feats_pos, feat_keep = self._unwrap_deferred(orig_feats, orig_feats_pos)
        self._check_maps(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth)
        if depth_pos is not None and depth is not None and (depth_pos.device != depth.device or depth_pos.shape[0] != depth.shape[0]):
            raise RuntimeError(f"depthg_amd: depth_pos {tuple(depth_pos.shape)} on {depth_pos.device} does not match depth "
                               f"{tuple(depth.shape)} on {depth.device}")
        coords1, coords2, shared = self._draw_coords(orig_feats, orig_feats_pos, orig_salience, orig_salience_pos,
                                                     depth, depth_pos, same_maps=orig_code.shape[-2:] == orig_feats.shape[-2:])
        state = None
        if getattr(self.cfg, "dg_graph_safe", False):
            state = self._graph_state(orig_feats.device)
        # the negatives' batch maps (super_perm, src/modules.py:1340-1342) are drawn by the forward itself: perms=None
        # (seed from torch's CPU generator unless the device generator is in use); `shared` is only ever set together with the
        # identity grid drawn above
        return self.forward_with(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, None,
                                 shared_coords=shared, identity_grid=shared, draw_state=state, _checked=True, feat_keep=feat_keep)

    @staticmethod
    def _unwrap_deferred(orig_feats, orig_feats_pos):
        """ops.DeferredDropout in place of a feature map (the head's forward_pair(..., defer_feats_dropout=True)): the un-dropped
        maps and (keep, keep_pos, scale) for dg_corr_forward_masked - or None when neither is deferred.  Two different scales
        cannot ride in one call: the second map is then materialised here."""
        da = orig_feats if isinstance(orig_feats, ops.DeferredDropout) else None
        db = orig_feats_pos if isinstance(orig_feats_pos, ops.DeferredDropout) else None
        if da is None and db is None:
            return orig_feats, orig_feats_pos, None
        if da is not None and db is not None and da.scale != db.scale:
            orig_feats_pos, db = db.materialize(), None
        scale = da.scale if da is not None else db.scale
        f32 = lambda k: k.detach().to(torch.float32).contiguous()
        return (da.feats if da is not None else orig_feats, db.feats if db is not None else orig_feats_pos,
                (f32(da.keep) if da is not None else None, f32(db.keep) if db is not None else None, scale))

    # -- everything after the RNG draws (explicit coords / perms: parity tests, DP shards) ----------
    def forward_with(self, orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms,
                     shared_coords=False, identity_grid=False, draw_state=None, _checked=False, feat_keep=None, intra_feats=None):
        """intra_feats: fp32 contiguous, the shape of orig_feats - the intra pair-set's feature map (DepthContrastiveCorrelationLoss)."""
        if feat_keep is None:
            orig_feats, orig_feats_pos, feat_keep = self._unwrap_deferred(orig_feats, orig_feats_pos)
        if not _checked:
            self._check_maps(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth)
        call = self._prepare(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms,
                             bool(shared_coords), bool(identity_grid), draw_state, feat_keep, intra_feats=intra_feats)
        wide = call.C > ops.BLOB_MAX_C and (call.identity_grid or call.P_pos > SMALL_GRID_POSITIONS)
        if call.feat_keep is not None and (wide or not call.identity_grid):
            # only the identity grid's own operand preparation takes the keep flags (dg_corr_forward_masked): the samplers, and the
            # normalisation in front of a wide map's chunks, read the dropped tensors - formed here, the same values
            call.feats, call.feats_pos = self._apply_keep(call.feats, call.feats_pos, call.feat_keep)
            call.feat_keep = None
        if not wide:
            out, total, chunks = self._run_chunks(call, [call.feats], [call.feats_pos], keep=call.feat_keep)
        elif call.identity_grid:
            # Feature maps wider than the operand kernels hold, on the dense identity grid: the loss is LINEAR in the feature
            # correlation fd = sum over channels (src/modules.py:797-809; helper(), :1231-1254: the centering of fd, the shift and
            # -clamp(cd) * (fd - shift)), and on this grid sample() is a transposition, so norm() can run in front of it.  The maps are
            # normalised over all C channels once (dg_normalize_split) and evaluated chunk by chunk (DG_FEATS_UNIT): the first chunk
            # with the recipe's shifts and depth term, the others with zero shifts and without it; the loss means and the code
            # gradients add up, the cd means (and everything of the depth term) are the first chunk's.
            chunk_c = self._chunk_channels(call.C)
            out, total, chunks = self._run_chunks(call, ops.normalize_split(call.feats, chunk_c), ops.normalize_split(call.feats_pos, chunk_c),
                                                  unit=True)
        else:
            fa, fb, feat_inv = self._wide_sampled_operands(call)
            out, total, chunks = self._run_chunks(call, fa, fb, feat_inv=feat_inv)
        desc, ws = chunks[0]
        d = self.__dict__                      # plain attributes: nn.Module.__setattr__ costs microseconds per assignment
        d["last_scalars"] = out.detach()
        d["scalars"] = out                     # the fused output vector with its grad_fn (DG_OUT_* order)
        d["total"] = total                     # weighted total of the loss means (src/train_segmentation.py:330-349)
        d["last_call"] = (desc, call.perms, ws)   # measurement aid (bench.py re-launches the fused kernel alone)
        # cd_histograms(): handles only - descriptor, batch maps and workspace of the (first) chunk, and the stamp its forward left on it
        d["_hist_call"] = (desc, call.perms, ws, getattr(ws, "_dg_forward", None))
        return self._outputs(call, out, chunks)

    def cd_histograms(self, bins=64, range=(-1., 1.)):
        """Histograms of the un-reduced code correlations of the most recent forward - what the reference's training_step logs every
        cfg.hist_freq steps (src/train_segmentation.py:229-231, 298-301): {"intra_cd", "inter_cd", "neg_cd"} -> int64 (bins,) device
        tensors over `range`, torch.histc's bins except that a value outside the range counts in the nearest end bin (every histogram
        sums to its tensor's element count).  `neg_cd` is the sum over the negatives: the reference histograms their concatenation.
        One small launch on the operands the forward left in its workspace (ops.corr_cd_hist), in both cfg.dg_outputs modes; a wide
        map run in channel chunks uses the first chunk's, since cd does not depend on the feature chunk.  Reads only: a later
        backward() is not affected."""
        call = self.__dict__.get("_hist_call")
        if call is None:
            raise RuntimeError("depthg_amd: cd_histograms() covers the most recent forward of this loss, and none has run yet")
        desc, perms, ws, stamp = call
        if stamp is None or getattr(ws, "_dg_forward", None) != stamp:
            raise RuntimeError("depthg_amd: cd_histograms(): the workspace of the last forward has been run on again since (its "
                               "operands are gone); call cd_histograms() right after the forward it is to describe")
        n_neg = int(desc.n_neg)
        counts = ops.corr_cd_hist(desc, ws, 0, 2 + n_neg, perms=perms, bins=bins, range=range)
        return {"intra_cd": counts[0], "inter_cd": counts[1], "neg_cd": counts[2:].sum(dim=0)}

    def _prepare(self, orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth, coords1, coords2, perms, shared_coords,
                 identity_grid, draw_state, feat_keep, intra_feats=None):
        """Everything forward_with checks and converts in front of the first launch, in the order the errors are promised in: the
        call's operands as the library reads them and its dimensions, as one namespace."""
        cfg = self.cfg
        if identity_grid and tuple(orig_code.shape[-2:]) != tuple(orig_feats.shape[-2:]):
            raise ValueError(f"depthg_amd: the identity grid needs code maps of the feature maps' size, got "
                             f"{orig_code.shape[-2]}x{orig_code.shape[-1]} against {orig_feats.shape[-2]}x{orig_feats.shape[-1]}")
        if identity_grid and int(cfg.feature_samples) ** 2 <= SMALL_GRID_POSITIONS and not getattr(cfg, "dg_small_identity_blobs", False):
            # Dense grids of at most 160 positions (7 x 7 ... 12 x 12) do NOT take the identity-grid launches: the identity
            # coordinates go through the sampler like any others (what the reference does with them) and the fused small-grid kernel
            # runs, whose clamp masks are exact.  The blob kernels' fp16 cd decides the mask there, and on so few positions a handful of
            # flipped elements is percents of a gradient (round 5's randomised sweep, seed 5133: 7 x 7, d/d code_pos 4.1e-2 rel-L2).
            # (cfg.dg_small_identity_blobs: the old route, kept for A/B runs and the C-ABI tests of DG_IDENTITY_GRID at small P.)
            identity_grid = False
        if feat_keep is not None:
            for name, k in (("orig_feats", feat_keep[0]), ("orig_feats_pos", feat_keep[1])):
                if k is not None and (tuple(k.shape) != tuple(orig_feats.shape[:2]) or k.device != orig_feats.device):
                    raise RuntimeError(f"depthg_amd: keep flags of `{name}` are {tuple(k.shape)} on {k.device}; the maps are "
                                       f"{tuple(orig_feats.shape)} on {orig_feats.device}")
        B, C, h, w = orig_feats.shape
        D, hc, wc = orig_code.shape[1:]
        S, N = int(cfg.feature_samples), int(cfg.neg_samples)
        if tuple(coords1.shape) != tuple(coords2.shape) or tuple(coords1.shape) not in ((B, S, S, 2), (B, S, 1, 2)):
            raise ValueError(f"depthg_amd: coords must both be (B,S,S,2) or (B,S,1,2) with B={B}, S={S}; got "
                             f"{tuple(coords1.shape)} and {tuple(coords2.shape)}")
        depth_term = bool(cfg.depth_feat_correlation_loss)
        if depth_term and depth is None:
            raise AttributeError("depth_feat_correlation_loss=True needs `depth` (reference: interpolate(None) raises)")
        dev = orig_feats.device
        feats = ops._f32c(orig_feats, "orig_feats")
        feats_pos = ops._f32c(orig_feats_pos, "orig_feats_pos")
        depth_c = ops._f32c(depth, "depth") if depth_term else None
        coords1 = ops._f32c(coords1, "coords1")
        coords2 = ops._f32c(coords2, "coords2")
        if coords1.device != dev or coords2.device != dev:
            raise RuntimeError(f"depthg_amd: coords live on {coords1.device} / {coords2.device}, the maps on {dev}")
        if perms is None:
            perms_t = None                 # drawn inside the forward (dg_corr_forward_draw)
        elif isinstance(perms, (list, tuple)):
            perms_t = torch.stack([p.to(device=dev, dtype=torch.long) for p in perms]) if N > 0 else \
                torch.zeros(0, B, dtype=torch.long, device=dev)
        else:
            perms_t = perms.to(device=dev, dtype=torch.long)
        if perms_t is not None:
            perms_t = perms_t.contiguous()
            assert perms_t.shape == (N, B), f"perms shape {tuple(perms_t.shape)} != {(N, B)}"
        code = orig_code if orig_code.dtype == torch.float32 else orig_code.float()
        code_pos = orig_code_pos if orig_code_pos.dtype == torch.float32 else orig_code_pos.float()
        return SimpleNamespace(
            feats=feats, feats_pos=feats_pos, code=code.contiguous(), code_pos=code_pos.contiguous(), depth=depth_c, coords1=coords1,
            coords2=coords2, perms=perms_t, feat_keep=feat_keep, intra_feats=intra_feats, draw_state=draw_state, dev=dev,
            B=B, C=C, h=h, w=w, D=D, S=S, N=N, code_hw=None if (hc, wc) == (h, w) else (hc, wc),
            P_pos=int(coords1.shape[1]) * int(coords1.shape[2]), line_grid=coords1.shape[2] == 1 and S != 1,       # S x 1 grid of depth_sampling='simple'
            depth_term=depth_term, shared_coords=shared_coords, identity_grid=identity_grid,
            need_grad=torch.is_grad_enabled() and (orig_code.requires_grad or orig_code_pos.requires_grad),
            shifts=(cfg.pos_intra_shift, cfg.pos_inter_shift, cfg.neg_inter_shift, cfg.depth_feat_shift if depth_term else 0.0))

    @staticmethod
    def _apply_keep(feats, feats_pos, feat_keep):
        """The deferred Dropout2d in torch: x * (keep * scale), the fp32 product the featurizer would have stored."""
        ka, kb, kscale = feat_keep
        if ka is not None:
            feats = feats * (ka * kscale)[:, :, None, None]
        if kb is not None:
            feats_pos = feats_pos * (kb * kscale)[:, :, None, None]
        return feats, feats_pos

    @staticmethod
    def _chunk_channels(C):
        """Channels per chunk of a map wider than the operand kernels hold: even chunks, a multiple of 8."""
        nch = (C + ops.BLOB_MAX_C - 1) // ops.BLOB_MAX_C
        return ((C + nch - 1) // nch + 7) // 8 * 8

    def _run_chunk(self, call, f_a, f_b, first, unit, keep, feat_inv):
        """One launch set of the C ABI on feature maps of the width the operand kernels hold (`first`: the recipe's shifts and depth
        term; else a further channel chunk of a wider map: zero shifts, no depth term).  -> (out, total, desc, workspace)."""
        cfg = self.cfg
        dt = call.depth_term and first
        # the total's weights are those of the CALL's depth term on every chunk: the caller's lhp balance scales all terms of the total
        # (src/train_segmentation.py:326-335), not the first chunk's alone; a further chunk has no depth term, so no depth weight
        weights = self._total_weights(call.depth_term)
        if not dt:
            weights = weights[:3] + (0.0,)
        desc = ops.make_desc(call.B, f_a.shape[1], call.D, call.h, call.w, call.S, call.N, pointwise=bool(cfg.pointwise),
                             zero_clamp=bool(cfg.zero_clamp), stabalize=bool(cfg.stabalize), depth_term=dt, need_grad=call.need_grad,
                             shared_coords=call.shared_coords, shifts=call.shifts if first else (0.0, 0.0, 0.0, 0.0),
                             depth_hw=tuple(call.depth.shape[-2:]) if (call.depth is not None and dt) else (0, 0),
                             identity_grid=call.identity_grid, weights=weights, line_grid=call.line_grid,
                             code_hw=call.code_hw, exact_masks=bool(getattr(cfg, "dg_exact_masks", False)), feats_unit=unit)
        launched = _Launched()
        out, total = _CorrLossFunction.apply(call.code, call.code_pos, f_a, f_b, call.depth if dt else None, call.coords1, call.coords2,
                                             call.perms, desc, call.draw_state, keep, feat_inv, call.intra_feats, launched)
        if call.perms is None:
            call.perms = launched.perms        # (drawn by the forward: what backward, materialize and further chunks read)
        return out, total, desc, launched.workspace

    def _run_chunks(self, call, fa, fb, unit=False, keep=None, feat_inv=None):
        """The channel chunks fa[k] / fb[k] of the two feature maps, one launch set each (a map the kernels hold whole: one chunk):
        the loss means and the total add up over the chunks, the cd means (and everything of the depth term) are the first chunk's.
        -> (out, total, [(desc, workspace) per chunk])."""
        chunks = []
        for k in range(len(fa)):
            o_k, t_k, desc_k, ws_k = self._run_chunk(call, fa[k], fb[k], k == 0, unit, keep, feat_inv)
            chunks.append((desc_k, ws_k, o_k, t_k))
        out, total = chunks[0][2], chunks[0][3]
        if len(chunks) > 1:
            lossmask = torch.zeros(ops._lib.DG_OUT_COUNT, device=call.dev)
            lossmask[[0, 1, 2, ops._lib.DG_OUT_TOTAL]] = 1.0
            for _, _, o_k, t_k in chunks[1:]:
                out = out + o_k * lossmask
                total = total + t_k
        return out, total, [c[:2] for c in chunks]

    def _wide_sampled_operands(self, call):
        """Wide maps on SAMPLED coordinates above 160 positions: the reference normalises behind sample(), so the norm of every
        sampled vector is formed over all channel chunks first (dg_sampled_sumsq per operand: feats at coords1, feats_pos at coords2
        and, with coordinates per image, feats through every negative's batch map at coords2), then each chunk runs with those norms
        (dg_corr_forward_extnorm) - shifts, depth term and the sums as on the dense grid.  -> (chunks of feats, of feats_pos, feat_inv)."""
        B, C, N, dev = call.B, call.C, call.N, call.dev
        if call.perms is None:
            call.perms = super_perms(N, B, dev) if N > 0 else torch.zeros(0, B, dtype=torch.long, device=dev)
        nops = 2 if (call.shared_coords or N == 0) else 2 + N
        chunk_c = self._chunk_channels(C)
        fa = [call.feats[:, k:k + chunk_c].contiguous() for k in range(0, C, chunk_c)]
        fb = [call.feats_pos[:, k:k + chunk_c].contiguous() for k in range(0, C, chunk_c)]
        sumsq = torch.empty(nops, B, call.P_pos, device=dev, dtype=torch.float32)
        for k in range(len(fa)):
            ops.sampled_sumsq(fa[k], call.coords1, None, sumsq[0], k > 0)
            ops.sampled_sumsq(fb[k], call.coords2, None, sumsq[1], k > 0)
            for j in range(2, nops):
                ops.sampled_sumsq(fa[k], call.coords2, call.perms[j - 2], sumsq[j], k > 0)     # (the negatives are orig_feats[perm] at coords2, src/modules.py:1341-1345)
        return fa, fb, (1.0 / sumsq.sqrt().clamp_min(1e-10)).contiguous()

    def _outputs(self, call, out, chunks):
        """The reference's 6- / 8-tuple (src/modules.py:1352-1367) from the fused scalars: cfg.dg_outputs "reduced" - the means
        alone; "full" - the un-reduced tensors, materialised from the operands the forward left in the chunks' workspaces."""
        mode = getattr(self.cfg, "dg_outputs", "full")
        if mode == "reduced":
            res = (out[0], out[4:5].detach(), out[1], out[5:6].detach(), out[2:3], out[6:7].detach())
            if call.depth_term:
                res = res + (out[3], out[7:8].detach())
            return res
        if mode != "full":
            raise ValueError(f"cfg.dg_outputs must be 'full' or 'reduced', got {mode!r}")
        # cd tensors carry no gradient (the caller only logs them)
        # (on the shared dense grid the negatives' operands are the anchors' operand read through the batch maps: the maps go along;
        #  a 28 x 28 tensor is 78.7 MB per pair-set at B = 32 - the reference materialises them on every step, here only when asked)
        (desc, ws), perms_t = chunks[0], call.perms
        intra_cd, _ = ops.corr_materialize(desc, 0, ws)
        inter_cd, _ = ops.corr_materialize(desc, 1, ws)
        neg_cd, neg_loss = [], []
        for k in range(call.N):
            c, l = ops.corr_materialize(desc, 2 + k, ws, want_cd=True, want_loss=True, perms=perms_t)
            for desc_j, ws_j in chunks[1:]:    # (a wide map in channel chunks: the un-reduced loss is the sum of the chunks' too)
                l = l + ops.corr_materialize(desc_j, 2 + k, ws_j, want_cd=False, want_loss=True, perms=perms_t)[1]
            neg_cd.append(c)
            neg_loss.append(l)
        if call.N > 0:
            neg_cd_t = torch.cat(neg_cd, dim=0)
            # un-reduced negative loss: values from the kernel; gradient routed through its mean (exact for the
            # uniform upstreams that .mean()/.sum() produce, which is how the caller consumes it,
            # src/train_segmentation.py:303)
            neg_loss_t = torch.cat(neg_loss, dim=0) + (out[2] - out[2].detach())
        else:
            sh = 1 if call.line_grid else call.S
            neg_cd_t = torch.zeros(0, sh, call.S, sh, call.S, device=call.dev)
            neg_loss_t = neg_cd_t.clone()
        res = (out[0], intra_cd, out[1], inter_cd, neg_loss_t, neg_cd_t)
        if call.depth_term:
            dd, _ = ops.corr_materialize(desc, -1, ws)
            res = res + (out[3], dd)
        return res


class DepthContrastiveCorrelationLoss(ContrastiveCorrelationLoss):
    """Drop-in for the reference class of the same name (src/modules.py:1370-1463): ContrastiveCorrelationLoss with ONE difference -
    the self-correlation (intra) pair-set takes its feature correlation from `depth_aug_feats` sampled at coords1 (:1433,
    1437-1438); the inter pair-set and the negatives keep `orig_feats` / `orig_feats_pos`.  Same constructor, same call signature,
    the 6-tuple with ContrastiveCorrelationLoss's conventions (detached cd tensors, `neg_inter_loss` routed through its mean; both
    cfg.dg_outputs modes), `.scalars`, `.total` and `.cd_histograms()`.  One launch set (dg_corr_forward_intra_feats): the second map
    costs one more gathered operand, not a second call.

    Coordinates as the reference draws them (:1415-1425): the five draws of the salience branch, else two `torch.rand`;
    `cfg.depth_sampling` is ignored (the class has no depth to sample by), and so is cfg.dg_dense_grid.  The negatives' batch maps
    are drawn as ContrastiveCorrelationLoss draws them.

    `depth_aug_feats_pos` is validated for shape, dtype and device and then NOT read: the reference samples it (:1434) and never
    uses the result.

    Refused, each with the way out: feature maps wider than 768 channels, ops.DeferredDropout inputs
    (`takes_deferred_dropout` is False), cfg.depth_feat_correlation_loss (the reference's caller would unpack eight values from
    this class's six) and cfg.dg_graph_safe."""

    def takes_deferred_dropout(self, feat_hw, code_hw=None) -> bool:
        return False

    def _refuse_cfg(self):
        cfg = self.cfg
        if getattr(cfg, "depth_feat_correlation_loss", False):
            raise ValueError("depthg_amd: DepthContrastiveCorrelationLoss has no depth term - the reference returns six values and its "
                             "caller would unpack eight (src/train_segmentation.py:310-329); set cfg.depth_feat_correlation_loss = False "
                             "or use ContrastiveCorrelationLoss")
        if getattr(cfg, "dg_graph_safe", False):
            raise ValueError("depthg_amd: DepthContrastiveCorrelationLoss does not run under cfg.dg_graph_safe (its draws are torch's); "
                             "set cfg.dg_graph_safe = False or use ContrastiveCorrelationLoss")

    @staticmethod
    def _check_aug(orig_feats, depth_aug_feats, depth_aug_feats_pos):
        for name, t in (("orig_feats", orig_feats), ("depth_aug_feats", depth_aug_feats), ("depth_aug_feats_pos", depth_aug_feats_pos)):
            if isinstance(t, ops.DeferredDropout):
                raise ValueError(f"depthg_amd: DepthContrastiveCorrelationLoss takes feature tensors, `{name}` is an ops.DeferredDropout: "
                                 f"pass `{name}.materialize()` (or call the head without defer_feats_dropout)")
        for name, t in (("depth_aug_feats", depth_aug_feats), ("depth_aug_feats_pos", depth_aug_feats_pos)):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise ValueError(f"depthg_amd: `{name}` must be a floating-point tensor, got "
                                 f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
            if isinstance(orig_feats, torch.Tensor) and tuple(t.shape) != tuple(orig_feats.shape):
                raise RuntimeError(f"depthg_amd: `{name}` {tuple(t.shape)} must have the shape of orig_feats {tuple(orig_feats.shape)} "
                                   f"(one featurizer produces both)")
            if isinstance(orig_feats, torch.Tensor) and t.device != orig_feats.device:
                raise RuntimeError(f"depthg_amd: `{name}` lives on {t.device}, `orig_feats` on {orig_feats.device}: all inputs of one "
                                   f"call must share a device")
        if isinstance(orig_feats, torch.Tensor) and orig_feats.dim() == 4 and orig_feats.shape[1] > ops.BLOB_MAX_C:
            raise ValueError(f"depthg_amd: DepthContrastiveCorrelationLoss takes feature maps of at most {ops.BLOB_MAX_C} channels, got "
                             f"{orig_feats.shape[1]}: reduce the maps' width, or form the loss from two ContrastiveCorrelationLoss calls "
                             f"(it is linear in the feature correlation)")

    def _draw_coords(self, orig_feats, orig_feats_pos, orig_salience, orig_salience_pos, depth=None, depth_pos=None, same_maps=True):
        if getattr(self.cfg, "use_salience", False):          # (the parent's first branch: the same five draws, src/modules.py:1415-1422)
            return super()._draw_coords(orig_feats, orig_feats_pos, orig_salience, orig_salience_pos, None, None, same_maps)
        coord_shape = [orig_feats.shape[0], int(self.cfg.feature_samples), int(self.cfg.feature_samples), 2]
        return _rand_coords(coord_shape, orig_feats.device), _rand_coords(coord_shape, orig_feats.device), False

    def forward(self, orig_feats, orig_feats_pos, orig_salience, orig_salience_pos, orig_code, orig_code_pos,
                depth_aug_feats, depth_aug_feats_pos):
        self._refuse_cfg()
        self._check_aug(orig_feats, depth_aug_feats, depth_aug_feats_pos)
        self._check_maps(orig_feats, orig_feats_pos, orig_code, orig_code_pos, None)
        coords1, coords2, _ = self._draw_coords(orig_feats, orig_feats_pos, orig_salience, orig_salience_pos)
        return self.forward_with(orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth_aug_feats, depth_aug_feats_pos,
                                 coords1, coords2, None, _checked=True)

    def forward_with(self, orig_feats, orig_feats_pos, orig_code, orig_code_pos, depth_aug_feats, depth_aug_feats_pos,
                     coords1, coords2, perms, _checked=False):
        """Everything after the RNG draws: explicit coords (B,S,S,2) and perms ((n_neg, B), or None: drawn by the forward)."""
        if not _checked:
            self._refuse_cfg()
            self._check_aug(orig_feats, depth_aug_feats, depth_aug_feats_pos)
            self._check_maps(orig_feats, orig_feats_pos, orig_code, orig_code_pos, None)
        if tuple(orig_code.shape[-2:]) != tuple(orig_feats.shape[-2:]):
            raise ValueError(f"depthg_amd: DepthContrastiveCorrelationLoss needs code maps of the feature maps' size, got "
                             f"{orig_code.shape[-2]}x{orig_code.shape[-1]} against {orig_feats.shape[-2]}x{orig_feats.shape[-1]}")
        if tuple(coords1.shape) != (orig_feats.shape[0], int(self.cfg.feature_samples), int(self.cfg.feature_samples), 2):
            raise ValueError(f"depthg_amd: DepthContrastiveCorrelationLoss takes (B,S,S,2) coordinates, got {tuple(coords1.shape)}")
        return super().forward_with(orig_feats, orig_feats_pos, orig_code, orig_code_pos, None, coords1, coords2, perms,
                                    _checked=True, intra_feats=ops._f32c(depth_aug_feats, "depth_aug_feats"))
