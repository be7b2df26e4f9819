"""The workspace sizes of the three auxiliary loss terms (dg_crfloss_workspace_bytes, dg_augalign_workspace_bytes,
dg_recloss_workspace_bytes; dg_loss_args.h lays them out with one cursor) against literal values, and the Python views of their leading
sections (ops.*_workspace_sections) against those sizes.  The sizers are host code: no GPU is needed.

The values are what the library returned in front of the change that gave the three layouts one cursor (include/depthg_corr.h documents
the layouts to callers: they may not move by a byte).  Per term: sections that are and are not multiples of 256 bytes, the shapes of
the GPU tests, and the refusals (0: B above 65535, D above 128, n above the term's limit, non-positive sizes, tap records that do not
fit the LDS, a tensor of 2^31 elements).  The reconstruction term has no limit on B of its own: 65536 images of 2 x 2 have a size."""
import pytest
import torch

# (B, D, n)
CRF = {
    (2, 5, 1): 1536, (2, 5, 4): 1536, (2, 5, 7): 2048, (2, 5, 14): 3328, (2, 6, 5): 2048, (2, 33, 40): 25856, (2, 70, 257): 311808,
    (2, 70, 514): 622080, (2, 70, 1000): 1208576, (2, 128, 64): 134912, (1, 64, 64): 34816, (1, 128, 4096): 4309504,
    (32, 70, 1000): 19332096, (5, 3, 3400): 1022976, (65, 73, 253): 10461696, (65535, 1, 1): 4456448,
    (65536, 5, 8): 0, (2, 129, 8): 0, (2, 5, 4097): 0, (0, 5, 1): 0, (2, 0, 1): 0, (2, 5, 0): 0,
}
# (B, D, h, w, n)
AUG = {
    (2, 5, 4, 4, 3): 3072, (2, 5, 7, 9, 6): 7680, (2, 33, 6, 6, 20): 154880, (2, 70, 28, 28, 28): 540160, (2, 128, 14, 14, 14): 227072,
    (2, 70, 56, 56, 56): 2158848, (5, 3, 8, 8, 58): 1215488, (1, 1, 1, 1, 1): 2048, (2, 64, 8, 8, 8): 41472, (3, 7, 5, 11, 13): 46080,
    (1, 3, 8, 8, 80): 462336, (32, 70, 28, 28, 28): 8634112, (2, 5, 32, 32, 63): 645888,
    (65536, 5, 4, 4, 3): 0, (2, 5, 4, 4, 256): 0, (2, 5, 128, 128, 100): 0, (2, 0, 4, 4, 3): 0, (2, 5, 0, 4, 3): 0, (2, 5, 4, 4, 0): 0,
}
# (B, D, C, h, w)
REC = {
    (2, 3, 5, 2, 2): 1536, (2, 70, 100, 5, 7): 58880, (2, 70, 384, 8, 8): 219904, (1, 27, 1024, 4, 4): 115712, (3, 128, 64, 9, 9): 201472,
    (2, 16, 32, 40, 40): 147712, (5, 3, 5, 58, 58): 225792, (1, 1, 1, 1, 1): 1536, (2, 64, 64, 8, 8): 35072,
    (32, 70, 384, 28, 28): 9028864, (4, 90, 768, 14, 14): 4483072, (1, 128, 1, 1, 1): 1792, (65536, 3, 5, 2, 2): 3708672,
    (2, 129, 5, 2, 2): 0, (0, 3, 5, 2, 2): 0, (2, 3, 0, 2, 2): 0, (2, 3, 5, 0, 2): 0, (2, 128, 1024, 2048, 2048): 0,
}


def _sections(term, ws, shape):
    from depthg_amd import ops
    if term == "crf":
        return ops.crf_loss_workspace_sections(ws, *shape)                    # (B, D, n)
    if term == "aug":
        return ops.aug_alignment_workspace_sections(ws, shape[0], shape[4])   # (B, n)
    return ops.rec_loss_workspace_sections(ws, shape[0], shape[3], shape[4])  # (B, h, w)


@pytest.mark.parametrize("term,sizer,table", [("crf", "dg_crfloss_workspace_bytes", CRF), ("aug", "dg_augalign_workspace_bytes", AUG),
                                              ("rec", "dg_recloss_workspace_bytes", REC)], ids=["crf", "aug", "rec"])
def test_sizes_are_the_pinned_ones_and_the_views_lie_inside(term, sizer, table):
    from depthg_amd import _lib
    fn = getattr(_lib.load(), sizer)
    assert sum(v == 0 for v in table.values()) >= 4 and sum(v > 0 for v in table.values()) >= 12
    for shape, want in table.items():
        total = fn(*shape)
        assert total == want, (sizer, shape, total, want)
        if total == 0:
            continue
        ws = torch.empty(total, dtype=torch.uint8)
        views = _sections(term, ws, shape)
        assert views
        end = 0
        for name, v in views.items():
            off = v.data_ptr() - ws.data_ptr()
            assert off % 256 == 0 and off >= end, (sizer, shape, name, off)  # in the layout's order, nothing overlapping
            end = off + v.numel() * v.element_size()
        assert end <= total, (sizer, shape, end, total)
