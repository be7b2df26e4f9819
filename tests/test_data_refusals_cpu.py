"""The refusals of the data path's seven C entries - GPU batch augmentation, batch preparation, the feature cache, the sample cache -
pinned by return code and full dg_last_error() text.  Every case hands the entry host buffers and sizes chosen so that one host check
fails in front of the first launch: no GPU is needed, and the addresses that stand for device memory are never dereferenced.  The
expected texts were recorded from the library, not written from its source; a change of any of them is a change of the C ABI's contract."""
import numpy as np
import pytest

from depthg_amd import _lib

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
DEV = 0x10000            # a 16-byte aligned address that stands for device memory
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _call(entry, order, args):
    """entry(*args in `order`): numpy arrays go as their host address, None as a null pointer."""
    assert set(args) == set(order), sorted(set(args) ^ set(order))
    lib = _lib.load()
    held = [args[k] for k in order]
    rc = getattr(lib, entry)(*[(v.ctypes.data if isinstance(v, np.ndarray) else v) for v in held])
    return rc, lib.dg_last_error().decode()


def _f3(v):
    return None if v is None else np.asarray(v, dtype=np.float32)


# ---- dg_augment_forward
AUGMENT = ("img stride_b stride_c stride_h stride_w records params mean stdv B C H W h w img_aug coord_aug workspace workspace_bytes "
           "stream").split()


def _augment_record(top=0, left=0, bh=8, bw=8, ops=(-1, -1, -1, -1), sigma=0.0):
    r = np.zeros(16, dtype=np.int32)
    r[1:5] = (top, left, bh, bw)
    r[5:9] = ops
    r[14:15] = np.asarray([sigma], dtype=np.float32).view(np.int32)
    return r


def augment(records=None, **kw):
    a = dict(B=1, C=3, H=8, W=8, h=4, w=4, img=DEV, params=DEV, mean=None, stdv=None, img_aug=DEV, coord_aug=DEV, workspace=DEV, stream=None)
    a.update(kw)
    H, W = a["H"], a["W"]
    for k, v in (("stride_b", 3 * H * W), ("stride_c", H * W), ("stride_h", W), ("stride_w", 1)):
        a.setdefault(k, v)
    a.setdefault("workspace_bytes", _lib.load().dg_augment_workspace_bytes(a["B"], a["h"], a["w"]))
    a["records"] = np.stack([_augment_record()] * max(a["B"], 1)) if records is None else np.stack(records)
    a["mean"], a["stdv"] = _f3(a["mean"]), _f3(a["stdv"])
    return _call("dg_augment_forward", AUGMENT, a)


# ---- dg_batch_prep and dg_samplecache_put: records over N = 2 samples of 4 x 4 source planes, output 4 x 4
def rec(kind, n, off=None, sw=4, sh=4, label_offset=0, rule=0):
    off = 48 * max(n, 0) if off is None else off
    lo = off & 0xffffffff
    return [kind, n, lo - (1 << 32) if lo >> 31 else lo, off >> 32, sw, sh, label_offset, rule]


IMAGES = [rec(0, 0), rec(0, 1)]


def _tables(N, H, W, tables):
    if tables is None:
        tables = np.tile(np.concatenate([np.arange(W), np.arange(H)]), (max(N, 1), 1))
    return np.ascontiguousarray(tables, dtype=np.int32)


BATCH = "packed packed_bytes records tables params n_records N H W mean stdv img label mask depth stream".split()


def batch(records=IMAGES, tables=None, **kw):
    a = dict(packed=DEV, packed_bytes=96, params=DEV, N=2, H=4, W=4, mean=MEAN, stdv=STD, img=DEV, label=None, mask=None, depth=None,
             stream=None)
    a.update(kw)
    a["records"] = None if records is None else np.asarray(records, dtype=np.int32).reshape(-1, 8)
    a.setdefault("n_records", 0 if records is None else len(a["records"]))
    a["tables"] = _tables(a["N"], a["H"], a["W"], tables) if tables is not False else None
    a["mean"], a["stdv"] = _f3(a["mean"]), _f3(a["stdv"])
    return _call("dg_batch_prep", BATCH, a)


SC_PUT = "cache n_images has_labels with_depth H W idx n packed packed_bytes records tables params n_records stream".split()


def sc_put(records=IMAGES, tables=None, **kw):
    a = dict(cache=DEV, n_images=8, has_labels=0, with_depth=0, H=4, W=4, idx=DEV, n=2, packed=DEV, packed_bytes=96, params=DEV, stream=None)
    a.update(kw)
    a["records"] = None if records is None else np.asarray(records, dtype=np.int32).reshape(-1, 8)
    a.setdefault("n_records", 0 if records is None else len(a["records"]))
    a["tables"] = _tables(min(a["n"], 4), a["H"], a["W"], tables) if tables is not False else None
    return _call("dg_samplecache_put", SC_PUT, a)


SC_GATHER = "cache n_images has_labels with_depth H W idx_a idx_b n mean stdv label_offset fill mask_rule img label mask depth stream".split()


def sc_gather(**kw):
    a = dict(cache=DEV, n_images=8, has_labels=0, with_depth=0, H=4, W=4, idx_a=DEV, idx_b=None, n=2, mean=MEAN, stdv=STD, label_offset=0,
             fill=-1, mask_rule=0, img=DEV, label=None, mask=None, depth=None, stream=None)
    a.update(kw)
    a["mean"], a["stdv"] = _f3(a["mean"]), _f3(a["stdv"])
    return _call("dg_samplecache_gather", SC_GATHER, a)


# ---- dg_featcache_put / dg_featcache_gather
FC_PUT = "cache dtype N L src idx n stream".split()
FC_GATHER = "cache dtype N L idx_a idx_b n out stream".split()


def fc_put(**kw):
    return _call("dg_featcache_put", FC_PUT, {**dict(cache=DEV, dtype=0, N=8, L=16, src=DEV, idx=DEV, n=2, stream=None), **kw})


def fc_gather(**kw):
    return _call("dg_featcache_gather", FC_GATHER, {**dict(cache=DEV, dtype=0, N=8, L=16, idx_a=DEV, idx_b=None, n=2, out=DEV, stream=None), **kw})


def _xs(i, v, N=2, H=4, W=4):
    t = np.tile(np.concatenate([np.arange(W), np.arange(H)]), (N, 1))
    t[0, i] = v
    return t


CASES = {
    # dg_augment_forward, in the order of its checks
    "augment-positive": lambda: augment(B=0),
    "augment-channels": lambda: augment(C=4),
    "augment-three-pixels": lambda: augment(h=2),
    "augment-too-large": lambda: augment(B=65536),
    "augment-strides": lambda: augment(stride_w=2),
    "augment-null": lambda: augment(img=None),
    "augment-mean-without-std": lambda: augment(mean=MEAN),
    "augment-aligned": lambda: augment(img=DEV + 2),
    "augment-workspace": lambda: augment(workspace_bytes=0),
    "augment-crop-box": lambda: augment(records=[_augment_record(top=1)]),
    "augment-op": lambda: augment(records=[_augment_record(ops=(-1, 4, -1, -1))]),
    "augment-two-contrasts": lambda: augment(records=[_augment_record(ops=(1, 0, 1, -1))]),
    "augment-sigma": lambda: augment(records=[_augment_record(sigma=-1.0)]),
    "augment-std": lambda: augment(mean=MEAN, stdv=(0.229, 0.0, 0.225)),
    # dg_batch_prep
    "batch-positive": lambda: batch(N=0),
    "batch-width": lambda: batch(W=6),
    "batch-too-large": lambda: batch(N=65536),
    "batch-null": lambda: batch(records=None, n_records=2),
    "batch-null-mean": lambda: batch(mean=None),
    "batch-aligned": lambda: batch(img=DEV + 4),
    "batch-params-aligned": lambda: batch(params=DEV + 2),
    "batch-std": lambda: batch(stdv=(0.229, 0.224, float("inf"))),
    "batch-mean-nan": lambda: batch(mean=(float("nan"), 0.456, 0.406)),
    "batch-kind": lambda: batch(records=[rec(5, 0)]),
    "batch-sample": lambda: batch(records=[rec(0, 2)]),
    "batch-null-output": lambda: batch(records=IMAGES + [rec(2, 0)]),
    "batch-null-mask": lambda: batch(records=IMAGES + [rec(1, 0)], label=DEV),
    "batch-twice": lambda: batch(records=[rec(0, 0), rec(0, 0)]),
    "batch-mask-rule": lambda: batch(records=IMAGES + [rec(4, 0, rule=2)], label=DEV, mask=DEV),
    "batch-two-mask-rules": lambda: batch(records=IMAGES + [rec(4, 0, rule=1), rec(4, 1, rule=0)], label=DEV, mask=DEV),
    "batch-source-empty": lambda: batch(records=[rec(0, 0, sw=0)]),
    "batch-source-too-large": lambda: batch(records=[rec(0, 0, sh=16385)]),
    "batch-source-leaves": lambda: batch(records=[rec(0, 0), rec(0, 1, off=49)]),
    "batch-source-offset": lambda: batch(records=[rec(0, 0, off=1 << 33)]),
    "batch-source-no-packed": lambda: batch(packed=None),
    "batch-column-table": lambda: batch(tables=_xs(3, 4)),
    "batch-row-table": lambda: batch(tables=_xs(4 + 1, -1)),
    "batch-count": lambda: batch(records=[rec(0, 0)]),
    "batch-depth-count": lambda: batch(records=IMAGES + [rec(3, 1)], depth=DEV),
    # dg_featcache_put / dg_featcache_gather: their shared checks through both entries, then each one's own
    **{f"fc-{name}-{k}": (lambda f=f, kw=kw: f(**kw)) for name, f in (("put", fc_put), ("gather", fc_gather)) for k, kw in (
        ("dtype", dict(dtype=3)), ("sizes", dict(L=0)), ("negative-n", dict(n=-1)), ("rows", dict(n=65536)), ("elements", dict(L=(1 << 40) + 1)),
        ("elements-product", dict(N=1 << 40, L=1 << 30)), ("null-cache", dict(cache=None)), ("cache-aligned", dict(cache=DEV + 2)),
        ("f16-cache-aligned", dict(cache=DEV + 1, dtype=1)), ("nothing", dict(n=0)))},
    "fc-gather-rows-two-lists": lambda: fc_gather(idx_b=DEV, n=32768),
    "fc-put-null": lambda: fc_put(src=None),
    "fc-put-aligned": lambda: fc_put(idx=DEV + 4),
    "fc-gather-null": lambda: fc_gather(out=None),
    "fc-gather-aligned": lambda: fc_gather(idx_b=DEV + 4),
    # dg_samplecache_put / dg_samplecache_gather: likewise
    **{f"sc-{name}-{k}": (lambda f=f, kw=kw: f(**kw)) for name, f in (("put", sc_put), ("gather", sc_gather)) for k, kw in (
        ("sizes", dict(n_images=0)), ("negative-n", dict(n=-1)), ("flags", dict(has_labels=2)), ("width", dict(W=6)), ("too-large", dict(H=16385)),
        ("rows", dict(n=65536)), ("bytes", dict(n_images=1 << 60)), ("null-cache", dict(cache=None)), ("cache-aligned", dict(cache=DEV + 2)),
        ("nothing", dict(n=0)))},
    "sc-gather-rows-two-lists": lambda: sc_gather(idx_b=DEV, n=32768),
    "sc-put-no-records": lambda: sc_put(n_records=0),
    "sc-put-too-many-records": lambda: sc_put(n_records=65536),
    "sc-put-null": lambda: sc_put(idx=None),
    "sc-put-null-tables": lambda: sc_put(tables=False),
    "sc-put-aligned": lambda: sc_put(idx=DEV + 4),
    "sc-put-params-aligned": lambda: sc_put(params=DEV + 2),
    "sc-put-kind": lambda: sc_put(records=[rec(-1, 0)]),
    "sc-put-sample": lambda: sc_put(records=[rec(0, -1)]),
    "sc-put-label-without-plane": lambda: sc_put(records=IMAGES + [rec(1, 1)]),
    "sc-put-fill-with-plane": lambda: sc_put(records=IMAGES + [rec(4, 1)], has_labels=1),
    "sc-put-depth-without-plane": lambda: sc_put(records=IMAGES + [rec(3, 0)]),
    "sc-put-twice": lambda: sc_put(records=IMAGES + [rec(4, 1), rec(4, 1)]),
    "sc-put-source-empty": lambda: sc_put(records=[rec(0, 0, sh=0)]),
    "sc-put-source-too-large": lambda: sc_put(records=[rec(0, 0, sw=16385)]),
    "sc-put-source-leaves": lambda: sc_put(records=IMAGES + [rec(2, 0, off=81)], with_depth=1),
    "sc-put-column-table": lambda: sc_put(tables=_xs(0, 7)),
    "sc-put-row-table": lambda: sc_put(tables=_xs(4, 4)),
    "sc-put-count": lambda: sc_put(records=[rec(0, 1)]),
    "sc-put-label-count": lambda: sc_put(records=IMAGES + [rec(1, 0, off=0, sw=4, sh=4)], has_labels=1),
    "sc-put-depth-count": lambda: sc_put(records=IMAGES + [rec(3, 0)], with_depth=1),
    "sc-gather-null": lambda: sc_gather(idx_a=None),
    "sc-gather-idx-aligned": lambda: sc_gather(idx_b=DEV + 4),
    "sc-gather-no-output": lambda: sc_gather(img=None),
    "sc-gather-aligned": lambda: sc_gather(label=DEV + 8),
    "sc-gather-depth-without-plane": lambda: sc_gather(depth=DEV),
    "sc-gather-mask-rule": lambda: sc_gather(mask=DEV, mask_rule=2),
    "sc-gather-null-mean": lambda: sc_gather(stdv=None),
    "sc-gather-std": lambda: sc_gather(stdv=(-0.229, 0.224, 0.225)),
}

EXPECTED = {
    'augment-positive': (-1, 'dg_augment_forward: B=0 C=3, image 8x8, output 4x4 must be positive'),
    'augment-channels': (-2, 'dg_augment_forward: 4 channels (the colour ops are RGB: 3)'),
    'augment-three-pixels': (-2, 'dg_augment_forward: image 8x8, output 2x4: reflect padding by 2 needs three pixels a side'),
    'augment-too-large': (-2, 'dg_augment_forward: B=65536 above 65535 or a side of 8x8 / 4x4 above 16384'),
    'augment-strides': (-2, 'dg_augment_forward: img is not contiguous (strides 192, 64, 8, 2): copy it once'),
    'augment-null': (-1, 'dg_augment_forward: null pointer'),
    'augment-mean-without-std': (-1, 'dg_augment_forward: mean and std come together: give both or neither'),
    'augment-aligned': (-1, 'dg_augment_forward: the tensors must be 4-byte aligned, workspace 16-byte aligned'),
    'augment-workspace': (-3, 'dg_augment_forward: workspace of 0 bytes, 256 needed (dg_augment_workspace_bytes)'),
    'augment-crop-box': (-2, 'dg_augment_forward: crop box (1, 0, 8, 8) of image 0 leaves the 8x8 image'),
    'augment-op': (-1, 'dg_augment_forward: image 0: op 4 in slot 1 (-1 .. 3)'),
    'augment-two-contrasts': (-2, 'dg_augment_forward: image 0 has 2 contrast ops (one image mean per image: one at most)'),
    'augment-sigma': (-1, 'dg_augment_forward: image 0: blur_sigma=-1'),
    'augment-std': (-1, 'dg_augment_forward: channel 1: mean=0.456 std=0'),
    'batch-positive': (-1, 'dg_batch_prep: n_records=2 N=0, output 4x4 must be positive'),
    'batch-width': (-2, 'dg_batch_prep: output width 6 is not a multiple of 4 (a lane stores four columns as one vector)'),
    'batch-too-large': (-2, 'dg_batch_prep: output 4x4 above 16384 a side, or N=65536 / n_records=2 above 65535'),
    'batch-null': (-1, 'dg_batch_prep: null pointer'),
    'batch-null-mean': (-1, 'dg_batch_prep: null pointer'),
    'batch-aligned': (-1, 'dg_batch_prep: img, label, mask and depth must be 16-byte aligned (whole-vector stores), params 4-byte aligned'),
    'batch-params-aligned': (-1, 'dg_batch_prep: img, label, mask and depth must be 16-byte aligned (whole-vector stores), params 4-byte aligned'),
    'batch-std': (-1, 'dg_batch_prep: channel 2: mean=0.406 std=inf'),
    'batch-mean-nan': (-1, 'dg_batch_prep: channel 0: mean=nan std=0.229'),
    'batch-kind': (-1, 'dg_batch_prep: record 0: unknown kind 5 (0 .. 4)'),
    'batch-sample': (-1, 'dg_batch_prep: record 0: sample 2 outside 0 .. 1'),
    'batch-null-output': (-1, 'dg_batch_prep: record 2 (kind 2) writes an output that is null'),
    'batch-null-mask': (-1, 'dg_batch_prep: record 2 (kind 1) writes an output that is null'),
    'batch-twice': (-1, 'dg_batch_prep: record 1: sample 0 of output 0 is written twice'),
    'batch-mask-rule': (-1, 'dg_batch_prep: record 2: unknown mask rule 2 (0, 1)'),
    'batch-two-mask-rules': (-1, 'dg_batch_prep: record 3: mask rule 0 after 1 (one mask tensor: one rule)'),
    'batch-source-empty': (-1, 'dg_batch_prep: record 0: zero-sized source plane 0x4'),
    'batch-source-too-large': (-2, 'dg_batch_prep: record 0: source plane 4x16385 above 16384 a side'),
    'batch-source-leaves': (-1, 'dg_batch_prep: record 1: plane of 48 bytes at offset 49 leaves the packed buffer of 96 bytes'),
    'batch-source-offset': (-1, 'dg_batch_prep: record 0: plane of 48 bytes at offset 8589934592 leaves the packed buffer of 96 bytes'),
    'batch-source-no-packed': (-1, 'dg_batch_prep: record 0: plane of 48 bytes at offset 0 leaves the packed buffer of 96 bytes'),
    'batch-column-table': (-1, 'dg_batch_prep: record 0: column table entry 3 = 4 outside the source width 4 (the plane is narrower than the tables address)'),
    'batch-row-table': (-1, 'dg_batch_prep: record 0: row table entry 1 = -1 outside the source height 4 (the plane is shorter than the tables address)'),
    'batch-count': (-1, 'dg_batch_prep: output 0 has records for 1 of 2 samples (every element must be written)'),
    'batch-depth-count': (-1, 'dg_batch_prep: output 2 has records for 1 of 2 samples (every element must be written)'),
    'fc-put-dtype': (-1, 'dg_featcache_put: unknown dtype 3 (0 float32, 1 float16, 2 bfloat16)'),
    'fc-put-sizes': (-1, 'dg_featcache_put: N=8 L=0 n=2 (N and L positive, n not negative)'),
    'fc-put-negative-n': (-1, 'dg_featcache_put: N=8 L=16 n=-1 (N and L positive, n not negative)'),
    'fc-put-rows': (-2, 'dg_featcache_put: 1 list(s) of 65536 rows in one call (at most 65535 rows)'),
    'fc-put-elements': (-2, 'dg_featcache_put: a cache of 8 x 1099511627777 elements'),
    'fc-put-elements-product': (-2, 'dg_featcache_put: a cache of 1099511627776 x 1073741824 elements'),
    'fc-put-null-cache': (-1, 'dg_featcache_put: null pointer'),
    'fc-put-cache-aligned': (-1, 'dg_featcache_put: the cache is not aligned to its element size'),
    'fc-put-f16-cache-aligned': (-1, 'dg_featcache_put: the cache is not aligned to its element size'),
    'fc-put-nothing': (0, ''),
    'fc-gather-dtype': (-1, 'dg_featcache_gather: unknown dtype 3 (0 float32, 1 float16, 2 bfloat16)'),
    'fc-gather-sizes': (-1, 'dg_featcache_gather: N=8 L=0 n=2 (N and L positive, n not negative)'),
    'fc-gather-negative-n': (-1, 'dg_featcache_gather: N=8 L=16 n=-1 (N and L positive, n not negative)'),
    'fc-gather-rows': (-2, 'dg_featcache_gather: 1 list(s) of 65536 rows in one call (at most 65535 rows)'),
    'fc-gather-elements': (-2, 'dg_featcache_gather: a cache of 8 x 1099511627777 elements'),
    'fc-gather-elements-product': (-2, 'dg_featcache_gather: a cache of 1099511627776 x 1073741824 elements'),
    'fc-gather-null-cache': (-1, 'dg_featcache_gather: null pointer'),
    'fc-gather-cache-aligned': (-1, 'dg_featcache_gather: the cache is not aligned to its element size'),
    'fc-gather-f16-cache-aligned': (-1, 'dg_featcache_gather: the cache is not aligned to its element size'),
    'fc-gather-nothing': (0, ''),
    'fc-gather-rows-two-lists': (-2, 'dg_featcache_gather: 2 list(s) of 32768 rows in one call (at most 65535 rows)'),
    'fc-put-null': (-1, 'dg_featcache_put: null pointer'),
    'fc-put-aligned': (-1, 'dg_featcache_put: src must be 4-byte aligned, idx 8-byte aligned'),
    'fc-gather-null': (-1, 'dg_featcache_gather: null pointer'),
    'fc-gather-aligned': (-1, 'dg_featcache_gather: out must be 4-byte aligned, idx_a and idx_b 8-byte aligned'),
    'sc-put-sizes': (-1, 'dg_samplecache_put: n_images=0, rows of 4x4, n=2 (n_images, H and W positive, n not negative)'),
    'sc-put-negative-n': (-1, 'dg_samplecache_put: n_images=8, rows of 4x4, n=-1 (n_images, H and W positive, n not negative)'),
    'sc-put-flags': (-1, 'dg_samplecache_put: has_labels=2 with_depth=0 (0 or 1 each)'),
    'sc-put-width': (-2, 'dg_samplecache_put: row width 6 is not a multiple of 4 (a lane moves four columns as one word)'),
    'sc-put-too-large': (-2, 'dg_samplecache_put: rows of 16385x4 above 16384 a side'),
    'sc-put-rows': (-2, 'dg_samplecache_put: 1 list(s) of 65536 rows in one call (at most 65535 rows)'),
    'sc-put-bytes': (-2, 'dg_samplecache_put: a cache of 1152921504606846976 rows of 4x4'),
    'sc-put-null-cache': (-1, 'dg_samplecache_put: null pointer'),
    'sc-put-cache-aligned': (-1, 'dg_samplecache_put: the cache must be 4-byte aligned (a lane moves four bytes as one word)'),
    'sc-put-nothing': (0, ''),
    'sc-gather-sizes': (-1, 'dg_samplecache_gather: n_images=0, rows of 4x4, n=2 (n_images, H and W positive, n not negative)'),
    'sc-gather-negative-n': (-1, 'dg_samplecache_gather: n_images=8, rows of 4x4, n=-1 (n_images, H and W positive, n not negative)'),
    'sc-gather-flags': (-1, 'dg_samplecache_gather: has_labels=2 with_depth=0 (0 or 1 each)'),
    'sc-gather-width': (-2, 'dg_samplecache_gather: row width 6 is not a multiple of 4 (a lane moves four columns as one word)'),
    'sc-gather-too-large': (-2, 'dg_samplecache_gather: rows of 16385x4 above 16384 a side'),
    'sc-gather-rows': (-2, 'dg_samplecache_gather: 1 list(s) of 65536 rows in one call (at most 65535 rows)'),
    'sc-gather-bytes': (-2, 'dg_samplecache_gather: a cache of 1152921504606846976 rows of 4x4'),
    'sc-gather-null-cache': (-1, 'dg_samplecache_gather: null pointer'),
    'sc-gather-cache-aligned': (-1, 'dg_samplecache_gather: the cache must be 4-byte aligned (a lane moves four bytes as one word)'),
    'sc-gather-nothing': (0, ''),
    'sc-gather-rows-two-lists': (-2, 'dg_samplecache_gather: 2 list(s) of 32768 rows in one call (at most 65535 rows)'),
    'sc-put-no-records': (-1, 'dg_samplecache_put: n_records=0 outside [1, 65535]'),
    'sc-put-too-many-records': (-1, 'dg_samplecache_put: n_records=65536 outside [1, 65535]'),
    'sc-put-null': (-1, 'dg_samplecache_put: null pointer'),
    'sc-put-null-tables': (-1, 'dg_samplecache_put: null pointer'),
    'sc-put-aligned': (-1, 'dg_samplecache_put: idx must be 8-byte aligned, params 4-byte aligned'),
    'sc-put-params-aligned': (-1, 'dg_samplecache_put: idx must be 8-byte aligned, params 4-byte aligned'),
    'sc-put-kind': (-1, 'dg_samplecache_put: record 0: unknown kind -1 (0 .. 4)'),
    'sc-put-sample': (-1, 'dg_samplecache_put: record 0: sample -1 outside 0 .. 1'),
    'sc-put-label-without-plane': (-1, 'dg_samplecache_put: record 2: sample 1 carries a label but the cache has no label plane'),
    'sc-put-fill-with-plane': (-1, 'dg_samplecache_put: record 2: sample 1 carries no label but the cache has a label plane'),
    'sc-put-depth-without-plane': (-1, 'dg_samplecache_put: record 2: sample 0 carries depth but the cache has no depth plane'),
    'sc-put-twice': (-1, 'dg_samplecache_put: record 3: plane group 1 of sample 1 is written twice'),
    'sc-put-source-empty': (-1, 'dg_samplecache_put: record 0: zero-sized source plane 4x0'),
    'sc-put-source-too-large': (-2, 'dg_samplecache_put: record 0: source plane 16385x4 above 16384 a side'),
    'sc-put-source-leaves': (-1, 'dg_samplecache_put: record 2: plane of 16 bytes at offset 81 leaves the packed buffer of 96 bytes'),
    'sc-put-column-table': (-1, 'dg_samplecache_put: record 0: column table entry 0 = 7 outside the source width 4 (the plane is narrower than the tables address)'),
    'sc-put-row-table': (-1, 'dg_samplecache_put: record 0: row table entry 0 = 4 outside the source height 4 (the plane is shorter than the tables address)'),
    'sc-put-count': (-1, 'dg_samplecache_put: records for 1 images, 0 labels and 0 depth maps of 2 samples (every byte of a row must be written)'),
    'sc-put-label-count': (-1, 'dg_samplecache_put: records for 2 images, 1 labels and 0 depth maps of 2 samples (every byte of a row must be written)'),
    'sc-put-depth-count': (-1, 'dg_samplecache_put: records for 2 images, 0 labels and 1 depth maps of 2 samples (every byte of a row must be written)'),
    'sc-gather-null': (-1, 'dg_samplecache_gather: null pointer'),
    'sc-gather-idx-aligned': (-1, 'dg_samplecache_gather: idx_a and idx_b must be 8-byte aligned'),
    'sc-gather-no-output': (-1, 'dg_samplecache_gather: no output asked for'),
    'sc-gather-aligned': (-1, 'dg_samplecache_gather: img, label, mask and depth must be 16-byte aligned (whole-vector stores)'),
    'sc-gather-depth-without-plane': (-1, 'dg_samplecache_gather: depth asked of a cache without a depth plane'),
    'sc-gather-mask-rule': (-1, 'dg_samplecache_gather: unknown mask rule 2 (0, 1)'),
    'sc-gather-null-mean': (-1, 'dg_samplecache_gather: img needs mean and stdv'),
    'sc-gather-std': (-1, 'dg_samplecache_gather: channel 0: mean=0.485 std=-0.229'),
}


def test_every_case_has_its_text():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case):
    rc, text = CASES[case]()
    want_rc, want_text = EXPECTED[case]
    if want_rc == OK:
        assert rc == OK                       # (an entry that has nothing to do leaves the error text alone)
    else:
        assert (rc, text) == (want_rc, want_text)


WS_SMALL, WS_LARGE = 256, 1536


def test_augment_workspace_bytes_of_unsupported_sizes():
    lib = _lib.load()
    assert lib.dg_augment_workspace_bytes(0, 4, 4) == 0 and lib.dg_augment_workspace_bytes(1, 2, 4) == 0
    assert lib.dg_augment_workspace_bytes(65536, 4, 4) == 0 and lib.dg_augment_workspace_bytes(1, 4, 16385) == 0
    assert lib.dg_augment_workspace_bytes(2, 4, 4) == WS_SMALL and lib.dg_augment_workspace_bytes(3, 1024, 1024) == WS_LARGE
