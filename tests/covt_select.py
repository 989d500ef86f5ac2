"""Reference feature selection (include/covt.h "Feature selection"): what the GPU passes of covt_select.hip are
held to, byte for byte.  Nothing here but numpy's nonzero, diff, cumsum, a concatenation and IEEE comparisons."""
import numpy as np

WINDOW, MIN_SIZE, KEEP_EMPTY = 0x1, 0x2, 0x4


def a16(x):
    return (x + 15) & ~15


def member_offsets(n):
    """Byte offsets of mask, sel, offsets and bytes inside a column's slice of n features."""
    sel = a16(n)
    offs = sel + a16(4 * n)
    return 0, sel, offs, offs + a16(4 * (n + 1))


def select_ref(wkb_offsets, wkb_bytes, mask):
    """(sel int32[k], offsets int32[k + 1], bytes uint8[offsets[k]]) of the features with a non-zero mask byte."""
    wkb_offsets = np.asarray(wkb_offsets, dtype=np.int64)
    wkb_bytes = np.asarray(wkb_bytes, dtype=np.uint8)
    sel = np.nonzero(np.asarray(mask))[0]
    lengths = np.diff(wkb_offsets)[sel]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    parts = [wkb_bytes[wkb_offsets[k]:wkb_offsets[k + 1]] for k in sel]
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return sel.astype(np.int32), offsets.astype(np.int32), data.astype(np.uint8)


def predicate_ref(xmin, ymin, xmax, ymax, area, length, pred):
    """mask uint8[n] of the definition; pred: anything with flags, window[4], min_area, min_length."""
    flags = int(pred.flags)
    w = [float(v) for v in pred.window]
    with np.errstate(invalid="ignore"):
        empty = np.isnan(xmin)
        W = np.ones(xmin.shape, bool)
        if flags & WINDOW:
            W = (xmin <= w[2]) & (xmax >= w[0]) & (ymin <= w[3]) & (ymax >= w[1])
            W &= w[0] <= w[2] and w[1] <= w[3]  # an inverted window selects nothing, whatever the box spans
        S = np.ones(xmin.shape, bool)
        if flags & MIN_SIZE:
            S = (area >= float(pred.min_area)) | (length >= float(pred.min_length)) | ((area == 0.0) & (length == 0.0))
    return np.where(empty, bool(flags & KEEP_EMPTY), W & S).astype(np.uint8)
