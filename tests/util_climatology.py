"""Checker of the climatology (nn.Climatology, dc_climatology_accumulate / dc_climatology_maps): the definition of include/deepcam_hip.h
implemented literally in numpy on int64, frame by frame, with no knowledge of the kernel's decomposition into pixels, quads and runs.

For frame b with g = group[b] >= 0, pixel p, class k = mask[b, p] and channel value v = fields[b, p, chan[c]]:  frames[g] += 1;  k in
{1, 2}: count[g, k - 1, p] += 1;  q = rint(ldexp(double(v), bits[c]));  v finite and |q| <= 2^40: sum[g, 0, p, c] += q, n[g, 0, p, c] += 1
and, for k in {1, 2}, the same into row k.  A frame with a negative group is not looked at.

The maps: frequency = float32(double(count) / double(frames)), 0 where frames == 0;  mean = float32(ldexp(double(sum), -bits) /
double(n)), NaN where n == 0;  share = float32(double(sum_k) / double(sum_all)), NaN where sum_all == 0;  contour = 1 where frequency_1 >=
t1, else 2 where frequency_2 >= t2, else 0."""
import numpy as np

LIMIT = float(2 ** 40)
KEYS = ("frames", "count", "sum", "n")
NAN32 = np.uint32(0x7FC00000).view(np.float32)


def empty(G, H, W, C):
    return {"frames": np.zeros(G, np.int64), "count": np.zeros((G, 2, H, W), np.int32), "sum": np.zeros((G, 3, H, W, C), np.int64),
            "n": np.zeros((G, 3, H, W, C), np.int32)}


def accumulate(state, mask, fields, chan, bits, group):
    """Adds the frames of one batch to `state` (in place; also returned).  mask: integers [B, H, W] of any width; fields: float32
    [B, H, W, ldc] or None; chan: the selected channels; bits: per selected channel; group: B ints."""
    mask = np.asarray(mask)
    chan = [int(c) for c in chan]
    C = len(chan)
    assert state["sum"].shape[-1] == C and len(bits) == C and len(group) == len(mask)
    for b, g in enumerate(int(v) for v in group):
        if g < 0:
            continue
        assert g < len(state["frames"])
        state["frames"][g] += 1
        m = mask[b].astype(np.int64)
        cls = [m == 1, m == 2]
        for k in range(2):
            state["count"][g, k] += cls[k]
        if C == 0:
            continue
        v = np.asarray(fields[b], np.float32)[:, :, chan]                                      # [H, W, C]
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.rint(np.ldexp(v.astype(np.float64), np.asarray(bits, np.int32)))           # exact scaling, one rint
            ok = np.isfinite(v) & (np.abs(q) <= LIMIT)
        q = np.where(ok, q, 0.0).astype(np.int64)
        for row, sel in ((0, np.ones_like(cls[0])), (1, cls[0]), (2, cls[1])):
            take = ok & sel[:, :, None]
            state["sum"][g, row] += np.where(take, q, 0)
            state["n"][g, row] += take
    return state


def reference(batches, G, H, W, chan, bits):
    """the state after the batches, each (mask, fields, group), on top of zeros"""
    state = empty(G, H, W, len(chan))
    for mask, fields, group in batches:
        accumulate(state, mask, fields, chan, bits, group)
    return state


def product(state, bits, prod):
    """float32 [G, H, W] of one product: ("frequency", k), ("mean", c, row) or ("share", c, k)"""
    frames, count, total, n = (state[k] for k in KEYS)
    G = len(frames)
    with np.errstate(divide="ignore", invalid="ignore"):
        if prod[0] == "frequency":
            f = frames.astype(np.float64)[:, None, None]
            quot = count[:, prod[1] - 1].astype(np.float64) / f
            out = np.where(np.broadcast_to(f, quot.shape) == 0, np.float32(0), quot.astype(np.float32))
        elif prod[0] == "mean":
            c, row = prod[1], prod[2]
            num, den = total[:, row, :, :, c], n[:, row, :, :, c]
            quot = np.ldexp(num.astype(np.float64), -int(bits[c])) / den.astype(np.float64)
            out = np.where(den == 0, NAN32, quot.astype(np.float32))
        elif prod[0] == "share":
            c, k = prod[1], prod[2]
            num, den = total[:, k, :, :, c], total[:, 0, :, :, c]
            quot = num.astype(np.float64) / den.astype(np.float64)
            out = np.where(den == 0, NAN32, quot.astype(np.float32))
        else:
            raise KeyError(prod)
    out = np.ascontiguousarray(out, np.float32)
    assert out.shape == (G,) + count.shape[2:]
    return out


def maps(state, bits, products, t1, t2):
    """(float32 [G, H, W, K], uint8 [G, H, W]): what dc_climatology_maps writes"""
    out = np.stack([product(state, bits, p) for p in products], axis=-1)
    f1, f2 = product(state, bits, ("frequency", 1)), product(state, bits, ("frequency", 2))
    contour = np.where(f1 >= np.float32(t1), 1, np.where(f2 >= np.float32(t2), 2, 0)).astype(np.uint8)
    return np.ascontiguousarray(out), contour


def same_bits(a, b) -> bool:
    """float32 arrays equal as bit patterns (NaN equals the same NaN, -0.0 does not equal +0.0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
