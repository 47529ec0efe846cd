"""A plain model of the reference's result order, vectorised, with a numpy and a torch backend from the same
code.  canonical_join(kR, idR, kS, idS, bits) returns the whole pair list of a join on `bits` radix bits:

  buckets ascending, the bucket of a key being key & (2^bits - 1);
  inside a bucket the probe side is R when histR >= histS, else S (rhjoin.c:86); a bucket with an empty side has no pairs;
  the probe tuples in input position order;
  each probe tuple's matches in descending build input position;
  every pair written as (row_idR, row_idS).

The order comes from input positions alone, never from row ids.  tests/test_canon_model.py holds the model to the oracle bit
for bit; on the device (torch backend) it then checks joins far beyond the oracle's reach, every pair and not a sample.
"""
import numpy as np


class _Numpy:
    def __init__(self):
        self.xp = np

    def i64(self, x):
        x = np.ascontiguousarray(x)
        return x.view(np.int64) if x.dtype == np.uint64 else x.astype(np.int64, copy=False)

    def arange(self, n, like):
        return np.arange(n, dtype=np.int64)

    def zeros(self, n, like):
        return np.zeros(n, dtype=np.int64)

    def bincount(self, x, n):
        return np.bincount(x, minlength=n)

    def argsort(self, x):
        return np.argsort(x, kind="stable")

    def searchsorted(self, a, v, right):
        return np.searchsorted(a, v, side="right" if right else "left").astype(np.int64)

    def repeat(self, x, counts, total):
        return np.repeat(x, counts)

    def cumsum(self, x):
        return np.cumsum(x)

    def cat(self, xs):
        return np.concatenate(xs)

    def flip(self, x):
        return x[::-1]

    def where(self, c, a, b):
        return np.where(c, a, b)

    def pairs(self, r, s):
        out = np.empty((len(r), 2), dtype=np.uint64)
        out[:, 0] = r.view(np.uint64)
        out[:, 1] = s.view(np.uint64)
        return out


class _Torch:
    def __init__(self, torch):
        self.xp = self.torch = torch

    def i64(self, x):
        return x.contiguous()

    def arange(self, n, like):
        return self.torch.arange(n, dtype=self.torch.int64, device=like.device)

    def zeros(self, n, like):
        return self.torch.zeros(n, dtype=self.torch.int64, device=like.device)

    def bincount(self, x, n):
        return self.torch.bincount(x, minlength=n)

    def argsort(self, x):
        return self.torch.sort(x, stable=True).indices

    def searchsorted(self, a, v, right):
        return self.torch.searchsorted(a, v, right=right)

    def repeat(self, x, counts, total):
        return self.torch.repeat_interleave(x, counts, output_size=total)

    def cumsum(self, x):
        return self.torch.cumsum(x, 0)

    def cat(self, xs):
        return self.torch.cat(xs)

    def flip(self, x):
        return self.torch.flip(x, (0,))

    def where(self, c, a, b):
        return self.torch.where(c, a, b)

    def pairs(self, r, s):
        return self.torch.stack([r, s], dim=1)


def _backend(x):
    if isinstance(x, np.ndarray):
        return _Numpy()
    import torch
    return _Torch(torch)


def canonical_join(kR, idR, kS, idS, bits):
    """Keys and row ids as four 1-D arrays: numpy (uint64 or int64) or torch int64 tensors on one device.  Returns an [M, 2]
    array of (row_idR, row_idS): uint64 for numpy, int64 for torch (the bytes of rhj_join_device's output)."""
    B = _backend(kR)
    kR, idR, kS, idS = B.i64(kR), B.i64(idR), B.i64(kS), B.i64(idS)
    nb = 1 << bits
    mask = nb - 1
    bR, bS = kR & mask, kS & mask
    hR, hS = B.bincount(bR, nb), B.bincount(bS, nb)
    sprobe = hR < hS                                       # S probes bucket b (R on a tie)
    pR, pS = ~sprobe[bR], sprobe[bS]                       # the probe tuples of either relation
    iR, iS = B.arange(len(kR), kR), B.arange(len(kS), kS)
    # probe tuples: R's then S's, each in position order; a stable sort on the bucket keeps that order inside a bucket (one
    # side probes a bucket)
    qR, qS = iR[pR], iS[pS]
    pkey = B.cat([kR[qR], kS[qS]])
    prid = B.cat([idR[qR], idS[qS]])
    pside = B.cat([B.zeros(len(qR), kR), B.zeros(len(qS), kS) + 1])
    o = B.argsort(B.cat([bR[qR], bS[qS]]))
    pkey, prid, pside = pkey[o], prid[o], pside[o]
    # build tuples: positions descending, then a stable sort on the key (equal keys share a bucket, so one side)
    uR, uS = B.flip(iR[~pR]), B.flip(iS[~pS])
    bkey = B.cat([kR[uR], kS[uS]])
    brid = B.cat([idR[uR], idS[uS]])
    o = B.argsort(bkey)
    bkey, brid = bkey[o], brid[o]
    lo = B.searchsorted(bkey, pkey, False)
    cnt = B.searchsorted(bkey, pkey, True) - lo
    total = int(cnt.sum())
    rep = B.repeat(B.arange(len(pkey), pkey), cnt, total)
    first = B.cumsum(cnt) - cnt
    bidx = lo[rep] + (B.arange(total, pkey) - first[rep])
    a, b, side = prid[rep], brid[bidx], pside[rep]
    return B.pairs(B.where(side == 0, a, b), B.where(side == 0, b, a))
