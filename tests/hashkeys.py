"""The join kernels' hashes restated in numpy, and constructors of keys that collide in them.

Every join test elsewhere draws keys whose slot, tag and hash bits look random, so the code that exists only for
collisions (slots longer than a window, foreign tag hits between a tuple's matches, the tag clamp, equal-tag clusters of
the tiled tables, the exactness argument of k_join_exact) runs by chance or not at all.  The constructors here build such
keys on purpose.  Every constructor returns DISTINCT uint64 keys of one chosen bucket: key & (2^bits - 1) == b.

Sources (sigmod-2018_amd/csrc):
  mix64                 rhj_common.hip.h, mix64()
  fused, mix64 form     rhj_join_fused.hip.h, FjHashT<false>: slot = umulhi(h >> 32, hs), tag = min((h >> 16) & 0xffff, 0xfffd) + 1
  fused, H32 form       rhj_join_fused.hip.h, FjHashT<true>:  x = (u32)(key >> bits) ^ rotl32((u32)(key >> 32) >> bits, 16),
                        h = x * 0x9e3779b1, h ^= h >> 15; slot = umul24(h >> 16, hs) >> 16, tag = min(h & 0xffff, 0xfffd) + 1
  Tab32                 rhj_join_tiled.hip.h, t32_home / t32_tag: home = umulhi(h >> 32, slots), tag = (h >> 16) & 0xffff
  Tab64                 rhj_join_tiled.hip.h, Tab64: home = h >> (64 - lg), tag = low 32 bits of h
  exact                 rhj_join_exact.hip.h, XjIndex: y = ((key >> bits) * 0x9e3779b97f4a7c15) << bits,
                        slot = umulhi((y >> 32) & 0xffffff00, hs), ent = (u32)(y >> bits), ext = (y >> (bits + 32)) & 0xff;
                        hs_min = 1 << (24 - bits) (xj_body)
"""
import numpy as np

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
MIX_C1 = 0xBF58476D1CE4E5B9
MIX_C2 = 0x94D049BB133111EB
H32_C = 0x9E3779B1
XJ_C = 0x9E3779B97F4A7C15
TAG_CLAMP = 0xFFFD

_u64 = np.uint64


def _a(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def _mul(a, c):                      # a * c mod 2^64 (numpy wraps uint64 arrays silently)
    return _a(a) * _u64(c)


def _unxorshift(y, s, width=64):
    """Inverse of x ^ (x >> s) on `width`-bit words."""
    y = _a(y)
    x = y.copy()
    for _ in range(width // s + 1):
        x = y ^ (x >> _u64(s))
    return x


# ---- mix64 ----------------------------------------------------------------------------------------------------------
def mix64(x):
    x = _a(x)
    x = x ^ (x >> _u64(30)); x = _mul(x, MIX_C1)
    x = x ^ (x >> _u64(27)); x = _mul(x, MIX_C2)
    return x ^ (x >> _u64(31))


def unmix64(h):
    """mix64 is a bijection of 64-bit words: three unshifts and two modular inverses."""
    x = _unxorshift(h, 31)
    x = _mul(x, pow(MIX_C2, -1, 1 << 64))
    x = _unxorshift(x, 27)
    x = _mul(x, pow(MIX_C1, -1, 1 << 64))
    return _unxorshift(x, 30)


def mix_slot(h, hs):
    """FjHashT<false>::slot and t32_home: umulhi(h >> 32, hs)."""
    return ((_a(h) >> _u64(32)) * _u64(hs)) >> _u64(32)


def mix_raw_tag(h):
    return (_a(h) >> _u64(16)) & _u64(0xFFFF)


def clamp_tag(raw):
    """min(raw, 0xfffd) + 1: raw tags 0xfffd, 0xfffe and 0xffff share one tag."""
    return np.minimum(_a(raw), _u64(TAG_CLAMP)) + _u64(1)


def tab64_home(h, lg):
    return _a(h) >> _u64(64 - lg)


def tab64_tag(h):
    return _a(h) & _u64(M32)


# ---- FjHashT<true> (H32) ----------------------------------------------------------------------------------------------
def _rotl32(x, r):
    x = _a(x) & _u64(M32)
    return ((x << _u64(r)) | (x >> _u64(32 - r))) & _u64(M32)


def h32(key, bits):
    key = _a(key)
    x = ((key >> _u64(bits)) & _u64(M32)) ^ _rotl32((key >> _u64(32)) >> _u64(bits), 16)
    h = (x * _u64(H32_C)) & _u64(M32)
    return h ^ (h >> _u64(15))


def h32_slot(h, hs):
    """__umul24(h >> 16, hs) >> 16 (both factors below 2^24)."""
    return ((_a(h) >> _u64(16)) * _u64(hs)) >> _u64(16)


def h32_raw_tag(h):
    return _a(h) & _u64(0xFFFF)


def h32_x_of(h):
    """The x a 32-bit hash value comes from: undo the xorshift-15 and the multiply."""
    g = _unxorshift(_a(h) & _u64(M32), 15, 32) & _u64(M32)
    return (g * _u64(pow(H32_C, -1, 1 << 32))) & _u64(M32)


# ---- k_join_exact (XjIndex) -------------------------------------------------------------------------------------------
def xj_product(key, bits):
    """(key >> bits) * 0x9e3779b97f4a7c15 mod 2^(64 - bits): the W bits y holds, left-aligned."""
    return _mul(_a(key) >> _u64(bits), XJ_C) & _u64((1 << (64 - bits)) - 1)


def xj_y(key, bits):
    return _mul(_a(key) >> _u64(bits), XJ_C) << _u64(bits)


def xj_ent(key, bits):
    return (xj_y(key, bits) >> _u64(bits)) & _u64(M32)


def xj_ext(key, bits):
    return (xj_y(key, bits) >> _u64(bits + 32)) & _u64(0xFF)


def xj_slot(key, bits, hs):
    t = (xj_y(key, bits) >> _u64(32)) & _u64(0xFFFFFF00)
    return (t * _u64(hs)) >> _u64(32)


def xj_hs_min(bits):
    return 1 if bits >= 24 else 1 << (24 - bits)


def xj_key_of(product, bits, b):
    """The key of bucket b whose product is `product` (the multiplier is odd, so invertible mod 2^W)."""
    W = 64 - bits
    inv = pow(XJ_C, -1, 1 << W)
    q = (int(product) * inv) & ((1 << W) - 1)
    return (q << bits) | int(b)


# ---- constructors -----------------------------------------------------------------------------------------------------
def _bucket_ok(keys, b, bits):
    keys = _a(keys)
    return bool(np.all((keys & _u64((1 << bits) - 1)) == _u64(b))) and len(np.unique(keys)) == len(keys)


def h32_basis(bits, shared_low=False):
    """The kernel of the linear map key -> x (the H32 hash before its multiply), inside one bucket: for j in
    [32 + bits, 64), flip bit j with bit bits + ((j - 32 - bits + 16) mod 32).  With shared_low, only the vectors whose
    second bit is >= 32: they leave the low 32 bits of the key alone."""
    out = []
    for j in range(32 + bits, 64):
        k = bits + ((j - 32 - bits + 16) % 32)
        if shared_low and k < 32:
            continue
        out.append((1 << j) | (1 << k))
    return out


def h32_clones(b, bits, n, seed=0, shared_low=False, base=None):
    """n distinct keys of bucket b with one identical H32 value (so one slot and one tag at every hs)."""
    basis = h32_basis(bits, shared_low)
    if n > 1 << len(basis):
        raise ValueError("only %d clones exist" % (1 << len(basis)))
    rng = np.random.default_rng(seed)
    if base is None:
        base = ((int(rng.integers(0, 1 << 63)) << bits) | b) & M64
    combos = rng.choice(1 << len(basis), size=n, replace=False) if len(basis) < 40 else None
    keys = np.full(n, base, dtype=np.uint64)
    for i, v in enumerate(basis):
        sel = ((combos >> i) & 1).astype(bool)
        keys[sel] ^= _u64(v)
    return keys


def h32_keys(b, bits, hvals, per=1, seed=0):
    """Keys of bucket b with the given 32-bit H32 values (`per` distinct keys each): invert the xorshift and the multiply to
    get x, then pick the high word freely and derive the low word from it."""
    rng = np.random.default_rng(seed)
    out = []
    for hv in np.atleast_1d(hvals):
        x = int(h32_x_of(int(hv))[0])
        hus = rng.choice(1 << (32 - bits), size=per, replace=False)
        for hu in hus:
            hu = int(hu)
            L = x ^ int(_rotl32(hu, 16)[0])                    # key bits [bits, bits + 32)
            H = ((hu << bits) | (L >> (32 - bits))) & M32
            out.append((H << 32) | ((L << bits) & M32) | b)
    return np.array(out, dtype=np.uint64)


def mix64_keys(b, bits, n, top_lo, top_span, tag16, seed=0, low32=None, low_mask=0xFFFF):
    """Distinct keys of bucket b whose mix64 has its top 32 bits in [top_lo, top_lo + top_span) and (h >> 16) & 0xffff ==
    tag16 (or, with low32, its low 32 bits equal low32): the inverse of mix64 applied to chosen hashes, kept when the key
    falls in the bucket (one in 2^bits)."""
    rng = np.random.default_rng(seed)
    keys = np.zeros(0, dtype=np.uint64)
    for _ in range(32):                                   # (a narrow hash range may hold fewer than n keys of the bucket)
        if len(keys) >= n:
            break
        m = max(1 << 16, (n << bits) * 2)
        top = _u64(top_lo) + rng.integers(0, top_span, size=m, dtype=np.uint64)
        if low32 is None:
            low = (_u64(tag16) << _u64(16)) | (rng.integers(0, 1 << 16, size=m, dtype=np.uint64) & _u64(low_mask))
        else:
            low = np.full(m, low32, dtype=np.uint64)
        k = unmix64((top << _u64(32)) | low)
        k = k[(k & _u64((1 << bits) - 1)) == _u64(b)]
        keys = np.unique(np.concatenate([keys, k]))
    return rng.permutation(keys)[:n]


def mix64_slot_range(s, hs):
    """The top-32-bit values x with umulhi(x, hs) == s: [ceil(s 2^32 / hs), ceil((s + 1) 2^32 / hs))."""
    lo = -(-(s << 32) // hs)
    hi = -(-((s + 1) << 32) // hs)
    return lo, hi - lo


def mix64_lowword_pairs(b, bits, hs, count, seed=0):
    """Pairs of keys of bucket b that share their low 32 bits and collide in fused slot (at hs) and clamped tag: a
    birthday search over 2^24 high words of one low word.  Returns an array [count, 2]."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        low = (int(rng.integers(0, 1 << 32)) & ~((1 << bits) - 1)) | b
        hi = np.arange(1 << 24, dtype=np.uint64) | (_u64(int(rng.integers(0, 256))) << _u64(24))
        k = (hi << _u64(32)) | _u64(low)
        h = mix64(k)
        code = (mix_slot(h, hs) << _u64(16)) | clamp_tag(mix_raw_tag(h))
        o = np.argsort(code, kind="stable")
        c = code[o]
        d = np.nonzero(c[1:] == c[:-1])[0]
        for i in rng.permutation(d)[:count - len(out)]:
            out.append((k[o[i]], k[o[i + 1]]))
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


def exact_colliders(key, bits):
    """(a, b) for one key of bucket key & mask: a = the key whose product differs from the key's only in bit 40, the
    lowest bit the index does not store (equal ent and ext; the neighbouring slot when hs == hs_min); b = the key whose
    product differs only in bit 39, inside ext (equal ent; same slot when hs == hs_min and the key's bit 39 is 0)."""
    key = int(key)
    b = key & ((1 << bits) - 1)
    p = int(xj_product(key, bits)[0])
    return xj_key_of(p ^ (1 << 40), bits, b), xj_key_of(p ^ (1 << 39), bits, b)


def exact_seed_keys(b, bits, n, seed=0):
    """Keys of bucket b whose product has bits 39 and 40 clear: their kind (b) collider shares their slot at hs_min and their
    kind (a) collider is the next slot up."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = int(rng.integers(0, 1 << 62)) & ((1 << (64 - bits)) - 1) & ~(3 << 39)
        out.append(xj_key_of(p, bits, b))
    return np.array(out, dtype=np.uint64)


def keys_with_hash(b, bits, targets, hash="h32", per=1, hs=None, seed=0):
    """Keys of bucket b with chosen hashes.  hash="h32": targets are 32-bit H32 values.  hash="mix64": targets are
    (slot, raw tag16) pairs of the fused / Tab32 form at hs slots.  hash="tab64": targets are low 32-bit words (the Tab64
    tag) under one shared top 16 bits."""
    out = []
    for i, t in enumerate(targets):
        if hash == "h32":
            out.append(h32_keys(b, bits, [t], per, seed + i))
        elif hash == "mix64":
            lo, span = mix64_slot_range(int(t[0]), hs)
            out.append(mix64_keys(b, bits, per, lo, span, int(t[1]), seed + i))
        elif hash == "tab64":
            out.append(mix64_keys(b, bits, per, 0x5A580000, 1 << 18, 0, seed + i, low32=int(t)))
        else:
            raise ValueError(hash)
    return np.concatenate(out)


EXTREME_KEYS = np.array([0, 1, (1 << 63) - 1, 1 << 63, M64], dtype=np.uint64)
