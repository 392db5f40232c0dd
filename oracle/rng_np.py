"""ORACLE — test infrastructure only; never the product path.

Host model of csrc/rng.hip: the counter-based Philox-4x32-10 stream behind ops.DeviceRNG, word for word.  Written from the
Philox definition (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the known-answer vectors of Random123
pin it in tests/test_rng_model_host.py) and from reading rng.hip; it is never fitted to GPU output.  NumPy only, vectorised.

Counter layout (rng.hip draw()): the 128-bit counter of index i of a draw that starts at `offset` is
{lo32(c), hi32(c), 0x5eed5eed, 0} with c = offset + i (mod 2^64), the key is (lo32(seed), hi32(seed)).  One counter gives four
32-bit words x, y, z, w; output element j of the flat draws uses word j % 4 of counter j // 4.

Integer-valued results (randint, uniform, bernoulli, feature_mask, patch_mask) are the kernel's bit for bit: the fp32 operations
involved are single IEEE operations evaluated here in np.float32.  randn / gumbel are returned in float64 from the kernel's exact
fp32 uniforms (and the exact fp32 product 2 pi u), so that the device's logf / sqrtf / sincosf can be judged against them.

Every entry point returns its values followed by the half-open range (lo, hi) of the counter values c that it read.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_S32 = np.uint64(32)
TAG = 0x5EED5EED                      # counter word 2 of every draw of rng.hip
TWO_PI_F32 = np.float32(6.283185307179586)
_F = np.float32


def philox4x32_10(ctr4, key2):
    """ctr4: four uint64 arrays (or scalars) holding 32-bit words, key2: two 32-bit ints -> four uint64 arrays of 32-bit words."""
    x, y, z, w = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & M32 for c in ctr4)
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * x, _M1 * z                                   # 32 x 32 -> 64 bits, no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & M32, p1 >> _S32, p1 & M32
        x, y, z, w = hi1 ^ y ^ np.uint64(k0), lo1, hi0 ^ w ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return x, y, z, w


def draw(seed, offset, idx):
    """The quad of counter index idx (array) of a draw at `offset`: uint64 [len(idx), 4] of 32-bit words in the order x, y, z, w."""
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    with np.errstate(over="ignore"):
        c = idx + np.uint64(offset)                                  # mod 2^64, as the kernel's uint64_t sum
    zero = np.zeros_like(c)
    return np.stack(philox4x32_10((c & M32, c >> _S32, zero + np.uint64(TAG), zero), (seed & 0xFFFFFFFF, seed >> 32)), axis=1)


def _quads(n):
    return (int(n) + 3) // 4


def words(n, seed, offset):
    """The first n words of the flat stream at `offset` (uint64 [n]) and the counter range read."""
    q = _quads(n)
    return draw(seed, offset, np.arange(q, dtype=np.uint64)).reshape(-1)[:n], (int(offset), int(offset) + q)


# ---- the uniform maps, in fp32 with the kernel's operations --------------------------------------------------------------------
def u01(v):
    """rng.hip u01: ((float)(v >> 8) + 0.5f) * 2^-24 — in (0, 1]: the top word's sum rounds to 2^24, so u01(0xFFFFFFFF) == 1.0f."""
    v = np.asarray(v, dtype=np.uint64)
    return ((v >> np.uint64(8)).astype(_F) + _F(0.5)) * _F(1.0 / 16777216.0)


def u01_open(v):
    """rng.hip u01_open: ((float)(v >> 9) + 0.5f) * 2^-23 — in (0, 1), the top value is 1 - 2^-24."""
    v = np.asarray(v, dtype=np.uint64)
    return ((v >> np.uint64(9)).astype(_F) + _F(0.5)) * _F(1.0 / 8388608.0)


def u_half_open(v):
    """The [0, 1) map of uniform_kernel / bernoulli_kernel: (float)(v >> 8) * 2^-24 (exact)."""
    v = np.asarray(v, dtype=np.uint64)
    return (v >> np.uint64(8)).astype(_F) * _F(1.0 / 16777216.0)


# ---- one function per entry point ---------------------------------------------------------------------------------------
def _onehot(k, span):
    oh = np.zeros((k.size, span), np.float32)
    oh[np.arange(k.size), k] = 1.0
    return oh


def randint(n, lo, hi, seed, offset, exclude=None):
    """pcg_randint: (out int64 [n], one-hot float32 [n, hi - lo] or None, counter range).  The one-hot rows are those the fused
    launches write next to the targets; they exist on the exclude path only (as in randint_quad)."""
    span = int(hi) - int(lo)
    v, rng = words(n, seed, offset)
    k = (v * np.uint64(span)) >> _S32                                # v < 2^32, span < 2^31: no overflow
    if exclude is None:
        return k.astype(np.int64) + int(lo), None, rng
    ex = np.asarray(exclude, dtype=np.int64) - int(lo)
    k = k.astype(np.int64)
    kk = np.where(k == ex, (k + 1) % span, k)
    return kk + int(lo), _onehot(kk, span), rng


def uniform(n, seed, offset):
    v, rng = words(n, seed, offset)
    return u_half_open(v), rng


def bernoulli(n, keep, seed, offset):
    v, rng = words(n, seed, offset)
    return (u_half_open(v) < _F(keep)).astype(np.float32), rng


def feature_mask(B, D, zero_cols, seed, offset):
    n = int(B) * int(D)
    v, rng = words(n, seed, offset)
    on = (v >> np.uint64(31)) != 0
    if zero_cols is not None and len(zero_cols):
        on &= ~np.isin(np.arange(n) % int(D), np.asarray(zero_cols, dtype=np.int64))
    return on.astype(np.float32).reshape(B, D), rng


def patch_bits(B, total, nsel, seed, offset):
    """patch_mask_kernel's selection: per sample b a partial Fisher-Yates over `total` <= 64 patches, min(nsel, total) steps; step s
    uses word s % 4 of counter b * 16 + s // 4 (the first quad is drawn even when nothing is selected).  -> (taken bits as
    uint64 [B], counter range)."""
    B, total = int(B), int(total)
    steps = max(0, min(int(nsel), total))
    nq = max(1, _quads(steps))
    idx = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(16) + np.arange(nq, dtype=np.uint64)[None, :]).reshape(-1)
    w = draw(seed, offset, idx).reshape(B, nq * 4)
    taken = np.zeros((B, total), bool)
    rows = np.arange(B)
    for s in range(steps):
        k = ((w[:, s] * np.uint64(total - s)) >> _S32).astype(np.int64)      # uniform in [0, remaining)
        free = ~taken
        pidx = np.argmax(free & (np.cumsum(free, axis=1) == (k + 1)[:, None]), axis=1)    # the k-th patch not yet taken
        taken[rows, pidx] = True
    bits = (taken.astype(np.uint64) << np.arange(total, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return bits, (int(offset), int(offset) + (B - 1) * 16 + nq)


def patch_mask(B, H, W, ps, nsel, seed, offset):
    """pcg_patch_mask: float32 [B, 1, H, W]; pixel (h, w) belongs to patch (h // ps, w // ps), remainder pixels stay 0."""
    nph, npw = int(H) // int(ps), int(W) // int(ps)
    bits, rng = patch_bits(B, nph * npw, nsel, seed, offset)
    ph, pw = np.arange(H) // ps, np.arange(W) // ps
    inside = (ph < nph)[:, None] & (pw < npw)[None, :]
    p = np.where(inside, ph[:, None] * npw + pw[None, :], 0).astype(np.uint64)
    on = ((bits[:, None, None] >> p[None]) & np.uint64(1)).astype(bool) & inside[None]
    return on.astype(np.float32).reshape(B, 1, H, W), rng


def _randn(n, mean, std, seed, offset, dt):
    q = _quads(n)
    r = draw(seed, offset, np.arange(q, dtype=np.uint64))
    out = np.empty((q, 4), dt)
    for a, b, c in ((0, 1, 0), (2, 3, 2)):                           # (x, y) -> elements 0, 1; (z, w) -> elements 2, 3
        rad = np.sqrt(dt(-2.0) * np.log(u01(r[:, a]).astype(dt)))
        th = (TWO_PI_F32 * u01(r[:, b])).astype(dt)                 # one IEEE fp32 multiply: the kernel's argument
        out[:, c], out[:, c + 1] = rad * np.cos(th), rad * np.sin(th)
    v = out.reshape(-1)[:n]
    return v * dt(_F(std)) + dt(_F(mean)), (int(offset), int(offset) + q)


def randn_f64(n, mean, std, seed, offset):
    """pcg_randn in float64 from the kernel's fp32 uniforms and fp32 angle; mean / std are rounded to fp32 as the ABI does."""
    return _randn(n, mean, std, seed, offset, np.float64)


def randn_f32(n, mean, std, seed, offset):
    """The same chain in np.float32 (the CPU yardstick of the GPU tests; v * std + mean is two roundings here, one on the device)."""
    return _randn(n, mean, std, seed, offset, np.float32)


def _gumbel(n, seed, offset, dt):
    v, rng = words(n, seed, offset)
    return -np.log(-np.log(u01_open(v).astype(dt))), rng


def gumbel_f64(n, seed, offset):
    return _gumbel(n, seed, offset, np.float64)


def gumbel_f32(n, seed, offset):
    return _gumbel(n, seed, offset, np.float32)


def house_draws_span(B, D, T):
    return _quads(B) + _quads(B * D) + _quads(B * T)


def house_draws(y, num_classes, D, T, zero_cols, seed, offset):
    """pcg_house_draws / pcg_house_draws_counter: the three sub-draws at consecutive offsets, in the order target (randint with
    exclude = y), feature mask, Gumbel noise.  -> (dict of target, onehot_t, onehot_y, mask, noise (float64), counter range)."""
    y = np.asarray(y, dtype=np.int64)
    B = y.size
    off_t = int(offset)
    off_m = off_t + _quads(B)
    off_n = off_m + _quads(B * D)
    t, oh_t, r_t = randint(B, 0, num_classes, seed, off_t, exclude=y)
    m, r_m = feature_mask(B, D, zero_cols, seed, off_m)
    g, r_n = gumbel_f64(B * T, seed, off_n)
    assert r_t[1] == r_m[0] and r_m[1] == r_n[0]
    out = {"target": t, "onehot_t": oh_t, "onehot_y": _onehot(y, num_classes), "mask": m, "noise": g.reshape(B, T)}
    return out, (off_t, r_n[1])


def gather_batch(X, Y, perm, cursor, B):
    """The gather of house_batch_draws_kernel: rows perm[cursor .. cursor + B) (index and row clamped as the kernel clamps them)
    -> (x [B, D], y [B], source rows [B])."""
    perm = np.asarray(perm, dtype=np.int64)
    p = np.minimum(int(cursor) + np.arange(B), perm.size - 1)
    rows = np.clip(perm[p], 0, np.asarray(X).shape[0] - 1)
    return np.asarray(X)[rows], np.asarray(Y, dtype=np.int64)[rows], rows


def house_batch_draws(X, Y, perm, cursor, B, num_classes, T, zero_cols, seed, offset):
    """pcg_house_batch_draws_counter: gather_batch, then house_draws on the gathered y."""
    x, y, rows = gather_batch(X, Y, perm, cursor, B)
    out, rng = house_draws(y, num_classes, np.asarray(X).shape[1], T, zero_cols, seed, offset)
    out.update(x=x, y=y, src=rows)
    return out, rng
