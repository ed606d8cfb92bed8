"""CPU truth for the optimizer-tail and MemVLA kernel tests (numpy, no device): Philox4x32-10 and the dropout mask drawn from it
exactly as dexbotic_amd/csrc/memvla.hip states it, and a float64 per-element AdamW after the header comment of
dexbotic_amd/csrc/optim.hip."""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised: counter = 4 uint32 arrays (or scalars), key = 2 -> 4 uint32 arrays"""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LO for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def dropout_uniforms(n, seed, offset):
    """u[i] of the n mask elements as float32: thread t draws elements 4t .. 4t+3 from counter (t_lo, t_hi, off_lo, off_hi) and key
    (seed_lo, seed_hi); u = float32(bits >> 8) * 2^-24 (24 bits: exact, < 1)"""
    quads = (n + 3) // 4
    t = np.arange(quads, dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    zero = np.zeros(quads, dtype=np.uint64)
    bits = philox4x32_10((t & _LO, t >> _S32, zero + np.uint64(offset & 0xFFFFFFFF), zero + np.uint64(offset >> 32)),
                         (seed & 0xFFFFFFFF, seed >> 32))
    bits = np.stack(bits, axis=1).reshape(-1)[:n]
    return (bits >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_keep(n, p, seed, offset, u=None):
    """bool [n]: element i survives iff u[i] >= float32(p)"""
    u = dropout_uniforms(n, seed, offset) if u is None else u
    return u >= np.float32(p)


def keep_scale(p):
    """1 / (1 - p) as the kernel's host code computes it, in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def f32(x):
    """a hyper-parameter as the C ABI hands it to the kernel (a float field), widened back to float64"""
    return float(np.float32(x))


def adamw_ref(p, g, m, v, chunks, lrs, wds, beta1, beta2, eps, step, clip=1.0):
    """one float64 AdamW step per element over ``chunks`` = [(start, mstart, length, group), ...]: p / g indexed from start, the
    moments from mstart (mstart == start: unpacked).  p, g, m, v: float64 arrays holding the kernel's fp32 (bf16-rounded) inputs;
    the scalars are rounded to fp32 first, as the kernel receives them, the bias corrections 1 - beta**t are formed in double.
      g *= clip; p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
    Returns new (p, m, v); elements outside the chunks are copied unchanged."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float64
    p, m, v = p.copy(), m.copy(), v.copy()
    bc1, bc2 = f32(1.0 - beta1 ** step), f32(1.0 - beta2 ** step)
    b1, b2, eps, clip = f32(beta1), f32(beta2), f32(eps), f32(clip)
    for start, mstart, length, grp in chunks:
        lr, wd = f32(lrs[grp]), f32(wds[grp])
        sp, sm = slice(start, start + length), slice(mstart, mstart + length)
        gc = g[sp] * clip
        pn = p[sp] * (1.0 - lr * wd)
        mn = b1 * m[sm] + (1.0 - b1) * gc
        vn = b2 * v[sm] + (1.0 - b2) * gc * gc
        p[sp] = pn - (lr / bc1) * mn / (np.sqrt(vn) / np.sqrt(bc2) + eps)
        m[sm], v[sm] = mn, vn
    return p, m, v
