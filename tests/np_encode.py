"""numpy restatement of csrc/jpt_encode.h (jpt_encode): every step one float32 operation, a compare and select, or an integer / bit
operation, in the header's order -- plus the decoders of the three formats, the float64 formula of the RGB9E5 specification, and the
edge list the host and GPU tests share.  Texels are float32 [n, 4]; the encoders return what the library writes: uint16 [n, 4]
(RGBA16F; view as float16 to decode), uint32 [n] (RGB9E5) and uint8 [n, 4] (RGBE8)."""
import numpy as np

F = np.float32
RGBA16F, RGB9E5, RGBE8 = 1, 2, 3                                            # JPT_ENCODE_*
MEAN, DENOISED, DISPLAY, LIGHTMAP, REFLECTION, PROBE_SH = range(6)          # JPT_ENCODE_SOURCE_*
ALL_LEVELS = -1
TEXEL_BYTES = {RGBA16F: 8, RGB9E5: 4, RGBE8: 4}
HALF_MAX, RGB9E5_MAX = F(65504.0), F(65408.0)
RGBE8_MAX = np.array([0x7effffff], np.uint32).view(F)[0]                    # the largest float32 below 2^127
RGBE8_MIN = F(1e-32)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _float(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


def clamp(x, lo, hi):
    """encode_clamp: a NaN gives +0, then two selects"""
    x = np.asarray(x, F)
    z = np.where(x != x, F(0.0), x)
    t = np.where(z > lo, z, F(lo))
    return np.where(t < hi, t, F(hi)).astype(F)


def pow2(k):
    """encode_pow2: 2^k from its bits, k in -126 .. 127"""
    return _float(((np.asarray(k, np.int64) + 127) << 23).astype(np.uint32))


def source(src4, divisor=1.0, alpha_one=False):
    """encode_source: rgb / divisor when the divisor is not 1 (one float32 division), alpha as it is or 1"""
    v = np.array(src4, F).reshape(-1, 4)
    if F(divisor) != F(1.0):
        with np.errstate(all="ignore"):
            v[:, :3] = v[:, :3] / F(divisor)
    if alpha_one:
        v[:, 3] = F(1.0)
    return v


def half(x):
    """encode_half per element: uint16 bits"""
    c = clamp(x, -HALF_MAX, HALF_MAX)
    u = _bits(c)
    sign = (u >> 16) & 0x8000
    a = u & 0x7fffffff
    r = (a - np.uint32(0x38000000)).astype(np.uint32)                        # (wraps where the other branch is taken)
    normal = (r + 0xfff + ((r >> 13) & 1)) >> 13
    sub = _bits(_float(a) + F(0.5)) - np.uint32(0x3f000000)
    return (sign | np.where(a >= 0x38800000, normal, sub)).astype(np.uint16)


def rgba16f(v4):
    return half(np.asarray(v4, F).reshape(-1, 4))


def rgb9e5(v4):
    v = np.asarray(v4, F).reshape(-1, 4)
    c = clamp(v[:, :3], F(0.0), RGB9E5_MAX)
    m = np.where(c[:, 0] > c[:, 1], c[:, 0], c[:, 1])
    m = np.where(m > c[:, 2], m, c[:, 2])
    eb = (_bits(m) >> 23).astype(np.int64) - 127
    e = np.maximum(eb, -16) + 16
    carry = np.floor(m * pow2(24 - e) + F(0.5)) == F(512.0)
    e = e + carry
    scale = pow2(24 - e)
    q = np.floor(c * scale[:, None] + F(0.5)).astype(np.uint32)
    return q[:, 0] | (q[:, 1] << 9) | (q[:, 2] << 18) | (e.astype(np.uint32) << 27)


def rgbe8(v4):
    v = np.asarray(v4, F).reshape(-1, 4)
    c = clamp(v[:, :3], F(0.0), RGBE8_MAX)
    m = np.where(c[:, 0] > c[:, 1], c[:, 0], c[:, 1])
    m = np.where(m > c[:, 2], m, c[:, 2])
    live = m >= RGBE8_MIN
    e = (_bits(m) >> 23).astype(np.int64) - 126
    scale = pow2(np.where(live, 8 - e, 0))
    q = np.floor(c * scale[:, None]).astype(np.uint32)
    out = np.zeros((len(v), 4), np.uint8)
    out[:, :3] = np.where(live[:, None], q, 0)
    out[:, 3] = np.where(live, e + 128, 0)
    return out


def encode(src4, fmt, divisor=1.0, alpha_one=False):
    """what jpt_encode / jpt_debug_encode write for float32 [n, 4] texels"""
    v = source(src4, divisor, alpha_one)
    return {RGBA16F: rgba16f, RGB9E5: rgb9e5, RGBE8: rgbe8}[fmt](v)


def empty(fmt, n):
    """an output array of the dtype and shape the encoders return"""
    return np.zeros((n, 4), np.uint16) if fmt == RGBA16F else np.zeros(n, np.uint32) if fmt == RGB9E5 else np.zeros((n, 4), np.uint8)


# ---- decoders ----------------------------------------------------------------------------------------------------------------------------

def decode_rgba16f(h):
    """uint16 [n, 4] -> float32 [n, 4] (exact)"""
    return np.ascontiguousarray(h, np.uint16).view(np.float16).astype(F)


def unpack_rgb9e5(w):
    """uint32 [n] -> (mantissas int64 [n, 3], exponent field int64 [n])"""
    w = np.asarray(w, np.uint32).astype(np.int64)
    return np.stack([w & 511, (w >> 9) & 511, (w >> 18) & 511], axis=1), w >> 27


def decode_rgb9e5(w):
    """uint32 [n] -> float64 [n, 3]: mantissa * 2^(e - 24) (exact in binary64)"""
    q, e = unpack_rgb9e5(w)
    return q * np.ldexp(1.0, e - 24)[:, None]


def decode_rgbe8(b):
    """uint8 [n, 4] -> float64 [n, 3]: the lower edge of each mantissa's cell, m * 2^(e - 136), 0 where e == 0 (hdrio.decode_rgbe
    returns the cell's centre)"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    return np.where(b[:, 3:] == 0, 0.0, b[:, :3] * np.ldexp(1.0, b[:, 3:] - 136))


def rgb9e5_spec64(v4):
    """the formula of EXT_texture_shared_exponent's specification evaluated in float64 on the clamped channels:
    exp_shared = max(-16, floor(log2(max_c))) + 16, max_s = floor(max_c / 2^(exp_shared - 24) + 0.5), exp_shared + 1 if max_s == 512,
    c_s = floor(c / 2^(exp_shared - 24) + 0.5) -- (mantissas int64 [n, 3], exponent int64 [n])"""
    c = clamp(np.asarray(v4, F).reshape(-1, 4)[:, :3], F(0.0), RGB9E5_MAX).astype(np.float64)
    m = c.max(axis=1)
    _, ex = np.frexp(m)                                                       # m = f * 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
    e = np.where(m > 0.0, np.maximum(ex - 1, -16), -16) + 16
    e = e + (np.floor(m / np.ldexp(1.0, e - 24) + 0.5) == 512.0)
    return np.floor(c / np.ldexp(1.0, e - 24)[:, None] + 0.5).astype(np.int64), e.astype(np.int64)


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------

def _next(x, steps=1):
    return _float(np.array([int(_bits(np.array([x], F))[0]) + steps], np.uint32))[0]


def edge_values():
    """the edge list, one float32 per entry"""
    inf, nan = F(np.inf), F(np.nan)
    below_half = _next(F(0.5), -1)
    return np.array([
        0.0, -0.0, 1e-40, -1e-40, nan, inf, -inf, -1.0, -0.25, -70000.0,
        # half boundaries: 2^-25 (a tie to even that gives 0) and its successor, the subnormal / normal seam, 1 + 2^-11 (a tie), the
        # largest half, the last float that would round to it and the first that would not
        2.0 ** -25, _next(F(2.0 ** -25)), 2.0 ** -24, 1.5 * 2.0 ** -24, _next(F(1.5 * 2.0 ** -24)), _next(F(2.0 ** -14), -1), 2.0 ** -14,
        1.0 + 2.0 ** -11, _next(F(1.0 + 2.0 ** -11)), 1.0 + 3 * 2.0 ** -11, 65504.0, _next(F(65520.0), -1), 65520.0, -65520.0,
        # RGB9E5: the largest value and its successor, the mantissa carry to 512, 2^-16 and its neighbours, the largest float below 0.5
        # as a mantissa (x + 0.5f rounds), a channel 2^-20 of the maximum
        65408.0, _next(F(65408.0)), 0.9995, 511.5 / 512.0, _next(F(511.5 / 512.0), -1), 2.0 ** -16, _next(F(2.0 ** -16)), _next(F(2.0 ** -16), -1),
        below_half * 2.0 ** -9, below_half * 2.0 ** -24, 1000.0 * 2.0 ** -20, 2.0 ** -25 * 1.5,
        # RGBE8: 1e-32f and its predecessor, 2^127 and its predecessor, exact powers of two
        RGBE8_MIN, _next(RGBE8_MIN, -1), _next(RGBE8_MIN), 2.0 ** 127, RGBE8_MAX, 3.0e38, 1.0, 2.0, 0.5, 2.0 ** -100, 2.0 ** 100, 256.0, 255.99998,
        1000.0, 3.14159, 1e-8, 1e6], F)


def edge_texels():
    """the edge list as texels: each value alone in every channel beside small ones (it is the texel's maximum when it is positive),
    each value beside a larger one, and every value in all four channels"""
    v = edge_values()
    n = len(v)
    t = np.zeros((5 * n, 4), F)
    with np.errstate(all="ignore"):
        small = v * F(2.0 ** -20)
    for ch in range(4):
        t[ch * n:(ch + 1) * n, ch] = v
        t[ch * n:(ch + 1) * n, (ch + 1) % 4] = small
        t[ch * n:(ch + 1) * n, (ch + 2) % 4] = np.roll(v, 7)
    t[4 * n:] = v[:, None]
    return t


def texels(n, seed=5):
    """n texels: the edge list first (as much of it as fits, from a row the seed picks), then seeded values spanning 1e-8 .. 1e6 with
    a few negatives"""
    e = edge_texels()
    e = np.roll(e, -((seed * 17) % len(e)), axis=0)
    rng = np.random.default_rng(seed)
    r = (10.0 ** rng.uniform(-8.0, 6.0, (n, 4))).astype(F)
    r[rng.random((n, 4)) < 0.05] *= F(-1.0)
    k = min(n, len(e))
    r[:k] = e[:k]
    return r


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
