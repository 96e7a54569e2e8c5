"""Radiance RGBE (.hdr) panoramas for jpt_set_environment: load_hdr / save_hdr.

Only what an environment map needs: the `-Y H +X W` orientation (row 0 at the top, the +y pole of the map), flat scanlines and
new-style run-length scanlines.  Other orientations, old-style run-length scanlines and malformed files raise ValueError.  Decoding
is pinned to Ward's rule, (m + 0.5) * 2^(e - 136) per channel and 0 for e == 0, rounded once to float32; include/jpt_host.hpp
load_hdr gives the same floats."""
import re

import numpy as np

_RES = re.compile(rb"^-Y (\d+) \+X (\d+)$")


def _header(data: bytes):
    """(width, height, offset of the first scanline)"""
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError("not a Radiance file (no #?RADIANCE / #?RGBE signature)")
    pos = 0
    while True:
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError("truncated header")
        line = data[pos:end].rstrip(b"\r")
        pos = end + 1
        if not line:
            break
        if line.startswith(b"FORMAT=") and line != b"FORMAT=32-bit_rle_rgbe":
            raise ValueError("unsupported pixel format %r" % line.decode(errors="replace"))
    end = data.find(b"\n", pos)
    if end < 0:
        raise ValueError("no resolution line")
    m = _RES.match(data[pos:end].rstrip(b"\r"))
    if not m:
        raise ValueError("unsupported resolution line %r (only -Y H +X W)" % data[pos:end][:40].decode(errors="replace"))
    h, w = int(m.group(1)), int(m.group(2))
    if w <= 0 or h <= 0:
        raise ValueError("empty image")
    return w, h, end + 1


def _scanline(data: bytes, pos: int, w: int):
    """one scanline's RGBE bytes [w, 4] and the offset after it"""
    if 8 <= w <= 0x7FFF and pos + 4 <= len(data) and data[pos] == 2 and data[pos + 1] == 2 and (data[pos + 2] & 0x80) == 0:
        if (data[pos + 2] << 8 | data[pos + 3]) != w:
            raise ValueError("run-length scanline of the wrong width")
        pos += 4
        out = np.empty((4, w), dtype=np.uint8)
        for c in range(4):
            x = 0
            while x < w:
                if pos >= len(data):
                    raise ValueError("truncated run-length scanline")
                n = data[pos]
                pos += 1
                if n > 128:
                    n -= 128
                    if x + n > w or pos >= len(data):
                        raise ValueError("bad run in a scanline")
                    out[c, x:x + n] = data[pos]
                    pos += 1
                else:
                    if n == 0 or x + n > w or pos + n > len(data):
                        raise ValueError("bad literal in a scanline")
                    out[c, x:x + n] = np.frombuffer(data, dtype=np.uint8, count=n, offset=pos)
                    pos += n
                x += n
        return out.T, pos
    if pos + 4 * w > len(data):
        raise ValueError("truncated scanline")
    px = np.frombuffer(data, dtype=np.uint8, count=4 * w, offset=pos).reshape(w, 4)
    if ((px[:, 0] == 1) & (px[:, 1] == 1) & (px[:, 2] == 1)).any():   # (never a pixel: the largest mantissa is >= 128)
        raise ValueError("old-style run-length scanlines are not supported")
    return px, pos + 4 * w


def decode_rgbe(rgbe: np.ndarray) -> np.ndarray:
    """[..., 4] uint8 -> [..., 3] float32: (m + 0.5) * 2^(e - 136), 0 where e == 0"""
    e = rgbe[..., 3].astype(np.int64)
    scale = np.ldexp(1.0, e - 136)
    v = (rgbe[..., :3].astype(np.float64) + 0.5) * scale[..., None]
    return np.where(e[..., None] == 0, 0.0, v).astype(np.float32)


def load_hdr(path) -> np.ndarray:
    """A Radiance .hdr file -> float32 [height, width, 3], row 0 the top row of the file."""
    with open(path, "rb") as f:
        data = f.read()
    w, h, pos = _header(data)
    rows = []
    for _ in range(h):
        px, pos = _scanline(data, pos, w)
        rows.append(px)
    return decode_rgbe(np.stack(rows))


def encode_rgbe(rgb: np.ndarray) -> np.ndarray:
    """[..., 3] float -> [..., 4] uint8 (Ward's float2rgbe: the largest channel's exponent, mantissas truncated)"""
    rgb = np.asarray(rgb, dtype=np.float64)
    v = rgb.max(axis=-1)
    mant, e = np.frexp(v)
    with np.errstate(all="ignore"):
        scale = np.where(v > 1e-32, mant * 256.0 / v, 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = np.clip(np.floor(rgb * scale[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(v > 1e-32, e + 128, 0).astype(np.uint8)
    return out


def _rle_channel(b: np.ndarray) -> bytes:
    out = bytearray()
    i, n = 0, len(b)
    while i < n:
        j = i
        while j < n and j - i < 127 and b[j] == b[i]:
            j += 1
        if j - i >= 3:
            out += bytes((128 + j - i, int(b[i])))
            i = j
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and b[j] == b[j + 1] == b[j + 2]):
            j += 1
        out.append(j - i)
        out += bytes(b[i:j].tolist())
        i = j
    return bytes(out)


def save_hdr(path, rgb, rle: bool = True) -> None:
    """float [height, width, 3] (finite, >= 0) -> a Radiance .hdr file, -Y H +X W; `rle`: new-style run-length scanlines
    (for widths 8..32767), else flat ones."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("save_hdr takes a [height, width, 3] array")
    save_hdr_rgbe(path, encode_rgbe(rgb), rle)


def save_hdr_rgbe(path, rgbe, rle: bool = True) -> None:
    """already-encoded texels, uint8 [height, width, 4] (r, g, b mantissas and the exponent byte: encode_rgbe's, or a
    JPT_ENCODE_RGBE8 read-back reshaped to the image) -> a Radiance .hdr file as save_hdr writes it, with no conversion"""
    px = np.asarray(rgbe)
    if px.ndim != 3 or px.shape[2] != 4 or px.dtype != np.uint8:
        raise ValueError("save_hdr_rgbe takes a uint8 [height, width, 4] array")
    h, w = px.shape[:2]
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
    use_rle = rle and 8 <= w <= 0x7FFF
    for y in range(h):
        if use_rle:
            out += bytes((2, 2, w >> 8, w & 255))
            for c in range(4):
                out += _rle_channel(px[y, :, c])
        else:
            out += px[y].tobytes()
    with open(path, "wb") as f:
        f.write(bytes(out))
