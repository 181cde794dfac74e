"""A small PNG writer and reader on the standard library's zlib and struct: what nn.FrameRenderer's bytes are stored with (predict.py
--plots, train.py --plots), so that the pictures need neither matplotlib nor PIL.

write_png stores 8-bit RGB or grey, every scanline with filter type 0, in one IDAT chunk.  read_png reads those files and any other
non-interlaced 8-bit RGB or grey file (filter types 0 - 4) and checks every chunk's CRC."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(rgb, level: int = 1) -> bytes:
    """The file's bytes for uint8 [H, W, 3] (RGB) or uint8 [H, W] (grey)."""
    a = np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png takes uint8 [H, W, 3] or uint8 [H, W], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    lines = np.empty((h, 1 + w * (3 if a.ndim == 3 else 1)), np.uint8)
    lines[:, 0] = 0                                             # filter type 0 on every scanline
    lines[:, 1:] = a.reshape(h, -1)
    head = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", head) + _chunk(b"IDAT", zlib.compress(lines.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path: str, rgb, level: int = 1) -> None:
    """level: zlib's, 0 (stored) to 9.  Level 1 is the default: a two-panel 768 x 1152 frame is 6 MB of scanlines, and the encoder, not
    the device, bounds the rate of a run that plots every sample."""
    data = encode_png(rgb, level)
    with open(path, "wb") as f:
        f.write(data)


def chunks(data: bytes):
    """[(type, body)] of a PNG file's bytes; raises ValueError on a wrong signature, a truncated chunk or a CRC that does not verify."""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file")
    out, pos = [], 8
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("truncated PNG chunk")
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("truncated PNG chunk")
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"PNG chunk {kind!r}: CRC mismatch")
        out.append((kind, body))
        pos += 12 + n
        if kind == b"IEND":
            break
    return out


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def decode_png(data: bytes) -> np.ndarray:
    """uint8 [H, W, 3] or [H, W] from a PNG file's bytes (8 bits per sample, colour type 2 or 0, not interlaced)."""
    parts = chunks(data)
    if not parts or parts[0][0] != b"IHDR" or parts[-1][0] != b"IEND":
        raise ValueError("PNG without IHDR or IEND")
    w, h, depth, ctype, comp, flt, interlace = struct.unpack(">IIBBBBB", parts[0][1])
    if depth != 8 or ctype not in (0, 2) or comp != 0 or flt != 0 or interlace != 0:
        raise ValueError(f"read_png reads non-interlaced 8-bit RGB or grey only (depth {depth}, colour type {ctype}, interlace {interlace})")
    bpp = 3 if ctype == 2 else 1
    stride = w * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(body for kind, body in parts if kind == b"IDAT")), np.uint8)
    if raw.size != h * (stride + 1):
        raise ValueError("PNG image data has the wrong length")
    raw = raw.reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 1:                                           # Sub: a running sum per channel, modulo 256
            cur = np.cumsum(line.reshape(w, bpp), axis=0, dtype=np.uint8).reshape(-1)
        elif ft == 2:                                           # Up
            cur = line + prev
        elif ft in (3, 4):                                      # Average, Paeth: each byte needs its finished left neighbour
            cur, src, up = [0] * stride, line.tolist(), prev.tolist()
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                if ft == 3:
                    cur[i] = (src[i] + ((a + up[i]) >> 1)) & 255
                else:
                    cur[i] = (src[i] + _paeth(a, up[i], up[i - bpp] if i >= bpp else 0)) & 255
            cur = np.asarray(cur, np.uint8)
        else:
            raise ValueError(f"PNG filter type {ft}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3) if ctype == 2 else out.reshape(h, w)


def read_png(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        return decode_png(f.read())
