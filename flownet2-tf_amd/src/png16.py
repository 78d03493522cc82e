"""A minimal 16-bit RGB PNG codec on zlib and struct alone: what KITTI's flow ground truth is stored in, and what an 8-bit
image library reduces to 8 bits.  The reader takes colour type 2 at bit depth 16, non-interlaced, with any of the five row
filters and any number of IDAT chunks, checks every CRC, and refuses everything else with a ValueError naming the file; the
writer uses filter 0.  Host code: a file format, nothing on the hot path."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_BPP = 6  # bytes per pixel: three 16-bit samples


def _chunks(data, name):
    """(type, payload) of every chunk, CRC checked."""
    if data[:8] != SIGNATURE:
        raise ValueError("%s: not a PNG file (bad signature)" % name)
    pos = 8
    while pos < len(data):
        if pos + 8 > len(data):
            raise ValueError("%s: truncated PNG file (chunk header)" % name)
        length, ctype = struct.unpack(">I4s", data[pos:pos + 8])
        end = pos + 8 + length + 4
        if end > len(data):
            raise ValueError("%s: truncated PNG file (chunk %s)" % (name, ctype.decode("latin-1")))
        payload = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[end - 4:end])
        if zlib.crc32(ctype + payload) & 0xFFFFFFFF != crc:
            raise ValueError("%s: CRC mismatch in PNG chunk %s" % (name, ctype.decode("latin-1")))
        yield ctype, payload
        pos = end
        if ctype == b"IEND":
            return
    raise ValueError("%s: truncated PNG file (no IEND chunk)" % name)


def _unfilter(raw, h, w, name):
    """The scanlines behind their filter bytes -> [h, 6 w] uint8.  None and Up are whole-row operations and Sub is a running
    sum per byte column; Average and Paeth depend on the reconstructed byte 6 to the left, so they walk the bytes of a
    row one by one (about a second for a KITTI frame whose every row uses them)."""
    stride = _BPP * w
    if len(raw) != h * (stride + 1):
        raise ValueError("%s: truncated PNG file (%d bytes of image data, %d expected)" % (name, len(raw), h * (stride + 1)))
    rows = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        if ft == 0:
            cur = line
        elif ft == 1:
            cur = np.cumsum(line.reshape(w, _BPP), axis=0, dtype=np.uint8).reshape(stride)  # wraps mod 256
        elif ft == 2:
            cur = line + prev  # uint8: wraps mod 256
        elif ft in (3, 4):
            src, up, res = line.tobytes(), prev.tobytes(), bytearray(stride)
            for i in range(stride):
                a = res[i - _BPP] if i >= _BPP else 0
                b = up[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[i - _BPP] if i >= _BPP else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                res[i] = (src[i] + pred) & 255
            cur = np.frombuffer(bytes(res), np.uint8)
        else:
            raise ValueError("%s: unknown PNG row filter %d in row %d" % (name, ft, y))
        out[y] = cur
        prev = out[y]
    return out


def read_rgb16(path):
    """A 16-bit RGB PNG -> [H, W, 3] uint16."""
    name = str(path)
    with open(path, "rb") as f:
        data = f.read()
    header, idat, ended = None, [], False
    for ctype, payload in _chunks(data, name):
        if ctype == b"IHDR":
            if len(payload) != 13:
                raise ValueError("%s: bad PNG header" % name)
            header = struct.unpack(">IIBBBBB", payload)
        elif header is None:
            raise ValueError("%s: PNG chunk %s in front of the header" % (name, ctype.decode("latin-1")))
        elif ctype == b"IDAT":
            idat.append(payload)
        elif ctype == b"IEND":
            ended = True
    if header is None or not ended:
        raise ValueError("%s: truncated PNG file (no header or no IEND chunk)" % name)
    w, h, depth, colour, compression, filt, interlace = header
    if depth != 16 or colour != 2:
        raise ValueError("%s: only 16-bit RGB PNG files are read (colour type 2, bit depth 16); this one has colour type %d, "
                         "bit depth %d" % (name, colour, depth))
    if interlace != 0:
        raise ValueError("%s: interlaced PNG files are not read" % name)
    if compression != 0 or filt != 0 or w < 1 or h < 1:
        raise ValueError("%s: bad PNG header" % name)
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError("%s: truncated or damaged PNG image data (%s)" % (name, e)) from None
    rows = _unfilter(raw, h, w, name)
    return rows.reshape(h, w, 3, 2).view(">u2").reshape(h, w, 3).astype(np.uint16)


def _chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload) & 0xFFFFFFFF)


def write_rgb16(path, image):
    """[H, W, 3] uint16 -> a 16-bit RGB PNG, every row with filter 0."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint16 or 0 in image.shape:
        raise ValueError("write_rgb16: image must be a non-empty (H, W, 3) uint16 array")
    h, w = image.shape[:2]
    rows = np.zeros((h, 1 + _BPP * w), np.uint8)
    rows[:, 1:] = image.astype(">u2").view(np.uint8).reshape(h, _BPP * w)
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
