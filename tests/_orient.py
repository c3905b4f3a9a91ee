"""What the tests of the oriented resample (include/jpeg_amd.h, "oriented resample") share, each stated once: the eight EXIF
orientations in numpy, the rectangle mapping restated independently of the library, and APP1 segments built byte by byte.
Importing this needs no GPU and no torch."""
import struct

import numpy as np

# o -> (T, fx, fy), the table of the header
BITS = {1: (0, 0, 0), 2: (0, 1, 0), 3: (0, 1, 1), 4: (0, 0, 1), 5: (1, 0, 0), 6: (1, 0, 1), 7: (1, 1, 1), 8: (1, 1, 0)}
TAG, SHORT, LONG, ASCII = 0x0112, 3, 4, 2


def orient(image, o):
    """The oriented image of a stored image [h, w, ...]: S[::-1] if fy, then [:, ::-1] if fx, then the transpose if T."""
    T, fx, fy = BITS[o]
    image = np.asarray(image)
    if fy:
        image = image[::-1]
    if fx:
        image = image[:, ::-1]
    if T:
        image = image.transpose((1, 0) + tuple(range(2, image.ndim)))
    return np.ascontiguousarray(image)


def oriented_size(o, w, h):
    return (h, w) if BITS[o][0] else (w, h)


def stored_rect(o, w, h, rect):
    """The header's mapping, in Python: an oriented rectangle (x, y, width, height) as the stored one."""
    T, fx, fy = BITS[o]
    x, y, rw, rh = rect
    if T:
        x, y, rw, rh = y, x, rh, rw
    return (w - x - rw if fx else x, h - y - rh if fy else y, rw, rh)


# ---- APP1 segments ---------------------------------------------------------------------------------------------------------

def entry(tag, type, count, value, big, value_bytes=None):
    """One 12-byte IFD entry; the value is written in the file's byte order from the start of the value field."""
    e = ">" if big else "<"
    if value_bytes is None:
        value_bytes = struct.pack(e + ("H" if type == SHORT else "I"), value).ljust(4, b"\0")
    return struct.pack(e + "HHI", tag, type, count) + value_bytes


def tiff(entries, big, ifd_offset=8, count=None):
    """A TIFF header, padding up to ifd_offset, IFD0 with `entries` (count: the entry count written, if it is to lie) and a
    zero link."""
    e = ">" if big else "<"
    head = (b"MM\0*" if big else b"II*\0") + struct.pack(e + "I", ifd_offset)
    return head + b"\0" * (ifd_offset - 8) + struct.pack(e + "H", len(entries) if count is None else count) + b"".join(entries) + b"\0" * 4


def app1(payload, length=None):
    """An APP1 segment around `payload` (length: the length field written, if it is to lie)."""
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2 if length is None else length) + payload


def exif_segment(value, big=False, type=SHORT, count=1, before=1, after=1):
    """A well-formed Exif segment whose IFD0 holds `before` other entries, the orientation, and `after` more."""
    other = [entry(0x0100 + i, SHORT, 1, 7, big) for i in range(before)] + [entry(TAG, type, count, value, big)]
    other += [entry(0x011a + i, LONG, 1, 72, big) for i in range(after)]
    return app1(b"Exif\0\0" + tiff(other, big))


XMP = app1(b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta/>")


def insert(data, segments):
    """The file `data` (uint8 array, SOI first) with `segments` (bytes) directly behind its SOI -> uint8 array."""
    raw = bytes(np.asarray(data, np.uint8))
    assert raw[:2] == b"\xff\xd8"
    return np.frombuffer(raw[:2] + segments + raw[2:], np.uint8).copy()


def insert_behind_sos(data, segments):
    """... directly behind the first scan's header and in front of its entropy-coded data: where no reader looks for it."""
    raw = bytes(np.asarray(data, np.uint8))
    sos = raw.index(b"\xff\xda")
    end = sos + 2 + struct.unpack(">H", raw[sos + 2:sos + 4])[0]
    return np.frombuffer(raw[:end] + segments + raw[end:], np.uint8).copy()
