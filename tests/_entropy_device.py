"""What the CPU and the GPU tests of the device entropy decoder share, each stated once: the files (reference fixtures, files
written here from constructed planes, seeded damage of some of them), the planner's expected verdict for each, and the host
decoder's answer that everything is compared with.  Importing this needs no GPU and no torch."""
import ctypes as C
import functools

import numpy as np

import _files as F
import _golden as G
from _calls import c_layout, plane_units
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, _lib.EINVAL, -5

LAYOUTS = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)],
           "411": [(4, 1), (1, 1), (1, 1)], "four": [(1, 1)] * 4}


# ---- the calls ----------------------------------------------------------------------------------------------------------------

def plan(data):
    """jpeg_amd_jpeg_plan_intervals -> (status, nscans, nintervals)."""
    info, nscans, nintervals = _lib.FrameInfo(), C.c_int32(-1), C.c_int64(-1)
    st = _lib.lib().jpeg_amd_jpeg_plan_intervals(data.ctypes.data, data.size, C.byref(info), C.byref(nscans), C.byref(nintervals))
    return st, nscans.value, nintervals.value


def _decode(call, data, fill=77):
    info = _lib.FrameInfo()
    if _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) != 0:
        return EINVAL, None, None, None
    planes = [np.full((info.units_y[c], info.units_x[c], 64), fill, np.int16) for c in range(info.ncomponents)]
    quanta = np.zeros((4, 64), np.uint16)
    st = call(data.ctypes.data, data.size, _lib.ptr_array([p.ctypes.data for p in planes]), quanta.ctypes.data, None)
    return st, info, planes, quanta


def host_decode(data):
    """jpeg_amd_jpeg_decode_spectral -> (status, info, planes, quanta); the planes started out as 77 everywhere."""
    return _decode(_lib.lib().jpeg_amd_jpeg_decode_spectral, data)


def intervals_host(data):
    """jpeg_amd_jpeg_decode_intervals_host, the planes starting out as -23131 everywhere."""
    return _decode(_lib.lib().jpeg_amd_jpeg_decode_intervals_host, data, fill=-23131)


# ---- constructed planes -------------------------------------------------------------------------------------------------------

def crafted_planes(units, seed, precision=8):
    """Planes whose blocks cycle through what the decoder has a path for: photograph-like blocks (F.sparse_planes); all-zero
    blocks; a single coefficient at index 20 (two ZRLs in front of the EOB: the encoder writes every complete run of 16
    zeros); coefficients at 17 and 63 only (runs of 16 and more, no EOB); all 63 AC coefficients set (no EOB); dense
    blocks of 10-bit magnitudes (code + magnitude longer than 10 bits, and enough FF bytes for stuffing); DC values that
    alternate between the ends of the range (DC size 11 at 8 bits)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    top = 1000 if precision == 8 else 16000
    planes = F.sparse_planes(units, seed)
    for p in planes:
        flat = p.reshape(-1, 64)
        kind = (np.arange(flat.shape[0]) + seed) % 8
        flat[kind == 0] = 0
        flat[kind == 1, 1:] = 0
        flat[kind == 1, 20] = 5
        flat[kind == 2, 1:] = 0
        flat[kind == 2, 17] = -3
        flat[kind == 2, 63] = 2
        n3 = int((kind == 3).sum())
        v = rng.integers(1, 40, (n3, 63)) * rng.choice([-1, 1], (n3, 63))
        flat[kind == 3, 1:] = v
        n4 = int((kind == 4).sum())
        flat[kind == 4, 1:] = rng.integers(512, 1024, (n4, 63)) * rng.choice([-1, 1], (n4, 63))
        flat[kind == 5, 0] = top * np.where(np.arange(int((kind == 5).sum())) % 2 == 0, 1, -1)
        flat[kind == 6, 0] = -top
    return planes


def constructed(layout, size, seed, restart=0, kind="sequential", precision=8):
    L = c_layout(size[0], size[1], LAYOUTS[layout], precision=precision, qi=list(range(len(LAYOUTS[layout]))))
    planes = crafted_planes(plane_units(L), seed, precision)
    return F.write_file(L, planes, F.tables(L.nplanes, seed), kind, restart), planes


# name -> (layout, (w, h), restart interval in MCUs, kind, precision)
CONSTRUCTED = {
    "grey-17x17-ri1": ("grey", (17, 17), 1, "sequential", 8),              # 3 x 3 MCUs: 9 intervals, RSTn wraps
    "grey-35x19-ri2": ("grey", (35, 19), 2, "sequential", 8),
    "grey-65-intervals": ("grey", (8 * 65, 8), 1, "sequential", 8),        # one past a wave
    "grey-257-intervals": ("grey", (8 * 257, 8), 1, "sequential", 8),      # one past four waves and past 256
    "444-17x17-nodri": ("444", (17, 17), 0, "sequential", 8),
    "444-35x19-ri5": ("444", (35, 19), 5, "sequential", 8),
    "420-35x19-ri1": ("420", (35, 19), 1, "sequential", 8),
    "420-64x48-row": ("420", (64, 48), 4, "sequential", 8),                # one MCU row
    "420-64x48-row+1": ("420", (64, 48), 5, "sequential", 8),
    "420-64x48-ri1": ("420", (64, 48), 1, "sequential", 8),                # 12 intervals
    "422-35x19-ri2": ("422", (35, 19), 2, "sequential", 8),
    "411-35x19-ri1": ("411", (35, 19), 1, "sequential", 8),
    "411-70x30-row": ("411", (70, 30), 3, "sequential", 8),
    "420-35x19-scans-ri2": ("420", (35, 19), 2, "scans", 8),               # a scan per component
    "444-17x17-scans-nodri": ("444", (17, 17), 0, "scans", 8),
    "four-12bit-35x19-ri2": ("four", (35, 19), 2, "scans", 12),
    "four-12bit-17x17-ri2": ("four", (17, 17), 2, "sequential", 12),
}


@functools.lru_cache(maxsize=None)
def constructed_file(name):
    layout, size, restart, kind, precision = CONSTRUCTED[name]
    seed = sorted(CONSTRUCTED).index(name) + 100
    return constructed(layout, size, seed, restart, kind, precision)


def fixture_files():
    """Every fixture of tests/golden/decode with its manifest entry."""
    return [(e["name"], np.fromfile(G.path(e["file"]), np.uint8), e) for e in G.decode_entries()]


# ---- what a file is made of ---------------------------------------------------------------------------------------------------

def scan_ranges(data):
    """[(begin, end)] of the entropy-coded segments of a file, by a marker walk."""
    b = bytes(data)
    out, pos = [], 2
    while pos + 3 < len(b):
        assert b[pos] == 0xFF
        m = b[pos + 1]
        if m == 0xD9:
            break
        seglen = (b[pos + 2] << 8) | b[pos + 3]
        pos += 2 + seglen
        if m == 0xDA:
            e = pos
            while e + 1 < len(b) and not (b[e] == 0xFF and b[e + 1] != 0 and not 0xD0 <= b[e + 1] <= 0xD7):
                e += 1
            if e + 1 >= len(b):
                e = len(b)
            out.append((pos, e))
            pos = e
    return out


def restart_markers(data, rng_):
    """Offsets of the RSTn markers inside [begin, end)."""
    b = bytes(data[rng_[0]:rng_[1]])
    return [rng_[0] + i for i in range(len(b) - 1) if b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7]


def dht_lengths(data):
    """The longest code length each DHT table of the file defines."""
    b, out, pos = bytes(data), [], 2
    while pos + 3 < len(b) and b[pos] == 0xFF and b[pos + 1] != 0xDA:
        seglen = (b[pos + 2] << 8) | b[pos + 3]
        if b[pos + 1] == 0xC4:
            i = pos + 4
            while i < pos + 2 + seglen:
                counts = b[i + 1:i + 17]
                out.append(max(l + 1 for l in range(16) if counts[l]))
                i += 17 + sum(counts)
        pos += 2 + seglen
    return out


# ---- seeded damage, the markers left in place ---------------------------------------------------------------------------------

def _plain(data, i):
    """Byte i may be changed to v without making or breaking a marker: neither it nor its neighbours are FF."""
    return data[i] != 0xFF and data[i - 1] != 0xFF and data[i + 1] != 0xFF


def damaged(name, data):
    """-> [(case name, bytes, the planner's verdict)]: seeded damage of one file with restart intervals."""
    rng = np.random.Generator(np.random.PCG64(sum(name.encode())))
    (begin, end), = scan_ranges(data)[:1]
    marks = restart_markers(data, (begin, end))
    assert len(marks) >= 2
    out = []

    def flips(burst, k):
        bad = data.copy()
        for _ in range(200):
            i = int(rng.integers(begin + 1, end - burst - 1))
            new = bad[i:i + burst] ^ rng.integers(1, 255, burst).astype(np.uint8) if burst > 1 else bad[i:i + 1] ^ np.uint8(1 << int(rng.integers(0, 8)))
            if all(_plain(bad, j) for j in range(i, i + burst)) and not (new == 0xFF).any():
                bad[i:i + burst] = new
                return out.append((f"{name}/flip{burst}-{k}", bad, OK))
        raise AssertionError("no place for a flip")

    for k in range(4):
        flips(1, k)
    for k in range(3):
        flips(3, k)
    # an interval emptied to zero bytes: the first (scan start to first marker) and one in the middle
    out.append((f"{name}/empty-first", np.concatenate([data[:begin], data[marks[0]:]]), OK))
    out.append((f"{name}/empty-middle", np.concatenate([data[:marks[0] + 2], data[marks[1]:]]), OK))
    # a stray marker inside the last interval of the LAST scan (an EOI: the scan ends there, with every restart marker in
    # front of it) ...
    lbegin, lend = scan_ranges(data)[-1]
    lmarks = restart_markers(data, (lbegin, lend))
    last = (lmarks[-1] + 2 + lend) // 2
    out.append((f"{name}/stray-last", np.concatenate([data[:last], np.array([0xFF, 0xD9], np.uint8), data[last:]]), OK))
    # ... and inside the first of the first scan: the scan ends there and its other intervals are gone (their markers are
    # missing); in a file of several scans the other components are never reached, which is malformed
    first = (begin + marks[0]) // 2
    out.append((f"{name}/stray-first", np.concatenate([data[:first], np.array([0xFF, 0xD9], np.uint8), data[first:]]),
                ENOSUP if len(scan_ranges(data)) == 1 else EINVAL))
    # truncation before EOI, inside the last interval
    out.append((f"{name}/truncated", data[:last].copy(), OK))
    # a restart marker removed, and one duplicated
    out.append((f"{name}/marker-removed", np.concatenate([data[:marks[1]], data[marks[1] + 2:]]), ENOSUP))
    out.append((f"{name}/marker-doubled", np.concatenate([data[:marks[1] + 2], data[marks[1]:]]), ENOSUP))
    return out


DAMAGE_BASES = ("420-64x48-row", "grey-35x19-ri2", "420-35x19-scans-ri2", "four-12bit-17x17-ri2")


@functools.lru_cache(maxsize=None)
def damaged_files():
    out = []
    for name in DAMAGE_BASES:
        out += damaged(name, constructed_file(name)[0])
    out += damaged("color-sequential-restart.jpg", np.fromfile(G.path("decode/color-sequential-restart.jpg"), np.uint8))
    return out


# ---- what a stream holds: a plain reader of sequential scans that counts symbols ------------------------------------------------

def stream_stats(data):
    """Walks every sequential scan of an undamaged file symbol by symbol (T.81 F.2.2) -> dict: the longest code read, the
    longest code + magnitude, the largest DC size, ZRL symbols, ZRLs read directly in front of an EOB, AC runs of 16 or
    more zeros in front of a coefficient, blocks that end without an EOB, blocks that are all zero, stuffed FF 00 pairs."""
    b = bytes(data)
    s = dict(longest_code=0, longest_code_and_magnitude=0, dc_size=0, zrl=0, zrl_before_eob=0, long_runs=0, no_eob=0, zero_blocks=0,
             stuffed=0, blocks=0)
    tables, comps, ri, pos = {}, {}, 0, 2
    while pos + 3 < len(b):
        m = b[pos + 1]
        if m == 0xD9:
            break
        seg = b[pos + 4:pos + 2 + ((b[pos + 2] << 8) | b[pos + 3])]
        pos += 4 + len(seg)
        if m == 0xC4:
            i = 0
            while i < len(seg):
                counts, code, k, codes = seg[i + 1:i + 17], 0, i + 17, {}
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        codes[(length, code)] = seg[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                tables[seg[i]] = codes
                i = k
        elif m in (0xC0, 0xC1):
            comps = {seg[6 + 3 * c]: (seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(seg[5])}
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            slots = []
            for j in range(ns):
                fx, fy = comps[seg[1 + 2 * j]] if ns > 1 else (1, 1)
                slots += [(seg[2 + 2 * j] >> 4, 0x10 | (seg[2 + 2 * j] & 15))] * (fx * fy)
            e = pos
            while e + 1 < len(b) and not (b[e] == 0xFF and b[e + 1] != 0 and not 0xD0 <= b[e + 1] <= 0xD7):
                e += 1
            ecs, pos = b[pos:e], e
            intervals, at = [], 0
            for i in range(len(ecs) - 1):
                if ecs[i] == 0xFF and 0xD0 <= ecs[i + 1] <= 0xD7:
                    intervals.append(ecs[at:i])
                    at = i + 2
            intervals.append(ecs[at:])
            for chunk in intervals:
                s["stuffed"] += chunk.count(b"\xff\x00")
                bits = "".join(format(x, "08b") for x in chunk.replace(b"\xff\x00", b"\xff"))
                p = 0

                def symbol(tid):
                    nonlocal p
                    for length in range(1, 17):
                        v = tables[tid].get((length, int(bits[p:p + length], 2)))
                        if v is not None:
                            p += length
                            s["longest_code"] = max(s["longest_code"], length)
                            return v, length
                    raise AssertionError("no codeword")

                while len(bits) - p >= 8 or (p < len(bits) and "0" in bits[p:]):      # (what is left is padding)
                    for td, ta in slots:
                        t, length = symbol(td)
                        s["dc_size"] = max(s["dc_size"], t)
                        s["longest_code_and_magnitude"] = max(s["longest_code_and_magnitude"], length + t)
                        p += t
                        k, zrls, nonzero, ended = 1, 0, t != 0, False
                        while k < 64:
                            rs, length = symbol(ta)
                            r, size = rs >> 4, rs & 15
                            if size == 0 and r == 15:
                                k, zrls = k + 16, zrls + 1
                                s["zrl"] += 1
                                continue
                            if size == 0:
                                s["zrl_before_eob"] += zrls > 0
                                ended = True
                                break
                            s["long_runs"] += zrls > 0
                            s["longest_code_and_magnitude"] = max(s["longest_code_and_magnitude"], length + size)
                            k, p, zrls, nonzero = k + r + 1, p + size, 0, True
                        s["no_eob"] += not ended
                        s["zero_blocks"] += not nonzero
                        s["blocks"] += 1
    return s


def twice_scanned(data):
    """A copy of a file of one scan per component whose last scan is in the file twice: its component is written by two scans."""
    b = bytes(data)
    sos = b.rindex(b"\xff\xda")
    assert b.endswith(b"\xff\xd9")
    return np.frombuffer(b[:-2] + b[sos:-2] + b"\xff\xd9", np.uint8).copy()


def dc_symbol_17(data):
    """A copy of an undamaged file in which one value of a DC Huffman table is 17: the planner takes it (a DHT may hold any
    byte), and the interval that reads that codeword has status EINVAL (a DC symbol above 16).  The first value for which the
    host decoder says so is the one patched."""
    b, pos = bytes(data), 2
    while pos + 3 < len(b) and b[pos + 1] != 0xDA:
        seglen = (b[pos + 2] << 8) | b[pos + 3]
        if b[pos + 1] == 0xC4:
            i = pos + 4
            while i < pos + 2 + seglen:
                total = sum(b[i + 1:i + 17])
                if b[i] >> 4 == 0:
                    for k in range(total):
                        bad = np.frombuffer(b, np.uint8).copy()
                        bad[i + 17 + k] = 17
                        if host_decode(bad)[0] == EINVAL:
                            return bad
                i += 17 + total
        pos += 2 + seglen
    raise AssertionError("no DC codeword of the file is ever read")
