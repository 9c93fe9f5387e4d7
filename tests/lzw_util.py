"""TIFF LZW in plain Python for the tests of the tree reader: a decoder written from the TIFF 6.0 text (section 13: a table of
strings, codes of 9 to 12 bits read from the high bit down, ClearCode 256, EndOfInformation 257, the width grows one code early),
an encoder with the schedule of libtiff's LZWEncode (with switches that make the streams a test needs: no leading Clear, no EOI,
never a Clear again), an inspector of a stream, the corpus of the host and device tests, the strips made for the device reader's
three strip classes and strips of a chosen compressed length (seam_corpus, sized_strip), and a small reader of TIFF directories.
Nothing here looks at csrc/tiff_lzw_dev.h: the decoder keeps strings, not offsets."""
import struct

import numpy as np

OK, CODE, FIRST, INPUT, OUTPUT, OLD_STYLE, TABLE = range(7)
STATUS_NAMES = ["ok", "code above the next free entry", "first code is not a literal", "input exhausted", "output passes the rows",
                "old-style LSB-first stream", "table overflow without Clear"]
CLEAR, EOI = 256, 257


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.n += width
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1
        return self

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
            self.n = 0
        return bytes(self.out)


def encode(data, clear_first=True, eoi=True, never_clear=False):
    """libtiff's schedule: Clear when the next free code reaches 4094, a bit more when it passes 511, 1023, 2047.
    never_clear: the table freezes at 4093 entries and 12-bit codes go on (a decoder must then refuse the stream)."""
    bw = BitWriter()
    nbits, free = 9, 258
    table = {}
    if clear_first:
        bw.put(CLEAR, nbits)
    if len(data) == 0:
        return bw.put(EOI, nbits).done() if eoi else bw.done()
    ent = data[0]
    for c in data[1:]:
        k = (ent, c)
        if k in table:
            ent = table[k]
            continue
        bw.put(ent, nbits)
        ent = c
        if never_clear and free >= 4094:
            continue
        table[k] = free
        free += 1
        if free == 4094 and not never_clear:
            table = {}
            free = 258
            bw.put(CLEAR, nbits)
            nbits = 9
        elif free > (1 << nbits) - 1 and nbits < 12:
            nbits += 1
    bw.put(ent, nbits)
    free += 1
    if free == 4094 and not never_clear:
        bw.put(CLEAR, nbits)
        nbits = 9
    elif free > (1 << nbits) - 1 and nbits < 12:
        nbits += 1
    if eoi:
        bw.put(EOI, nbits)
    return bw.done()


def inspect(stream, want):
    """Decodes `want` bytes from the stream as TIFF 6.0 describes it; {"data", "widths" (set), "clears" (after the first code),
    "leading_clear", "eoi" (EOI is the next code once the bytes are out), "max_string", "codes", "rest" (whole bytes never looked at),
    "max_used_offset" (an entry's string begins where the code before it was emitted: the largest such output offset among the table
    codes the stream uses, -1 without any), "far_long_codes" (table codes in use whose entry begins above offset 65535 and is longer
    than 64 bytes), "full_tables" (Clears that came when entry 4092, the last before the encoders' Clear, was in the table)}"""
    padded = bytes(stream) + b"\0\0\0"
    total = 8 * len(stream)
    at = 0

    def nxt(width):
        nonlocal at
        if at + width > total:
            raise ValueError("input exhausted")
        v = (int.from_bytes(padded[at >> 3:(at >> 3) + 3], "big") >> (24 - (at & 7) - width)) & ((1 << width) - 1)
        at += width
        return v

    def fresh():
        return {i: bytes([i]) for i in range(256)}, 258, 9

    table, free, width = fresh()
    out = bytearray()
    info = {"widths": set(), "clears": 0, "leading_clear": False, "max_string": 0, "codes": 0, "max_used_offset": -1, "far_long_codes": 0,
            "full_tables": 0}
    begins = {}      # table code -> the output offset its string was defined at
    old = old_at = None
    first = True
    while len(out) < want:
        code = nxt(width)
        info["widths"].add(width)
        info["codes"] += 1
        if code == EOI:
            raise ValueError("EOI before the rows are full")
        if code == CLEAR:
            if first:
                info["leading_clear"] = True
            else:
                info["clears"] += 1
            info["full_tables"] += free >= 4093
            table, free, width = fresh()
            old = None
            first = False
            continue
        first = False
        if old is None:
            if code > 255:
                raise ValueError("first code is not a literal")
            s = table[code]
        else:
            if code in table:
                s = table[code]
                if code > EOI:
                    info["max_used_offset"] = max(info["max_used_offset"], begins[code])
                    info["far_long_codes"] += begins[code] > 65535 and len(s) > 64
            elif code == free:
                s = table[old] + table[old][:1]
            else:
                raise ValueError("code above the next free entry")
            if free > 4093:
                raise ValueError("table overflow")
            table[free] = table[old] + s[:1]
            begins[free] = old_at
            free += 1
            if free + 1 >= (1 << width) and width < 12:   # "as soon as 511 is stored": the next code has ten bits
                width += 1
        if len(out) + len(s) > want:
            raise ValueError("output passes the rows")
        old_at = len(out)
        out += s
        info["max_string"] = max(info["max_string"], len(s))
        old = code
    info["data"] = bytes(out)
    info["eoi"] = at + width <= total and nxt(width) == EOI
    info["rest"] = (total - at) // 8
    return info


def decode(stream, want):
    return inspect(stream, want)["data"]


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


_CORPUS = None


def corpus():
    """name -> (stream, raw bytes); built once"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    c = {}
    for name, data in (("empty", b""), ("one_byte", b"\x5a"), ("noise_526", _noise(526, 1)), ("noise_2408", _noise(2408, 2)),
                       ("noise_4816", _noise(4816, 3)), ("noise_9632", _noise(9632, 4)), ("const_526", b"\x07" * 526),
                       ("const_65536", b"\xc3" * 65536),
                       ("ramp_u16", (np.arange(8 * 301, dtype=np.uint16).reshape(8, 301) // 3 + 1000).tobytes())):
        c[name] = (encode(data), data)
    text = _noise(40, 5) * 30
    c["no_leading_clear"] = (encode(text, clear_first=False), text)
    c["no_eoi"] = (encode(text, eoi=False), text)
    c["bytes_after_eoi"] = (encode(text) + b"\x00\xff\x55\xaa\x13", text)
    _CORPUS = c
    return c


_SEAMS = None


def seam_corpus():
    """name -> (stream, raw bytes): strips for the three classes of the device reader (rows of at most 16 384 bytes in LDS, rows in
    global memory with 16-bit offsets up to 65 536 bytes, 32-bit offsets above); tests/test_tiff_seam_streams_host.py asserts what
    each one holds.  far_strings: after 66 000 bytes of noise a period of 3 bytes, so that strings grow by a byte every third code."""
    global _SEAMS
    if _SEAMS is None:
        datas = {"noise_40000": _noise(40000, 11), "noise_65536": _noise(65536, 12), "noise_70001": _noise(70001, 13),
                 "far_strings": _noise(66000, 14) + b"\x11\x5a\xe7" * 4000}
        _SEAMS = {k: (encode(d), d) for k, d in datas.items()}
    return _SEAMS


def sized_strip(width, target, seed):
    """(strip of exactly `target` bytes, its `width` raw bytes, bytes after EOI): noise trimmed until the encoder gives that length,
    then one byte (or a period of 2 to 4 bytes) repeated to the row's end.  Not every length is the encoder's: behind Clear and 254
    codes of 9 bits a strip has 2295 + 10 k bits, and no k puts that into (8 * 512, 8 * 513] -- such a length is the strip of one
    byte less with one byte after EOI, which a reader does not look at (the corpus' bytes_after_eoi)."""
    noise = _noise(width, seed)
    for after in (0, 1):
        for period in (1, 2, 3, 4):
            got = _sized(noise, width, target - after, bytes(b ^ 0x80 for b in noise[:period]))
            if got:
                return got[0] + b"\xa5" * after, got[1], after
    raise ValueError(f"no strip of {target} bytes")


def _sized(noise, width, target, fill):
    def make(m):
        data = noise[:m] + (fill * width)[:width - m]
        return encode(data), data

    lo, hi = 1, width       # the length grows with the noise, nearly steadily: bisect, then look around
    while lo < hi:
        mid = (lo + hi) // 2
        if len(make(mid)[0]) < target:
            lo = mid + 1
        else:
            hi = mid
    for m in range(max(1, lo - 4), min(width, lo + 4) + 1):
        stream, data = make(m)
        if len(stream) == target:
            return stream, data
    return None


def malformed():
    """[(name, stream, expected size, status)]: one stream per status, each a valid stream with an edit"""
    c = corpus()
    out = [("code_above_free", BitWriter().put(CLEAR, 9).put(97, 9).put(98, 9).put(300, 9).put(EOI, 9).done(), 8, CODE),
           ("first_not_literal", BitWriter().put(CLEAR, 9).put(258, 9).put(EOI, 9).done(), 4, FIRST),
           ("first_not_literal_after_clear", BitWriter().put(CLEAR, 9).put(97, 9).put(CLEAR, 9).put(258, 9).done(), 4, FIRST),
           ("cut_short", c["noise_2408"][0][:1200], 2408, INPUT),
           ("eoi_early", c["noise_526"][0], 527, INPUT),
           ("nothing", b"", 4, INPUT),
           ("string_passes_rows", c["const_526"][0], 525, OUTPUT),
           ("old_style", b"\x00\x01" + c["noise_526"][0][2:], 526, OLD_STYLE),
           ("table_full", encode(_noise(4816, 3), never_clear=True), 4816, TABLE),
           ("no_clear_code_above", BitWriter().put(97, 9).put(259, 9).put(EOI, 9).done(), 8, CODE)]
    return out


# ---------------------------------------------------------------------------------------------------------------- TIFF directories
def tiff_pages(path):
    """[{tag: value or tuple}] of every page of a little-endian classic or BigTIFF file, and the file's bytes"""
    b = open(path, "rb").read()
    assert b[:2] == b"II"
    big = struct.unpack_from("<H", b, 2)[0] == 43
    off = struct.unpack_from("<Q", b, 8)[0] if big else struct.unpack_from("<I", b, 4)[0]
    size = {1: 1, 2: 1, 3: 2, 4: 4, 16: 8}
    fmt = {1: "B", 2: "B", 3: "H", 4: "I", 16: "Q"}
    pages = []
    while off:
        n = struct.unpack_from("<Q" if big else "<H", b, off)[0]
        at = off + (8 if big else 2)
        tags = {}
        for _ in range(n):
            tag, typ = struct.unpack_from("<HH", b, at)
            cnt = struct.unpack_from("<Q" if big else "<I", b, at + 4)[0]
            field = at + (12 if big else 8)
            nbytes = size[typ] * cnt
            src = field if nbytes <= (8 if big else 4) else struct.unpack_from("<Q" if big else "<I", b, field)[0]
            vals = struct.unpack_from(f"<{cnt}{fmt[typ]}", b, src)
            tags[tag] = vals[0] if cnt == 1 else vals
            at += 20 if big else 12
        pages.append(tags)
        off = struct.unpack_from("<Q" if big else "<I", b, at)[0]
    return pages, b


def tiff_strips(path):
    """[(page, strip, stream bytes, raw size)] of every strip of an LZW file"""
    pages, b = tiff_pages(path)
    out = []
    for p, t in enumerate(pages):
        w, h, bps, rps = t[256], t[257], t[258], min(t.get(278, t[257]), t[257])
        offs = t[273] if isinstance(t[273], tuple) else (t[273],)
        cnts = t[279] if isinstance(t[279], tuple) else (t[279],)
        for s, (o, n) in enumerate(zip(offs, cnts)):
            rows = min(rps, h - s * rps)
            out.append((p, s, b[o:o + n], rows * w * bps // 8))
    return out
