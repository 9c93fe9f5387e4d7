"""Shared by the tests of the device TIFF reader's inflater (csrc/tiff_inflate_dev.h, csrc/tiff_inflate.hip); no test in here.

  make_tiff / image_tiff   a minimal TIFF maker in pure ``struct``: classic little-endian, one directory, strips; any byte strings as
                           strips, so that a test can put any stream into a file
  BitWriter, fixed_code,   what a hand-made deflate stream takes
  dynamic_header
  inspect                  a plain-Python inflater that reports what a stream contains (block types, code lengths, distances ...)
  corpus()                 the valid streams, each with the bytes it stands for
  malformed()              the short, fixed list of streams an inflater must refuse, each with the status expected
  seam_corpus(),           valid streams made for the seams of the device context (pending window, staged input, Adler sums), and the
  pending_trace            replay of its flush rule over a stream's tokens
"""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

# the status words of csrc/tiff_inflate_dev.h (InfStatus)
OK, HEADER, BLOCK_TYPE, STORED_LEN, CODE_OVER, CODE_INCOMPLETE, CODE_NO_EOB, SYMBOL, DISTANCE, INPUT, OUTPUT, CHECKSUM = range(12)
STATUS_NAMES = ["ok", "zlib header", "block type", "stored length", "over-subscribed code", "incomplete code", "no end-of-block code",
                "invalid symbol", "distance before the start", "input exhausted", "output size", "checksum"]

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ------------------------------------------------------------------------------------------------ TIFF
def make_tiff(path, strips, nx, ny, bits=8, rows_per_strip=None, compression=1, predictor=1, sample_format=1, counts=None):
    """One classic little-endian TIFF: header | strips | strip tables | directory.  ``strips``: the byte strings as they go into the
    file (a strip may be longer than its rows need).  compression 1 / 8 / 32946, predictor 1 / 2.  ``counts``: the StripByteCounts
    the directory claims, when they are not to be the strips' lengths."""
    rps = ny if rows_per_strip is None else rows_per_strip
    body, off, cnt = bytearray(8), [], []
    for s in strips:
        off.append(len(body))
        cnt.append(len(s))
        body += s
        if len(body) & 1:
            body += b"\0"
    ns = len(strips)
    cnt = list(counts) if counts is not None else cnt
    off_at = len(body)
    if ns > 1:
        body += struct.pack(f"<{ns}I", *off)
    cnt_at = len(body)
    if ns > 1:
        body += struct.pack(f"<{ns}I", *cnt)
    ents = [(256, 4, 1, nx), (257, 4, 1, ny), (258, 3, 1, bits), (259, 3, 1, compression), (262, 3, 1, 1),
            (273, 4, ns, off_at if ns > 1 else off[0]), (277, 3, 1, 1), (278, 4, 1, rps), (279, 4, ns, cnt_at if ns > 1 else cnt[0]),
            (284, 3, 1, 1)]
    if predictor != 1:
        ents.append((317, 3, 1, predictor))
    ents.append((339, 3, 1, sample_format))
    ifd = len(body)
    body += struct.pack("<H", len(ents))
    for tag, typ, count, value in ents:
        body += struct.pack("<HHII", tag, typ, count, value)
    body += struct.pack("<I", 0)
    body[0:8] = b"II" + struct.pack("<HI", 42, ifd)
    with open(path, "wb") as f:
        f.write(bytes(body))
    return path


def image_tiff(path, img, rows_per_strip, compression=8, predictor=1, level=1, pad=0):
    """``img`` (2-D uint8 / uint16 / float32) as a TIFF of deflate (8 / 32946) or raw (1) strips; predictor 2: every row is stored
    as differences to the left neighbour, wrapping in the sample's width.  ``pad``: bytes appended to every strip."""
    img = np.ascontiguousarray(img)
    ny, nx = img.shape
    stored = img
    if predictor == 2:
        stored = img.copy()
        stored[:, 1:] = img[:, 1:] - img[:, :-1]
    strips = []
    for r0 in range(0, ny, rows_per_strip):
        raw = stored[r0:r0 + rows_per_strip].tobytes()
        strips.append((raw if compression == 1 else zlib.compress(raw, level)) + b"\0" * pad)
    return make_tiff(path, strips, nx, ny, 8 * img.dtype.itemsize, rows_per_strip, compression, predictor, 3 if img.dtype == np.float32 else 1)


def stream_tiff(path, stream, expected_size, compression=8):
    """a stream as the single strip of a one-row uint8 TIFF of ``expected_size`` pixels"""
    return make_tiff(path, [bytes(stream)], expected_size, 1, 8, 1, compression)


# ------------------------------------------------------------------------------------------------ hand-made streams
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        """n bits of value, least significant first (every field of deflate but the Huffman codes)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, n):
        """a Huffman code of n bits: most significant bit first"""
        for k in range(n - 1, -1, -1):
            self.bits(code >> k & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def done(self):
        return bytes(self.align().out)


def fixed_code(sym):
    """(code, bits) of a literal / length symbol in the fixed code (RFC 1951 3.2.6)"""
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def canonical_codes(lengths):
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


_CL_LENGTHS = [4] * 13 + [5] * 6      # a complete code-length code of 19 symbols: every length is sent plainly


def dynamic_header(bw, lit_lengths, dist_lengths, final=1):
    """BFINAL, BTYPE 2 and the header of a dynamic block that declares exactly these code lengths (no repeat symbols)"""
    bw.bits(final, 1).bits(2, 2).bits(len(lit_lengths) - 257, 5).bits(len(dist_lengths) - 1, 5).bits(15, 4)
    for s in _ORDER:
        bw.bits(_CL_LENGTHS[s], 3)
    cc = canonical_codes(_CL_LENGTHS)
    for l in list(lit_lengths) + list(dist_lengths):
        bw.code(cc[l], _CL_LENGTHS[l])
    return bw


def adler_bytes(data):
    return struct.pack(">I", zlib.adler32(data) & 0xffffffff)


# ------------------------------------------------------------------------------------------------ the inspector
def _table(lengths):
    """[the next maxlen bits as they lie in the stream] -> symbol << 4 | length (0: no code), and maxlen"""
    maxlen = max(lengths) if lengths else 0
    if maxlen == 0:
        return [0], 0
    table = [0] * (1 << maxlen)
    for s, (l, c) in enumerate(zip(lengths, canonical_codes(lengths))):
        if l:
            r = int(format(c, f"0{l}b")[::-1], 2)
            for i in range(r, 1 << maxlen, 1 << l):
                table[i] = s << 4 | l
    return table, maxlen


def inspect(stream):
    """What a zlib stream contains, from a plain-Python inflater: a dict with ``data`` (the bytes), ``block_types`` (a list),
    ``max_code_length`` (of the literal / length and distance codes in use or declared), ``max_dist_symbol``, ``max_distance``,
    ``len3``, ``len258``, ``len258_dist1``, ``matches``, ``matches_dist1``, ``cl_symbols`` (which of 16 / 17 / 18 occur),
    ``dist_codes`` (per dynamic block: the lengths of the distance codes declared), ``empty_stored`` (stored blocks of no bytes),
    ``tokens`` (in order: (1, 0) per literal or stored byte, (length, distance) per match) and ``codes_across`` (the byte offsets,
    multiples of 1024, that lie strictly inside a literal / length or distance code)."""
    data = bytes(stream)
    src = data + b"\0" * 8
    pos = 16
    out = bytearray()
    info = dict(block_types=[], max_code_length=0, max_dist_symbol=-1, max_distance=0, len3=0, len258=0, len258_dist1=0, matches=0,
                matches_dist1=0, cl_symbols=set(), dist_codes=[], empty_stored=0, tokens=[], codes_across=set())
    tokens = info["tokens"]

    def across(start, n):
        if n and start // 8192 != (start + n - 1) // 8192:
            info["codes_across"].add((start + n - 1) // 8192 * 1024)
    assert data[0] & 15 == 8 and (data[0] << 8 | data[1]) % 31 == 0 and not data[1] & 32

    def peek(n):
        at = pos >> 3
        return (int.from_bytes(src[at:at + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    final = 0
    while not final:
        final = peek(1)
        btype = peek(3) >> 1
        pos += 3
        info["block_types"].append(btype)
        if btype == 0:
            pos = (pos + 7) & ~7
            n = peek(16)
            pos += 16
            nn = peek(16)
            pos += 16
            assert n ^ 0xffff == nn
            out += src[pos >> 3:(pos >> 3) + n]
            tokens += [(1, 0)] * n
            pos += 8 * n
            info["empty_stored"] += n == 0
            continue
        assert btype in (1, 2)
        if btype == 1:
            lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
            dist = [5] * 32
        else:
            hlit, hdist, hclen = peek(5) + 257, (peek(10) >> 5) + 1, (peek(14) >> 10) + 4
            pos += 14
            cl = [0] * 19
            for i in range(hclen):
                cl[_ORDER[i]] = peek(3)
                pos += 3
            ctab, cmax = _table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                e = ctab[peek(cmax)]
                assert e
                pos += e & 15
                s = e >> 4
                if s < 16:
                    lens.append(s)
                    continue
                info["cl_symbols"].add(s)
                if s == 16:
                    lens += [lens[-1]] * (3 + peek(2))
                    pos += 2
                elif s == 17:
                    lens += [0] * (3 + peek(3))
                    pos += 3
                else:
                    lens += [0] * (11 + peek(7))
                    pos += 7
            assert len(lens) == hlit + hdist
            lit, dist = lens[:hlit], lens[hlit:]
            info["dist_codes"].append([l for l in dist if l])
            info["max_code_length"] = max(info["max_code_length"], max(lit), max(dist))
        ltab, lmax = _table(lit)
        dtab, dmax = _table(dist)
        while True:
            e = ltab[peek(lmax)]
            assert e
            across(pos, e & 15)
            pos += e & 15
            s = e >> 4
            if s < 256:
                out.append(s)
                tokens.append((1, 0))
                continue
            if s == 256:
                break
            length = _LEN_BASE[s - 257] + peek(_LEN_EXTRA[s - 257])
            pos += _LEN_EXTRA[s - 257]
            e = dtab[peek(dmax)]
            assert e
            across(pos, e & 15)
            pos += e & 15
            ds = e >> 4
            d = _DIST_BASE[ds] + peek(_DIST_EXTRA[ds])
            pos += _DIST_EXTRA[ds]
            assert d <= len(out)
            tokens.append((length, d))
            info["matches"] += 1
            info["matches_dist1"] += d == 1
            info["len3"] += length == 3
            info["len258"] += length == 258
            info["len258_dist1"] += length == 258 and d == 1
            info["max_dist_symbol"] = max(info["max_dist_symbol"], ds)
            info["max_distance"] = max(info["max_distance"], d)
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                for _ in range(length):
                    out.append(out[-d])
    pos = (pos + 7) & ~7
    assert src[pos >> 3:(pos >> 3) + 4] == adler_bytes(bytes(out))
    info["data"] = bytes(out)
    return info


# ------------------------------------------------------------------------------------------------ the corpus
RUNS_BYTES = b"\0" * 5000 + b"\1\2" * 700 + b"xyz" * 500 + b"\0" * 3
FIXED_BYTES = b"abcabcabd" * 300 + bytes(range(256))


def _deflate(data, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def skew_bytes():
    """24 symbols (the bytes 0 .. 23) with the Fibonacci counts 1, 1, 2 ... 46368, shuffled"""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    a = np.repeat(np.arange(24, dtype=np.uint8), fib)
    np.random.default_rng(3).shuffle(a)
    return a.tobytes()


def img_array():
    rng = np.random.default_rng(1)
    a = rng.poisson(30.0, (512, 1024)).astype(np.uint16) + (np.arange(1024, dtype=np.uint16) // 8)[None, :]
    a[:, :300] = 0
    return a


def far_stream():
    """(stream, bytes): a stored block of 32 768 random bytes, then a fixed block of one match of 258 bytes at distance 32 768"""
    head = np.random.default_rng(9).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    bw = BitWriter()
    bw.bits(0x78, 8).bits(0x01, 8)
    bw.bits(0, 1).bits(0, 2).align().bits(32768, 16).bits(32768 ^ 0xffff, 16).raw(head)
    bw.bits(1, 1).bits(1, 2)
    bw.code(*fixed_code(285))
    bw.code(29, 5).bits(32768 - 24577, 13)
    bw.code(*fixed_code(256))
    data = head + head[:258]
    return bw.done() + adler_bytes(data), data


def strip_host(data, bps, rowb, pred, runs):
    """the stream of ``mi_tiff_deflate_strip_host`` for one strip, and whether it took the run form"""
    from ipp_amd import capi
    lib = capi.lib()
    cap = len(data) + len(data) // 32 + 4096
    out = (C.c_ubyte * cap)()
    n, used = C.c_size_t(0), C.c_int(0)
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    capi.check(lib.mi_tiff_deflate_strip_host(buf, len(data), bps, rowb, pred, runs, out, cap, C.byref(n), C.byref(used)))
    return bytes(out[:n.value]), bool(used.value)


def sparse_strip():
    """64 x 1024 uint16: zero but for a bright disc (the background of a stitched volume)"""
    y, x = np.mgrid[0:64, 0:1024]
    rng = np.random.default_rng(3)
    a = np.where((y - 32) ** 2 + (x - 500) ** 2 < 20 ** 2, 900 + rng.integers(0, 64, (64, 1024)), 0).astype(np.uint16)
    return a


def dense_strip():
    """64 x 1024 uint16: a smooth field with noise on it"""
    y, x = np.mgrid[0:64, 0:1024]
    rng = np.random.default_rng(4)
    return (400 + 200 * np.sin(x / 90.0) * np.cos(y / 17.0) + rng.normal(0, 12, (64, 1024))).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def corpus(with_library=True):
    """{name: (stream, bytes)}; ``with_library``: also the streams of the library's own strip coder (needs the built library)"""
    c = {}
    stored = np.random.default_rng(1).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    c["stored"] = (_deflate(stored, 0), stored)
    c["fixed"] = (_deflate(FIXED_BYTES, 9, zlib.Z_FIXED), FIXED_BYTES)
    skew = skew_bytes()
    c["skew"] = (_deflate(skew, 1, zlib.Z_HUFFMAN_ONLY), skew)
    c["runs"] = (_deflate(RUNS_BYTES, 1), RUNS_BYTES)
    c["runs_rle"] = (_deflate(RUNS_BYTES, 1, zlib.Z_RLE), RUNS_BYTES)
    z = zlib.compressobj(1)
    parts = z.compress(RUNS_BYTES[:3000]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(RUNS_BYTES[3000:6000]) + z.flush(zlib.Z_FULL_FLUSH)
    parts += z.compress(RUNS_BYTES[6000:]) + z.flush()
    c["flush"] = (parts, RUNS_BYTES)
    img = img_array().tobytes()
    c["img"] = (_deflate(img, 1), img)
    c["far"] = far_stream()
    if with_library:
        for name, a in (("sparse", sparse_strip()), ("dense", dense_strip())):
            raw = a.tobytes()
            for runs in (0, 1):
                stream, used = strip_host(raw, 2, 2048, 0, runs)
                c[f"writer_{name}_{'runs' if runs else 'literal'}"] = (stream, raw)
    return c


# ------------------------------------------------------------------------------------------------ the malformed list
def _zs(bw, data=b""):
    return bw.done() + adler_bytes(data)


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, stream, expected size, status)]: short and fixed.  The streams are refused for the reason named and no other."""
    m = []
    m.append(("block_type_3", _zs(BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(3, 2)), 16, BLOCK_TYPE))
    m.append(("stored_len", _zs(BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(0, 2).align().bits(5, 16).bits(5 ^ 0xfffe, 16)
                                .raw(b"hello"), b"hello"), 5, STORED_LEN))
    over = [0] * 257
    over[0] = over[1] = over[256] = 1
    m.append(("oversubscribed_literal_code", _zs(dynamic_header(BitWriter().bits(0x78, 8).bits(0x01, 8), over, [1, 1]).bits(0, 16)), 16,
              CODE_OVER))
    noeob = [0] * 257
    noeob[0] = noeob[1] = 1
    m.append(("no_end_of_block", _zs(dynamic_header(BitWriter().bits(0x78, 8).bits(0x01, 8), noeob, [1, 1]).bits(0, 16)), 16, CODE_NO_EOB))
    bw = BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(1, 2)
    bw.code(*fixed_code(ord("a"))).code(*fixed_code(257)).code(30, 5).code(*fixed_code(256))
    m.append(("distance_symbol_30", _zs(bw, b"aaaa"), 4, SYMBOL))
    bw = BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(1, 2)
    bw.code(*fixed_code(ord("a"))).code(*fixed_code(ord("b"))).code(*fixed_code(257)).code(2, 5).code(*fixed_code(256))
    m.append(("match_before_start", _zs(bw, b"ababa"), 5, DISTANCE))
    stream, img = corpus(False)["img"]
    m.append(("img_truncated", stream[:len(stream) // 2], len(img), INPUT))
    m.append(("img_one_row_short", stream, len(img) - 2048, OUTPUT))
    m.append(("img_one_row_long", stream, len(img) + 2048, OUTPUT))
    flipped = bytearray(stream)
    flipped[-2] ^= 0x10
    m.append(("adler_flipped", bytes(flipped), len(img), CHECKSUM))
    bad = bytearray(stream)
    bad[1] ^= 1
    m.append(("bad_fcheck", bytes(bad), len(img), HEADER))
    return m


# ------------------------------------------------------------------------------------------------ the seam streams
# Streams aimed at the device context of csrc/tiff_inflate.hip (its pending window of PEND bytes in LDS, its input staged STAGE bytes
# at a time, its Adler sums); tests/test_tiff_seam_streams_host.py asserts what each one claims through inspect() and pending_trace().
PEND, STAGE = 4096, 1024


def pending_trace(tokens):
    """The flush rule of the device context replayed over inspect()'s tokens: the output waits until PEND bytes or more are pending
    after a token, then all of it goes out.  [(pos, flushed, npend, length, distance)] per match, as they stand before the match,
    and [flushed after each flush]."""
    flushed = npend = 0
    matches, flushes = [], []
    for length, dist in tokens:
        if dist:
            matches.append((flushed + npend, flushed, npend, length, dist))
        npend += length
        if npend >= PEND:
            flushed += npend
            npend = 0
            flushes.append(flushed)
    return matches, flushes


class FixedBlock:
    """one final block in the fixed code behind a zlib header, the bytes it stands for, and the bytes pending by the flush rule"""

    def __init__(self, seed):
        self.bw = BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(1, 2)
        self.data = bytearray()
        self.rng = np.random.default_rng(seed)
        self.npend = 0

    def _token(self, length):
        self.npend += length
        if self.npend >= PEND:
            self.npend = 0

    def literals(self, n):
        for b in self.rng.integers(0, 256, n, dtype=np.uint8).tolist():
            self.bw.code(*fixed_code(b))
            self.data.append(b)
            self._token(1)
        return self

    def match(self, length, dist):
        ls = max(k for k in range(29) if _LEN_BASE[k] <= length) if length < 258 else 28
        ds = max(k for k in range(30) if _DIST_BASE[k] <= dist)
        assert 3 <= length <= 258 and 1 <= dist <= len(self.data) and length - _LEN_BASE[ls] < 1 << _LEN_EXTRA[ls]
        self.bw.code(*fixed_code(257 + ls)).bits(length - _LEN_BASE[ls], _LEN_EXTRA[ls])
        self.bw.code(ds, 5).bits(dist - _DIST_BASE[ds], _DIST_EXTRA[ds])
        for _ in range(length):
            self.data.append(self.data[-dist])
        self._token(length)
        return self

    def done(self):
        self.bw.code(*fixed_code(256))
        data = bytes(self.data)
        return self.bw.done() + adler_bytes(data), data


def pend_offset_stream(r):
    """PEND - 1 literals and a match that leaves ``flushed % 4 == r`` at the first flush; PEND - 1 literals and 258 bytes at distance
    1 (they end at the last byte the pending window can hold when r is 3); 200 literals and 258 bytes whose source begins 100 bytes
    before ``flushed`` and ends 158 after it; a match at distance npend (its source begins at ``flushed``) and one at npend + 1"""
    f = FixedBlock(40 + r)
    f.literals(PEND - 1).match({0: 5, 1: 6, 2: 7, 3: 4}[r], 1000)
    f.literals(PEND - 1).match(258, 1)
    f.literals(200).match(258, 300)
    f.match(20, f.npend).match(20, f.npend + 1)
    return f.done()


OVERLAP_DISTANCES = (1, 2, 3, 63, 64, 65)


def overlap_stream():
    """per distance d: literals up to a few bytes below PEND pending, 258 bytes at distance d (the match crosses PEND and the flush
    follows it), one literal, and 258 bytes at distance d again: for d > 1 that source begins before ``flushed`` and repeats"""
    f = FixedBlock(50)
    for i, d in enumerate(OVERLAP_DISTANCES):
        f.literals(PEND - 2 - 41 * i - f.npend)
        f.match(258, d).literals(1).match(258, d)
    return f.done()


def stored_stream(n):
    """(stream of n bytes in all, bytes): one stored block of n - 11 random bytes"""
    data = np.random.default_rng(n).integers(0, 256, n - 11, dtype=np.uint8).tobytes()
    bw = BitWriter().bits(0x78, 8).bits(0x01, 8).bits(1, 1).bits(0, 2).align().bits(len(data), 16).bits(len(data) ^ 0xffff, 16).raw(data)
    stream = bw.done() + adler_bytes(data)
    assert len(stream) == n
    return stream, data


def dynamic_edge_stream():
    """(stream, bytes): one dynamic block of Huffman codes only, its payload the shortest of a fixed sequence for which a code lies
    across byte STAGE of the stream (found by trial: which payload does it depends on the zlib at hand; the claim is asserted)"""
    rng = np.random.default_rng(21)
    pool = (rng.gamma(2.0, 9.0, 6000) % 256).astype(np.uint8).tobytes()
    for n in range(3000, 3200):
        stream = _deflate(pool[:n], 9, zlib.Z_HUFFMAN_ONLY)
        info = inspect(stream)
        if info["block_types"] == [2] and STAGE in info["codes_across"] and len(stream) > STAGE + 16:
            return stream, pool[:n]
    raise AssertionError("no payload puts a code across byte %d" % STAGE)


STAGE_EDGE_SIZES = tuple(range(1021, 1029)) + tuple(range(2047, 2051))
ADLER_TAIL_SIZES = (1, 2, 3, 5, 4099)
ADLER_BIG = 3 << 19          # 1.5 MiB


@functools.lru_cache(maxsize=None)
def seam_corpus():
    """{name: (stream, bytes)}: the streams for the seams of the device context"""
    c = {}
    for r in range(4):
        c[f"pend_offset_{r}"] = pend_offset_stream(r)
    c["overlap_across_flush"] = overlap_stream()
    for n in STAGE_EDGE_SIZES:
        c[f"stage_edge_{n}"] = stored_stream(n)
    c["stage_edge_dyn"] = dynamic_edge_stream()
    for n in ADLER_TAIL_SIZES:
        data = np.random.default_rng(100 + n).integers(0, 256, n, dtype=np.uint8).tobytes()
        c[f"adler_tail_{n}"] = (_deflate(data, 1), data)
    big = b"\xff" * ADLER_BIG
    c["adler_big"] = (_deflate(big, 1), big)
    return c
