"""A small reader of a zlib stream that holds ONE dynamic-Huffman deflate block (RFC 1950 / 1951), as the device TIFF writer and
``mi_tiff_deflate_strip_host`` produce it -- it returns the tokens, not only the bytes -- and the token rule of the run form
("TIFF on the device") evaluated in plain Python.  Shared by the tests of the run form; no test in here."""
import zlib

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data):
        self.data = bytes(data) + b"\0\0\0\0"
        self.pos = 0

    def take(self, n):            # n <= 16 bits, least significant first
        at = self.pos >> 3
        r = (int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return r

    def rest_is_zero(self):
        at = self.pos >> 3
        return self.data[at] >> (self.pos & 7) == 0 and not any(self.data[at + 1:])


def _decoder(lengths):
    """{(length, code): symbol} of the canonical code of RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)        # Huffman codes come most significant bit first
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no such code")


def read_block(stream):
    """(tokens, info) of a zlib stream of one final dynamic block.  A token is a literal (int) or (length, distance, length symbol);
    info: hlit (the number of literal / length codes), hdist, bits (of the block, header included).  The stream's length, its
    Adler-32 and the padding bits (zero) are checked."""
    assert stream[0] == 0x78 and (stream[0] << 8 | stream[1]) % 31 == 0 and not stream[1] & 0x20
    bits = _Bits(stream[2:-4])
    assert bits.take(1) == 1, "one final block"
    assert bits.take(2) == 2, "dynamic Huffman"
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[_ORDER[i]] = bits.take(3)
    cl_table = _decoder(cl)
    lengths = []
    while len(lengths) < hlit + hdist:
        s = _symbol(bits, cl_table)
        if s < 16:
            lengths.append(s)
        elif s == 16:
            lengths += [lengths[-1]] * (3 + bits.take(2))
        elif s == 17:
            lengths += [0] * (3 + bits.take(3))
        else:
            lengths += [0] * (11 + bits.take(7))
    assert len(lengths) == hlit + hdist
    lit, dist = _decoder(lengths[:hlit]), _decoder(lengths[hlit:])
    tokens, out = [], bytearray()
    while True:
        s = _symbol(bits, lit)
        if s < 256:
            tokens.append(s)
            out.append(s)
        elif s == 256:
            break
        else:
            length = _LEN_BASE[s - 257] + bits.take(_LEN_EXTRA[s - 257])
            d = _symbol(bits, dist)
            distance = _DIST_BASE[d] + bits.take(_DIST_EXTRA[d])
            assert distance <= len(out), "a match reaches back before the first byte of the stream"
            for _ in range(length):
                out.append(out[-distance])
            tokens.append((length, distance, s))
    nbits = bits.pos
    assert len(stream) == 2 + (nbits + 7) // 8 + 4, "nothing but padding between the end of block and the checksum"
    assert bits.rest_is_zero(), "padding bits are zero"
    assert int.from_bytes(stream[-4:], "big") == zlib.adler32(bytes(out))
    return tokens, {"hlit": hlit, "hdist": hdist, "bits": nbits, "bytes": bytes(out)}


def length_symbol(length):
    """the length symbol of RFC 1951 3.2.5; 258 is symbol 285"""
    if length == 258:
        return 285
    return 257 + max(k for k, b in enumerate(_LEN_BASE[:-1]) if b <= length)


def rule_tokens(data):
    """the tokens of the run form of ``data`` (the bytes of a strip as stored)"""
    tokens, i, n = [], 0, len(data)
    while i < n:
        e = i + 1
        while e < n and data[e] == data[i]:
            e += 1
        tokens.append(data[i])
        r = e - i - 1
        while r >= 3:
            m = min(r, 258)
            tokens.append((m, 1, length_symbol(m)))
            r -= m
        tokens += [data[i]] * r
        i = e
    return tokens


EQUAL_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 518, 2049, 8193, 8192 + 259)
RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 600, 9000)


def run_pattern(seed, total=40000):
    """about ``total`` bytes: runs of lengths drawn from RUN_LENGTHS, of random values that differ from run to run (uint8 array)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    parts, n, last = [], 0, -1
    while n < total:
        length = int(rng.choice(RUN_LENGTHS))
        v = int(rng.integers(0, 256))
        if v == last:
            v = (v + 1) % 256
        parts.append(np.full(length, v, np.uint8))
        n, last = n + length, v
    return np.concatenate(parts)


def straddle_pattern(n, spans):
    """n bytes 1, 2, 1, 2, ... (no two neighbours equal) with zeros over every [a, b) of ``spans`` (clipped to the strip)"""
    import numpy as np
    d = (np.arange(n) % 2 + 1).astype(np.uint8)
    for a, b in spans:
        d[max(0, a):max(0, min(n, b))] = 0
    return d


def sparse_disc(dtype, n=1024, seed=21):
    """the sparse fixture: a noisy disc on a zero background, n x n"""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:n, :n]
    inside = (y - n * 0.47) ** 2 + (x - n * 0.55) ** 2 < (n * 0.3) ** 2
    top = 3000 if np.dtype(dtype) == np.uint16 else 200
    return np.where(inside, rng.normal(top * 0.5, top * 0.08, (n, n)).clip(1, top), 0).astype(dtype)


def rle_size(data):
    """bytes of zlib's stream of ``data`` at level 1 with the Z_RLE strategy (matches at distance 1 only)"""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(data) + c.flush())


def file_strips(path):
    """(streams, predictor flag 0 / 1, rows per strip) of a TIFF slice, through tags 273, 279, 317 and 278"""
    from PIL import Image
    im = Image.open(path)
    raw = open(path, "rb").read()
    return ([raw[o:o + c] for o, c in zip(im.tag_v2[273], im.tag_v2[279])], 1 if im.tag_v2.get(317, 1) == 2 else 0, int(im.tag_v2[278]))


def host_strip(data, bps, rowb, pred, runs):
    """(zlib stream, used_runs) of one strip through ``mi_tiff_deflate_strip_host``; ``data``: the strip's samples as bytes"""
    import ctypes as C
    from ipp_amd import capi
    data = bytes(data)
    cap = len(data) + len(data) // 32 + 4096
    out = (C.c_ubyte * cap)()
    n, used = C.c_size_t(0), C.c_int(-1)
    capi.check(capi.lib().mi_tiff_deflate_strip_host(data, len(data), bps, rowb, int(pred), int(runs), out, cap, C.byref(n), C.byref(used)))
    return bytes(out[:n.value]), used.value


def stored(a, pred):
    """the bytes of a strip of rows ``a`` (2-D numpy array) as stored: plain, or horizontally differenced (TIFF predictor 2)"""
    import numpy as np
    if not pred:
        return a.tobytes()
    d = a.copy()
    d[:, 1:] = a[:, 1:] - a[:, :-1]
    return np.ascontiguousarray(d).tobytes()
