"""The strips of the LZW encoder tests (tests/test_tiff_lzw_enc_host.py on the CPU, tests/test_gpu_tiff_lzw_enc.py on the device).
The reference of every test is ``lzw_util.encode``, the Python restatement of libtiff's schedule; nothing here looks at
csrc/tiff_lzw_enc_dev.h.  ``corpus()`` asserts through ``lzw_util.inspect`` that each strip reaches what it is for."""
import numpy as np

from tests import lzw_util as lu

# prefix length of lu._noise(5000, 21) -> (next free code after the last code, stream bytes): the issue's table, a cross-check of
# the search below
TAILS = {254: (512, 289), 767: (1024, 929), 1805: (2048, 2337), 3928: (4094, 5407)}


def end_states(data):
    """[next free code once the last code of data[:L] is counted] for L = 1 .. len(data): the schedule of ``lzw_util.encode``
    without the bits (an entry per emitted code, everything forgotten when the next free code reaches 4094)."""
    out = []
    table, free = {}, 258
    ent = data[0]
    out.append(free + 1)
    for c in data[1:]:
        k = (ent, c)
        if k in table:
            ent = table[k]
        else:
            ent = c
            table[k] = free
            free += 1
            if free == 4094:
                table, free = {}, 258
        out.append(free + 1)
    return out


def tail_prefixes():
    """{next free code after the last code: prefix length}: the first prefix of the noise after whose last code the next free code
    is 512, 1024, 2048 (EOI gets a bit more) or 4094 (a Clear stands before EOI), found by search"""
    states = end_states(lu._noise(5000, 21))
    return {want: states.index(want) + 1 for want in (512, 1024, 2048, 4094)}


_CORPUS = None


def corpus():
    """name -> raw bytes, in a fixed order; built and checked once"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    base = lu.corpus()
    c = {k: base[k][1] for k in ("one_byte", "noise_526", "noise_2408", "noise_4816", "noise_9632", "const_526", "const_65536", "ramp_u16")}
    c["two_bytes"] = b"\x5a\xa5"
    c["period3"] = b"\x11\x5a\xe7" * 4000
    c["noise_70001"] = lu.seam_corpus()["noise_70001"][1]
    noise = lu._noise(5000, 21)
    found = tail_prefixes()
    assert {n: f for f, n in found.items()} == {n: f for n, (f, _) in TAILS.items()}, found
    for free, n in found.items():
        c[f"tail_{free}"] = noise[:n]

    info = {k: lu.inspect(lu.encode(v), len(v)) for k, v in c.items()}
    for k, i in info.items():
        assert i["data"] == c[k] and i["leading_clear"], k
    assert info["one_byte"]["codes"] == 2 and info["two_bytes"]["codes"] == 3
    assert info["noise_526"]["widths"] == {9, 10} and info["noise_526"]["clears"] == 0
    assert info["noise_2408"]["widths"] == {9, 10, 11, 12} and info["noise_2408"]["clears"] == 0
    assert info["noise_4816"]["clears"] == 1 and info["noise_9632"]["clears"] == 2
    assert info["const_526"]["max_string"] == 31
    assert info["const_65536"]["max_string"] == 361 and info["const_65536"]["widths"] == {9, 10}
    assert info["ramp_u16"]["widths"] >= {9, 10, 11}
    # a period of 3 bytes: strings grow by a byte every third code (KwKwK growth), so 12 000 = 3 (1 + ... + k) bytes give k of
    # about 89 and some 270 codes
    assert 80 <= info["period3"]["max_string"] <= 95 and info["period3"]["codes"] < 300
    assert info["noise_70001"]["clears"] >= 17 and len(c["noise_70001"]) > 65536
    # the four ends: the last code is the one after which the next free code is 512 / 1024 / 2048 / 4094
    for free, n in found.items():
        stream = lu.encode(noise[:n])
        assert len(stream) == TAILS[n][1], (n, len(stream))
        i = info[f"tail_{free}"]
        if free == 4094:
            # Clear (12 bits) stands before EOI (9 bits): the inspector's next code is that Clear
            assert not i["eoi"] and i["clears"] == 0 and max(i["widths"]) == 12
            ncodes = i["codes"] - 1                        # without the leading Clear
            bits = 9 + 9 * 254 + 10 * 512 + 11 * 1024 + 12 * (ncodes - 1790) + 12 + 9
            assert ncodes == lu_entries() and len(stream) == (bits + 7) // 8
        else:
            assert i["eoi"] and i["clears"] == 0
            wide = {512: 10, 1024: 11, 2048: 12}[free]
            assert max(i["widths"]) == wide - 1            # every code before EOI is narrower: only EOI has the new width
            # one prefix byte less and EOI keeps the old width
            assert len(lu.encode(noise[:n - 1])) * 8 < len(stream) * 8
    _CORPUS = c
    return c


def lu_entries():
    return 4094 - 258


def noise_strips(count, size, seed0=1000):
    """`count` strips of `size` noise bytes, a different seed each"""
    return [lu._noise(size, seed0 + k) for k in range(count)]


_ENC = {}


def reference(data):
    """``lzw_util.encode(data)``, computed once per strip"""
    data = bytes(data)
    got = _ENC.get(data)
    if got is None:
        got = _ENC[data] = lu.encode(data)
    return got


def pack_align():
    """the alignment of a stream in the packed buffer mi_tiff_lzw_encode_strips_device returns (include/mi_pyramid.h)"""
    return 4


def strips_of_block(level, z0, y0, x0, nz, ny, nx, rps):
    """the raw bytes of every strip of the block level[z0:z0+nz, y0:y0+ny, x0:x0+nx] in (page, strip) order"""
    out = []
    for p in range(nz):
        for r in range(0, ny, rps):
            out.append(np.ascontiguousarray(level[z0 + p, y0 + r:y0 + min(ny, r + rps), x0:x0 + nx]).tobytes())
    return out
