"""CPU: the run form of the device TIFF writer through its host yardstick ``mi_tiff_deflate_strip_host`` (include/mi_tiffio.h) -- a
strip's runs of equal bytes as deflate matches at distance 1.  The token rule ("TIFF on the device"): a run's first byte
is a literal; of the R bytes after it, while R >= 3 one match of min(R, 258) bytes; the last 0 - 2 bytes are literals; length 258 is
symbol 285; no match reaches back before the strip."""
import zlib

import numpy as np
import pytest

from tests import deflate_util as du


def _check(data, bps=1, rowb=None, pred=0):
    """the run form of one strip: inflates to the stored bytes, and its tokens are those of the rule"""
    rowb = rowb or len(data)
    stream, used = du.host_strip(data, bps, rowb, pred, 1)
    a = np.frombuffer(data, {1: np.uint8, 2: np.uint16}[bps]).reshape(-1, rowb // bps)
    want = du.stored(a, pred)
    assert zlib.decompress(stream) == want
    tokens, info = du.read_block(stream)
    assert info["bytes"] == want
    lit, _ = du.host_strip(data, bps, rowb, pred, 0)
    assert zlib.decompress(lit) == want
    lit_tokens, lit_info = du.read_block(lit)
    assert lit_tokens == list(want) and lit_info["hlit"] == 257 and lit_info["hdist"] == 2
    if used:
        assert tokens == du.rule_tokens(want) and info["hdist"] == 2
        assert all(t[1] == 1 and t[2] == du.length_symbol(t[0]) for t in tokens if isinstance(t, tuple))
        assert len(stream) < len(lit) or info["bits"] < lit_info["bits"]
    else:                                   # the literal form was not longer: the very same stream
        assert stream == lit
    return tokens, used, stream


@pytest.mark.parametrize("n", du.EQUAL_LENGTHS)
@pytest.mark.parametrize("value", [0, 173])
def test_all_equal_strips(n, value):
    tokens, used, _ = _check(bytes([value]) * n)
    if n >= 262:   # (from some length on the run form must win: a handful of tokens against n literals of at least one bit)
        assert used
    if used:
        r, want = n - 1, [value]
        while r >= 3:
            want.append((min(r, 258), 1, 285 if r >= 258 else du.length_symbol(r)))
            r -= min(r, 258)
        assert tokens == want + [value] * r


def test_length_258_is_symbol_285():
    tokens, used, _ = _check(bytes(259))
    assert used and tokens == [0, (258, 1, 285)]
    tokens, used, _ = _check(bytes(1 + 257) + bytes([9]) * 40)
    assert used and tokens[:2] == [0, (257, 1, 284)]
    tokens, used, _ = _check(bytes(8192 + 259))
    assert used and [t for t in tokens if isinstance(t, tuple) and t[0] == 258 and t[2] != 285] == []


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_concatenated_runs(seed):
    data = du.run_pattern(seed).tobytes()
    tokens, used, _ = _check(data)
    assert used and tokens == du.rule_tokens(data)


def test_differenced_rows_break_the_run_at_every_row_start():
    a = np.full((64, 70), 1234, np.uint16)
    tokens, used, _ = _check(a.tobytes(), bps=2, rowb=140, pred=1)
    assert used
    # a row: the sample (two literals), then 138 zero bytes = literal + match of 137
    assert tokens == [0xD2, 0x04, 0, (137, 1, du.length_symbol(137))] * 64
    b = np.zeros((40, 301), np.uint8)
    b[:, 0] = 5
    b[:, 200:] = 9
    _, used, _ = _check(b.tobytes(), bps=1, rowb=301, pred=1)
    assert used
    rng = np.random.default_rng(5)
    c = (rng.random((30, 211)) > 0.97).astype(np.uint16) * 700
    for pred in (0, 1):
        _, used, _ = _check(c.tobytes(), bps=2, rowb=422, pred=pred)
        assert used


def test_uniform_random_bytes_stay_in_the_literal_form():
    data = np.random.default_rng(9).integers(0, 256, size=200000, dtype=np.uint8).tobytes()
    s1, used = du.host_strip(data, 1, len(data), 0, 1)
    s0, used0 = du.host_strip(data, 1, len(data), 0, 0)
    assert used == 0 and used0 == 0 and s1 == s0 and zlib.decompress(s1) == data


@pytest.mark.parametrize("n", [1 << 16, (1 << 16) + 1, 1 << 20, 2048 * 2 * 256])
def test_zero_strip_size(n):
    """one literal + ceil((n - 1) / 258) matches; at most four literal / length symbols in use, the dominant one of 1 bit, + 1
    distance bit: n / 1032 bytes and a header below 200 bytes -- the bound leaves a factor of two"""
    stream, used = du.host_strip(bytes(n), 1, n, 0, 1)
    assert used and len(stream) <= n / 512 + 512, (n, len(stream))
    assert zlib.decompress(stream) == bytes(n)


def test_invalid_arguments_are_reported():
    import ctypes as C
    from ipp_amd import capi
    out = (C.c_ubyte * 64)()
    n = C.c_size_t(0)
    lib = capi.lib()
    assert lib.mi_tiff_deflate_strip_host(bytes(10), 10, 2, 4, 0, 1, out, 64, C.byref(n), None) != 0     # not whole rows
    assert lib.mi_tiff_deflate_strip_host(bytes(8), 8, 4, 8, 1, 1, out, 64, C.byref(n), None) != 0       # float samples are not differenced
    assert lib.mi_tiff_deflate_strip_host(bytes(100000), 100000, 1, 100000, 0, 0, out, 64, C.byref(n), None) != 0   # out too small
    assert lib.mi_tiff_deflate_strip_host(bytes(10000), 10000, 1, 10000, 0, 1, out, 64, C.byref(n), None) == 0 and n.value <= 64
