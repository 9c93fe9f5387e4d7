"""TEST INFRASTRUCTURE for the two selection kernels of csrc/lightsheet.hip (tests/test_lightsheet_select_host.py,
tests/test_gpu_lightsheet_select.py): crafted windows and a host model of the selection.

Windows.  A stack [count, h, w] run with ``selem=(2h, 2w), spacing=(h, w)`` is ONE box window of exactly h * w samples per tile, so
one launch of ``box_percentile_kernel`` ranks ``count`` crafted multisets (``whole_tile_*``).  A stack [count, rows, pad + 3 L] run
with ``selem=(1, L)`` gives rows * (width // L) runs of ``row_percentile_kernel`` per tile (``row_*``).

Model.  ``model_select`` restates the radix select (the thread-strided histogram with its run coalescing, prefix, ``r``, ``equal``,
the next-key sweep) and the row ranking in numpy, for a whole stack of windows at once, and reports what each window reached.
``model_percentile`` adds ``pct_indices`` / ``pct_value`` (numpy's ``_lerp``) in the data's float type.  The reference of every
test stays ``numpy.percentile``; the model exists to PROVE which branches the cases reach and that the cases are sharp (each seeded
mutation of it fails at least one of them).
"""
from __future__ import annotations

import numpy as np

THREADS = 256                      # kThreads of csrc/lightsheet.hip
MAX_WINDOW, MAX_LENGTH = 16384, 4096
PERCENTILES = (0.0, 1.0, 0.5, 0.25, 0.75, 1 / 3, 2 / 3, 0.03, 0.999, 1e-9)
BOX_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4099, 16384)
ROW_LENGTHS = (1, 2, 63, 64, 65, 256, 257, 1000, 4096)
ROW_ROWS, ROW_CX, ROW_PAD = 3, 3, 5
DTYPES = (np.uint8, np.uint16, np.float32)
MUTATIONS = ("sweep_gt", "row_le", "no_sign", "hi_eq_lo", "no_half")
# sweep_gt  `r + 1 > equal` in place of `>=`          row_le    the row tie-break `j <= idx` in place of `<`
# no_sign   to_key without the sign branch            hi_eq_lo  `hi = lo` always          no_half   the `g >= 0.5` form dropped


def passes_of(dtype):
    return {1: 1, 2: 2, 4: 4}[np.dtype(dtype).itemsize]


# ---------------------------------------------------------------------------------------------------------------------------------
# keys, indices, the lerp: make_pct, pct_indices, pct_value, to_key, from_key of csrc/lightsheet.hip

def to_key(values, mutation=None):
    """Order-preserving uint32 keys: integers as they are; floats with the sign bit flipped, negative ones wholly inverted."""
    values = np.asarray(values)
    if values.dtype != np.float32:
        return values.astype(np.uint32)
    b = values.view(np.uint32)
    if mutation == "no_sign":
        return b ^ np.uint32(0x80000000)
    return np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def from_key(keys, dtype, mutation=None):
    keys = np.asarray(keys, np.uint32)
    if np.dtype(dtype) != np.float32:
        return keys.astype(dtype)
    if mutation == "no_sign":
        return (keys ^ np.uint32(0x80000000)).view(np.float32)
    return np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32).view(np.float32)


def virtual_index(n, p, f32):
    """(n - 1) * q with q = (100 p) / 100, in float32 for float32 data and in float64 for integers."""
    hundred_p = 100.0 * float(p)
    if f32:
        return np.float32(n - 1) * (np.float32(hundred_p) / np.float32(100))
    return np.float64(n - 1) * np.float64(hundred_p / 100.0)


def pct_indices(n, p, f32, mutation=None):
    """(lo, hi, g): the two order statistics and the weight of the second."""
    v = virtual_index(n, p, f32)
    f = int(np.floor(v))
    if v >= n - 1 or f >= n - 1:
        return n - 1, n - 1, type(v)(0)
    lo = max(f, 0)
    return lo, (lo if mutation == "hi_eq_lo" else lo + 1), v - np.floor(v)


def pct_value(a, b, g, f32, mutation=None):
    """numpy's _lerp on arrays a, b of samples: a + (b - a) g, and b - (b - a) (1 - g) from g = 0.5 on."""
    ft = np.float32 if f32 else np.float64
    a, b, g = np.asarray(a).astype(ft), np.asarray(b).astype(ft), ft(g)
    d = b - a
    out = a + d * g
    if g >= 0.5 and mutation != "no_half":
        out = b - d * (ft(1) - g)
    return out


def whole_p(n, f32):
    """A percentile strictly inside (0, 1) at which (n - 1) * p is a whole number in the data's arithmetic (g == 0 with lo < n - 1),
    nearest the middle; None for n < 3."""
    best = None
    for k in range(1, n - 1):
        p = k / (n - 1)
        v = virtual_index(n, p, f32)
        if v == np.floor(v) and 0 < v < n - 1 and (best is None or abs(k - (n - 1) / 2) < abs(best[0] - (n - 1) / 2)):
            best = (k, p)
        if best is not None and k > (n - 1) / 2 + abs(best[0] - (n - 1) / 2):
            break
    return None if best is None else best[1]


def percentiles_for(n, f32):
    extra = whole_p(n, f32)
    return PERCENTILES + ((extra,) if extra is not None and extra not in PERCENTILES else ())


# ---------------------------------------------------------------------------------------------------------------------------------
# the model

def _box_select(keys, lo, hi, passes, mutation):
    """box_percentile_kernel on every row of keys[C, n]: (key of statistic lo, key of statistic hi, record)."""
    C, n = keys.shape
    rows = np.arange(C)[:, None]
    steps = -(-n // THREADS)
    padded = np.zeros((C, steps * THREADS), np.uint32)
    padded[:, :n] = keys
    live = (np.arange(steps * THREADS) < n).reshape(steps, THREADS)
    padded = padded.reshape(C, steps, THREADS)
    prefix = np.zeros(C, np.uint32)
    r = np.full(C, lo, np.int64)
    equal = np.zeros(C, np.int64)
    bins = np.zeros((C, passes), np.int64)
    coalesced = np.zeros(C, bool)
    for pi, pas in enumerate(range(passes - 1, -1, -1)):
        shift = 8 * pas
        hist = np.zeros((C, 256), np.int64)
        cur = np.full((C, THREADS), -1, np.int64)
        run = np.zeros((C, THREADS), np.int64)
        for s in range(steps):                      # thread t walks i = t, t + 256, ...
            k = padded[:, s]
            match = np.broadcast_to(live[s], k.shape).copy()
            if pas != passes - 1:
                match &= (k >> np.uint32(shift + 8)) == prefix[:, None]
            b = ((k >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
            change = match & (b != cur)
            flush = change & (run > 0)
            coalesced |= (flush & (run > 1)).any(axis=1)
            np.add.at(hist, (np.broadcast_to(rows, cur.shape)[flush], cur[flush]), run[flush])
            cur = np.where(change, b, cur)
            run = np.where(change, 0, run) + match
        flush = run > 0
        coalesced |= (flush & (run > 1)).any(axis=1)
        np.add.at(hist, (np.broadcast_to(rows, cur.shape)[flush], cur[flush]), run[flush])
        incl = np.cumsum(hist, axis=1)
        holds = (hist > 0) & (incl - hist <= r[:, None]) & (r[:, None] < incl)
        assert (holds.sum(axis=1) == 1).all()       # exactly one bin holds rank r
        sbin = holds.argmax(axis=1)
        prefix = (prefix << np.uint32(8)) | sbin.astype(np.uint32)
        r = r - (incl - hist)[np.arange(C), sbin]
        equal = hist[np.arange(C), sbin]
        bins[:, pi] = (hist > 0).sum(axis=1)
    reach = r + 1 - equal
    sweep = (reach > 0) if mutation == "sweep_gt" else (reach >= 0)
    sweep &= hi != lo
    larger = np.where(keys > prefix[:, None], keys, np.uint32(0xFFFFFFFF)).min(axis=1)
    nxt = np.where(sweep, larger, prefix)
    return prefix, nxt, dict(bins=bins, coalesced=coalesced, sweep=sweep, reach=reach)


def _row_select(keys, lo, hi, mutation):
    """row_percentile_kernel: a key's rank is the count of smaller keys plus the equal keys in front of it, so the ranks are the
    inverse of the stable sorting permutation (tests/test_lightsheet_select_host.py counts them out for short runs)."""
    C, n = keys.shape
    cnt = np.empty((C, n), np.int64)
    np.put_along_axis(cnt, np.argsort(keys, axis=1, kind="stable"), np.broadcast_to(np.arange(n), (C, n)), axis=1)
    if mutation == "row_le":
        cnt = cnt + 1                                # `j <= idx` counts the key itself as well
    sel = np.zeros((C, 2), np.uint32)                # a rank that no lane holds leaves the slot as it was
    for slot, want in ((0, lo), (1, hi)):
        hit = cnt == want
        sel[:, slot] = np.where(hit.any(axis=1), np.take_along_axis(keys, hit.argmax(axis=1)[:, None], axis=1)[:, 0], sel[:, slot])
    return sel[:, 0], sel[:, 1]


def count_ranks(keys):
    """The row kernel's comparison written out: rank[i] = #{j: k[j] < k[i] or (k[j] == k[i] and j < i)} for keys[C, n], n small."""
    k = keys.astype(np.int64)
    j = np.arange(k.shape[1])
    return ((k[:, None, :] < k[:, :, None]) | ((k[:, None, :] == k[:, :, None]) & (j[None, None, :] < j[None, :, None]))).sum(axis=2)


def model_select(keys, lo, hi, passes=4, route="box", mutation=None):
    """The selection of one route on keys[C, n] (or one window keys[n]): (sample key of statistic lo, of statistic hi, record).
    The record of the box route holds per window: ``bins`` occupied bins per pass (most significant byte first), ``coalesced``
    whether a thread-strided run of equal bins was added in one atomicAdd, ``sweep`` whether the next-key sweep ran, ``reach``
    ``r + 1 - equal`` (0: the equal samples end AT rank lo; -1: they reach exactly rank lo + 1; below: further; never above 0,
    since r counts equal samples in front of rank lo)."""
    keys = np.asarray(keys, np.uint32)
    single = keys.ndim == 1
    k2 = keys[None] if single else keys
    if route == "row":
        a, b = _row_select(k2, lo, hi, mutation)
        rec = {}
    else:
        a, b, rec = _box_select(k2, lo, hi, passes, mutation)
    if single:
        return a[0], b[0], {k: v[0] for k, v in rec.items()}
    return a, b, rec


def model_percentile(samples, p, route="box", mutation=None):
    """The kernels' whole computation on samples[C, n] of one dtype: (values in the data's float type, record of model_select with
    ``lo``, ``hi``, ``g``, and the selected samples ``a``, ``b``)."""
    samples = np.asarray(samples)
    dtype, f32 = samples.dtype, samples.dtype == np.float32
    n = samples.shape[-1]
    lo, hi, g = pct_indices(n, p, f32, mutation)
    ka, kb, rec = model_select(to_key(samples, mutation), lo, hi, passes_of(dtype), route, mutation)
    a, b = from_key(ka, dtype, mutation), from_key(kb, dtype, mutation)
    with np.errstate(all="ignore"):
        value = a.astype(np.float32 if f32 else np.float64) if virtual_index(n, p, f32) >= n - 1 else pct_value(a, b, g, f32, mutation)
    return value, dict(rec, lo=lo, hi=hi, g=g, a=a, b=b)


# ---------------------------------------------------------------------------------------------------------------------------------
# sample families

def generic_samples(rng, n, dtype):
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(n) * 1000).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, n).astype(dtype)


def _f32_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _byte_only(rng, n, byte, base):
    """float32 samples whose bit patterns differ in one byte only.  The highest byte holds the sign and seven exponent bits: all
    but the two patterns of the top exponents (infinities, NaNs and finite values past 1e38) are used."""
    if byte == 3:
        tops = np.array([t for t in range(256) if (t & 0x7F) != 0x7F], np.uint32)
        vary = tops[rng.integers(0, len(tops), n)]
    else:
        vary = rng.integers(0, 256, n).astype(np.uint32)
    return _f32_bits((np.uint32(base) & ~np.uint32(0xFF << (8 * byte))) | (vary << np.uint32(8 * byte)))


def family_rows(n, dtype, seed=0):
    """[(name, samples[n])] of every family of one dtype at window size n; the tie families once per rank ``lo`` that the
    percentiles of this n reach."""
    dt = np.dtype(dtype)
    f32 = dt == np.float32
    rng = np.random.default_rng([seed, n, dt.itemsize])
    out = []
    top = None if f32 else np.iinfo(dt).max
    for name, v in (("const", -2.5 if f32 else 7), ("const_zero", 0), ("const_top", 1e38 if f32 else top)):
        out.append((name, np.full(n, v, dt)))
    los = sorted({pct_indices(n, p, f32)[0] for p in percentiles_for(n, f32)})
    a, c, b = {1: (3, 4, 200), 2: (0x12FF, 0x1300, 0xC805), 4: (-0.75, 2.5, 2.5000002)}[dt.itemsize]
    if n >= 2:      # two values a < b with exactly m copies of a
        for m in sorted({min(max(lo + d, 1), n - 1) for lo in los for d in (-1, 0, 1, 2)} | {n - 1}):
            row = np.full(n, b, dt)
            row[rng.permutation(n)[:m]] = a
            out.append((f"two_m{m}", row))
    if n >= 3:      # three values, the middle one once, at rank m: lo, lo + 1, or neither
        for m in sorted({min(max(lo + d, 0), n - 1) for lo in los for d in (0, 1, 3)}):
            row = np.full(n, b, dt)
            order = rng.permutation(n)
            row[order[:m]] = a
            row[order[m]] = c
            out.append((f"three_m{m}", row))
    g = generic_samples(rng, n, dt)
    out += [("ascending", np.sort(g)), ("descending", np.sort(g)[::-1].copy()), ("shuffled", g)]
    if dt == np.uint8:
        out.append(("0_255", (rng.integers(0, 2, n) * 255).astype(dt)))
    elif dt == np.uint16:
        out.append(("0_65535", (rng.integers(0, 2, n) * 65535).astype(dt)))
        out.append(("uniform", generic_samples(rng, n, dt)))
        out.append(("high_equal", (0x5A00 | rng.integers(0, 256, n)).astype(dt)))
        out.append(("low_equal", ((rng.integers(0, 256, n) << 8) | 0xA5).astype(dt)))
    else:
        out.append(("normal_1000", generic_samples(rng, n, dt)))
        out.append(("denormal", (rng.standard_normal(n) * 1e-38).astype(dt)))
        out.append(("pow2", (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-100, 101, n))).astype(dt)))
        out.append(("zeros", rng.choice(np.array([-1.5, -0.0, 0.0, 3.25], dt), n)))
        out.append(("huge", (rng.choice([-1.0, 1.0], n) * rng.uniform(1e37, 1e38, n)).astype(dt)))
        out.append(("negative", (-np.abs(rng.standard_normal(n) * 1000) - 1).astype(dt)))
        for byte in range(4):
            out.append((f"byte{byte}_pos", _byte_only(rng, n, byte, 0x4225C33B)))
            out.append((f"byte{byte}_neg", _byte_only(rng, n, byte, 0xC225C33B)))
    for name, row in out:
        assert row.dtype == dt and row.shape == (n,), name
        if f32:
            assert np.isfinite(row).all() and (np.abs(row) <= 1e38).all(), name
    return out


def family_stack(n, dtype, seed=0):
    """(names, samples[count, n])"""
    rows = family_rows(n, dtype, seed)
    return [r[0] for r in rows], np.stack([r[1] for r in rows])


# ---------------------------------------------------------------------------------------------------------------------------------
# windows

def whole_tile_shape(n):
    """(h, w) with h * w == n: one row for an odd n (and for 2), else the most square split."""
    if n % 2 or n == 2:
        return 1, n
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def whole_tile_stack(samples):
    """samples[count, n] -> (tiles[count, h, w], keywords of local_percentile that make each tile one window)"""
    h, w = whole_tile_shape(samples.shape[1])
    return samples.reshape(-1, h, w), dict(selem=(2 * h, 2 * w), spacing=(h, w))


def row_layout(L, cx=ROW_CX, pad=ROW_PAD):
    """(width, runs per row, first sample of the first run) of a row of pad + cx * L samples under windows (1, L)"""
    width = pad + cx * L
    n = width // L
    left = (width - (n - 1) * L) // 2
    return width, n, left - L // 2


def row_stack(samples, L, rows=ROW_ROWS, seed=0):
    """samples[count, L] laid out as the runs of tiles [tiles, rows, width], the last tile filled up by repeating the first runs;
    everything outside the runs holds other samples.  Returns (tiles, index[tiles, rows, runs per row] into samples)."""
    width, per_row, first = row_layout(L)
    per_tile = rows * per_row
    tiles = -(-samples.shape[0] // per_tile)
    index = (np.arange(tiles * per_tile) % samples.shape[0]).reshape(tiles, rows, per_row)
    rng = np.random.default_rng([seed, L, 77])
    out = np.stack([generic_samples(rng, rows * width, samples.dtype).reshape(rows, width) for _ in range(tiles)])
    out[:, :, first:first + per_row * L] = samples[index].reshape(tiles, rows, per_row * L)
    return out, index


def coverage(dtype, sizes, route="box", seed=0):
    """What the cases of one dtype reach on the model, over all sizes, families and percentiles (the table of the host test)."""
    f32 = np.dtype(dtype) == np.float32
    passes = passes_of(dtype)
    cov = dict(sweep=set(), reach=set(), one_bin=[False] * passes, many_bins=[0] * passes, coalesced=set(), lo_eq_hi=False, g_zero=False,
               g_low=False, g_high=False, negative=False, neg_zero=False, denormal=False, windows=0)
    for n in sizes:
        _, stack = family_stack(n, dtype, seed)
        for p in percentiles_for(n, f32):
            _, rec = model_percentile(stack, p, route)
            cov["windows"] += len(stack)
            cov["lo_eq_hi"] |= rec["lo"] == rec["hi"]
            inner = rec["lo"] != rec["hi"]
            cov["g_zero"] |= inner and rec["g"] == 0
            cov["g_low"] |= inner and 0 < rec["g"] < 0.5
            cov["g_high"] |= inner and rec["g"] >= 0.5
            if f32:
                for s in (rec["a"], rec["b"]):
                    cov["negative"] |= bool((s < 0).any())
                    cov["neg_zero"] |= bool(((s == 0) & np.signbit(s)).any())
                    cov["denormal"] |= bool(((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny)).any())
            if route == "box":
                cov["sweep"] |= set(rec["sweep"].tolist())
                cov["reach"] |= set(np.clip(rec["reach"], -2, 1).tolist())
                cov["coalesced"] |= set(rec["coalesced"].tolist())
                for i in range(passes):
                    cov["one_bin"][i] |= bool((rec["bins"][:, i] == 1).any())
                    cov["many_bins"][i] = max(cov["many_bins"][i], int(rec["bins"][:, i].max()))
    return cov
