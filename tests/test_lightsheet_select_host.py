"""CPU: the cases of tests/test_gpu_lightsheet_select.py without a device.  The host model of tests/lightsheet_select_util.py (radix
select, row ranking, numpy's lerp) equals ``numpy.percentile`` on every generated window; over the very parametrisation the GPU file
runs, the model's records show that every branch named below is reached; and each seeded mutation of the model fails at least one
case, so the case set is sharp.  No kernel is built or run here, mutated or not.

``r + 1 - equal`` ("reach"): ``r`` counts the equal samples IN FRONT of rank lo, so 0 <= r < equal and the value is never positive.
0 (the equal samples end at rank lo: the sweep runs), -1 (they reach exactly rank lo + 1: the first value at which it must not
run) and below -1 are the three regimes; all three are asserted, and that no case is positive.
"""
import numpy as np
import pytest

from tests import lightsheet_select_util as S
from tests import lightsheet_util as L

MUTATION_SIZES = (2, 3, 65, 257, 1023)
NAMES = [np.dtype(d).name for d in S.DTYPES]


def report(line):
    print("[lightsheet-select] " + line, flush=True)


def per_window(stack, p):
    """numpy.percentile called per window"""
    return np.array([np.percentile(w, 100 * p) for w in stack])


@pytest.mark.parametrize("dtype", NAMES)
def test_model_equals_numpy_percentile(dtype):
    """Both routes of the model, every family, size and percentile.  Up to 257 samples numpy is called per window; above, once per
    stack over the window axis and per window on every seventh one (the two agree: tests/test_lightsheet_host.py)."""
    f32 = dtype == "float32"
    for n in sorted(set(S.BOX_SIZES + S.ROW_LENGTHS)):
        names, stack = S.family_stack(n, dtype)
        for p in S.percentiles_for(n, f32):
            want = per_window(stack, p) if n <= 257 else np.percentile(stack, 100 * p, axis=1)
            if n > 257:
                assert np.array_equal(per_window(stack[::7], p), want[::7])
            for route in ("box", "row"):
                if n > (S.MAX_WINDOW if route == "box" else S.MAX_LENGTH):
                    continue
                got, _ = S.model_percentile(stack, p, route)
                assert got.dtype == want.dtype
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (dtype, n, p, route, names[bad[0]], got[bad[0]], want[bad[0]])


def test_row_ranks_counted_out():
    """The row kernel's comparison, written out pair by pair, is the inverse of the stable sorting permutation the model uses."""
    for dtype in S.DTYPES:
        for n in (1, 2, 63, 64, 65, 257):
            keys = S.to_key(S.family_stack(n, dtype)[1])
            ranks = S.count_ranks(keys)
            assert np.array_equal(np.sort(ranks, axis=1), np.broadcast_to(np.arange(n), ranks.shape))      # a permutation
            for lo in {0, n // 3, n - 1}:
                a, b, _ = S.model_select(keys, lo, min(lo + 1, n - 1), route="row")
                assert np.array_equal(a, np.take_along_axis(keys, (ranks == lo).argmax(axis=1)[:, None], axis=1)[:, 0])
                assert np.array_equal(b, np.take_along_axis(keys, (ranks == min(lo + 1, n - 1)).argmax(axis=1)[:, None], axis=1)[:, 0])


def test_keys_keep_the_order_and_come_back():
    v = np.array([-1e38, -3.25, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 1.17549435e-38, 2.5, 1e38], np.float32)
    k = S.to_key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert np.array_equal(S.from_key(k, np.float32).view(np.uint32), v.view(np.uint32))
    for dt in (np.uint8, np.uint16):
        top = np.iinfo(dt).max
        assert np.array_equal(S.from_key(S.to_key(np.array([0, 1, top], dt)), dt), np.array([0, 1, top], dt))


def test_windows_are_laid_out_as_claimed():
    """A whole-tile stack is one window per tile and a row stack holds the runs where windows (1, L) fall, by the restatement."""
    for n in (2, 63, 64, 4099):
        _, stack = S.family_stack(n, np.uint16)
        tiles, kw = S.whole_tile_stack(stack[:4])
        assert tiles.shape[1] * tiles.shape[2] == n
        for t, row in zip(tiles, stack):
            got = L.percentile_grid(t, 0.5, kw["selem"], kw["spacing"], dtype=np.float64)
            assert got.shape == (1, 1) and got[0, 0] == np.percentile(row, 50)
    for length in (1, 2, 63, 257):
        _, stack = S.family_stack(length, np.float32)
        tiles, index = S.row_stack(stack, length)
        width, per_row, first = S.row_layout(length)
        assert tiles.shape[1:] == (S.ROW_ROWS, width) and (length < 63 or (per_row == S.ROW_CX and first > 0))
        assert (S.ROW_ROWS * per_row) % 4 != 0 or length < 63           # the last work-group has inactive waves
        assert set(index.ravel().tolist()) == set(range(len(stack)))    # every family is in some run
        for t, idx in zip(tiles, index):
            assert np.array_equal(L.row_grid(t, 1 / 3, length), np.percentile(stack[idx], 100 / 3, axis=2))
            assert np.array_equal(L.row_grid(t, 1 / 3, length), L.percentile_grid(t, 1 / 3, (1, length)))


@pytest.fixture(scope="module")
def table():
    return {np.dtype(d).name: S.coverage(d, S.BOX_SIZES) for d in S.DTYPES}


@pytest.mark.parametrize("dtype", NAMES)
def test_cases_reach_every_branch(table, dtype):
    cov = table[dtype]
    assert cov["sweep"] == {False, True}
    assert cov["reach"] == {-2, -1, 0}           # clipped to [-2, 1]: below -1, exactly -1, 0; never positive
    assert all(cov["one_bin"]) and all(m >= 200 for m in cov["many_bins"]), (cov["one_bin"], cov["many_bins"])
    assert cov["coalesced"] == {False, True}
    assert cov["lo_eq_hi"] and cov["g_zero"] and cov["g_low"] and cov["g_high"]
    if dtype == "float32":
        assert cov["negative"] and cov["neg_zero"] and cov["denormal"]


def test_row_cases_select_the_special_floats():
    cov = S.coverage(np.float32, S.ROW_LENGTHS, route="row")
    assert cov["negative"] and cov["neg_zero"] and cov["denormal"] and cov["lo_eq_hi"] and cov["g_zero"] and cov["g_low"] and cov["g_high"]


@pytest.fixture(scope="module")
def caught():
    """{mutation: {dtype: windows of MUTATION_SIZES at which the mutated model differs from numpy.percentile}}"""
    out = {m: {} for m in S.MUTATIONS}
    for dtype in S.DTYPES:
        f32 = np.dtype(dtype) == np.float32
        for n in MUTATION_SIZES:
            _, stack = S.family_stack(n, dtype)
            for p in S.percentiles_for(n, f32):
                want = np.percentile(stack, 100 * p, axis=1)
                for m in S.MUTATIONS:
                    if m == "no_sign" and not f32:
                        continue
                    miss = 0
                    for route in ("box", "row"):
                        if (m, route) in (("sweep_gt", "row"), ("row_le", "box")):
                            continue
                        got, _ = S.model_percentile(stack, p, route, mutation=m)
                        miss += int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
                    out[m][np.dtype(dtype).name] = out[m].get(np.dtype(dtype).name, 0) + miss
    return out


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_mutation_fails_a_case(caught, mutation):
    assert sum(caught[mutation].values()) > 0, caught[mutation]


def test_coverage_table(table, caught):
    report("dtype    windows  sweep taken/not  r+1-equal  bins per pass (min..max)  coalesced  lo==hi g==0 g<.5 g>=.5  neg -0.0 denorm")
    for name, c in table.items():
        bins = " ".join(f"{1 if o else '>1'}..{m}" for o, m in zip(c["one_bin"], c["many_bins"]))
        reach = ",".join({-2: "<-1", -1: "-1", 0: "0", 1: ">0"}[v] for v in sorted(c["reach"]))
        flags = " ".join("yes" if c[k] else "no" for k in ("lo_eq_hi", "g_zero", "g_low", "g_high"))
        special = " ".join("yes" if c[k] else "-" for k in ("negative", "neg_zero", "denormal"))
        report(f"{name:8s} {c['windows']:7d}  {'yes' if True in c['sweep'] else 'no'}/{'yes' if False in c['sweep'] else 'no'}          "
               f"{reach:9s}  {bins:24s}  {'yes/no' if c['coalesced'] == {False, True} else c['coalesced']}     {flags}   {special}")
    report(f"mutations (windows of sizes {MUTATION_SIZES} whose value leaves numpy.percentile), uint8 / uint16 / float32:")
    for m, per in caught.items():
        report(f"  {m:9s} " + " / ".join(str(per.get(n, "n/a")) for n in NAMES))
