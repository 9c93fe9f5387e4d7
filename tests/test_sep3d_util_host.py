"""CPU: tests/sep3d_util.py on its own -- the float64 reference against scipy and the oracle, the transpose rule, the derived bound
against an fp32 restatement, the exactness of the tap lines, the route table of the cases against the restated launch decision, and
the proof that the GPU test can fail: an offset wrong by one or a reversed line breaks the bound on most voxels of every case."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import rl_oracle as R
from tests import sep3d_util as S

SCIPY_MODE = {S.ZERO: "constant", S.REPLICATE: "nearest", S.CIRCULAR: "wrap"}


def _peak_rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("rule", [S.ZERO, S.REPLICATE, S.CIRCULAR])
@pytest.mark.parametrize("shape,taps", [((9, 8, 12), (5, 3, 7)), ((10, 9, 12), (4, 6, 5)), ((11, 10, 13), (5, 4, 2)), ((7, 7, 8), (1, 1, 3))])
def test_reference_is_scipys_convolution_under_uniform_rules_and_default_shifts(rule, shape, taps):
    """float64 white noise, a dense (not rank-1-looking) check: the reference's three passes against ndimage.convolve of the outer
    product, whose centre k // 2 is moved to the default placement with ``origin``."""
    rng = np.random.default_rng(sum(shape) + 31 * rule)
    k = taps[::-1]
    lines = tuple(rng.standard_normal(kk) for kk in k)
    shifts = S.resolve_shifts(shape, k, None, (rule,) * 3)
    vol = rng.standard_normal(shape)
    psf = lines[2][:, None, None] * lines[1][None, :, None] * lines[0][None, None, :]
    origin = [shifts[2 - ax] - psf.shape[ax] // 2 for ax in range(3)]
    want = ndimage.convolve(vol, psf, mode=SCIPY_MODE[rule], cval=0.0, origin=origin)
    got = S.apply(vol, lines, shifts, (rule,) * 3)
    assert _peak_rel(got, want) < 1e-12
    if rule != S.CIRCULAR:   # the centred placements: origin 0 for zero, -1 on even axes for replicate (conv3d_gpu's centre)
        assert origin == [0 if rule == S.ZERO or kk % 2 else -1 for kk in psf.shape]


@pytest.mark.parametrize("taps", [(5, 3, 7), (4, 6, 5), (2, 4, 3)])
def test_reference_is_the_oracles_convn_same_and_conv3d_replicate(taps):
    """Small integers: every sum is exact in float32, so the oracle's float32 result can be compared to 1e-12."""
    rng = np.random.default_rng(sum(taps))
    shape, k = (9, 10, 12), taps[::-1]
    lines = tuple(rng.integers(1, 4, kk).astype(np.float64) for kk in k)
    vol = rng.integers(0, 4, shape).astype(np.float32)
    psf = S.psf3d(lines)
    for rule, oracle in ((S.ZERO, R.convn_same), (S.REPLICATE, R.conv3d_replicate)):
        got = S.apply(vol.astype(np.float64), lines, S.resolve_shifts(shape, k, None, (rule,) * 3), (rule,) * 3)
        assert np.abs(got - oracle(vol, psf).astype(np.float64)).max() < 1e-12
    # the adjoint of psf_inv = None under these rules is the oracle's convolution with flip3(psf) (decon.m:64)
    for rule, oracle in ((S.ZERO, R.convn_same), (S.REPLICATE, R.conv3d_replicate)):
        shifts = S.resolve_shifts(shape, k, None, (rule,) * 3)
        al, tr = S.adjoint_operator(lines, None, shifts, (rule,) * 3)
        got = S.apply(vol.astype(np.float64), al, shifts, (rule,) * 3, tr)
        assert np.abs(got - oracle(vol, R.flip3(psf)).astype(np.float64)).max() < 1e-12


def test_psf_inv_none_rule():
    """rl_create's reading of psf_inv = None, case by case."""
    assert S.adjoint_kind((5, 3, 7), (2, 1, 3), (0, 1, 2)) == "transpose"          # centred everywhere
    assert S.adjoint_kind((5, 4, 7), (0, 3, 6), (2, 2, 2)) == "transpose"          # skewed, but only on circular axes
    assert S.adjoint_kind((5, 4, 7), (2, 2, 3), (0, 1, 2)) == "flip"               # even extent under replicate: off the transpose
    assert S.adjoint_kind((5, 4, 7), (2, 2, 0), (0, 1, 2)) == "refused"            # ... and a skewed circular axis as well
    lines = (np.arange(1.0, 6.0), np.arange(1.0, 5.0), np.arange(1.0, 8.0))
    got, tr = S.adjoint_operator(lines, None, (2, 2, 3), (0, 1, 2))
    assert not tr and all(np.array_equal(g, w[::-1]) for g, w in zip(got, lines))
    with pytest.raises(ValueError):
        S.adjoint_operator(lines, None, (2, 2, 0), (0, 1, 2))


@pytest.mark.parametrize("name", ["transpose_circular_skew", "transpose_circular_default", "transpose_zero_default", "all_rules_222"])
def test_transpose_identity(name):
    """<A x, y> = <x, A^T y> in float64 where psf_inv = None is the transpose and the rule has one (circular; zero)."""
    s = S.case_setup(name)
    assert s["kind"] == "transpose" and S.REPLICATE not in s["rules"]
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(S.CASES[name]["shape"]), rng.standard_normal(S.CASES[name]["shape"])
    lines, tr = S.adjoint_operator(s["sgn"], None, s["shifts"], s["rules"])
    assert tr
    lhs = float((S.apply(x, s["sgn"], s["shifts"], s["rules"]) * y).sum())
    rhs = float((x * S.apply(y, lines, s["shifts"], s["rules"], True)).sum())
    scale = float((S.apply(np.abs(x), tuple(np.abs(w) for w in s["sgn"]), s["shifts"], s["rules"]) * np.abs(y)).sum())
    assert abs(lhs - rhs) < 1e-12 * scale


def _factor_rank1(p):
    """factor_rank1 (rl.hip) restated: the lines (x, y, z) through the largest sample, in the arithmetic of the host code"""
    kz, ky, kx = p.shape
    z0, y0, x0 = np.unravel_index(int(np.abs(p).argmax()), p.shape)
    p0 = float(p[z0, y0, x0])
    fx = np.array([np.float32(float(p[z0, y0, x])) for x in range(kx)])
    fy = np.array([np.float32(float(p[z0, y, x0]) / p0) for y in range(ky)])
    fz = np.array([np.float32(float(p[z, y0, x0]) / p0) for z in range(kz)])
    return fx, fy, fz


@pytest.mark.parametrize("name", S.case_names())
def test_tap_lines_are_exact_and_asymmetric(name):
    s = S.case_setup(name)
    for lines in (s["pos"], s["sgn"], s["inv_pos"], s["inv_sgn"]):
        if lines is None:
            continue
        for w in lines:
            m = np.abs(w) * 16
            assert np.array_equal(m, np.round(m)) and (np.sort(m)[:-1] <= 31).all() and m.min() >= 1 and m.max() == 32
            assert (np.abs(w) == 2.0).sum() == 1
            assert all(abs(w[j]) != abs(w[len(w) - 1 - j]) for j in range(len(w) // 2))
        exact = lines[2][:, None, None] * lines[1][None, :, None] * lines[0][None, None, :]     # float64
        p = S.psf3d(lines)
        assert np.array_equal(p.astype(np.float64), exact)
        # every product in float32, in both association orders
        x, y, z = (np.asarray(w, np.float32) for w in lines)
        assert np.array_equal((z[:, None, None] * (y[None, :, None] * x[None, None, :])).astype(np.float64), exact)
        # the lines the library extracts multiply back to the PSF exactly, in float32 and in float64
        assert (np.abs(p) == 8.0).sum() == 1
        fx, fy, fz = _factor_rank1(p)
        back = fz.astype(np.float64)[:, None, None] * fy.astype(np.float64)[None, :, None] * fx.astype(np.float64)[None, None, :]
        assert np.array_equal(back, exact)
        for f, w in zip((fx, fy, fz), lines):       # each is the case's line times a signed power of two
            q = f.astype(np.float64) / w
            assert np.all(q == q[0]) and abs(q[0]) in (0.5, 4.0)
    if s["kind"] == "explicit":
        assert not np.array_equal(S.psf3d(s["inv_pos"]), R.flip3(S.psf3d(s["pos"])))


@pytest.mark.parametrize("name", S.case_names())
def test_case_reaches_the_route_its_table_names(name):
    c, s = S.CASES[name], S.case_setup(name)
    for r in S.case_routes(name):
        assert r is not None, "the single-pass kernel does not take this case"
        assert {f: r[f] for f in S.ROUTE_FIELDS} == c["route"]
        assert r["lds_bytes"] <= (S.LDS_ACC_MAX if r["family"] == "acc" else S.LDS_RING_MAX)
    for d in range(3):
        assert 0 <= s["shifts"][d] < s["k"][d]
        assert s["rules"][d] != S.CIRCULAR or s["k"][d] <= c["shape"][2 - d]     # mi_rl_create_ex's own condition
    assert int(np.prod(c["shape"])) < 350_000 and c["shape"][2] % 4 == 0


def test_case_table_covers_what_it_claims():
    names = S.case_names()
    routes = {n: S.case_routes(n) for n in names}
    fam = {(r["family"], r["kzb"], r["npre"]) for n in names for r in routes[n]}
    assert fam >= {("acc", 8, 3), ("acc", 16, 3), ("acc", 32, 3), ("acc", 8, 6), ("ring", 0, 3)}
    # a chunk seam inside the volume for every window size and the ring; a last chunk shorter than the window; both walk parities
    for key in (("acc", 8), ("acc", 16), ("acc", 32), ("ring", 0)):
        assert any(r["chunks"] >= 2 for n in names for r in routes[n] if (r["family"], r["kzb"]) == key), key
    r = routes["acc16_seams"][0]
    assert 47 - (r["chunks"] - 1) * r["zchunk"] == 3 < 11
    r = routes["acc8_even"][0]
    assert {(min(r["zchunk"], 21 - i * r["zchunk"]) + 8 - 1) % 2 for i in range(r["chunks"])} == {0, 1}
    assert all(rr["lds_bytes"] == S.RING_35_LDS for rr in routes["ring_35"]) and S.RING_35_LDS <= S.LDS_RING_MAX < S.RING_35_LDS + 4 * 16 * 64
    # full register windows, every x alignment of the first tap under the register-window kernel
    assert {S.CASES[n]["taps"][0] for n in names} >= {8, 16, 32, 33, 35}
    xoffs = set()
    for n in names:
        s = S.case_setup(n)
        for off in S.window_offsets(s["k"], s["shifts"], s["kind"] == "transpose"):
            xoffs.add(S.xoff(s["k"], off))
    assert xoffs == {0, 1, 2, 3}
    # what psf_inv = None means: the transpose (>= 3 cases, among them uniform circular rules with skewed shifts and centred odd
    # lines under the other two rules), the flipped kernel, an explicit kernel where None is refused; default shifts twice or more
    kinds = [S.case_setup(n)["kind"] for n in names]
    assert kinds.count("transpose") >= 3 and "flip" in kinds and "explicit" in kinds
    s = S.case_setup("transpose_circular_skew")
    assert s["kind"] == "transpose" and all(k - 1 - sh != sh for k, sh in zip(s["k"], s["shifts"]))
    for n, rule in (("transpose_zero_default", S.ZERO), ("transpose_replicate_default", S.REPLICATE)):
        s = S.case_setup(n)
        assert s["kind"] == "transpose" and s["rules"] == (rule,) * 3 and all(k % 2 for k in s["k"])
    assert sum(S.CASES[n]["shift"] is None for n in names) >= 2
    assert {S.CASES["all_rules_%d%d%d" % r]["rules"] for r in np.ndindex(3, 3, 3)} == set(np.ndindex(3, 3, 3))
    assert S.CASES["one_voxel_row"]["shape"] == (1, 1, 4) and S.CASES["acc16_full"]["rules"][0] == S.CIRCULAR


@pytest.mark.parametrize("name", S.case_names())
def test_fp32_restatement_stays_inside_the_bound(name):
    """The same loops in float32 with a separately rounded product and sum per term -- two roundings where the kernels' fmaf has
    one -- and the epilogues in float32: inside the propagated bound on every voxel of every result."""
    s = S.case_setup(name)
    f32 = np.float32
    cf, _ = S.conv_refs(name, "forward", dtype=f32)
    ca, _ = S.conv_refs(name, "adjoint", dtype=f32)
    assert cf.dtype == f32 and ca.dtype == f32
    lam = f32(S.LAMBDA)
    got = {"ratio": s["bl_pos"] / np.maximum(cf, f32(S.EPS)),
           "update": np.abs(s["bl_sgn"] * ca),
           "update_reg": np.abs(s["bl_sgn"] * ca * (f32(1.0) - lam) + s["reg"] * lam)}
    terms = S.sep_terms(s["k"])
    figures = {}
    for what, g in got.items():
        assert g.dtype == f32
        figures[what] = S.worst(g, name, what, terms)
    S.report(f"{name}: fp32 restatement, observed / allowed: " + ", ".join(f"{w} {v:.3f}" for w, v in figures.items()))
    assert max(figures.values()) <= 1.0


# A mutation the geometry of the case cannot show, with the reason; everything else must break the bound on most voxels.
def _invisible(name, which, mutate):
    c, s = S.CASES[name], S.case_setup(name)
    kind, d = mutate
    n, k, rule = c["shape"][2 - d], s["k"][d], s["rules"][d]
    if kind == "reverse" and k == 1:
        return "a one-tap line is its own reverse"
    if n == 1 and rule != S.ZERO:
        return "one sample along the axis under replicate / circular: every tap reads it, whatever the window or the order"
    if n == 1 and kind == "reverse" and k % 2 == 1 and s["shifts"][d] == k // 2:
        return "one sample under the zero rule: only the centre tap of the odd line meets it, before and after the reversal"
    return None


MUTATIONS = [(kind, d) for kind in ("offset", "reverse") for d in range(3)]


@pytest.mark.parametrize("name", S.case_names())
def test_a_wrong_operator_breaks_the_bound(name):
    s = S.case_setup(name)
    lowest = 1.0
    for which in ("forward", "adjoint"):
        ref, B = S.conv_refs(name, which)
        for mutate in MUTATIONS:
            bad, _ = S.conv_refs(name, which, mutate)
            why = _invisible(name, which, mutate)
            if why is not None:
                assert np.abs(bad - ref).max() <= 1e-13 * np.abs(B).max(), (mutate, why)   # the same operator indeed
                continue
            for terms in (S.sep_terms(s["k"]), S.dense_terms(s["k"])):   # the bound of the separable routes, of the dense loop
                frac = float((np.abs(bad - ref) > S.conv_bound(B, terms)).mean())
                lowest = min(lowest, frac)
                assert frac > 0.5, (which, mutate, terms, frac)
    S.report(f"{name}: a window off by one / a reversed line breaks the bound on >= {100 * lowest:.1f} % of the voxels")
