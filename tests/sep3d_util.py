"""Plain float64 reference of the direct RL engine's rank-1 convolution with its epilogues (csrc/sep3d.hip, and the routes of
csrc/conv3d_direct.hip that serve the same PSFs), the derived error bound, and the cases of tests/test_gpu_sep3d_operator.py with
the kernel build each one is meant to reach.  numpy only: importable without a GPU.

Operator, at the level of mi_rl_create_ex (include/mi_lsdeconv.h), one axis at a time -- x, then y, then z -- with ``rule`` one of
zero / replicate / circular applied to the source index:
  forward                          out[i] = sum_j in[rule(i - j + shift)] psf[j]
  adjoint, explicit psf_inv        the same formula with psf_inv
  adjoint, psf_inv = None          the transpose  out[i] = sum_j in[rule(i + j - shift)] psf[j]  -- unless a NON-circular axis has
                                   k - 1 - shift != shift: then None stands for the explicit kernel flip3(psf) (rl.hip, rl_create),
                                   which rl_create refuses when a circular axis is skewed as well.
Epilogues, eps = 2^-23:  ratio a / max(c, eps);  update |a c|;  regularised update |a c (1 - l) + b l|.

Inputs.  Volumes are seeded white noise.  Tap lines are seeded, strictly asymmetric (w[j] != w[k-1-j] for every j off the middle)
and dyadic: every tap is m / 16 with m in 1 .. 31, and ONE tap per line is raised to exactly 2.  The PSF a_z b_y c_x then has one
largest sample, 8, every fp32 product is exact (three 5- or 6-bit integers), and the three lines that factor_rank1 (rl.hip) takes
through that sample are c * 4, b / 2, a / 2 up to sign: exact, so the kernels convolve with exactly this operator.  The signed
variant gives every tap a random sign.

Bound (derived, not measured).  A 1-D sum of k terms accumulated with fmaf is within k 2^-24 of sum |in| |w| of its exact value
(first order); three nested sums, each rounded to fp32, give (kx + ky + kz) 2^-24 B with B = conv(|in|, |w|), and three more
roundings are allowed for the factor lines: per voxel
      |c_got - c_ref| <= t = (kx + ky + kz + 3) 2^-24 B.
The dense tap loop (MI_NO_SEPARABLE=1) is ONE sum of kxp ky kz terms: t = (kxp ky kz + 3) 2^-24 B, kxp = kx rounded up to 4.
Through the epilogues, in float64:
      ratio     |a| t / (c_ref (c_ref - t)) + 2^-23 |ref|          (inputs positive: c_ref is far above t)
      updates   |a| t |1 - l| + 4 2^-24 (|a c (1 - l)| + |b l|)    (the roundings of a c, (1 - l), b l and the sum)
tests/test_sep3d_util_host.py holds an fp32 restatement with TWO roundings per term (harsher than fmaf) to this bound on every case
and shows that an offset wrong by one or a reversed line breaks it on most voxels.
"""
import functools
import itertools

import numpy as np

ZERO, REPLICATE, CIRCULAR = 0, 1, 2
EPS = 2.0 ** -23
U = 2.0 ** -24
LAMBDA = float(np.float32(0.3))   # the regularised update's weight as the kernel receives it


# ------------------------------------------------------------------ the reference
def default_shift(n, k, rule):
    """PSF placement of one axis when shift_xyz is None (rl.hip, default_shift)."""
    if rule == CIRCULAR:
        return n // 2 - (n - k) // 2          # ifftshift(zero-pad-centre(psf))
    return (k - 1) // 2 if rule == REPLICATE else k // 2   # conv3d_gpu's centre / convn 'same'


def resolve_shifts(shape_zyx, k_xyz, shift_xyz, rules_xyz):
    n_xyz = shape_zyx[::-1]
    return tuple(default_shift(n_xyz[d], k_xyz[d], rules_xyz[d]) if shift_xyz is None else int(shift_xyz[d]) for d in range(3))


def _index(i, n, rule):
    """source index under a rule, and where the sample exists (None: everywhere)"""
    if rule == REPLICATE:
        return np.clip(i, 0, n - 1), None
    if rule == CIRCULAR:
        return np.mod(i, n), None
    return np.clip(i, 0, n - 1), (i >= 0) & (i < n)


def conv_axis(a, w, shift, rule, axis, transpose=False, dtype=np.float64):
    """One 1-D pass along numpy axis ``axis``; the terms are added in window order (rising source index).  ``dtype=np.float32``
    rounds every product and every sum: two roundings per term."""
    n, k = a.shape[axis], len(w)
    i = np.arange(n)
    bshape = [1, 1, 1]
    bshape[axis] = n
    src = a.astype(dtype)
    acc = np.zeros(a.shape, dtype)
    for j in (range(k) if transpose else range(k - 1, -1, -1)):
        idx, ok = _index(i + j - shift if transpose else i - j + shift, n, rule)
        v = np.take(src, idx, axis=axis)
        if ok is not None:
            v = v * ok.reshape(bshape).astype(dtype)
        acc = acc + v * dtype(w[j])
    return acc


def apply(vol, lines_xyz, shifts_xyz, rules_xyz, transpose=False, dtype=np.float64):
    """The rank-1 operator on ``vol`` (z, y, x): x, then y, then z."""
    out = vol
    for d in range(3):
        out = conv_axis(out, lines_xyz[d], shifts_xyz[d], rules_xyz[d], 2 - d, transpose, dtype)
    return out


def adjoint_kind(k_xyz, shifts_xyz, rules_xyz):
    """What psf_inv = None means to rl_create: "transpose", "flip" (the explicit kernel flip3(psf)) or "refused"."""
    skew = [k_xyz[d] - 1 - shifts_xyz[d] != shifts_xyz[d] for d in range(3)]
    off_transpose = any(skew[d] and rules_xyz[d] != CIRCULAR for d in range(3))
    circular_skew = any(skew[d] and rules_xyz[d] == CIRCULAR for d in range(3))
    if not off_transpose:
        return "transpose"
    return "refused" if circular_skew else "flip"


def adjoint_operator(lines_xyz, inv_lines_xyz, shifts_xyz, rules_xyz):
    """(lines, transpose) of the adjoint convolution: ``inv_lines_xyz`` is the explicit psf_inv or None."""
    if inv_lines_xyz is not None:
        return inv_lines_xyz, False
    kind = adjoint_kind([len(w) for w in lines_xyz], shifts_xyz, rules_xyz)
    if kind == "refused":
        raise ValueError("psf_inv = None is ambiguous here (mi_rl_create_ex refuses it)")
    if kind == "flip":
        return tuple(w[::-1] for w in lines_xyz), False
    return lines_xyz, True


def ratio_ref(a, c):
    return a / np.maximum(c, EPS)


def update_ref(a, c, lam=0.0, b=None):
    return np.abs(a * c) if b is None else np.abs(a * c * (1.0 - lam) + b * lam)


# ------------------------------------------------------------------ the bound
def sep_terms(k_xyz):
    return k_xyz[0] + k_xyz[1] + k_xyz[2] + 3


def dense_terms(k_xyz):
    return (k_xyz[0] + 3) // 4 * 4 * k_xyz[1] * k_xyz[2] + 3


def conv_bound(B, terms):
    return terms * U * B


def ratio_bound(a, c, t):
    assert (c - t > 0).all(), "the ratio bound needs c_ref above its own error"
    return np.abs(a) * t / (c * (c - t)) + 2.0 ** -23 * np.abs(ratio_ref(a, c))


def update_bound(a, c, t, lam=0.0, b=None):
    blend = 0.0 if b is None else np.abs(b * lam)
    return np.abs(a) * t * abs(1.0 - lam) + 4 * U * (np.abs(a * c * (1.0 - lam)) + blend)


# ------------------------------------------------------------------ the route decision of sep3d_launch, restated
SF_TX, SF_TY, SF_THREADS, MAX_TAPS = 64, 16, 256, 51
LDS_ACC_MAX, LDS_RING_MAX = 64 * 1024, 150 * 1024


def _xhalo(k, c):
    return (c[0] + 3) // 4, (k[0] - 1 - c[0] + 3) // 4      # float4 left / right of the 64-wide tile


def xoff(k, c):
    """staged column of an output's first x tap: 4 cql - cx"""
    return 4 * _xhalo(k, c)[0] - c[0]


def lds_ring(k, c):
    cql, cqr = _xhalo(k, c)
    seg, rows = 4 * (SF_TX // 4 + cql + cqr), SF_TY + k[1] - 1
    return 4 * (rows * seg + rows * SF_TX + k[2] * SF_TY * SF_TX)


def lds_acc(k, c):
    cql, cqr = _xhalo(k, c)
    seg, rows = 4 * (SF_TX // 4 + cql + cqr), SF_TY + k[1] - 1
    kyp = (k[1] + 3) & ~3
    nxc = (4 * cql - c[0] + k[0] + 6) // 4
    return 4 * (rows * seg + (SF_TY + kyp - 1) * SF_TX + 4 * nxc + 4 + kyp)


def patch_quads(k, c):
    cql, cqr = _xhalo(k, c)
    return (SF_TY + k[1] - 1) * (SF_TX // 4 + cql + cqr)


def fits(nx, k, c):
    if any(kk < 1 or kk > MAX_TAPS or cc < 0 or cc >= kk for kk, cc in zip(k, c)):
        return False
    lds_ok = lds_acc(k, c) <= LDS_ACC_MAX if k[2] <= 32 else lds_ring(k, c) <= LDS_RING_MAX
    return nx % 4 == 0 and lds_ok and patch_quads(k, c) <= 6 * SF_THREADS


def route(n_xyz, k_xyz, off_xyz):
    """What ``RLContext.sep_route`` reports for window offsets ``off_xyz`` (None: the single-pass kernel does not take it)."""
    nx, ny, nz = n_xyz
    k, c = list(k_xyz), list(off_xyz)
    if not fits(nx, k, c):
        return None
    tiles_xy = ((nx + SF_TX - 1) // SF_TX) * ((ny + SF_TY - 1) // SF_TY)
    zc = max(64, 8 * k[2])
    while zc > 2 * k[2] and zc > 16 and tiles_xy * ((nz + zc - 1) // zc) < 1024:
        zc //= 2
    zc = min(zc, nz)
    acc = k[2] <= 32
    return {"family": "acc" if acc else "ring", "kzb": (8 if k[2] <= 8 else 16 if k[2] <= 16 else 32) if acc else 0,
            "npre": 6 if patch_quads(k, c) > 3 * SF_THREADS else 3, "zchunk": zc, "chunks": (nz + zc - 1) // zc,
            "lds_bytes": lds_acc(k, c) if acc else lds_ring(k, c)}


def window_offsets(k_xyz, shifts_xyz, adjoint_transposed):
    """(off_fwd, off_adj) of a context: the window starts k - 1 - shift before the output sample, the transpose's ``shift``."""
    fwd = tuple(k - 1 - s for k, s in zip(k_xyz, shifts_xyz))
    return fwd, (tuple(shifts_xyz) if adjoint_transposed else fwd)


# ------------------------------------------------------------------ the cases
ROUTE_FIELDS = ("family", "kzb", "npre", "zchunk", "chunks")


def _case(shape, taps_zyx, shift_xyz, rules_xyz, route_):
    return {"shape": shape, "taps": taps_zyx, "shift": shift_xyz, "rules": rules_xyz, "route": dict(zip(ROUTE_FIELDS, route_))}


# name -> shape (z, y, x), taps (z, y, x), shift (x, y, z) or None for the defaults, rules (x, y, z),
#         route: family, KZB, NPRE, planes of a z chunk, chunks -- the same for the forward and the adjoint launch
CASES = {
    # 3 chunks of 16 / 16 / 5; second x tile of one quad; ragged y tile
    "acc8_seams": _case((37, 19, 68), (5, 3, 7), (0, 2, 1), (2, 0, 1), ("acc", 8, 3, 16, 3)),
    # the 8-plane window full, an even count; 2 chunks of 16 / 5; walks of 23 and 12 planes: both parities
    "acc8_even": _case((21, 17, 64), (8, 4, 6), (5, 0, 7), (1, 2, 0), ("acc", 8, 3, 16, 2)),
    # 3 chunks of 22 / 22 / 3: the last one shorter than the window
    "acc16_seams": _case((47, 18, 68), (11, 5, 9), (8, 4, 0), (0, 1, 2), ("acc", 16, 3, 22, 3)),
    # the 16-plane window full; circular x of 8 under a 64-wide tile: the staged row wraps nine times
    "acc16_full": _case((36, 5, 8), (16, 3, 4), (0, 1, 15), (2, 2, 1), ("acc", 16, 3, 32, 2)),
    "acc32_19": _case((41, 17, 68), (19, 5, 7), (3, 2, 9), (1, 0, 2), ("acc", 32, 3, 38, 2)),
    # the 32-plane window full; z shift at its end
    "acc32_full": _case((67, 3, 12), (32, 2, 3), (1, 1, 31), (0, 2, 0), ("acc", 32, 3, 64, 2)),
    # one-tap x and y lines; nx = 4; 2 chunks of 34 / 6
    "acc32_zonly": _case((40, 16, 4), (17, 1, 1), (0, 0, 16), (1, 1, 1), ("acc", 32, 3, 34, 2)),
    "ring_33": _case((69, 17, 68), (33, 3, 5), (2, 1, 16), (2, 1, 0), ("ring", 0, 3, 66, 2)),
    # the ring kernel at its LDS limit (152 864 B of 153 600); z shift at the window's end
    "ring_35": _case((73, 5, 8), (35, 3, 3), (0, 2, 34), (1, 0, 2), ("ring", 0, 3, 70, 2)),
    # patches of 864 and 1008 quads: six per thread
    "wide_33": _case((19, 50, 72), (5, 33, 9), (4, 16, 2), (0, 2, 1), ("acc", 8, 6, 16, 2)),
    "wide_41": _case((9, 45, 8), (3, 41, 3), (1, 40, 0), (2, 1, 0), ("acc", 8, 6, 9, 1)),
    # the longest x window at both ends of its offset; three x tiles
    "kx51_lo": _case((7, 9, 132), (3, 3, 51), (50, 1, 1), (1, 0, 1), ("acc", 8, 3, 7, 1)),
    "kx51_hi": _case((7, 9, 132), (3, 3, 51), (0, 1, 1), (0, 2, 0), ("acc", 8, 3, 7, 1)),
    # nz = ny = 1, nx = 4: every sample resolved by a rule
    "one_voxel_row": _case((1, 1, 4), (5, 3, 3), (1, 1, 2), (1, 0, 1), ("acc", 8, 3, 1, 1)),
    # fewer planes than z taps; x window wider than the row
    "fewer_planes": _case((3, 33, 4), (11, 5, 7), (3, 2, 5), (0, 1, 0), ("acc", 16, 3, 3, 1)),
    # psf_inv = None as the pure transpose: circular axes with skewed shifts; centred odd lines under the other two rules with the
    # default placement; the circular default placement (skewed for these extents)
    "transpose_circular_skew": _case((21, 18, 68), (6, 4, 7), (1, 3, 0), (2, 2, 2), ("acc", 8, 3, 16, 2)),
    "transpose_zero_default": _case((20, 19, 68), (7, 5, 9), None, (0, 0, 0), ("acc", 8, 3, 16, 2)),
    "transpose_replicate_default": _case((23, 17, 8), (9, 3, 5), None, (1, 1, 1), ("acc", 16, 3, 18, 2)),
    "transpose_circular_default": _case((12, 10, 16), (5, 4, 3), None, (2, 2, 2), ("acc", 8, 3, 12, 1)),
    # short lines: the PSF sums to less than 2^7, so a volume of 2^-30 drives max(c, eps) to the clamp everywhere
    "clamp_small_taps": _case((20, 17, 68), (3, 2, 2), None, (1, 2, 0), ("acc", 8, 3, 16, 2)),
}
# one geometry under all 27 rule triples: x and y skewed, z centred -- the transpose (x and y circular), the flipped kernel (neither)
# and an explicit adjoint kernel (one of them)
for _r in itertools.product((0, 1, 2), repeat=3):
    CASES["all_rules_%d%d%d" % _r] = _case((13, 21, 72), (5, 4, 6), (4, 0, 2), _r, ("acc", 8, 3, 13, 1))

RING_35_LDS = 152864


def case_names():
    return sorted(CASES)


def _line(rng, k):
    """k dyadic taps m / 16, strictly asymmetric, one of them raised to 2"""
    while True:
        w = rng.integers(1, 32, k).astype(np.float64) / 16.0
        if all(w[j] != w[k - 1 - j] for j in range(k // 2)):
            break
    w[int(rng.integers(0, k))] = 2.0
    return w


def psf3d(lines_xyz):
    """the PSF (z, y, x) of three lines, in float32 (every product is exact)"""
    x, y, z = (np.asarray(w, np.float32) for w in lines_xyz)
    return np.ascontiguousarray(z[:, None, None] * y[None, :, None] * x[None, None, :])


@functools.lru_cache(maxsize=None)
def case_setup(name):
    """Everything a caller needs of one case, the same for every caller: the resolved shifts, what the adjoint is, positive and
    signed lines (x, y, z) of the PSF and of the explicit adjoint kernel (None where psf_inv = None is accepted), the noise volumes.
    Callers must not write into the arrays."""
    c = CASES[name]
    rng = np.random.default_rng(7000 + case_names().index(name))
    k = tuple(c["taps"][::-1])
    shifts = resolve_shifts(c["shape"], k, c["shift"], c["rules"])
    kind = adjoint_kind(k, shifts, c["rules"])
    pos = tuple(_line(rng, kk) for kk in k)
    sgn = tuple(w * rng.choice([-1.0, 1.0], len(w)) for w in pos)
    inv_pos = inv_sgn = None
    if kind == "refused":   # an independent rank-1 kernel, not the flip
        inv_pos = tuple(_line(rng, kk) for kk in k)
        inv_sgn = tuple(w * rng.choice([-1.0, 1.0], len(w)) for w in inv_pos)
    shape = c["shape"]
    return {"k": k, "shifts": shifts, "rules": tuple(c["rules"]), "kind": "explicit" if kind == "refused" else kind,
            "pos": pos, "sgn": sgn, "inv_pos": inv_pos, "inv_sgn": inv_sgn,
            "bl_pos": (rng.random(shape, dtype=np.float32) + np.float32(0.5)),      # [0.5, 1.5)
            "ratio_sgn": (rng.random(shape, dtype=np.float32) - np.float32(0.5)),   # the adjoint's input
            "bl_sgn": (rng.random(shape, dtype=np.float32) - np.float32(0.5)),      # the update's operand a
            "reg": (rng.random(shape, dtype=np.float32) - np.float32(0.5))}         # ... and b


def case_routes(name):
    """(forward, adjoint) routes of the case's context by the restatement above (None: not single-pass)."""
    c, s = CASES[name], case_setup(name)
    off_f, off_a = window_offsets(s["k"], s["shifts"], s["kind"] == "transpose")
    n = c["shape"][::-1]
    return route(n, s["k"], off_f), route(n, s["k"], off_a)


def conv_refs(name, which, mutate=None, dtype=np.float64):
    """(c, B) of one of the case's convolutions: ``which`` "forward" (positive lines on bl_pos) or "adjoint" (signed lines on
    ratio_sgn).  ``mutate`` = (kind, axis) makes a deliberately wrong operator: ("offset", d) moves the window of axis d by one
    sample, ("reverse", d) reverses its line.  B is None for a mutated or fp32 operator."""
    s = case_setup(name)
    if which == "forward":
        vol, lines, transpose = s["bl_pos"], s["pos"], False
    else:
        vol = s["ratio_sgn"]
        lines, transpose = adjoint_operator(s["sgn"], s["inv_sgn"], s["shifts"], s["rules"])
    shifts = list(s["shifts"])
    if mutate is not None:
        kind, d = mutate
        if kind == "offset":
            shifts[d] += 1
        else:
            lines = tuple(w[::-1] if a == d else w for a, w in enumerate(lines))
    c = apply(vol if dtype is np.float32 else vol.astype(np.float64), lines, shifts, s["rules"], transpose, dtype)
    if mutate is not None or dtype is not np.float64:
        return c, None
    return c, apply(np.abs(vol).astype(np.float64), tuple(np.abs(w) for w in lines), shifts, s["rules"], transpose)


@functools.lru_cache(maxsize=None)
def case_expected(name):
    """The three results of a case in float64 with what the bound needs: name -> (ref, a, c, B, lambda, b).  Shared: do not write."""
    s = case_setup(name)
    cf, Bf = conv_refs(name, "forward")
    ca, Ba = conv_refs(name, "adjoint")
    a_pos, a_sgn, reg = s["bl_pos"].astype(np.float64), s["bl_sgn"].astype(np.float64), s["reg"].astype(np.float64)
    return {"ratio": (ratio_ref(a_pos, cf), a_pos, cf, Bf, 0.0, None),
            "update": (update_ref(a_sgn, ca), a_sgn, ca, Ba, 0.0, None),
            "update_reg": (update_ref(a_sgn, ca, LAMBDA, reg), a_sgn, ca, Ba, LAMBDA, reg)}


def allowed(name, what, terms):
    """per-voxel bound of result ``what`` ("ratio", "update", "update_reg") for a convolution of ``terms`` rounded terms"""
    _, a, c, B, lam, b = case_expected(name)[what]
    t = conv_bound(B, terms)
    return ratio_bound(a, c, t) if what == "ratio" else update_bound(a, c, t, lam, b)


def worst(got, name, what, terms):
    """largest observed / allowed over the voxels (a voxel with allowed == 0 must be exact)"""
    ref = case_expected(name)[what][0]
    err, tol = np.abs(np.asarray(got, np.float64) - ref), allowed(name, what, terms)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def report(line):
    print("[sep3d] " + line, flush=True)
