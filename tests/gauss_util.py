"""Plain restatement of the reference's separable Gaussian (gauss3d_gpu.cu:81-138,163-192) for odd AND even kernel sizes, and the
cases of tests/test_gpu_gauss3d.py with the kernel route of csrc/gauss3d.hip that each one is meant to reach.

Arithmetic (the reference kernel's own, in loop form):
  taps   make_gaussian_kernel: sigma * sigma rounded in float, exp in double, stored as float; the sum (double, in order) runs over
         the 2 (k / 2) + 1 values that loop writes -- one more than k for an even k -- and the first k values are divided by it;
  pass   out[i] = sum_s in[clamp(i + s - k / 2)] * w[s], s = 0 .. k - 1 in that order, accumulated in float64 here (float32 in
         the kernels), rounded to float32 after every pass; x, then y, then z.
For an even k the window is i - k/2 .. i + k/2 - 1: one more sample before the centre than after it.

Tolerance of the GPU tests.  Hard cap (kx + ky + kz) 2^-23 max|x|: a pass is a convex combination, so float32 accumulation of k
taps adds at most k 2^-24 max|x| and the rounding of the pass another half ulp; later passes do not amplify it.  The cap is loose
for long kernels, so the asserted bound is measured: FP32_FORM_DEV is the largest deviation, over every case below, of the same
restatement accumulated in float32 with a separately rounded multiply and add per tap from the float64-per-pass one
(tests/test_gauss_util_host.py measures it per case, prints it and holds the constant to it).  The kernels use fmaf, which rounds
once where that form rounds twice, so they should be no worse; GPU_FACTOR = 4 covers the spread from case to case.
"""
import math

import numpy as np

# mi_gauss3d_route (include/mi_lsdeconv.h)
WAVE1, WAVE2, FUSED = 1, 2, 3
RING_RING, WIN_RING, RING_WIN, WIN_WIN = 4, 5, 6, 7      # two passes: xy kernel, z kernel
ROUTE_NAMES = {WAVE1: "k_gauss3d_wave<KZ,1>", WAVE2: "k_gauss3d_wave<KZ,2>", FUSED: "k_gauss3d_fused",
               RING_RING: "k_gauss_xy + k_gauss_z", WIN_RING: "k_gauss_xy_win + k_gauss_z",
               RING_WIN: "k_gauss_xy + k_gauss_z_win", WIN_WIN: "k_gauss_xy_win + k_gauss_z_win"}

FP32_FORM_DEV = 2.0 ** -22   # 2.384e-7, measured: 6.0e-8 .. 2.384e-7 over CASES (test_gauss_util_host.py prints every case's figure)
GPU_FACTOR = 4.0
BASE_SIGMA = (0.8, 1.3, 0.6)   # anisotropic: a mix-up of the axes' taps shows


def case_sigma(ksize):
    """BASE_SIGMA scaled per axis with the kernel size, so that the outermost tap of every axis stays far above the tolerance
    (radius / sigma between 1.5 and 3.4)."""
    return [b * max(k, 3) / 4.0 for b, k in zip(BASE_SIGMA, ksize)]


def _case(shape, ksize, route, sigma=None):
    return {"shape": shape, "ksize": ksize, "route": route, "sigma": sigma if sigma is not None else case_sigma(ksize)}


# name -> shape (z, y, x), ksize [kx, ky, kz] (None: the default 2 ceil(3 sigma) + 1), sigma [sx, sy, sz], route
CASES = {}
for _kz in (3, 5, 7):
    # two z chunks of 128, the second (3 planes) no longer than the run-in; ragged in x (68 = 64 + 4) and y (33 = 32 + 1)
    CASES[f"wave1_7_3_{_kz}"] = _case((131, 33, 68), [7, 3, _kz], WAVE1)
    CASES[f"wave1_1_7_{_kz}"] = _case((131, 33, 68), [1, 7, _kz], WAVE1)
    # tiles of 128 columns, the last one 4 columns wide
    CASES[f"wave2_5_7_{_kz}"] = _case((131, 37, 516), [5, 7, _kz], WAVE2)
CASES["wave1_all_clamped"] = _case((2, 1, 4), [7, 3, 5], WAVE1)
CASES["wave1_one_plane"] = _case((1, 5, 64), [1, 7, 7], WAVE1)
# the work-group kernel: z chunks of 256 for kz >= 9, of 128 below
CASES["fused_default_11"] = _case((259, 17, 68), None, FUSED, sigma=[1.5, 1.4, 1.6])    # 2 ceil(3 sigma) + 1 = 11 on every axis
CASES["fused_5_5_9"] = _case((259, 17, 68), [5, 5, 9], FUSED)
CASES["fused_13_13_5"] = _case((131, 17, 68), [13, 13, 5], FUSED)
CASES["fused_3_9_7"] = _case((131, 17, 68), [3, 9, 7], FUSED)
CASES["fused_25_19_3"] = _case((131, 17, 68), [25, 19, 3], FUSED)     # patch of 748 quads out of 768: the patch budget's inside
CASES["fused_all_clamped"] = _case((3, 1, 4), [5, 5, 9], FUSED)
CASES["patch_budget_outside"] = _case((131, 17, 68), [25, 21, 3], RING_WIN)   # 792 quads
CASES["lds_budget_inside"] = _case((21, 19, 68), [11, 13, 11], FUSED)         # 61 184 B of 65 536
CASES["lds_budget_outside"] = _case((21, 19, 68), [11, 11, 13], WIN_WIN)      # 68 224 B
CASES["ragged_rows_never_fuse"] = _case((9, 9, 70), [5, 5, 5], WIN_WIN)       # nx % 4 != 0
for _n in range(3, 26, 2):
    CASES[f"win_{_n}"] = _case((21, 19, 70), [_n, _n, _n], WIN_WIN)           # every built k_gauss_xy_win<N> / k_gauss_z_win<N>
CASES["ring_9_11_15"] = _case((21, 19, 70), [9, 11, 15], RING_WIN)
CASES["ring_13_13_27"] = _case((21, 19, 70), [13, 13, 27], WIN_RING)
CASES["ring_27"] = _case((21, 19, 70), [27, 27, 27], RING_RING)
CASES["ring_51"] = _case((21, 19, 70), [51, 51, 51], RING_RING)
CASES["even_4_6_2"] = _case((21, 19, 70), [4, 6, 2], RING_RING)
CASES["even_50_2_26"] = _case((21, 19, 70), [50, 2, 26], RING_RING)
CASES["even_2_2_2"] = _case((21, 19, 70), [2, 2, 2], RING_RING)
CASES["even_6_6_4_whole_quads"] = _case((21, 19, 68), [6, 6, 4], RING_RING)   # nx % 4 == 0: even sizes never fuse
CASES["even_z_only_5_5_4"] = _case((21, 19, 70), [5, 5, 4], WIN_RING)
CASES["even_xy_only_4_6_5"] = _case((21, 19, 70), [4, 6, 5], RING_WIN)
# chunk seams of the two-pass walks: GXY_YCHUNK = 256 (second chunk: 7 rows, fewer than the window's 8), GZ_ZCHUNK = 512
CASES["yseam_win_9"] = _case((3, 263, 5), [9, 9, 3], WIN_WIN)
CASES["yseam_ring_27"] = _case((3, 263, 5), [3, 27, 3], RING_WIN)
CASES["yseam_ring_even_6"] = _case((3, 263, 5), [3, 6, 3], RING_WIN)
CASES["zseam_win_9"] = _case((515, 2, 7), [3, 3, 9], WIN_WIN)
CASES["zseam_ring_27"] = _case((515, 2, 7), [3, 3, 27], WIN_RING)
CASES["zseam_ring_even_8"] = _case((515, 2, 7), [3, 3, 8], WIN_RING)
CASES["one_plane_two_pass"] = _case((1, 7, 70), [5, 5, 5], WIN_WIN)
CASES["one_row_rings"] = _case((5, 1, 70), [27, 5, 27], RING_RING)
CASES["one_line_even"] = _case((1, 1, 9), [4, 4, 4], RING_RING)

EVEN_CASES = sorted(n for n, c in CASES.items() if c["ksize"] is not None and any(k % 2 == 0 for k in c["ksize"]))


def default_ksize(sigma):
    """2 ceil(3 sigma) + 1 of the float sigma (gauss3d_gpu.cu:244-261)."""
    return [2 * int(math.ceil(3.0 * float(np.float32(s)))) + 1 for s in sigma]


def case_ksize(c):
    return list(c["ksize"]) if c["ksize"] is not None else default_ksize(c["sigma"])


def case_input(name):
    """Random data in [0, 1), the same for every caller."""
    seed = sorted(CASES).index(name)
    return np.random.default_rng(1000 + seed).random(CASES[name]["shape"], dtype=np.float32)


def taps(sigma, ksize):
    """make_gaussian_kernel (gauss3d_gpu.cu:81-90) for any ksize >= 1."""
    s = np.float32(sigma)
    s2 = float(np.float32(s * s))
    r = ksize // 2
    w = [np.float32(math.exp(-0.5 * (i * i) / s2)) for i in range(-r, r + 1)]   # 2 r + 1 values: ksize + 1 for an even ksize
    total = 0.0
    for v in w:
        total += float(v)
    return np.array([np.float32(float(v) / total) for v in w[:ksize]], np.float32)


def _pass(a, w, axis, shift, acc_dtype):
    """One 1-D pass of gauss1d_kernel_const_float (gauss3d_gpu.cu:124-137) along numpy axis ``axis``; ``shift`` moves the whole
    window (0 is the reference)."""
    n, k = a.shape[axis], len(w)
    base = np.arange(n)
    acc = np.zeros(a.shape, acc_dtype)
    src = a.astype(acc_dtype)
    for s in range(k):
        idx = np.clip(base + (s - k // 2 + shift), 0, n - 1)
        term = np.take(src, idx, axis=axis) * acc_dtype(w[s])   # (float32: the product is rounded, then the sum)
        acc = acc + term
    return acc.astype(np.float32)


def gauss3d(vol, sigma, ksize=None, shift=(0, 0, 0), acc_dtype=np.float64):
    """``gauss3d_gpu(x, sigma[, ksize])`` restated: sigma / ksize / shift in reference order [x, y, z], ``vol`` is (z, y, x).
    ``acc_dtype=np.float32`` is the form that accumulates like a kernel without fused multiply-add."""
    sigma = [float(sigma)] * 3 if np.isscalar(sigma) else [float(s) for s in sigma]
    if ksize is None:
        ksize = default_ksize(sigma)
    elif np.isscalar(ksize):
        ksize = [int(ksize)] * 3
    out = np.ascontiguousarray(vol, dtype=np.float32)
    for ref_axis in range(3):  # x, y, z
        out = _pass(out, taps(sigma[ref_axis], int(ksize[ref_axis])), 2 - ref_axis, int(shift[ref_axis]), acc_dtype)
    return out


def gauss3d_triple_loop(vol, sigma, ksize):
    """The same arithmetic voxel by voxel, as the reference kernel's thread does it (tiny volumes only)."""
    nz, ny, nx = vol.shape
    n = (nx, ny, nz)
    src = np.array(vol, np.float32)
    for axis in range(3):
        w = taps(sigma[axis], ksize[axis])
        k = len(w)
        dst = np.empty_like(src)
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    pos = [x, y, z]
                    acc = 0.0
                    for s in range(k):
                        q = list(pos)
                        q[axis] = min(max(pos[axis] + s - k // 2, 0), n[axis] - 1)
                        acc += float(src[q[2], q[1], q[0]]) * float(w[s])
                    dst[z, y, x] = np.float32(acc)
        src = dst
    return src


def hard_cap(ksize, peak):
    return sum(ksize) * 2.0 ** -23 * peak


def gpu_tolerance(ksize, peak):
    """4 x the measured deviation of the float32 form, never more than the hard cap."""
    return min(GPU_FACTOR * FP32_FORM_DEV, hard_cap(ksize, peak))


def report(line):
    print("[gauss3d] " + line, flush=True)
