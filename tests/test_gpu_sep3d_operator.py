"""GPU: the rank-1 convolution of the direct RL engine as an operator, build by build (csrc/sep3d.hip), and the two other routes of the
same contexts (three launches of k_conv3d_direct with 1-D tables, the dense tap loop) on the same cases.

Every case of tests/sep3d_util.py runs on RLContext(..., engine=1, boundary=rules, shift_xyz=shifts) with white noise and asymmetric
dyadic tap lines, asserts the kernel build it means to cover (RLContext.sep_route: the function the launch itself is decided by) and
compares forward_ratio, adjoint_update and the regularised adjoint_update voxel by voxel with the float64 reference, to the bound
derived in sep3d_util's docstring -- no measured constant.  The output lives inside a canary tensor; its guards and every input other
than the output must come back untouched.  The worst observed / allowed figure of each result is printed."""
import numpy as np
import pytest
import torch

from tests import sep3d_util as S

pytestmark = pytest.mark.gpu

SENTINEL = 7.25e33
# route -> (environment switch, what the context must report, rounded terms of the convolution sum)
MODES = {"single_pass": (None, (True, True), S.sep_terms),
         "three_launches": ("MI_NO_SEP_SINGLE", (True, False), S.sep_terms),
         "dense": ("MI_NO_SEPARABLE", (False, False), S.dense_terms)}


class Canary:
    """A volume inside a larger tensor, a plane and more of guard on either side, at a 16-byte aligned offset"""

    def __init__(self, shape, dev, fill=None):
        self.n = int(np.prod(shape))
        self.g = (shape[1] * shape[2] + 64 + 3) // 4 * 4
        self.flat = torch.full((self.n + 2 * self.g,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.flat[self.g:self.g + self.n].view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()
        if fill is not None:
            self.view.copy_(torch.from_numpy(fill))

    def check(self):
        lo, hi = self.flat[:self.g], self.flat[self.g + self.n:]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), "the kernel wrote outside its output"
        return self.view.cpu().numpy()


def _contexts(dev, name, mode, monkeypatch):
    """(context with the positive lines, context with the signed lines) of a case under a route switch; the route is asserted"""
    from ipp_amd import decon
    c, s = S.CASES[name], S.case_setup(name)
    env, (separable, single), _ = MODES[mode]
    if env:
        monkeypatch.setenv(env, "1")       # read when the context is created
    out = []
    for lines, inv in ((s["pos"], s["inv_pos"]), (s["sgn"], s["inv_sgn"])):
        ctx = decon.RLContext(c["shape"], S.psf3d(lines), None if inv is None else S.psf3d(inv), boundary=list(s["rules"]), engine=1,
                              device=dev, shift_xyz=c["shift"])
        assert ctx.engine == 1 and ctx.separable == separable and ctx.separable_single_pass == single
        if single:
            want_f, want_a = S.case_routes(name)
            got_f, got_a = ctx.sep_route(False), ctx.sep_route(True)
            assert {f: got_f[f] for f in S.ROUTE_FIELDS} == c["route"] and {f: got_a[f] for f in S.ROUTE_FIELDS} == c["route"]
            assert got_f == want_f and got_a == want_a          # ... and the LDS bytes of the restatement
        else:
            assert ctx.sep_route(False) is None and ctx.sep_route(True) is None
        out.append(ctx)
    if env:
        monkeypatch.delenv(env)
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", S.case_names())
def test_operator_against_float64_reference(dev, name, mode, monkeypatch):
    c, s = S.CASES[name], S.case_setup(name)
    terms = MODES[mode][2](s["k"])
    ctx_pos, ctx_sgn = _contexts(dev, name, mode, monkeypatch)
    figures = {}

    # forward_ratio on positive noise
    bl = torch.from_numpy(s["bl_pos"]).to(dev)
    out = Canary(c["shape"], dev)
    ctx_pos.forward_ratio(bl, out.view)
    got = out.check()
    assert np.isfinite(got).all() and np.array_equal(bl.cpu().numpy(), s["bl_pos"])
    figures["ratio"] = S.worst(got, name, "ratio", terms)

    # adjoint_update on signed noise with signed taps: |a c|, then |a c (1 - l) + b l|
    ratio, reg = torch.from_numpy(s["ratio_sgn"]).to(dev), torch.from_numpy(s["reg"]).to(dev)
    for what, lam, b in (("update", 0.0, None), ("update_reg", S.LAMBDA, reg)):
        out = Canary(c["shape"], dev, fill=s["bl_sgn"])
        ctx_sgn.adjoint_update(ratio, out.view, lam, b)
        got = out.check()
        assert np.isfinite(got).all() and (got >= 0).all()
        assert np.array_equal(ratio.cpu().numpy(), s["ratio_sgn"]) and np.array_equal(reg.cpu().numpy(), s["reg"])
        figures[what] = S.worst(got, name, what, terms)

    r = ctx_pos.sep_route(False)
    build = "k_conv3d_direct" if r is None else f"{r['family']} KZB {r['kzb']} NPRE {r['npre']}, {r['chunks']} x {r['zchunk']} planes"
    S.report(f"{name} [{mode}: {build}] observed / allowed: " + ", ".join(f"{w} {v:.3f}" for w, v in figures.items()))
    for what, v in figures.items():
        assert v <= 1.0, (what, v)


@pytest.mark.parametrize("mode", list(MODES))
def test_ratio_clamps_the_denominator_at_eps(dev, mode, monkeypatch):
    """bl = 2^-30 everywhere under a PSF that sums to less than 2^7: conv(bl) < eps = 2^-23 at every voxel, so the ratio is exactly
    2^-30 / 2^-23 = 2^-7 (a division of powers of two: no rounding)."""
    name = "clamp_small_taps"
    c, s = S.CASES[name], S.case_setup(name)
    vol = np.full(c["shape"], 2.0 ** -30, np.float32)
    conv = S.apply(vol.astype(np.float64), s["pos"], s["shifts"], s["rules"])
    assert 0 < conv.max() < S.EPS
    ctx_pos, _ = _contexts(dev, name, mode, monkeypatch)
    bl = torch.from_numpy(vol).to(dev)
    out = Canary(c["shape"], dev)
    ctx_pos.forward_ratio(bl, out.view)
    assert np.array_equal(out.check(), np.full(c["shape"], 2.0 ** -7, np.float32))
