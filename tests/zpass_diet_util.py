"""Cases, inputs and digests shared by tests/test_gpu_zpass_diet.py and tests/golden/zpass_parent/record.py.

Every case is one context: (z length, 16, 32) volumes through the paired z pass in one form of the OTF.  Per case the forward
convolution, the adjoint convolution and three fused iterations are taken; the recorded results are those of the commit before the
paired z pass lost its integer work, and must be reproduced bit for bit."""
import contextlib
import hashlib
import os

import numpy as np
import torch

from oracle import rl_oracle as R
from tests import real_otf_util as U
from tests.test_gpu_pair_layout import _conv_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zpass_parent")

# z = 64, 256, 512, 1024: powers of two (1024: the 246-register form); 192: radix-3 front; 576: no LDS table, stored form only;
# 768: 16 waves and a row per wave
LENGTHS = [64, 256, 512, 1024, 192, 576, 768]
FORM_ENV = {"factored": {}, "stored": {"MI_FFT_STORED_OTF": "1"}, "complex": {"MI_FFT_COMPLEX_OTF": "1"}}
PADDED_VSHAPE, PADDED_KSHAPE = (50, 40, 60), (15, 9, 5)   # grid 64 x 48 x 64 (tests/test_gpu_factored_otf.py)


def cases():
    """[(case id, dict)]: the circular cases of every length and form, one padded zero-boundary case, one explicit adjoint."""
    out = []
    for nz in LENGTHS:
        for form in ("factored", "stored", "complex"):
            if nz == 576 and form == "factored":
                continue
            out.append((f"nz{nz}_{form}", dict(shape=(nz, 16, 32), form=form, kind="circular")))
    out.append(("padded_zero", dict(shape=PADDED_VSHAPE, form="factored", kind="padded")))
    out.append(("explicit_adjoint", dict(shape=PADDED_VSHAPE, form="factored", kind="adjoint")))
    return out


@contextlib.contextmanager
def switches(env):
    """The environment switches a plan reads when it is created, set for the body only."""
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_ctx(case, dev, extra_env=None):
    from ipp_amd import capi, decon
    env = dict(FORM_ENV[case["form"]])
    env.update(extra_env or {})
    shape = case["shape"]
    if case["kind"] in ("padded", "adjoint"):   # (a circular context has no use for an explicit adjoint: it is a padded one too)
        psf = R.gaussian_psf(PADDED_KSHAPE, (2.5, 1.5, 0.8))
        inv = R.gaussian_psf(PADDED_KSHAPE, (1.5, 1.0, 1.2)) if case["kind"] == "adjoint" else None
        env["MI_FFT_NATIVE_INFLATE"] = "100"   # (as test_paired_layout_on_padded_grids)
        boundary = capi.BOUNDARY_ZERO
    else:
        psf, inv = R.gaussian_psf(U.KSHAPE, U.SIGMA), None
        boundary = capi.BOUNDARY_CIRCULAR
    with switches(env):
        ctx = decon.RLContext(shape, psf, inv, boundary=boundary, engine=capi.ENGINE_FFT, device=dev)
    assert ctx.engine == capi.ENGINE_FFT and ctx.pair_layout and ctx.fft_route["z_kernel"] == 2
    assert ctx.otf_form["form"] == case["form"], (case, ctx.otf_form)   # (a fall-back to another form would hide what is tested)
    return ctx


def inputs(case):
    """(a, b, volume): rand + 0.5 operands seeded by the shape and a bead volume; float32, host."""
    shape = case["shape"]
    an, bn = U.operands(shape)
    vol = R.bead_volume(shape, seed=5, psf=R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0)))
    return an, bn, np.ascontiguousarray(vol, dtype=np.float32)


def run(ctx, ins, dev):
    """(forward, adjoint, three fused iterations) as host float32 arrays"""
    an, bn, vol = ins
    fwd, adj = _conv_pair(ctx, torch.from_numpy(an).to(dev), torch.from_numpy(bn).to(dev))
    bl = torch.from_numpy(vol).to(dev)
    ctx.iterate(bl, None, 3)
    return fwd, adj, bl.cpu().numpy()


NAMES = ("forward", "adjoint", "iterate3")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype == np.float32
        h.update(a.tobytes())
    return h.hexdigest()
