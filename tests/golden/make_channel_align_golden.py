#!/usr/bin/env python3
"""Golden fixtures of channel alignment from the numpy restatement (tests/channel_align_util.py); no device, no reference tree.

tests/golden/channel_align/recorded.npz:
    ecc_shapes [k, 2], ecc_truth [k, 2], ecc_found [k, 2], ecc_iterations [k], ecc_error [k]
        the restatement's ECC on the smooth planes of ``ecc_case``: the translation it finds, its iteration count and its error
        against the synthetic truth, max(|tx - truth_x|, |ty - truth_y|) -- the device test allows this much plus 1e-3
    factoring_rel
        the largest relative difference between the factored one-pass quantities and the two-pass ones over the ECC cases and the
        test translations (what factoring the means out costs in float64; quoted in DESIGN section 18)
    align_seed, align_moves [3, iterations], align_sums [iterations, 3], align_margin
        the outer loop of align_images on ``blob_volume(seed=align_seed)``: moves in x, y, z per outer iteration, the pre-rounding
        sums, and their smallest distance to a half-integer (asserted >= 0.1: a 1e-3 difference cannot flip ``round``)
    main_seed, main_alignments [3, 3], main_residuals [3, 3], main_margin
        the same for the three channels of ``main_fixture(main_seed)`` (-1000 and NaN mark None)
The inputs themselves are regenerated from the seeds by the tests.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import channel_align_util as U  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "channel_align")
TRANSLATIONS = [(0.0, 0.0), (0.5, -0.25), (2.3, -1.7), (-6.0, 4.0)]
MARGIN = 0.1
MAX_ECC_ITERATIONS = 200   # a fixture on which every ECC run settles quickly: a run that wanders for thousands of iterations may stop elsewhere


def ecc_records():
    shapes, truth, found, iterations, error = [], [], [], [], []
    worst = 0.0
    for shape in U.ECC_CASES:
        tmpl, subj, (tx0, ty0) = U.ecc_case(shape)
        tx, ty, _, count, status = U.ecc_translation(tmpl, subj)
        assert status == U.ECC_OK, (shape, status)
        shapes.append(shape)
        truth.append((tx0, ty0))
        found.append((tx, ty))
        iterations.append(count)
        error.append(max(abs(tx - tx0), abs(ty - ty0)))
        planes = U.ecc_prepare(tmpl, subj)
        for t in TRANSLATIONS:
            one, two = U.derived(U.ecc_sums(planes, *t)[0]), U.derived_two_pass(planes, *t)
            for k, v in two.items():
                s = U.natural_scale(k, two)
                if s:
                    worst = max(worst, abs(one[k] - v) / s)
    return dict(ecc_shapes=np.array(shapes), ecc_truth=np.array(truth), ecc_found=np.array(found), ecc_iterations=np.array(iterations),
                ecc_error=np.array(error), factoring_rel=np.float64(worst))


def align_records():
    for seed in range(5, 40):
        ref, sub = U.blob_volume(seed=seed)
        del U.ITERATIONS[:]
        xs, ys, zs, _, sums = U.align_images(ref, sub, 10)
        margin = U.half_integer_margin(sums)
        if margin >= MARGIN and len(xs) >= 2 and max(U.ITERATIONS) <= MAX_ECC_ITERATIONS:
            return dict(align_seed=np.int64(seed), align_moves=np.array([xs, ys, zs]), align_sums=np.array(sums), align_margin=np.float64(margin))
    raise AssertionError("no seed keeps every pre-rounding sum 0.1 away from a half-integer")


def main_records():
    for seed in range(11, 40):
        down, orig = U.main_fixture(seed)
        del U.ITERATIONS[:]
        try:
            want = U.main_expected(down, orig, 0, 10, "uint16", (1, 2), (1, 2), (1, 1))
        except U.EccFailure:
            continue
        margin = min(U.half_integer_margin(s) for s in want["sums"].values())
        if margin >= MARGIN and max(U.ITERATIONS) <= MAX_ECC_ITERATIONS:
            moves = np.array([[-1000 if v is None else v for v in a] for a in want["alignments"]])
            residuals = np.array([[np.nan] * 3 if r is None else [float(v) for v in r] for r in want["residuals"]])
            return dict(main_seed=np.int64(seed), main_alignments=moves, main_residuals=residuals, main_margin=np.float64(margin))
    raise AssertionError("no seed keeps every pre-rounding sum 0.1 away from a half-integer")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    records = {**ecc_records(), **align_records(), **main_records()}
    np.savez(os.path.join(OUT, "recorded.npz"), **records)
    for k, v in records.items():
        print(k, np.array2string(np.asarray(v), precision=6).replace("\n", " "))
