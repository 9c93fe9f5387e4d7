"""Records what tests/test_gpu_zpass_diet.py holds the paired z pass to: run once, on the GPU, at the commit BEFORE the pass lost
its integer work (the parent of "Paired z pass: literal LDS addresses ..."), from the repository root:

    python tests/golden/zpass_parent/record.py [output directory, default: this one]

Per case of tests/zpass_diet_util.py: forward convolution, adjoint convolution, three fused iterations.  The 64-point cases are kept as
arrays (nz64_<form>.npy, [3][64][16][32] float32), everything as SHA-256 digests of the float32 bytes in digests.json, beside a digest
of the inputs (so that a changed random stream is told from a changed kernel)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import zpass_diet_util as Z  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else Z.GOLDEN
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", 0)
    digests = {}
    for cid, case in Z.cases():
        ins = Z.inputs(case)
        ctx = Z.make_ctx(case, dev)
        res = Z.run(ctx, ins, dev)
        ctx.close()
        digests[cid] = {"inputs": Z.digest(*ins), **{n: Z.digest(r) for n, r in zip(Z.NAMES, res)}}
        if case["kind"] == "circular" and case["shape"][0] == 64:
            np.save(os.path.join(out, f"{cid}.npy"), np.stack(res))
        print(cid, digests[cid]["iterate3"][:16], flush=True)
    with open(os.path.join(out, "digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
