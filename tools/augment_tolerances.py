"""CPU: measure the tolerances of tests/test_gpu_augment.py.

For every (case, transform) of that test: the largest |fp32 restatement - fp64 restatement| of the normalised
image over the test's own inputs (tests/aug_ref.py in both modes), and the share of mask tie pixels; for every
case the same for the elastic displacement field.  Prints the TOL / FIELD_TOL entries (4 x the measured value,
the measured value in the comment).  Needs no GPU and never sees device output.

    python tools/augment_tolerances.py
"""

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "tests", ROOT / "unet-segment-pytorch_amd", ROOT):
    sys.path.insert(0, str(p))

import aug_ref as R  # noqa: E402
import test_gpu_augment as T  # noqa: E402

MARGIN = 4.0


def main():
    print("TOL")
    for case in T.CASES:
        for kind in T.KINDS:
            a, ma, tie = T.reference(case, kind)
            b, mb, _ = T.reference(case, kind, np.float32)
            e = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
            off = int(((ma != mb) & ~tie).sum())
            print(f'    ("{case}", "{kind}"): {MARGIN * e:.3e},   # measured {e:.3e}; ties {tie.mean():.2%}'
                  + (f"; {off} fp32 mask pixels differ off the ties" if off else ""))
    print("FIELD_TOL")
    for case, c in T.CASES.items():
        tab = T.table(case, "mixed")
        e = 0.0
        for i in (3, 1, 4):
            a = R.elastic_field(c["S"], tab["key"][i], 50.0, c["sigma"])
            b = R.elastic_field(c["S"], tab["key"][i], 50.0, c["sigma"], np.float32)
            e = max(e, float(np.abs(a - b).max()))
        print(f'    "{case}": {MARGIN * e:.3e},   # measured {e:.3e} px')


if __name__ == "__main__":
    main()
