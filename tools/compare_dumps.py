#!/usr/bin/env python3
"""tools/compare_dumps.py A B: compare two `bench.py --dump-outputs` directories array by array.

One line per array: its shape, the largest absolute difference, that difference relative to the largest magnitude in B,
and how many elements differ at all.  Exit status 1 when an array is missing on one side or the shapes differ."""
import glob
import os
import sys

import numpy as np


def main(a: str, b: str) -> int:
    names = sorted({os.path.basename(f) for d in (a, b) for f in glob.glob(os.path.join(d, "*.npy"))})
    bad = 0
    for n in names:
        fa, fb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print(f"{n[:-4]:16s} missing in {'B' if os.path.exists(fa) else 'A'}")
            bad = 1
            continue
        x, y = np.load(fa).astype(np.float64), np.load(fb).astype(np.float64)
        if x.shape != y.shape:
            print(f"{n[:-4]:16s} shapes differ: {x.shape} vs {y.shape}")
            bad = 1
            continue
        d = np.abs(x - y)
        dmax = float(d.max()) if d.size else 0.0
        scale = float(np.abs(y).max()) if y.size else 0.0
        print(f"{n[:-4]:16s} shape {str(x.shape):12s} max|A-B| {dmax:.3e}  relative {dmax / scale if scale else 0.0:.3e}  "
              f"differing {int((d > 0).sum())} of {d.size}")
    return bad


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    raise SystemExit(main(sys.argv[1], sys.argv[2]))
