"""Compares two directories of `bench.py --dump-outputs`, array by array, as float32 values and as uint32 bit patterns:
    python tools/compare_outputs.py DIR_NEW DIR_REFERENCE
One line per array: rel-L2 and largest difference against the reference, and how many elements differ in their bits."""
import glob
import os
import sys

import numpy as np


def main():
    new, ref = sys.argv[1:3]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ref, '*.npy')))
    assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(new, '*.npy'))), 'the two directories hold different arrays'
    moved = []
    for name in names:
        x, y = np.load(os.path.join(new, name)).astype(np.float32).ravel(), np.load(os.path.join(ref, name)).astype(np.float32).ravel()
        differ = int((x.view(np.uint32) != y.view(np.uint32)).sum())
        d = x.astype(np.float64) - y
        rel = float(np.linalg.norm(d) / max(np.linalg.norm(y.astype(np.float64)), 1e-300)) if differ else 0.0
        print(f'{name:22s} n={x.size:8d} relL2={rel:.3e} maxabs={float(np.abs(d).max()) if differ else 0.0:.3e} max|y|={float(np.abs(y).max()):.3e} '
              f'nan={int(np.isnan(x).sum())}/{int(np.isnan(y).sum())} differ={differ}')
        if differ:
            moved.append(name)
    print('ALL BIT-IDENTICAL' if not moved else 'differ: ' + ' '.join(moved))


if __name__ == '__main__':
    main()
