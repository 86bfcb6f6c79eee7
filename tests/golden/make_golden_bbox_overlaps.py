#!/usr/bin/env python3
"""Record the reference's own bbox_overlaps (detectron/utils/cython_bbox.pyx, compiled where it
lies by `make -C oracle ref` into oracle/_ref/) on the boxes of
tests/test_roi_iou_vs_reference_bbox.py and tests/test_datasets.py.

Runs ONLY where oracle/_ref has been built (it needs the reference tree).  Writes
reference_bbox_overlaps.npz.  The square matrices are far too large to store (2500 x 2500
float32 = 25 MB), so each is kept as the SHA-256 of its bytes - a bit-for-bit equality check -
plus its values at 4096 seeded positions, which say where a mismatch lies:
  int<i>_sha256 / int<i>_idx / int<i>_val   CASES[i], bbox_overlaps(b, b)
  frac_trunc_*                              the fractional boxes, truncated, off the diagonal
  frac_float_*                              the fractional boxes as they are, off the diagonal
  frac_n_differ                             off-diagonal pairs where the two differ
  fresh_<n>x<k>                             bbox_overlaps(b, q) on test_datasets' fresh boxes

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bbox_overlaps.py
"""
import glob
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), ROOT, os.path.join(ROOT, 'na-fwebsod_amd')]
SAMPLE = 4096


def compiled_reference():
    so = glob.glob(os.path.join(ROOT, 'oracle', '_ref', 'cython_bbox*.so'))
    if not so:
        sys.exit('oracle/_ref/cython_bbox not built: make -C oracle ref')
    spec = importlib.util.spec_from_file_location('cython_bbox', so[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha256(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def record(out, key, flat, idx):
    out[key + '_sha256'] = sha256(flat)
    out[key + '_idx'] = idx.astype(np.int64)
    out[key + '_val'] = flat[idx]


def main():
    sys.dont_write_bytecode = True
    import test_datasets as d
    import test_roi_iou_vs_reference_bbox as t
    ref = compiled_reference()
    out = {}
    for i, (_name, make) in enumerate(t.CASES):
        b = make()
        ov = ref.bbox_overlaps(b, b).reshape(-1)
        record(out, 'int%d' % i, ov, np.unique(np.random.default_rng(i).integers(0, ov.size, SAMPLE)))
    bf, tr = t.fractional_boxes()
    off = ~np.eye(len(bf), dtype=bool)
    ov_t = ref.bbox_overlaps(tr, tr)[off]
    ov_f = ref.bbox_overlaps(bf, bf)[off]
    differ = np.flatnonzero(ov_t != ov_f)
    rng = np.random.default_rng(99)
    idx = np.unique(np.concatenate([rng.integers(0, ov_t.size, SAMPLE // 2),
                                    rng.choice(differ, min(SAMPLE // 2, differ.size), replace=False)]))
    record(out, 'frac_trunc', ov_t, idx)
    record(out, 'frac_float', ov_f, idx)
    out['frac_n_differ'] = np.array(differ.size)
    for n, k, b, q in d.fresh_box_pairs():
        out['fresh_%dx%d' % (n, k)] = ref.bbox_overlaps(b, q)
    np.savez_compressed(os.path.join(HERE, 'reference_bbox_overlaps.npz'), **out)
    print('%d arrays, %d off-diagonal pairs differ under truncation' % (len(out), differ.size))


if __name__ == '__main__':
    main()
