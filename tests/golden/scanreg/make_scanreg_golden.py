"""Writes scan16x900.npz: one raw 16 x 900 scan of the synthetic room and what tests/scanreg_ref.py makes of it (labels, ring table,
less-flat counts).  Run from the repository root: python tests/golden/scanreg/make_scanreg_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
import scanreg_ref as ref  # noqa: E402
from mvil_fusion_amd import scanreg  # noqa: E402
from mvil_fusion_amd.vgicp import _rot  # noqa: E402

raw = scanreg.make_raw_scan(_rot(-0.01, 0.015, -0.7), np.array([-2.0, 1.5, 0.2]), seed=7, rings=16, az=900)
o = ref.extract(raw)
np.savez_compressed(os.path.join(HERE, "scan16x900.npz"), raw=raw, labels=o.labels, ring_table=o.ring_table, n_less_flat_raw=np.int32(o.n_less_flat_raw),
                    n_less_flat=np.int32(len(o.surf_less_flat)))
print(len(raw), np.bincount(o.labels + 1), o.n_less_flat_raw, len(o.surf_less_flat))
