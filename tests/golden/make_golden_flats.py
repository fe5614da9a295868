#!/usr/bin/env python3
"""Generate ``valley_ridge_flats.npz``: the valley / ridge index with more than four flat fractions,
computed by RUNNING THE REAL REFERENCE (its ``valley_ridge`` takes a ``flat_list`` of any length).

Run once, where the reference is importable, like ``make_golden.py``:

    python tests/golden/make_golden_flats.py

The reference's absent dependencies are replaced by ``make_golden.py``'s inert stand-ins (imported
from there, not repeated).  Only data is written: the inputs, the reference's outputs, the
parameters and the reference's noise floor against the float64 oracle (``<tag>_norm_floor``).
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins and imports the reference)

orc = mg.orc

# (tag, DEM, size, mode, flats, sigma): the register-resident folded form (7, 9 px), the streamed form (21 px), a smoothed
# fractional DEM; 5, 6 and 8 planes (two groups of four, the second partial or full)
CASES = [
    ("int_valley_s7_f5", "dem_int", 7, "valley", [0, 0.1, 0.2, 0.3, 0.4], None),
    ("int_ridge_s9_f6", "dem_int", 9, "ridge", [0, 0.1, 0.2, 0.3, 0.4, 0.5], None),
    ("int_valley_s21_f5", "dem_int", 21, "valley", [0, 0.1, 0.2, 0.3, 0.4], None),
    ("frac_valley_s9_f8_sig", "dem_frac", 9, "valley", [0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35], 1.125),
]


def main():
    dems = {"dem_int": orc.synthetic_dem(72, 88, seed=14, integer=True),
            "dem_frac": orc.synthetic_dem(64, 80, seed=15, integer=False)}
    out = dict(dems)
    for tag, which, size, mode, flats, sigma in CASES:
        dem = dems[which]
        norm, direction = mg.ref_topo.valley_ridge(dem, size, mode, flats, sigma)
        out[f"{tag}_norm"] = norm
        out[f"{tag}_norm_exact"] = orc.valley_ridge_exact(dem, size, mode, flats, sigma)[0]
        out[f"{tag}_dir"] = direction
        out[f"{tag}_params"] = np.array([size, 0 if mode == "valley" else 1, -1.0 if sigma is None else sigma] + list(flats),
                                        dtype=np.float64)
        print(tag, "done", flush=True)
    mg.save("valley_ridge_flats", **out)


if __name__ == "__main__":
    main()
