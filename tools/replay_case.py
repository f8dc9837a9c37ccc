import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oracle
from remotesensingproject_amd import depth as rs
from tools import fuzz_parity as fp
seed, i = int(sys.argv[1]), int(sys.argv[2])
rng = np.random.default_rng([seed, i])
c = fp.draw_case(rng)
print(c)
import tests.util as tu
orig = tu.assert_pile_parity
def verbose(got, ref, label=""):
    for k in ("edge_confidence", "edge_mask", "depth_idx", "score", "rbar", "depth_raw", "disp_confidence", "depth"):
        g = got[k]; r = getattr(ref, k)
        if g.dtype.kind == "f":
            bad = ~((g == r) | (np.isnan(g) & np.isnan(r)))
            if k == "disp_confidence":
                bad = np.abs(g - r) > 1e-5
        else:
            bad = g != r
        print(k, "mismatches:", int(bad.sum()), "of", bad.size)
        if bad.any():
            idx = np.argwhere(bad)[:12]
            for t in idx:
                t = tuple(t)
                print("   at", t, "gpu", g[t], "ref", r[t])
fp.assert_pile_parity = verbose
fp.run_case(i, c, rng)
