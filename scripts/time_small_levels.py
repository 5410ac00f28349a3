"""relax (the default dispatch) vs colour passes vs forced fused launches on mid-size levels, 5 and 10 sweeps (dev aid)
usage: time_small_levels.py [n ...]
NDSM_BLOCK_CFG=0,<points> in the environment sends levels below <points> to the block launch first, so that the
"relax" column times it where the default dispatch would take the fused kernel (the cut-over measurement)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, ndsm_amd
from ndsm_amd import _lib
L = ndsm_amd.load_library(); assert L.ndsm_hip_init(0) == 0
print("NDSM_BLOCK_CFG =", os.environ.get("NDSM_BLOCK_CFG", "(unset)"), " NDSM_HIP_NO_BLOCK =",
      os.environ.get("NDSM_HIP_NO_BLOCK", "(unset)"), flush=True)
for n in [int(a) for a in sys.argv[1:]] or (32, 64, 96, 128, 160):
    mesh = [np.linspace(0, 1, n)] * 3
    S = _lib.MGSolver([n, n, n], mesh, "NDDNDD")
    rng = np.random.default_rng(1)
    S.upload(1, _lib.BUF_U, rng.uniform(-1, 1, (n, n, n))); S.upload(1, _lib.BUF_RHS, rng.uniform(-1, 1, (n, n, n)))
    for cnt in (5, 10):
        for name, op in (("relax", _lib.OP_RELAX), ("colour", _lib.OP_RELAX_COLOR), ("fused", _lib.OP_RELAX_FUSED)):
            S.op(op, 1, cnt); S.sync()
            t = min(S.timed(lambda: [S.op(op, 1, cnt) for _ in range(10)]) / 10 for _ in range(3))
            print(f"{n}^3 {cnt} sweeps {name}: {t*1e3:.1f} us", flush=True)
    S.close()
