"""The oracle port against the reference under EVERY boundary letter set (no GPU).

tests/golden/reference_bc_matrix.json holds the sha256 of the reference's own relax3d, residual3d and vcycle for the 63
not all-Neumann sets of six letters, and of its relax_nd and residual_nd for the 15 of four letters, on the shapes of
golden_inputs.BC_MATRIX_3D / BC_MATRIX_2D (an odd nx on aniso_mesh, an even one on uniform_mesh); the port must
reproduce every one of them bit for bit.  The all-Neumann outputs carry a mean whose summation order the reference
leaves open: they are stored in full (reference_bc_matrix_NN.npz) and compared within the 1e-14 absolute that
test_oracle.py uses for them.  With this the GPU tests' "equal to the port" means "equal to the reference" for all
64 + 16 sets, not only for the six of BCS_RANDOM / BCS_ANISO.
"""
import json
import os

import numpy as np

from golden_inputs import ALL_BCS_2D, ALL_BCS_3D, BC_MATRIX_2D, BC_MATRIX_3D, bc_matrix_case, digest


def _tag(ns):
    return "x".join(str(n) for n in ns)


def _check(want, nn, tag, bcs, outputs):
    """one set on one shape: `outputs` = {name: array}; returns (digests compared, arrays compared within 1e-14)"""
    nd = na = 0
    for k, a in outputs.items():
        if set(bcs) == {"N"}:
            np.testing.assert_allclose(a, nn[f"{k}_{tag}"], rtol=0, atol=1e-14, err_msg=f"{k} {tag} {bcs}")
            na += 1
        else:
            assert digest(a) == want[f"{k}_{tag}_{bcs}"], (k, tag, bcs)
            nd += 1
    return nd, na


def test_port_equals_reference_under_every_boundary_set_3d(port, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_bc_matrix.json")))
    nn = np.load(os.path.join(golden_dir, "reference_bc_matrix_NN.npz"))
    assert len(ALL_BCS_3D) == len(set(ALL_BCS_3D)) == 64
    for ns, mname in BC_MATRIX_3D:
        mesh, u, rhs = bc_matrix_case(ns, mname)
        exact = loose = 0
        for bcs in ALL_BCS_3D:
            nd, na = _check(want, nn, _tag(ns), bcs, {"relax": port.relax3d(u, rhs, mesh, bcs),
                                                      "residual": port.residual3d(u, rhs, mesh, bcs),
                                                      "vcycle": port.vcycle(u, rhs, mesh, bcs)})
            exact += nd == 3
            loose += na == 3
        assert (exact, loose) == (63, 1), (ns, exact, loose)


def test_port_equals_reference_under_every_boundary_set_2d(port, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_bc_matrix.json")))
    nn = np.load(os.path.join(golden_dir, "reference_bc_matrix_NN.npz"))
    assert len(ALL_BCS_2D) == len(set(ALL_BCS_2D)) == 16
    for ns, mname in BC_MATRIX_2D:
        mesh, u, rhs = bc_matrix_case(ns, mname)
        exact = loose = 0
        for bcs in ALL_BCS_2D:
            nd, na = _check(want, nn, _tag(ns), bcs, {"relax": port.relax_nd(u, rhs, mesh, bcs),
                                                      "residual": port.residual_nd(u, rhs, mesh, bcs)})
            exact += nd == 2
            loose += na == 2
        assert (exact, loose) == (15, 1), (ns, exact, loose)


def test_fixture_holds_every_set_and_nothing_else(golden_dir):
    """the committed files name exactly the 63 + 15 digest sets and the two all-Neumann ones per shape"""
    want = json.load(open(os.path.join(golden_dir, "reference_bc_matrix.json")))
    nn = np.load(os.path.join(golden_dir, "reference_bc_matrix_NN.npz"))
    keys = {f"{k}_{_tag(ns)}_{b}" for ns, _m in BC_MATRIX_3D for b in ALL_BCS_3D[:-1] for k in ("relax", "residual", "vcycle")}
    keys |= {f"{k}_{_tag(ns)}_{b}" for ns, _m in BC_MATRIX_2D for b in ALL_BCS_2D[:-1] for k in ("relax", "residual")}
    assert ALL_BCS_3D[-1] == "NNNNNN" and ALL_BCS_2D[-1] == "NNNN"
    assert set(want) == keys and len(keys) == 2 * 63 * 3 + 2 * 15 * 2
    assert set(nn.files) == ({f"{k}_{_tag(ns)}" for ns, _m in BC_MATRIX_3D for k in ("relax", "residual", "vcycle")} |
                             {f"{k}_{_tag(ns)}" for ns, _m in BC_MATRIX_2D for k in ("relax", "residual")})
