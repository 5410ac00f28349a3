#!/usr/bin/env python3
"""Generate the committed golden vectors from the REFERENCE ITSELF.

Run in the build container only (needs /root/reference and `make -C oracle ref`):

    python tests/golden/make_golden.py

Every expected output below is produced by the reference's own Fortran,
compiled unmodified into oracle/_ref/ (oracle/Makefile), either through its
public C ABI (`ndsm_vector_solve`, ndsm_python_wrapper.f90:56) or through
oracle/ref_shim.f90, a pass-through to its PUBLIC module procedures.  Inputs
are re-creatable from the seeds stored next to the outputs (see
tests/golden_inputs.py), so the files stay small.  Nothing here is reference
source text - only numbers.

OMP_NUM_THREADS is forced to 1 so the all-Neumann `mean` reduction
(ndsm_multigrid_core.f90:1214) is summed in serial order.
"""
import json
import os
import sys

os.environ["OMP_NUM_THREADS"] = "1"

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from golden_inputs import (BCS3, BCS_ANISO, BCS_RANDOM, analytic_case, aniso_mesh, aniso_pipeline_cases,  # noqa: E402
                           digest, digest16, manufactured_poisson, negative_option_cases, noisy_case, option_matrix,
                           pipeline_option_cases, quirk_case, rand_field, random_reference_cases, scalar_kw,
                           scalar_option_problems, zero_field_cases, bc_matrix_case,
                           ALL_BCS_2D, ALL_BCS_3D, BC_MATRIX_2D, BC_MATRIX_3D,
                           ANISO_SHAPE_2D, ANISO_SHAPES_3D, KERNEL_SHAPES_3D, KERNEL_SHAPES_2D, OPTION_PIPELINE_SHAPE,
                           OPTION_SCALAR_3D)
from oracle import Oracle, have_ref, uniform_mesh  # noqa: E402


def main():
    assert have_ref(), "build the reference first: make -C oracle ref"
    R = Oracle("ref")

    # ---- per-operator vectors, 3-D --------------------------------------
    for ns in KERNEL_SHAPES_3D:
        tag = "x".join(str(n) for n in ns)
        mesh = uniform_mesh(ns)
        shp = tuple(ns[::-1])
        u = rand_field(shp, 2112)
        rhs = rand_field(shp, 2113)
        out = {}
        shapes, meshes = R.hierarchy(ns, mesh)
        out["level_shapes"] = shapes
        for l, lv in enumerate(meshes):
            for d, m in enumerate(lv):
                out[f"mesh_l{l+1}_d{d+1}"] = m
        for bcs in BCS3:
            out[f"relax_{bcs}"] = R.relax3d(u, rhs, mesh, bcs)
            out[f"residual_{bcs}"] = R.residual3d(u, rhs, mesh, bcs)
            out[f"vcycle_{bcs}"] = R.vcycle(u, rhs, mesh, bcs)
        for lvl in range(1, len(shapes)):
            f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
            c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
            out[f"restrict_l{lvl}"] = R.restrict(f, ns, mesh, lvl)
            out[f"interp_l{lvl}"] = R.interp(c, ns, mesh, lvl)
        un = u.copy()
        out["update_u"] = np.array(R.update_u(rhs, un))
        np.savez(os.path.join(HERE, f"kernels3d_{tag}.npz"), **out)
        print("wrote kernels3d_" + tag)

    # ---- per-operator vectors, 2-D (generic N-D path) --------------------
    for ns in KERNEL_SHAPES_2D:
        tag = "x".join(str(n) for n in ns)
        mesh = uniform_mesh(ns)
        shp = tuple(ns[::-1])
        u = rand_field(shp, 2112)
        rhs = rand_field(shp, 2113)
        rhs0 = rhs - rhs.mean()
        out = {}
        shapes, _ = R.hierarchy(ns, mesh)
        out["level_shapes"] = shapes
        for bcs in ("NNNN", "DNND"):
            out[f"relax_{bcs}"] = R.relax_nd(u, rhs, mesh, bcs)
            out[f"residual_{bcs}"] = R.residual_nd(u, rhs, mesh, bcs)
        out["vcycle_NNNN"] = R.vcycle(u, rhs0, mesh, "NNNN")
        ierr, us, du = R.solve_bvp(np.zeros(shp), rhs0, mesh, "NNNN")
        out["solve_NNNN"] = us
        out["solve_NNNN_meta"] = np.array([ierr, du])
        for lvl in range(1, len(shapes)):
            f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
            c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
            out[f"restrict_l{lvl}"] = R.restrict(f, ns, mesh, lvl)
            out[f"interp_l{lvl}"] = R.interp(c, ns, mesh, lvl)
        np.savez(os.path.join(HERE, f"kernels2d_{tag}.npz"), **out)
        print("wrote kernels2d_" + tag)

    # ---- full Poisson solves (manufactured solution), history of du ------
    hist = {}
    for ns in ([22, 22, 22], [33, 22, 27], [64, 64, 64]):
        tag = "x".join(str(n) for n in ns)
        mesh = uniform_mesh(ns)
        for bcs in BCS3:
            us, rhs = manufactured_poisson(mesh, bcs)
            u = np.zeros_like(us)
            dus = []
            # the reference only prints du; replay its loop (ndsm_poisson.f90:116-141)
            # one v_cycle + update_u at a time to record it
            prev = u.copy()
            for it in range(64):
                cur = R.vcycle(prev, rhs, mesh, bcs)
                d = float(np.abs(cur - prev).max())
                dus.append(d)
                prev = cur
                if d < 1e-10:
                    break
            ierr, uref, du_last = R.solve_bvp(u, rhs, mesh, bcs)
            assert ierr == 0 and np.array_equal(uref, prev) and du_last == dus[-1]
            key = f"{tag}_{bcs}"
            hist[key] = {"du": dus, "ncycles": len(dus), "err_vs_exact": float(np.abs(uref - us).max())}
            if ns[0] <= 33:
                np.save(os.path.join(HERE, f"solve3d_{key}.npy"), uref)
            else:  # 64^3: keep three orthogonal mid-planes only
                np.savez(os.path.join(HERE, f"solve3d_{key}_planes.npz"), kz=uref[ns[2] // 2],
                         jy=uref[:, ns[1] // 2], ix=uref[:, :, ns[0] // 2])
    with open(os.path.join(HERE, "solve3d_history.json"), "w") as fh:
        json.dump(hist, fh, indent=1)
    print("wrote solve3d_*")

    # ---- full pipeline through the reference C ABI -----------------------
    rows = {}
    for n in (22, 44):
        x, y, z, A1, b1 = analytic_case(n)
        ierr, A, B, ioptc, ropt = R.vector_potential(x, y, z, b1)
        eA = np.linalg.norm(A1 - A, axis=0)
        eB = np.linalg.norm(b1 - B, axis=0)
        rows[str(n)] = {"ierr": int(ierr), "dx": float(x[1] - x[0]), "Ea_max": float(eA.max()),
                        "Ea_avg": float(eA.mean()), "Eb_max": float(eB.max()), "Eb_avg": float(eB.mean())}
        if n == 22:
            np.savez(os.path.join(HERE, "pipeline_22.npz"), A=A, B=B, ioptc=ioptc)
    # anisotropic shape, equal spacing (unequal spacings, where quirk Q4 is live: aniso() below)
    ns = [33, 22, 27]
    x, y, z, A1, b1 = analytic_case(ns)
    ierr, A, B, ioptc, ropt = R.vector_potential(x, y, z, b1)
    np.savez(os.path.join(HERE, "pipeline_33x22x27.npz"), A=A, B=B, ioptc=ioptc)
    rows["33x22x27"] = {"ierr": int(ierr)}
    with open(os.path.join(HERE, "pipeline_rows.json"), "w") as fh:
        json.dump(rows, fh, indent=1)
    print("wrote pipeline_*")
    random_and_quirks(R)


def random_and_quirks(R):
    """test_oracle.py's random-input and quirk checks: sha256 of the bit-identical outputs, the all-Neumann
    sweeps (compared within 1e-14) in full, and the flags of the quirk calls"""
    digests, nn = {}, {}
    for ns, mesh, u, rhs in random_reference_cases():
        tag = "x".join(str(n) for n in ns)
        for bcs in BCS_RANDOM:
            a = R.relax3d(u, rhs, mesh, bcs)
            if bcs == "NNNNNN":
                nn[f"relax_{tag}"] = a
            else:
                digests[f"relax_{tag}_{bcs}"] = digest(a)
            digests[f"residual_{tag}_{bcs}"] = digest(R.residual3d(u, rhs, mesh, bcs))
        digests[f"vcycle_{tag}_DNDDND_ms3"] = digest(R.vcycle(u, rhs, mesh, "DNDDND", ms=3))
    with open(os.path.join(HERE, "reference_random.json"), "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "reference_random_NNNNNN.npz"), **nn)
    x, y, z, b = quirk_case()
    ierr, _, _, ioptc, _ = R.vector_potential(x, y, z, b, ncycles_max=2)
    quirks = {"top_face_zero": {"ierr": int(ierr), "ioptc": [int(v) for v in ioptc]}}
    x, y, z, A1, b1 = analytic_case(24)
    ierr, _, _, ioptc, _ = R.vector_potential(x, y, z, b1, ncycles_max=2)
    quirks["analytic"] = {"ierr": int(ierr), "ioptc": [int(v) for v in ioptc]}
    with open(os.path.join(HERE, "reference_quirks.json"), "w") as fh:
        json.dump(quirks, fh, indent=1)
    print("wrote reference_random*, reference_quirks.json")
    aniso(R)


def aniso(R):
    """test_oracle.py's anisotropic checks (golden_inputs.aniso_mesh: a spacing of its own on every axis, no origin
    at 0): sha256 of the bit-identical 3-D outputs and solve histories in reference_aniso.json, the 2-D outputs that
    carry the all-Neumann mean in reference_aniso_2d.npz, and the pipeline - where quirk Q4 is live - in
    pipeline_aniso_*.npz"""
    want = {}
    for ns in ANISO_SHAPES_3D:
        tag = "x".join(str(n) for n in ns)
        mesh = aniso_mesh(ns)
        shp = tuple(ns[::-1])
        u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
        out = {}
        shapes, meshes = R.hierarchy(ns, mesh)
        out["level_shapes"] = shapes.tolist()
        for l, lv in enumerate(meshes):
            for d, m in enumerate(lv):
                out[f"mesh_l{l+1}_d{d+1}"] = digest(m)
        for bcs in BCS_ANISO:
            out[f"relax_{bcs}"] = digest(R.relax3d(u, rhs, mesh, bcs))
            out[f"residual_{bcs}"] = digest(R.residual3d(u, rhs, mesh, bcs))
            out[f"vcycle_{bcs}"] = digest(R.vcycle(u, rhs, mesh, bcs))
        for lvl in range(1, len(shapes)):
            f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
            c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
            out[f"restrict_l{lvl}"] = digest(R.restrict(f, ns, mesh, lvl))
            out[f"interp_l{lvl}"] = digest(R.interp(c, ns, mesh, lvl))
        want[tag] = out
    # solve histories (the loop of main(), one V-cycle at a time) on the first shape
    ns = ANISO_SHAPES_3D[0]
    tag = "x".join(str(n) for n in ns)
    mesh = aniso_mesh(ns)
    for bcs in BCS3:
        us, rhs = manufactured_poisson(mesh, bcs)
        prev, dus = np.zeros_like(us), []
        for it in range(64):
            cur = R.vcycle(prev, rhs, mesh, bcs)
            d = float(np.abs(cur - prev).max())
            dus.append(d)
            prev = cur
            if d < 1e-10:
                break
        ierr, uref, du_last = R.solve_bvp(np.zeros_like(us), rhs, mesh, bcs)
        assert ierr == 0 and np.array_equal(uref, prev) and du_last == dus[-1]
        want[f"solve_{tag}_{bcs}"] = {"du": dus, "ncycles": len(dus), "u": digest(uref)}
    with open(os.path.join(HERE, "reference_aniso.json"), "w") as fh:
        json.dump(want, fh, indent=1, sort_keys=True)
    # 2-D: the generic N-D path, as in main()
    ns = ANISO_SHAPE_2D
    mesh = aniso_mesh(ns)
    shp = tuple(ns[::-1])
    u, rhs = rand_field(shp, 2112), rand_field(shp, 2113)
    rhs0 = rhs - rhs.mean()
    out = {}
    shapes, _ = R.hierarchy(ns, mesh)
    out["level_shapes"] = shapes
    for bcs in ("NNNN", "DNND"):
        out[f"relax_{bcs}"] = R.relax_nd(u, rhs, mesh, bcs)
        out[f"residual_{bcs}"] = R.residual_nd(u, rhs, mesh, bcs)
    out["vcycle_NNNN"] = R.vcycle(u, rhs0, mesh, "NNNN")
    ierr, us, du = R.solve_bvp(np.zeros(shp), rhs0, mesh, "NNNN")
    out["solve_NNNN"] = us
    out["solve_NNNN_meta"] = np.array([ierr, du])
    for lvl in range(1, len(shapes)):
        f = rand_field(tuple(int(v) for v in shapes[lvl - 1][::-1]), 3000 + lvl)
        c = rand_field(tuple(int(v) for v in shapes[lvl][::-1]), 4000 + lvl)
        out[f"restrict_l{lvl}"] = R.restrict(f, ns, mesh, lvl)
        out[f"interp_l{lvl}"] = R.interp(c, ns, mesh, lvl)
    np.savez_compressed(os.path.join(HERE, "reference_aniso_2d.npz"), **out)
    for name, x, y, z, b in aniso_pipeline_cases():
        ierr, A, B, ioptc, ropt = R.vector_potential(x, y, z, b)
        np.savez_compressed(os.path.join(HERE, f"pipeline_aniso_{name}.npz"), A=A, B=B, ioptc=ioptc)
    print("wrote reference_aniso*, pipeline_aniso_*")
    options(R)
    bc_matrix(R)


def options(R):
    """test_oracle.py's option checks (edge values of ms, ncycles, nmaxex, the tolerances and the metric; negative
    values; an all-zero field): reference_options.json holds numbers only - per case what the call returned (ierr,
    the ioptc it left, du_last where the entry returns one) and digest16 of the arrays.  The case lists are
    golden_inputs' (pipeline_option_cases, negative_option_cases, zero_field_cases, scalar_option_problems x
    option_matrix), in their order."""
    def pipe(x, y, z, b, kw):
        ierr, A, B, ioptc, _ropt = R.vector_potential(x, y, z, b, **kw)
        assert np.isfinite(A).all() and np.isfinite(B).all(), kw
        return [int(ierr), [int(v) for v in ioptc], digest16(A), digest16(B)]

    def scalar(u, rhs, mesh, bcs, kw):
        ierr, us, du = R.solve_bvp(u, rhs, mesh, bcs, **kw)
        assert np.isfinite(us).all(), (bcs, kw)
        return [int(ierr), float(du), digest16(us)]

    out = {}
    x, y, z, b = noisy_case(OPTION_PIPELINE_SHAPE)
    out["pipeline"] = [pipe(x, y, z, b, kw) for kw in pipeline_option_cases()]
    out["pipeline_negative"] = [pipe(x, y, z, b, kw) for kw in negative_option_cases()]
    out["pipeline_zero_field"] = [pipe(x, y, z, np.zeros_like(b), kw) for kw in zero_field_cases()]
    out["scalar"] = {}
    for name, ns, mesh, bcs, u, rhs in scalar_option_problems():
        out["scalar"][name] = [scalar(u, rhs, mesh, bcs, scalar_kw(*t)) for t in option_matrix()]
    name, ns, mesh, bcs, u, rhs = next(iter(scalar_option_problems()))
    assert ns == OPTION_SCALAR_3D
    out["scalar_negative"] = [scalar(u, rhs, mesh, bcs, kw) for kw in (
        dict(ms=-1, nmax=3), dict(nmax=-2), dict(nmax_exact=-3, nmax=3), dict(vc_tol=-1.0, nmax=3),
        dict(ex_tol=-1.0, nmax=3, nmax_exact=50), dict(vc_tol=float("nan"), nmax=3))]
    z0 = np.zeros_like(u)
    out["scalar_zero_field"] = [scalar(z0, z0, mesh, bcs, dict(vc_tol=vt, nmax=3)) for vt in (0.0, 1e-10)]
    with open(os.path.join(HERE, "reference_options.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote reference_options.json")


def bc_matrix(R):
    """test_oracle_bc_matrix.py: every boundary letter set (golden_inputs.ALL_BCS_3D / ALL_BCS_2D) on the shapes of
    BC_MATRIX_3D / BC_MATRIX_2D - sha256 of relax3d, residual3d and vcycle (3-D) and of relax_nd and residual_nd (2-D)
    in reference_bc_matrix.json for every set but the all-Neumann one, whose outputs (the mean is summed in the
    reference's own order) go to reference_bc_matrix_NN.npz in full"""
    want, nn = {}, {}
    for ns, mname in BC_MATRIX_3D:
        tag = "x".join(str(n) for n in ns)
        mesh, u, rhs = bc_matrix_case(ns, mname)
        for bcs in ALL_BCS_3D:
            out = {"relax": R.relax3d(u, rhs, mesh, bcs), "residual": R.residual3d(u, rhs, mesh, bcs),
                   "vcycle": R.vcycle(u, rhs, mesh, bcs)}
            for k, a in out.items():
                assert np.isfinite(a).all(), (tag, bcs, k)
                if bcs == "NNNNNN":
                    nn[f"{k}_{tag}"] = a
                else:
                    want[f"{k}_{tag}_{bcs}"] = digest(a)
    for ns, mname in BC_MATRIX_2D:
        tag = "x".join(str(n) for n in ns)
        mesh, u, rhs = bc_matrix_case(ns, mname)
        for bcs in ALL_BCS_2D:
            out = {"relax": R.relax_nd(u, rhs, mesh, bcs), "residual": R.residual_nd(u, rhs, mesh, bcs)}
            for k, a in out.items():
                assert np.isfinite(a).all(), (tag, bcs, k)
                if bcs == "NNNN":
                    nn[f"{k}_{tag}"] = a
                else:
                    want[f"{k}_{tag}_{bcs}"] = digest(a)
    with open(os.path.join(HERE, "reference_bc_matrix.json"), "w") as fh:
        json.dump(want, fh, indent=0, sort_keys=True)
        fh.write("\n")
    np.savez_compressed(os.path.join(HERE, "reference_bc_matrix_NN.npz"), **nn)
    print("wrote reference_bc_matrix*")


if __name__ == "__main__":
    if sys.argv[1:] == ["options"]:         # only reference_options.json
        assert have_ref(), "build the reference first: make -C oracle ref"
        options(Oracle("ref"))
    elif sys.argv[1:] == ["bc_matrix"]:     # only reference_bc_matrix*
        assert have_ref(), "build the reference first: make -C oracle ref"
        bc_matrix(Oracle("ref"))
    else:
        main()
