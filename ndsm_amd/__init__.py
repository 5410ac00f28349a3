"""ndsm_amd - MI355X-native multigrid V-cycle behind the NDSM C ABI.

The product is the shared library ndsm_amd/lib/libndsm_hip.so (HIP kernels for
gfx950 + a Fortran 2003 host driver).  This package only holds the Python
loader that mirrors the reference's ndsm.py, and thin ctypes wrappers for the
additive C entry points.  There is no CPU fallback: without the library or
without an MI355X every call raises.
"""
from .ndsm import vector_potential, vector_potential_slab, get_lib_path  # noqa: F401
from ._lib import (load_library, lib_path, MGSolver, VecPot, World, slab_plan, poisson_solve,  # noqa: F401
                   NdsmHipError, Helicity, vector_potential_field, relative_helicity, Projection,
                   solenoidal_projection, devore_potentials, FieldLines, trace_field_lines,
                   field_line_helicity, QMap, squashing_factor, seed_plane, Nulls, find_nulls, FieldPaths, trace_paths,
                   path_of, whole_line, Skeleton, find_skeleton, spine_of, fan_of, connections, Separators,
                   find_separators, separator_of, QPerpMap, perpendicular_squashing, seed_cut, boundary_alpha,
                   map_alpha, vector_potential_current, force_free_field, boundary_weight, force_free_optimize,
                   preprocess_magnetogram, magnetogram_balance, resample, cascade_shapes, force_free_cascade,
                   measurement_weight, force_free_optimize_obs, resample_weighted, force_free_obs_cascade,
                   green_field_points, magnetogram_field, potential_open, lfff_field_points,
                   linear_force_free_field, best_alpha, Dips, find_dips, bald_patches, Flow, Fluxes, flow_fit,
                   plane_vector_potential, plane_vector_potential_points, boundary_fluxes, Patches,
                   partition_magnetogram, Connectivity, find_connectivity, connectivity_matrix)

__all__ = ["vector_potential", "vector_potential_slab", "get_lib_path", "load_library", "lib_path", "MGSolver", "VecPot", "poisson_solve",
           "NdsmHipError", "Helicity", "vector_potential_field", "relative_helicity", "Projection", "solenoidal_projection",
           "devore_potentials", "FieldLines", "trace_field_lines", "field_line_helicity", "QMap",
           "squashing_factor", "seed_plane", "Nulls", "find_nulls", "FieldPaths", "trace_paths", "path_of", "whole_line",
           "Skeleton", "find_skeleton", "spine_of", "fan_of", "connections", "Separators", "find_separators",
           "separator_of", "QPerpMap", "perpendicular_squashing", "seed_cut", "boundary_alpha", "map_alpha",
           "vector_potential_current", "force_free_field", "boundary_weight", "force_free_optimize",
           "preprocess_magnetogram", "magnetogram_balance", "resample", "cascade_shapes", "force_free_cascade",
           "measurement_weight", "force_free_optimize_obs", "resample_weighted", "force_free_obs_cascade",
           "green_field_points", "magnetogram_field", "potential_open", "lfff_field_points",
           "linear_force_free_field", "best_alpha", "Dips", "find_dips", "bald_patches", "Flow", "Fluxes", "flow_fit",
           "plane_vector_potential", "plane_vector_potential_points", "boundary_fluxes", "Patches",
           "partition_magnetogram", "Connectivity", "find_connectivity", "connectivity_matrix"]
