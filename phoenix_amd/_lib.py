"""ctypes binding of the C ABI declared in include/phoenix_hip.h.

There is NO fallback: if libphoenix_hip.so is missing the import fails loudly (build it with
`python -m phoenix_amd.build` or `__graft_entry__.build()`), and every entry point requires a GPU."""
import ctypes as C
import os

from . import build as _build

_LIB = None


class PhxParams(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Ws", "bs", "Wp", "bp", "WaT", "g")] + [("N", C.c_int), ("H", C.c_int),
                                                                                 ("wimg", C.c_void_p)]


class PhxGrads(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Ws", "bs", "Wp", "bp", "WaT", "g")] + [("overwrite", C.c_int), ("Wa", C.c_void_p)]


class PhxSolveOpts(C.Structure):
    _fields_ = [("method", C.c_int), ("control", C.c_int), ("rtol", C.c_double), ("atol", C.c_double),
                ("t_per_sample", C.c_int), ("t_is_f32", C.c_int), ("max_num_steps", C.c_longlong), ("calls", C.c_int),
                ("ws_keep", C.c_int)]


EXPORTS = ("phx_abi_version", "phx_status_string", "phx_device_cus", "phx_workspace_bytes", "phx_rhs_forward",
           "phx_rhs_vjp", "phx_odeint", "phx_odeint_adjoint_backward", "phx_debug_profile_region", "phx_debug_set_kernel_events",
           "phx_prior_targets", "phx_hill_rhs", "phx_hill_simulate", "phx_prior_mse", "phx_debug_adjoint_kernel",
           "phx_odeint_calls_workspace_bytes", "phx_weight_image_bytes", "phx_pack_weight_images", "phx_prior_targets_sell",
           "phx_debug_adjoint_kernel_m", "phx_prior_z_bytes", "phx_prior_mse_save", "phx_prior_vjp_saved",
           "phx_layout_params", "phx_debug_forward_kernel_m", "phx_debug_queue_kernel_events", "phx_debug_solve_launches",
           "phx_odeint_stepped", "phx_odeint_adjoint_backward_stepped", "phx_odeint_backprop_backward",
           "phx_odeint_backprop_workspace_bytes", "phx_debug_backprop_kernel_m", "phx_debug_backprop_launches",
           "phx_debug_backprop_plan",
           "phx_odeint_calls_grids_workspace_bytes", "phx_debug_calls_grids_kernel_m", "phx_debug_calls_grids_plan",
           "phx_debug_calls_grids_launches", "phx_debug_plan", "phx_influence_workspace_bytes", "phx_influence_scores",
           "phx_effects_workspace_bytes", "phx_effects_matrix", "phx_effects_edges_workspace_bytes", "phx_effects_edges",
           "phx_effects_rank_workspace_bytes", "phx_effects_gather", "phx_effects_rank_counts",
           "phx_effects_neighbors_workspace_bytes", "phx_effects_neighbors", "phx_pathway_permutations_workspace_bytes",
           "phx_pathway_permutations", "phx_hill_jacobian_workspace_bytes", "phx_hill_jacobian",
           "phx_odeint_clamped_workspace_bytes", "phx_odeint_clamped", "phx_knockout_effects_workspace_bytes",
           "phx_knockout_effects", "phx_hill_knockouts", "phx_debug_hill_knockouts_kpt", "phx_odeint_clamped_sets",
           "phx_knockout_epistasis_workspace_bytes", "phx_knockout_epistasis", "phx_debug_adj3_tail_words",
           "phx_hill_knockout_sets", "phx_effects_apply_workspace_bytes", "phx_effects_apply",
           "phx_odeint_clamped_rows_workspace_bytes", "phx_odeint_clamped_rows",
           "phx_odeint_adjoint_backward_clamped_rows", "phx_debug_clamped_rows_plan",
           "phx_reduced_jacobian_workspace_bytes", "phx_reduced_jacobian", "phx_steady_residual", "phx_steady_update",
           "phx_steady_solve_workspace_bytes", "phx_steady_solve", "phx_hill_steady_lds_bytes", "phx_hill_steady",
           "phx_steady_adjoint_project_workspace_bytes", "phx_steady_adjoint_project", "phx_steady_adjoint_back",
           "phx_steady_param_grads_workspace_bytes", "phx_steady_param_grads",
           "phx_steady_inverse_workspace_bytes", "phx_steady_inverse", "phx_steady_response_factors", "phx_steady_response")

OP_RHS_FORWARD, OP_RHS_VJP, OP_ODEINT, OP_ADJOINT = 0, 1, 2, 3
METHODS = {"euler": 0, "midpoint": 1, "rk4": 2, "dopri5": 3}
CTRL_SHARED, CTRL_PER_TRAJECTORY = 0, 1
EFFECTS_MODES = {"effects": 0, "mean": 1, "mean_abs": 2}     # phx_effects_mode
EDGES_ORIENT, EDGES_DIAGONAL = 1, 2                          # phx_edges_flags
EDGES_COUNT, EDGES_EMIT = 0, 1                               # phx_edges_pass
NEIGHBORS_AXES = {"regulator": 0, "target": 1}                # phx_neighbors_axis
NEIGHBORS_MAX_K = 64
APPLY_WEIGHTS = {"value": 0, "abs": 1, "unit": 2}            # phx_apply_weight
APPLY_MAX_R = 32                                             # columns of a block of phx_effects_apply
PATHWAYS_MAX_N = 16384                                       # phx_pathway_permutations: a gene is 14 bits of its sort key
PATHWAYS_MAX_R = 1 << 50                                     # ... and first + n_perm stays below this
EDGES_BINS = 4096                                            # workspace: uint32 hist[EDGES_BINS], then uint32 count
STATUS_TEXT = {
    1: "max_num_steps exceeded",
    2: "underflow in dt",
    3: "non-finite values in state `y`",
    4: "bad argument (t must be strictly increasing or decreasing)",
    5: "workspace too small",
    6: "HIP launch failure",
    7: "in-kernel grid barrier timed out",
}


def lib_path():
    # PHX_LIB names a diagnostic build of the same ABI (A/B timing of two builds); it is honoured only together with
    # PHX_DIAG=1 so that a stray variable in a production environment cannot swap the engine
    if os.environ.get("PHX_DIAG") == "1" and os.environ.get("PHX_LIB"):
        return os.environ["PHX_LIB"]
    return _build.LIB


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "phoenix_amd: %s not found. The HIP engine is the only execution path (no CPU fallback); "
            "build it with `python -m phoenix_amd.build`." % path)
    lib = C.CDLL(path)
    lib.phx_status_string.restype = C.c_char_p
    lib.phx_workspace_bytes.restype = C.c_size_t
    lib.phx_workspace_bytes.argtypes = [C.c_int] * 5
    vp = C.c_void_p
    lib.phx_rhs_forward.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    lib.phx_rhs_vjp.argtypes = [C.POINTER(PhxParams), vp, vp, vp, C.POINTER(PhxGrads), vp, C.c_int, C.c_int, vp,
                                C.c_size_t, vp]
    lib.phx_odeint.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, C.c_int, C.POINTER(PhxSolveOpts), vp, vp, vp,
                               vp, vp, C.c_size_t, vp]
    lib.phx_odeint_adjoint_backward.argtypes = [C.POINTER(PhxParams), vp, C.c_int, C.c_int, C.POINTER(PhxSolveOpts),
                                                vp, vp, vp, C.POINTER(PhxGrads), vp, vp, vp, vp, C.c_size_t, vp]
    lib.phx_odeint_stepped.argtypes = lib.phx_odeint.argtypes + [C.c_double]
    lib.phx_odeint_adjoint_backward_stepped.argtypes = lib.phx_odeint_adjoint_backward.argtypes + [C.c_double]
    lib.phx_odeint_backprop_backward.argtypes = lib.phx_odeint_adjoint_backward.argtypes + [C.c_double, C.c_longlong]
    lib.phx_odeint_backprop_workspace_bytes.argtypes = [C.c_int] * 4 + [C.c_longlong]
    lib.phx_odeint_backprop_workspace_bytes.restype = C.c_size_t
    lib.phx_debug_backprop_kernel_m.argtypes = [C.c_int] * 5
    lib.phx_debug_backprop_launches.argtypes = [C.c_int] * 5
    lib.phx_debug_backprop_plan.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]
    lib.phx_prior_targets.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.phx_prior_targets_sell.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.phx_prior_mse.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, vp, vp, vp, C.c_size_t, vp]
    lib.phx_prior_z_bytes.restype = C.c_size_t
    lib.phx_prior_z_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.phx_prior_mse_save.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]
    lib.phx_prior_vjp_saved.argtypes = [C.POINTER(PhxParams), vp, vp, vp, C.POINTER(PhxGrads), C.c_int, vp, C.c_size_t, vp]
    lib.phx_hill_rhs.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.phx_hill_simulate.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_double, vp, C.c_int, C.c_int, vp]
    lib.phx_debug_set_kernel_events.argtypes = [vp, vp]
    lib.phx_debug_set_kernel_events.restype = None
    lib.phx_debug_queue_kernel_events.argtypes = [vp, vp]
    lib.phx_debug_queue_kernel_events.restype = None
    lib.phx_debug_adjoint_kernel.argtypes = [C.c_int] * 5
    lib.phx_debug_adjoint_kernel_m.argtypes = [C.c_int] * 6
    lib.phx_odeint_calls_workspace_bytes.argtypes = [C.c_int] * 5
    lib.phx_odeint_calls_workspace_bytes.restype = C.c_size_t
    lib.phx_odeint_calls_grids_workspace_bytes.argtypes = [C.c_int] * 6
    lib.phx_odeint_calls_grids_workspace_bytes.restype = C.c_size_t
    lib.phx_debug_calls_grids_kernel_m.argtypes = [C.c_int] * 6
    lib.phx_debug_calls_grids_plan.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]
    lib.phx_debug_calls_grids_launches.argtypes = [C.c_int] * 6
    lib.phx_debug_plan.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_longlong)]
    lib.phx_weight_image_bytes.argtypes = [C.c_int, C.c_int]
    lib.phx_weight_image_bytes.restype = C.c_size_t
    lib.phx_pack_weight_images.argtypes = [C.POINTER(PhxParams), vp, vp]
    lib.phx_layout_params.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.phx_debug_forward_kernel_m.argtypes = [C.c_int] * 6
    lib.phx_debug_solve_launches.argtypes = [C.c_int] * 7
    lib.phx_debug_adj3_tail_words.argtypes = [C.POINTER(C.c_size_t)] * 2
    lib.phx_influence_workspace_bytes.argtypes = [C.c_int] * 4
    lib.phx_influence_workspace_bytes.restype = C.c_size_t
    lib.phx_influence_scores.argtypes = [vp] + [C.c_int] * 4 + [C.POINTER(C.c_int), vp, vp, vp, C.c_size_t, vp]
    lib.phx_effects_workspace_bytes.argtypes = [C.c_int] * 4
    lib.phx_effects_workspace_bytes.restype = C.c_size_t
    lib.phx_effects_matrix.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp] + [C.c_int] * 3 + [vp, vp, C.c_size_t, vp]
    lib.phx_effects_edges_workspace_bytes.argtypes = [C.c_int] * 4
    lib.phx_effects_edges_workspace_bytes.restype = C.c_size_t
    lib.phx_effects_edges.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp] + [C.c_int] * 4 + \
        [C.c_uint, C.c_float, vp, vp, C.c_uint, vp, C.c_size_t, vp]
    lib.phx_effects_rank_workspace_bytes.argtypes = [C.c_int] * 4
    lib.phx_effects_rank_workspace_bytes.restype = C.c_size_t
    lib.phx_effects_gather.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_uint, vp, vp]
    lib.phx_effects_rank_counts.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_uint, vp, vp,
                                            C.c_size_t, vp]
    lib.phx_effects_neighbors_workspace_bytes.argtypes = [C.c_int] * 6
    lib.phx_effects_neighbors_workspace_bytes.restype = C.c_size_t
    lib.phx_effects_neighbors.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp] + [C.c_int] * 4 + \
        [C.c_float, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.phx_effects_apply_workspace_bytes.argtypes = [C.c_int] * 6
    lib.phx_effects_apply_workspace_bytes.restype = C.c_size_t
    lib.phx_effects_apply.argtypes = [C.POINTER(PhxParams), C.c_int, vp, vp] + [C.c_int] * 4 + \
        [C.c_float, vp, vp, vp, C.c_int, vp, vp, C.c_size_t, vp]
    lib.phx_pathway_permutations_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong]
    lib.phx_pathway_permutations_workspace_bytes.restype = C.c_size_t
    lib.phx_pathway_permutations.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_longlong, C.c_ulonglong, C.c_longlong,
                                             C.c_longlong, vp, vp, vp, vp, vp, C.c_size_t, vp]
    lib.phx_hill_jacobian_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int]
    lib.phx_hill_jacobian_workspace_bytes.restype = C.c_size_t
    lib.phx_hill_jacobian.argtypes = [vp] * 7 + [C.c_int, C.c_int, C.c_longlong, C.c_int, vp, vp, C.c_size_t, vp]
    lib.phx_odeint_clamped_workspace_bytes.argtypes = [C.c_int] * 5
    lib.phx_odeint_clamped_workspace_bytes.restype = C.c_size_t
    lib.phx_odeint_clamped.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, C.c_int, C.POINTER(PhxSolveOpts), vp, vp, vp,
                                       vp, vp, vp, C.c_size_t, vp]
    lib.phx_knockout_effects_workspace_bytes.argtypes = [C.c_int] * 4
    lib.phx_knockout_effects_workspace_bytes.restype = C.c_size_t
    lib.phx_knockout_effects.argtypes = [vp, vp] + [C.c_int] * 4 + [C.POINTER(C.c_int), vp, vp, vp, vp, C.c_size_t, vp]
    lib.phx_hill_knockouts.argtypes = [vp] * 6 + [C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, vp,
                                       C.c_int, C.c_int, vp]
    lib.phx_debug_hill_knockouts_kpt.argtypes = [C.c_int]
    lib.phx_hill_knockout_sets.argtypes = [vp] * 6 + [C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                           C.c_int, vp, C.c_int, C.c_int, vp]
    lib.phx_odeint_clamped_sets.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, C.c_int, C.POINTER(PhxSolveOpts), vp,
                                            C.c_int, vp, vp, vp, vp, vp, C.c_size_t, vp]
    # (an earlier build of ABI 7 named by PHX_LIB for an A/B timing of the unclamped paths has no per-row clamp)
    if path == _build.LIB or hasattr(lib, "phx_odeint_clamped_rows"):
        lib.phx_odeint_clamped_rows_workspace_bytes.argtypes = [C.c_int] * 5
        lib.phx_odeint_clamped_rows_workspace_bytes.restype = C.c_size_t
        lib.phx_odeint_clamped_rows.argtypes = lib.phx_odeint_clamped_sets.argtypes
        lib.phx_odeint_adjoint_backward_clamped_rows.argtypes = [C.POINTER(PhxParams), vp, C.c_int, C.c_int,
                                                                 C.POINTER(PhxSolveOpts), vp, C.c_int, vp, vp, vp,
                                                                 C.POINTER(PhxGrads), vp, vp, vp, vp, C.c_size_t, vp]
        lib.phx_debug_clamped_rows_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    lib.phx_knockout_epistasis_workspace_bytes.argtypes = [C.c_int] * 5
    lib.phx_knockout_epistasis_workspace_bytes.restype = C.c_size_t
    lib.phx_knockout_epistasis.argtypes = ([vp] * 3 + [C.c_int] * 5 + [C.POINTER(C.c_int)] * 3 + [vp] * 7 +
                                           [C.c_size_t, vp])
    # (the same: an earlier build of ABI 7 has no steady-state unit)
    if path == _build.LIB or hasattr(lib, "phx_reduced_jacobian"):
        lib.phx_reduced_jacobian_workspace_bytes.argtypes = [C.c_int] * 3
        lib.phx_reduced_jacobian_workspace_bytes.restype = C.c_size_t
        lib.phx_reduced_jacobian.argtypes = [C.POINTER(PhxParams), vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]
        lib.phx_steady_residual.argtypes = [C.POINTER(PhxParams), vp, C.c_int, vp, vp, vp]
        lib.phx_steady_update.argtypes = [C.POINTER(PhxParams), vp, vp, vp, vp, C.c_int, vp, vp]
        lib.phx_steady_solve_workspace_bytes.argtypes = [C.c_int] * 2
        lib.phx_steady_solve_workspace_bytes.restype = C.c_size_t
        lib.phx_steady_solve.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_size_t, vp]
    if path == _build.LIB or hasattr(lib, "phx_hill_steady"):
        lib.phx_hill_steady_lds_bytes.argtypes = [C.c_int, C.c_longlong, C.c_int]
        lib.phx_hill_steady_lds_bytes.restype = C.c_size_t
        lib.phx_hill_steady.argtypes = [vp] * 6 + [C.c_longlong, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int,
                                        C.c_double, C.c_int, C.c_double, vp, vp, vp, vp, vp, vp]
    # (the same: an earlier build of ABI 7 has no steady-state adjoint)
    if path == _build.LIB or hasattr(lib, "phx_steady_param_grads"):
        lib.phx_steady_adjoint_project_workspace_bytes.argtypes = [C.c_int] * 3
        lib.phx_steady_adjoint_project_workspace_bytes.restype = C.c_size_t
        lib.phx_steady_adjoint_project.argtypes = [C.POINTER(PhxParams), vp, vp, C.c_int, vp, vp, C.c_size_t, vp]
        lib.phx_steady_adjoint_back.argtypes = [C.POINTER(PhxParams), vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
        lib.phx_steady_param_grads_workspace_bytes.argtypes = [C.c_int] * 3
        lib.phx_steady_param_grads_workspace_bytes.restype = C.c_size_t
        lib.phx_steady_param_grads.argtypes = [C.POINTER(PhxParams), vp, vp, vp, vp, C.c_int, C.POINTER(PhxGrads), vp, C.c_size_t,
                                               vp]
    # (the same: an earlier build of ABI 7 has no steady-state response)
    if path == _build.LIB or hasattr(lib, "phx_steady_response"):
        lib.phx_steady_inverse_workspace_bytes.argtypes = [C.c_int] * 2
        lib.phx_steady_inverse_workspace_bytes.restype = C.c_size_t
        lib.phx_steady_inverse.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_size_t, vp]
        lib.phx_steady_response_factors.argtypes = [C.POINTER(PhxParams), vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp,
                                                    vp]
        lib.phx_steady_response.argtypes = [C.POINTER(PhxParams), vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp,
                                            C.c_longlong, vp]
    assert lib.phx_abi_version() == 7
    _LIB = lib
    return lib
