"""ctypes binding of the libdfx C ABI (``include/dfx.h``).

The product loads ``difflexmm_amd/libdfx.so`` (hand-written HIP kernels for gfx950) and raises when it is
missing -- there is no CPU fallback.  ``Engine`` is a thin, NumPy-only wrapper of one ``dfx_handle``.
"""
import ctypes as C
import os

import numpy as np

DFX_MAX_FNS = 2
DFX_FN_PARAMS = 5

BOND_LINEARIZED, BOND_NONLINEAR, BOND_SIMPLE_SPRING, BOND_STRETCH_TORSION = 0, 1, 2, 3
CONTACT_NONE, CONTACT_ANGLE, CONTACT_DISTANCE = 0, 1, 2
TABLEAU = {"dopri5": 0, "rk4": 1}
OBJ_KINETIC, OBJ_ANGULAR_MOMENTUM = 0, 1
XCORR_NORMS = {"reference": 0, "coefficient": 1, "none": 2}          # DFX_XCORR_NORM_*
XCORR_REDUCES = {"at": 0, "max": 1, "softmax": 2}                    # DFX_XCORR_AT / _MAX / _SOFTMAX
PEAK_KS, PEAK_PNORM = 0, 1                                           # DFX_PEAK_*
FN_ZERO, FN_PULSE, FN_HARMONIC, FN_RAMP, FN_SECH2TANH, FN_CONSTANT, FN_RAMP_CAP, FN_TABLE = range(8)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class dfx_special(C.Structure):
    _fields_ = [("block", C.c_int32), ("con_mask", C.c_int32),
                ("con_coef", (C.c_double * DFX_MAX_FNS) * 3), ("load_coef", (C.c_double * DFX_MAX_FNS) * 3)]


class dfx_problem(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_npb", C.c_int32), ("n_bonds", C.c_int32), ("bonds", _ip),
                ("bond_model", C.c_int32), ("contact", C.c_int32), ("n_special", C.c_int32),
                ("special", C.POINTER(dfx_special)), ("n_fns", C.c_int32), ("fn_type", C.c_int32 * DFX_MAX_FNS),
                ("batch", C.c_int32), ("tableau", C.c_int32), ("device", C.c_int32),
                ("fn_table_n", C.c_int32 * DFX_MAX_FNS), ("fn_table", _dp * DFX_MAX_FNS), ("streams", C.c_int32)]


_PARAM_FIELDS = ["centroid_node_vectors", "reference_vector", "k_bond", "inertia", "damping", "void_angle0",
                 "contact", "fn_params"]


class dfx_params(C.Structure):
    _fields_ = [(n, _dp) for n in _PARAM_FIELDS + ["block_centroids"]]


class dfx_grads(C.Structure):
    _fields_ = [(n, _dp) for n in _PARAM_FIELDS + ["state0", "block_centroids"]]


class dfx_stats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("rhs_evals", C.c_int64), ("launches", C.c_int64),
                ("kernel_ms", C.c_double), ("stage_kernel_us", C.c_double), ("streams", C.c_int64),
                ("stage_checkpoint", C.c_int64), ("checkpoint_records", C.c_int64), ("tile_kernels", C.c_int64)]


class dfx_design_map(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_npb", C.c_int32), ("n_bonds", C.c_int32), ("n_design", C.c_int32),
                ("base", _dp), ("gather", _ip), ("ref_points", _dp), ("bonds", _ip)]


EXPORTS = ["dfx_create", "dfx_destroy", "dfx_last_error", "dfx_set_params", "dfx_reserve", "dfx_forward", "dfx_forward_grid", "dfx_forward_grid_members",
           "dfx_forward_adaptive", "dfx_forward_adaptive_keep", "dfx_adaptive_step_counts", "dfx_adaptive_step_times", "dfx_adjoint",
           "dfx_objective_kinetic", "dfx_adjoint_kinetic", "dfx_kinetic_value_and_grad", "dfx_response_data", "dfx_rhs", "dfx_rhs_vjp", "dfx_energy",
           "dfx_device_count", "dfx_version", "dfx_share_checkpoint", "dfx_abi_layout", "dfx_member_status", "dfx_set_failure_policy",
           "dfx_test_set_spin_limit", "dfx_design_forward", "dfx_design_vjp"]
# multi-GPU collective (RCCL inside libdfx), device helpers and forward mode: HIP library only
COMM_EXPORTS = ["dfx_comm_unique_id", "dfx_comm_init", "dfx_comm_destroy", "dfx_comm_rccl_version", "dfx_comm_rank", "dfx_comm_size",
                "dfx_gather_objectives", "dfx_reduce_grads", "dfx_comm_allreduce", "dfx_comm_barrier", "dfx_comm_last_error",
                "dfx_mem_info", "dfx_device_synchronize", "dfx_kinetic_value_and_grad_device", "dfx_download", "dfx_forward_kinetic_value_and_grad",
                "dfx_forward_tangent", "dfx_forward_tangent_dense", "dfx_dense_output_map", "dfx_forward_tangent_multi",
                "dfx_forward_tangent_dense_multi", "dfx_rhs_jvp", "dfx_objective_value", "dfx_objective_value_and_grad",
                "dfx_strain_objective_value", "dfx_strain_objective_value_and_grad", "dfx_signal_values", "dfx_signal_hinge_channels", "dfx_signal_misfit_value",
                "dfx_signal_misfit_value_and_grad", "dfx_signal_projections", "dfx_signal_projection_value",
                "dfx_signal_projection_value_and_grad", "dfx_forward_tangent_signals_multi", "dfx_forward_tangent_signals_dense_multi",
                "dfx_signal_xcorr", "dfx_signal_xcorr_value", "dfx_signal_xcorr_value_and_grad", "dfx_strain_peak_value",
                "dfx_strain_peak_value_and_grad", "dfx_fn_table_values", "dfx_fn_table_grads", "dfx_fn_table_grad", "dfx_drive_cotangent",
                "dfx_fn_table_tangents"]
EXPORTS = EXPORTS + COMM_EXPORTS


def abi_layout():
    """sizeof + field offsets of the five public structs as THIS module mirrors them, in the order dfx_abi_layout reports."""
    out = []
    for cls in (dfx_special, dfx_problem, dfx_params, dfx_grads, dfx_stats):
        out.append(C.sizeof(cls))
        out += [getattr(cls, name).offset for name, _ in cls._fields_]
    return out


def check_abi_layout(lib):
    """A library whose structs are laid out differently from the ctypes mirrors above would read garbage silently: refuse it."""
    want = abi_layout()
    buf = (C.c_int32 * len(want))()
    lib.dfx_abi_layout.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    lib.dfx_abi_layout.restype = C.c_int
    n = lib.dfx_abi_layout(buf, len(want))
    if n != len(want) or list(buf) != want:
        raise RuntimeError(f"difflexmm_amd: struct layout of the library ({n} entries: {list(buf)[:n]}) differs from the binding's ({want}); "
                           "include/dfx.h and difflexmm_amd/_binding.py are out of step")


def declare(lib):
    """Attach argument / result types to every entry point of include/dfx.h."""
    H = C.c_void_p
    check_abi_layout(lib)
    lib.dfx_create.argtypes = [C.POINTER(dfx_problem), C.POINTER(H)]
    lib.dfx_destroy.argtypes = [H]
    if hasattr(lib, "dfx_share_checkpoint"):
        lib.dfx_share_checkpoint.argtypes = [H, H]
    lib.dfx_last_error.argtypes = [H]
    lib.dfx_last_error.restype = C.c_char_p
    lib.dfx_set_params.argtypes = [H, C.POINTER(dfx_params)]
    lib.dfx_reserve.argtypes = [H, C.c_int64, C.c_int32, C.c_int32]
    lib.dfx_forward.argtypes = [H, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, C.POINTER(dfx_stats)]
    lib.dfx_forward_grid.argtypes = [H, _dp, _dp, C.c_int32, _ip, _dp, C.c_int32, _dp, C.POINTER(dfx_stats)]
    lib.dfx_forward_grid_members.argtypes = [H, _dp, _dp, C.c_int32, _ip, _dp, C.c_int32, _dp, C.POINTER(dfx_stats)]
    lib.dfx_adaptive_step_counts.argtypes = [H, _ip]
    lib.dfx_adaptive_step_times.argtypes = [H, C.c_int32, _dp, C.c_int64, C.POINTER(C.c_int64)]
    lib.dfx_forward_adaptive.argtypes = [H, _dp, _dp, C.c_int32, C.c_double, C.c_double, C.c_int64, _dp, C.POINTER(dfx_stats)]
    lib.dfx_forward_adaptive_keep.argtypes = [H, _dp, _dp, C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_int32, _dp, C.POINTER(dfx_stats)]
    lib.dfx_design_forward.argtypes = [C.POINTER(dfx_design_map), _dp, C.c_int32, C.c_double, _dp, _dp, _dp, _dp]
    lib.dfx_design_vjp.argtypes = [C.POINTER(dfx_design_map), _dp, C.c_int32, C.c_double, _dp, _dp, _dp, _dp, _dp]
    lib.dfx_member_status.argtypes = [H, _ip]
    lib.dfx_set_failure_policy.argtypes = [H, C.c_int32]
    lib.dfx_test_set_spin_limit.argtypes = [H, C.c_int32]
    lib.dfx_adjoint.argtypes = [H, _dp, C.POINTER(dfx_grads), C.POINTER(dfx_stats)]
    lib.dfx_objective_kinetic.argtypes = [H, _ip, C.c_int32, _dp]
    lib.dfx_adjoint_kinetic.argtypes = [H, _ip, C.c_int32, C.POINTER(dfx_grads), C.POINTER(dfx_stats)]
    lib.dfx_kinetic_value_and_grad.argtypes = [H, _ip, C.c_int32, _dp, C.POINTER(dfx_grads), C.POINTER(dfx_grads), C.POINTER(dfx_stats)]
    lib.dfx_response_data.argtypes = [H, _dp, _dp, _dp, _dp]
    lib.dfx_rhs.argtypes = [H, _dp, C.c_double, _dp]
    lib.dfx_rhs_vjp.argtypes = [H, _dp, C.c_double, _dp, _dp, C.POINTER(dfx_grads)]
    lib.dfx_energy.argtypes = [H, _dp, _dp]
    lib.dfx_device_count.restype = C.c_int
    lib.dfx_version.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("dfx_last_error", "dfx_version", "dfx_comm_last_error") and (name not in COMM_EXPORTS or hasattr(lib, name)):
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "dfx_forward_tangent"):      # (the CPU port of the oracle has no forward mode)
        lib.dfx_forward_tangent.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), _dp, C.c_int32, _ip, _dp, C.c_int32, _dp, _dp,
                                            C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_forward_tangent_dense"):
        _lp = C.POINTER(C.c_int64)
        lib.dfx_forward_tangent_dense.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), _dp, C.c_int32, _dp, _lp, C.c_int64, _dp, _dp,
                                                  C.POINTER(dfx_stats)]
        lib.dfx_dense_output_map.argtypes = [_dp, _lp, C.c_int64, C.c_int32, _dp, C.c_int32, _ip, _dp]
    if hasattr(lib, "dfx_forward_tangent_multi"):
        lib.dfx_forward_tangent_multi.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), C.c_int32, _dp, C.c_int32, _ip, _dp, C.c_int32, _dp, _dp,
                                                  C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_forward_tangent_dense_multi"):
        lib.dfx_forward_tangent_dense_multi.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), C.c_int32, _dp, C.c_int32, _dp, C.POINTER(C.c_int64),
                                                        C.c_int64, _dp, _dp, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_forward_tangent_signals_multi"):
        _terms = [C.c_int32, _ip, _ip, _ip, _dp, C.c_int32]
        lib.dfx_forward_tangent_signals_multi.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), C.c_int32, _dp, C.c_int32, _ip, _dp, C.c_int32] + _terms + [
            _dp, _dp, C.POINTER(dfx_stats)]
        lib.dfx_forward_tangent_signals_dense_multi.argtypes = [H, _dp, _dp, C.POINTER(dfx_params), C.c_int32, _dp, C.c_int32, _dp,
                                                                C.POINTER(C.c_int64), C.c_int64] + _terms + [_dp, _dp, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_rhs_jvp"):
        lib.dfx_rhs_jvp.argtypes = [H, _dp, C.c_double, _dp, C.POINTER(dfx_params), C.c_int32, _dp, _dp]
    if hasattr(lib, "dfx_objective_value_and_grad"):
        lib.dfx_objective_value.argtypes = [H, C.c_int32, _dp, C.c_int32, _dp, _dp, C.c_int32, _dp]
        lib.dfx_objective_value_and_grad.argtypes = [H, C.c_int32, _dp, C.c_int32, _dp, _dp, C.c_int32, _dp, C.POINTER(dfx_grads),
                                                     C.POINTER(dfx_grads), C.c_int32, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_strain_objective_value_and_grad"):
        lib.dfx_strain_objective_value.argtypes = [H, _dp, C.c_int32, _dp, _dp, _dp]
        lib.dfx_strain_objective_value_and_grad.argtypes = [H, _dp, C.c_int32, _dp, _dp, _dp, C.POINTER(dfx_grads), C.POINTER(dfx_grads),
                                                            C.c_int32, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_signal_misfit_value_and_grad"):
        terms = [C.c_int32, _ip, _ip, _ip, _dp, C.c_int32]
        lib.dfx_signal_values.argtypes = [H] + terms + [_dp]
    if hasattr(lib, "dfx_signal_hinge_channels"):
        lib.dfx_signal_hinge_channels.argtypes = [H, C.c_int32]
        lib.dfx_signal_misfit_value.argtypes = [H] + terms + [_dp, C.c_int32, _dp, _dp, _dp]
        lib.dfx_signal_misfit_value_and_grad.argtypes = [H] + terms + [_dp, C.c_int32, _dp, _dp, _dp, C.POINTER(dfx_grads), C.POINTER(dfx_grads),
                                                                        C.c_int32, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_signal_projection_value_and_grad"):
        terms = [C.c_int32, _ip, _ip, _ip, _dp, C.c_int32]
        lib.dfx_signal_projections.argtypes = [H] + terms + [_dp, C.c_int32, _dp]
        lib.dfx_signal_projection_value.argtypes = [H] + terms + [_dp, C.c_int32, _dp, _dp, C.c_int32, _dp]
        lib.dfx_signal_projection_value_and_grad.argtypes = [H] + terms + [_dp, C.c_int32, _dp, _dp, C.c_int32, _dp, C.POINTER(dfx_grads),
                                                                            C.POINTER(dfx_grads), C.c_int32, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_signal_xcorr_value_and_grad"):
        terms = [C.c_int32, _ip, _ip, _ip, _dp, C.c_int32]
        corr = [C.c_int32, _ip, _ip, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]      # pairs, templates, max_lag, normalisation
        value = [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp]
        lib.dfx_signal_xcorr.argtypes = [H] + terms + corr + [_dp]
        lib.dfx_signal_xcorr_value.argtypes = [H] + terms + corr + value
        lib.dfx_signal_xcorr_value_and_grad.argtypes = [H] + terms + corr + value + [C.POINTER(dfx_grads), C.POINTER(dfx_grads), C.c_int32,
                                                                                      C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_strain_peak_value_and_grad"):
        peak = [_dp, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, C.c_double, _dp, _dp, _ip]      # coef, weights, tau, aggregate, sharpness, outputs
        lib.dfx_strain_peak_value.argtypes = [H] + peak
        lib.dfx_strain_peak_value_and_grad.argtypes = [H] + peak + [C.POINTER(dfx_grads), C.POINTER(dfx_grads), C.c_int32, C.POINTER(dfx_stats)]
    if hasattr(lib, "dfx_fn_table_grads"):
        lib.dfx_fn_table_values.argtypes = [H, C.c_int32, _dp, C.c_int32]
        lib.dfx_fn_table_grads.argtypes = [H, C.c_int32]
        lib.dfx_fn_table_grad.argtypes = [H, C.c_int32, _dp]
        lib.dfx_drive_cotangent.argtypes = [H, C.c_int32, _dp, _dp, C.c_int64, C.POINTER(C.c_int64)]
        lib.dfx_fn_table_tangents.argtypes = [H, C.c_int32, _dp, C.c_int32]
    if hasattr(lib, "dfx_comm_init"):
        lib.dfx_comm_unique_id.argtypes = [C.c_char_p]
        lib.dfx_comm_init.argtypes = [C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(H)]
        for n in ("dfx_comm_destroy", "dfx_comm_rank", "dfx_comm_size", "dfx_comm_barrier"):
            getattr(lib, n).argtypes = [H]
        lib.dfx_comm_rccl_version.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.dfx_gather_objectives.argtypes = [H, _dp, C.c_int32, _dp]
        lib.dfx_reduce_grads.argtypes = [H, _dp, C.c_int64]
        lib.dfx_comm_allreduce.argtypes = [H, _dp, C.c_int64, C.c_int32]
        lib.dfx_comm_last_error.argtypes = []
        lib.dfx_comm_last_error.restype = C.c_char_p
        lib.dfx_mem_info.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.dfx_device_synchronize.argtypes = [C.c_int32]
        lib.dfx_kinetic_value_and_grad_device.argtypes = lib.dfx_kinetic_value_and_grad.argtypes
        lib.dfx_download.argtypes = [H, _dp, C.c_void_p, C.c_int64]
        lib.dfx_forward_kinetic_value_and_grad.argtypes = [H, _dp, _dp, C.c_int32, _ip, _ip, C.c_int32, _dp, C.POINTER(dfx_grads), C.POINTER(dfx_grads),
                                                           C.c_int32, C.POINTER(dfx_stats), C.POINTER(dfx_stats)]
    return lib


def mem_info(device=0, lib=None):
    """(free, total) bytes of HBM on a device."""
    lib = lib if lib is not None else load_library()
    f, t = C.c_int64(0), C.c_int64(0)
    if lib.dfx_mem_info(int(device), C.byref(f), C.byref(t)) != 0:
        raise RuntimeError("dfx_mem_info failed: " + lib.dfx_comm_last_error().decode())
    return f.value, t.value


def device_synchronize(device=0, lib=None):
    lib = lib if lib is not None else load_library()
    if lib.dfx_device_synchronize(int(device)) != 0:
        raise RuntimeError("dfx_device_synchronize failed: " + lib.dfx_comm_last_error().decode())


def padded_step_times(step_times, t0):
    """Per-member accepted step END times (a list of 1-D arrays, as :meth:`Engine.adaptive_step_times` returns them) -> the padded
    ``(batch, stride)`` array ``t_0 .. t_{N_m}`` (the rest of a row repeats its last entry) and ``n_steps`` (batch,) int64 that
    ``dfx_forward_tangent_dense`` / ``dfx_dense_output_map`` take."""
    n_steps = np.array([len(a) for a in step_times], dtype=np.int64)
    out = np.empty((len(step_times), int(n_steps.max(initial=0)) + 1))
    for m, a in enumerate(step_times):
        out[m, 0] = t0
        out[m, 1:len(a) + 1] = a
        out[m, len(a) + 1:] = out[m, len(a)]
    return out, n_steps


_MAP_ERRORS = {1: "step times must be strictly increasing", 2: "every member's t_0 must be timepoints[0]",
               3: "every member's last step must end at or beyond the last timepoint", 4: "n_steps[m] must lie in [0, stride - 1]"}


def dense_output_map(step_times, n_steps, timepoints, lib=None):
    """``dfx_dense_output_map``: which outputs of an adaptive solve lie in which of its frozen accepted steps, and where.
    ``step_times`` (batch, stride) rows ``t_0 .. t_{N_m}``, ``n_steps`` (batch,), ``timepoints`` (T,).  Returns ``out_ptr`` (batch, stride)
    int32 -- outputs ``out_ptr[m, n] .. out_ptr[m, n + 1] - 1`` lie in step n -- and ``theta`` (batch, T).  Pure host code of the HIP
    library (no device needed)."""
    lib = lib if lib is not None else load_library()
    st = _f64(step_times)
    ns = np.ascontiguousarray(n_steps, dtype=np.int64)
    ts = _f64(timepoints)
    if st.ndim != 2 or ns.shape != (st.shape[0],) or ts.ndim != 1:
        raise ValueError("dense_output_map: step_times (batch, stride), n_steps (batch,), timepoints (T,)")
    out_ptr = np.zeros(st.shape, dtype=np.int32)
    theta = np.zeros((st.shape[0], len(ts)))
    rc = lib.dfx_dense_output_map(_ptr(st), ns.ctypes.data_as(C.POINTER(C.c_int64)), st.shape[1], st.shape[0], _ptr(ts), len(ts),
                                  out_ptr.ctypes.data_as(_ip), _ptr(theta))
    if rc != 0:
        raise ValueError("dense_output_map: " + _MAP_ERRORS.get(rc, f"error {rc}"))
    return out_ptr, theta


_LIB = None


def library_path():
    """``DFX_LIBRARY`` (a path) selects another build of the same HIP engine: kernel experiments side by side on one box."""
    return os.environ.get("DFX_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdfx.so")


def is_hip_engine(lib):
    """A build of the gfx950 engine says so in ``dfx_version()``; anything else with the same symbols (the CPU port of the oracle) is
    test infrastructure and must never stand in for the product."""
    try:
        lib.dfx_version.restype = C.c_char_p
        return b"gfx950" in lib.dfx_version()
    except Exception:       # noqa: BLE001
        return False


def check_engine_library(lib):
    """The product accepts only the HIP engine.  Test infrastructure hands over the CPU port by marking the handle it loaded
    (``oracle.cpu.load()`` sets ``lib._dfx_test_only = True``): an explicit, test-only door -- no environment variable opens it."""
    if is_hip_engine(lib) or getattr(lib, "_dfx_test_only", False) is True:
        return lib
    raise RuntimeError("difflexmm_amd: the library handed in is not the gfx950 engine (dfx_version() = %r): there is no CPU fallback"
                       % (getattr(lib, "dfx_version", lambda: b"?")(),))


def load_library():
    """Load the HIP engine.  Fails loudly when it has not been built, and when ``DFX_LIBRARY`` points at something that is not a
    build of the gfx950 engine: there is no fallback."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"difflexmm_amd: {path} not found -- build the HIP engine first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C difflexmm_amd/csrc)")
        lib = declare(C.CDLL(path))
        if not is_hip_engine(lib):
            raise RuntimeError(f"difflexmm_amd: {path} is not a build of the gfx950 engine (dfx_version() = {lib.dfx_version()!r}); "
                               "DFX_LIBRARY selects between builds of the HIP engine only")
        _LIB = lib
    return _LIB


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = np.ascontiguousarray(np.broadcast_to(a, shape))
    return a


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


_WANTED = np.zeros(1)        # what a non-null field of a ``want`` points at (the library tests the pointer only)


class Engine:
    """One ``dfx_handle``: a lattice + boundary-condition pattern, ``batch`` members wide."""

    def __init__(self, n_blocks, n_npb, bonds, bond_model, contact, special, fn_types, batch=1,
                 tableau="dopri5", device=0, lib=None, fn_tables=None, streams=0):
        self.lib = check_engine_library(lib) if lib is not None else load_library()
        self.n_blocks, self.n_npb, self.batch = int(n_blocks), int(n_npb), int(batch)
        self.bonds = np.ascontiguousarray(bonds, dtype=np.int32).reshape(-1, 2)
        self.n_bonds = len(self.bonds)
        self.fn_types = list(fn_types)
        self.n_fns = len(self.fn_types)
        self.contact = int(contact)
        spec = (dfx_special * max(1, len(special)))()
        for i, (block, mask, con, load) in enumerate(special):
            spec[i].block, spec[i].con_mask = int(block), int(mask)
            for d in range(3):
                for f in range(DFX_MAX_FNS):
                    spec[i].con_coef[d][f] = float(con[d][f]) if f < self.n_fns else 0.0
                    spec[i].load_coef[d][f] = float(load[d][f]) if f < self.n_fns else 0.0
        prob = dfx_problem()
        prob.n_blocks, prob.n_npb, prob.n_bonds = self.n_blocks, self.n_npb, self.n_bonds
        prob.bonds = self.bonds.ctypes.data_as(_ip)
        prob.bond_model, prob.contact = int(bond_model), self.contact
        prob.n_special, prob.special = len(special), spec
        prob.n_fns = self.n_fns
        for f in range(DFX_MAX_FNS):
            prob.fn_type[f] = int(self.fn_types[f]) if f < self.n_fns else 0
        prob.batch, prob.tableau, prob.device = self.batch, TABLEAU[tableau], int(device)
        prob.streams = int(streams or 0)
        tables = []                                   # (times, values) of FN_TABLE functions: static data, copied by dfx_create
        for f in range(DFX_MAX_FNS):
            tab = fn_tables[f] if fn_tables is not None and f < len(fn_tables) else None
            if tab is not None:
                tv = np.ascontiguousarray(np.concatenate([np.asarray(tab[0], dtype=float), np.asarray(tab[1], dtype=float)]))
                tables.append(tv)
                prob.fn_table_n[f], prob.fn_table[f] = len(tv) // 2, tv.ctypes.data_as(_dp)
            else:
                prob.fn_table_n[f], prob.fn_table[f] = 0, None
        self.fn_table_n = [int(prob.fn_table_n[f]) for f in range(DFX_MAX_FNS)]
        self._h = C.c_void_p()
        rc = self.lib.dfx_create(C.byref(prob), C.byref(self._h))
        if rc != 0:
            raise RuntimeError("dfx_create failed: " + self.lib.dfx_last_error(None).decode())
        self.n_timepoints = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.dfx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: " + self.lib.dfx_last_error(self._h).decode())

    # -- parameters ---------------------------------------------------------------------------
    def shapes(self):
        B, nb, npb, nbd = self.batch, self.n_blocks, self.n_npb, self.n_bonds
        return {"centroid_node_vectors": (B, nb, npb, 2), "reference_vector": (B, nbd, 2), "k_bond": (B, nbd, 3),
                "inertia": (B, nb, 3), "damping": (B, nb, 3), "void_angle0": (B, nbd, 2), "contact": (B, 3),
                "fn_params": (B, max(1, self.n_fns), DFX_FN_PARAMS), "state0": (B, 2, nb, 3), "block_centroids": (B, nb, 2)}

    def set_params(self, **arrays):
        """Arrays by ``dfx_params`` field name; shapes as in :meth:`shapes` (broadcast over batch)."""
        sh = self.shapes()
        p = dfx_params()
        keep = []
        for name in _PARAM_FIELDS + ["block_centroids"]:
            a = arrays.get(name)
            if a is None:
                continue
            a = _f64(a, sh[name])
            keep.append(a)
            setattr(p, name, _ptr(a))
        self._check(self.lib.dfx_set_params(self._h, C.byref(p)), "dfx_set_params")

    def share_checkpoint(self, other):
        """Keep this engine's trajectory checkpoint in ``other``'s buffers (engines whose solves never overlap in time)."""
        self._check(self.lib.dfx_share_checkpoint(self._h, other._h), "dfx_share_checkpoint")

    def reserve(self, max_steps, max_timepoints, keep_trajectory=True):
        self._check(self.lib.dfx_reserve(self._h, int(max_steps), int(max_timepoints), int(bool(keep_trajectory))), "dfx_reserve")

    # -- solves -------------------------------------------------------------------------------
    def forward(self, state0, timepoints, steps_per_interval, keep_trajectory=False, want_fields=True, step_times=None):
        B, nb = self.batch, self.n_blocks
        state0 = _f64(state0, (B, 2, nb, 3)) if state0 is not None else None      # None: at rest (no upload)
        ts = _f64(timepoints)
        T = ts.shape[-1]
        fields = np.empty((B, T, 2, nb, 3)) if want_fields else None
        st = dfx_stats()
        if ts.ndim == 2:        # (batch, T): every member its own output times and step boundaries, shared step counts
            if ts.shape[0] != B:
                raise ValueError(f"per-member timepoints must be (batch={B}, T)")
            spis = np.ascontiguousarray(np.broadcast_to(steps_per_interval, (max(T - 1, 0),)), dtype=np.int32)
            n = int(spis.sum())
            if step_times is None:      # equal steps inside every member's own intervals
                step_times = np.stack([np.concatenate([a + (b - a) * np.arange(k) / k for a, b, k in zip(row[:-1], row[1:], spis)] + [row[-1:]])
                                       for row in ts])
            step_times = _f64(step_times, (B, n + 1))
            self._check(self.lib.dfx_forward_grid_members(self._h, _ptr(state0), _ptr(ts), T, spis.ctypes.data_as(_ip), _ptr(step_times),
                                                          int(bool(keep_trajectory)), _ptr(fields), C.byref(st)), "dfx_forward_grid_members")
        elif np.ndim(steps_per_interval) == 0 and step_times is None:
            self._check(self.lib.dfx_forward(self._h, _ptr(state0), _ptr(ts), T, int(steps_per_interval),
                                             int(bool(keep_trajectory)), _ptr(fields), C.byref(st)), "dfx_forward")
        else:   # its own number of equal steps in every output interval
            spis = np.ascontiguousarray(np.broadcast_to(steps_per_interval, (max(T - 1, 0),)), dtype=np.int32)
            if step_times is not None:      # caller-chosen step boundaries (every timepoint must be one of them)
                step_times = _f64(step_times, (int(spis.sum()) + 1,))
            self._check(self.lib.dfx_forward_grid(self._h, _ptr(state0), _ptr(ts), T, spis.ctypes.data_as(_ip), _ptr(step_times),
                                                  int(bool(keep_trajectory)), _ptr(fields), C.byref(st)), "dfx_forward_grid")
        self.n_timepoints = T
        return fields, _stats(st)

    # -- forward mode: the single-direction entries are the K-direction ones at K = 1, and share their marshalling -------------------
    def _need(self, entry, family="forward mode", why="the CPU port of the oracle is reverse mode only"):
        if not hasattr(self.lib, entry):
            raise NotImplementedError(f"{family}: the library {getattr(self.lib, '_name', self.lib)!r} has no {entry} ({why}; build the HIP engine)")

    _STALE = "a stale libdfx.so, or the CPU port of the oracle"          # why a library lacks an entry of the later objective families

    def _params_dots(self, params_dots, K):
        """K ``dfx_params`` (one per direction) from a list of dicts of arrays by field name (None / a missing name: zero tangent)."""
        sh = self.shapes()
        arr = (dfx_params * K)()
        keep = []
        for k in range(K):
            pd = params_dots[k] if params_dots is not None else None
            for name in _PARAM_FIELDS + ["block_centroids"]:
                a = pd.get(name) if pd else None
                if a is None:
                    continue
                a = _f64(a, sh[name])
                keep.append(a)
                setattr(arr[k], name, _ptr(a))
        return arr, keep

    def _state0_dots(self, state0_dots, K):
        if state0_dots is None:
            return None
        B, nb = self.batch, self.n_blocks
        a = np.ascontiguousarray(state0_dots, dtype=np.float64)
        if a.shape != (B, K, 2, nb, 3):
            raise ValueError(f"state0_dots must be (batch={B}, n_dirs={K}, 2, {nb}, 3), got {a.shape}")
        return a

    def _fixed_grid_args(self, state0, timepoints, steps_per_interval, step_times):
        """(state0, timepoints, T, steps_per_interval, step_times, per_member) as the fixed-grid tangent entries take them."""
        B, nb = self.batch, self.n_blocks
        state0 = _f64(state0, (B, 2, nb, 3)) if state0 is not None else None
        ts = _f64(timepoints)
        T = ts.shape[-1]
        spis = np.ascontiguousarray(np.broadcast_to(steps_per_interval, (max(T - 1, 0),)), dtype=np.int32)
        n = int(spis.sum())
        per_member = ts.ndim == 2
        if per_member:
            if ts.shape[0] != B:
                raise ValueError(f"per-member timepoints must be (batch={B}, T)")
            if step_times is None:      # equal steps inside every member's own intervals (as forward)
                step_times = np.stack([np.concatenate([a + (b - a) * np.arange(k) / k for a, b, k in zip(row[:-1], row[1:], spis)] + [row[-1:]])
                                       for row in ts])
            step_times = _f64(step_times, (B, n + 1))
        elif step_times is not None:
            step_times = _f64(step_times, (n + 1,))
        return state0, ts, T, spis, step_times, per_member

    def _dense_grid_args(self, who, state0, timepoints, step_times, n_steps):
        """(state0, timepoints, T, step_times, n_steps) as the dense tangent entries take them."""
        B, nb = self.batch, self.n_blocks
        state0 = _f64(state0, (B, 2, nb, 3)) if state0 is not None else None
        ts = _f64(timepoints)
        if ts.ndim != 1:
            raise ValueError(f"{who}: one row of timepoints for all members")
        st_times = _f64(step_times)
        ns = np.ascontiguousarray(n_steps, dtype=np.int64)
        if st_times.ndim != 2 or st_times.shape[0] != B or ns.shape != (B,):
            raise ValueError(f"{who}: step_times (batch={B}, stride) and n_steps (batch,)")
        return state0, ts, len(ts), st_times, ns

    @property
    def has_forward_tangent(self):
        return hasattr(self.lib, "dfx_forward_tangent")

    def forward_tangent(self, state0, state0_dot, params_dot, timepoints, steps_per_interval, step_times=None):
        """Primal fields and their directional derivative along (state0_dot, params_dot) of the fixed-grid solve (``dfx_forward_tangent``)
        on the parameters of the last :meth:`set_params`.  ``params_dot``: arrays by ``dfx_params`` field name (a missing one: zero
        tangent); ``timepoints`` (T,) or (batch, T) (then every member its own grid, as :meth:`forward`).  Returns (fields, fields_dot, stats)."""
        self._need("dfx_forward_tangent")
        B, nb = self.batch, self.n_blocks
        state0, ts, T, spis, step_times, per_member = self._fixed_grid_args(state0, timepoints, steps_per_interval, step_times)
        state0_dot = _f64(state0_dot, (B, 2, nb, 3)) if state0_dot is not None else None
        p, keep = self._params_dots([params_dot], 1)
        fields, fields_dot = np.empty((B, T, 2, nb, 3)), np.empty((B, T, 2, nb, 3))
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent(self._h, _ptr(state0), _ptr(state0_dot), p, _ptr(ts), T, spis.ctypes.data_as(_ip),
                                                 _ptr(step_times), int(per_member), _ptr(fields), _ptr(fields_dot), C.byref(st)),
                    "dfx_forward_tangent")
        return fields, fields_dot, _stats(st)

    @property
    def has_forward_tangent_dense(self):
        return hasattr(self.lib, "dfx_forward_tangent_dense")

    def forward_tangent_dense(self, state0, state0_dot, params_dot, timepoints, step_times, n_steps):
        """Primal fields and their directional derivative of the ADAPTIVE solve's dense output on every member's own frozen accepted steps
        (``dfx_forward_tangent_dense``): ``step_times`` (batch, stride) rows ``t_0 .. t_{N_m}``, ``n_steps`` (batch,)
        (:func:`padded_step_times`), ``timepoints`` (T,).  Otherwise as :meth:`forward_tangent`.  Returns (fields, fields_dot, stats)."""
        self._need("dfx_forward_tangent_dense")
        B, nb = self.batch, self.n_blocks
        state0, ts, T, st_times, ns = self._dense_grid_args("forward_tangent_dense", state0, timepoints, step_times, n_steps)
        state0_dot = _f64(state0_dot, (B, 2, nb, 3)) if state0_dot is not None else None
        p, keep = self._params_dots([params_dot], 1)
        fields, fields_dot = np.empty((B, T, 2, nb, 3)), np.empty((B, T, 2, nb, 3))
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent_dense(self._h, _ptr(state0), _ptr(state0_dot), p, _ptr(ts), T, _ptr(st_times),
                                                       ns.ctypes.data_as(C.POINTER(C.c_int64)), st_times.shape[1], _ptr(fields),
                                                       _ptr(fields_dot), C.byref(st)), "dfx_forward_tangent_dense")
        return fields, fields_dot, _stats(st)

    @property
    def has_forward_tangent_multi(self):
        return hasattr(self.lib, "dfx_forward_tangent_multi")

    def forward_tangent_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, steps_per_interval, step_times=None):
        """:meth:`forward_tangent` for ``n_dirs`` directions per member with the primal evaluated once per stage
        (``dfx_forward_tangent_multi``): ``state0_dots`` (batch, n_dirs, 2, nb, 3) or None, ``params_dots`` a list of ``n_dirs`` dicts of
        arrays by ``dfx_params`` field name (or None).  Returns (fields (batch, T, ...), fields_dots (batch, n_dirs, T, ...), stats)."""
        self._need("dfx_forward_tangent_multi")
        K = int(n_dirs)
        if K < 1 or (params_dots is not None and len(params_dots) != K):
            raise ValueError(f"forward_tangent_multi: need n_dirs >= 1 and one params_dot per direction (n_dirs={K})")
        B, nb = self.batch, self.n_blocks
        state0, ts, T, spis, step_times, per_member = self._fixed_grid_args(state0, timepoints, steps_per_interval, step_times)
        state0_dots = self._state0_dots(state0_dots, K)
        p, keep = self._params_dots(params_dots, K)
        fields, fields_dots = np.empty((B, T, 2, nb, 3)), np.empty((B, K, T, 2, nb, 3))
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent_multi(self._h, _ptr(state0), _ptr(state0_dots), p, K, _ptr(ts), T, spis.ctypes.data_as(_ip),
                                                       _ptr(step_times), int(per_member), _ptr(fields), _ptr(fields_dots), C.byref(st)),
                    "dfx_forward_tangent_multi")
        return fields, fields_dots, _stats(st)

    @property
    def has_forward_tangent_dense_multi(self):
        return hasattr(self.lib, "dfx_forward_tangent_dense_multi")

    def forward_tangent_dense_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, step_times, n_steps):
        """:meth:`forward_tangent_dense` for ``n_dirs`` directions per member (``dfx_forward_tangent_dense_multi``); arguments as
        :meth:`forward_tangent_multi` and :meth:`forward_tangent_dense`.  Returns (fields, fields_dots (batch, n_dirs, T, ...), stats)."""
        self._need("dfx_forward_tangent_dense_multi")
        K = int(n_dirs)
        if K < 1 or (params_dots is not None and len(params_dots) != K):
            raise ValueError(f"forward_tangent_dense_multi: need n_dirs >= 1 and one params_dot per direction (n_dirs={K})")
        B, nb = self.batch, self.n_blocks
        state0, ts, T, st_times, ns = self._dense_grid_args("forward_tangent_dense_multi", state0, timepoints, step_times, n_steps)
        state0_dots = self._state0_dots(state0_dots, K)
        p, keep = self._params_dots(params_dots, K)
        fields, fields_dots = np.empty((B, T, 2, nb, 3)), np.empty((B, K, T, 2, nb, 3))
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent_dense_multi(self._h, _ptr(state0), _ptr(state0_dots), p, K, _ptr(ts), T, _ptr(st_times),
                                                             ns.ctypes.data_as(C.POINTER(C.c_int64)), st_times.shape[1], _ptr(fields),
                                                             _ptr(fields_dots), C.byref(st)), "dfx_forward_tangent_dense_multi")
        return fields, fields_dots, _stats(st)

    @property
    def has_forward_tangent_signals(self):
        return hasattr(self.lib, "dfx_forward_tangent_signals_multi")

    def forward_tangent_signals_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, steps_per_interval, terms, n_signals,
                                      step_times=None):
        """:meth:`forward_tangent_multi` with the history kept on the device (``dfx_forward_tangent_signals_multi``): the signals of
        ``terms`` (sequence of (signal, block, component, coef), as :meth:`signal_values`) and their tangents along the ``n_dirs``
        directions.  Returns (signals (batch, T, n_signals), signals_dots (batch, n_dirs, T, n_signals), stats)."""
        self._need("dfx_forward_tangent_signals_multi")
        K = int(n_dirs)
        if K < 1 or (params_dots is not None and len(params_dots) != K):
            raise ValueError(f"forward_tangent_signals_multi: need n_dirs >= 1 and one params_dot per direction (n_dirs={K})")
        B, ns = self.batch, max(int(n_signals), 1)
        state0, ts, T, spis, step_times, per_member = self._fixed_grid_args(state0, timepoints, steps_per_interval, step_times)
        state0_dots = self._state0_dots(state0_dots, K)
        p, keep = self._params_dots(params_dots, K)
        targs, tkeep = self._signal_terms(terms, n_signals)
        signals, signals_dots = np.zeros((B, T, ns)), np.zeros((B, K, T, ns))      # (a refusal comes before the library writes)
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent_signals_multi(self._h, _ptr(state0), _ptr(state0_dots), p, K, _ptr(ts), T,
                                                               spis.ctypes.data_as(_ip), _ptr(step_times), int(per_member), *targs,
                                                               _ptr(signals), _ptr(signals_dots), C.byref(st)),
                    "dfx_forward_tangent_signals_multi")
        return signals, signals_dots, _stats(st)

    def forward_tangent_signals_dense_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, step_times, n_steps, terms, n_signals):
        """:meth:`forward_tangent_dense_multi` with the history kept on the device (``dfx_forward_tangent_signals_dense_multi``);
        ``terms`` and the results as :meth:`forward_tangent_signals_multi`."""
        self._need("dfx_forward_tangent_signals_dense_multi")
        K = int(n_dirs)
        if K < 1 or (params_dots is not None and len(params_dots) != K):
            raise ValueError(f"forward_tangent_signals_dense_multi: need n_dirs >= 1 and one params_dot per direction (n_dirs={K})")
        B, ns = self.batch, max(int(n_signals), 1)
        state0, ts, T, st_times, nst = self._dense_grid_args("forward_tangent_signals_dense_multi", state0, timepoints, step_times, n_steps)
        state0_dots = self._state0_dots(state0_dots, K)
        p, keep = self._params_dots(params_dots, K)
        targs, tkeep = self._signal_terms(terms, n_signals)
        signals, signals_dots = np.zeros((B, T, ns)), np.zeros((B, K, T, ns))
        st = dfx_stats()
        self._check(self.lib.dfx_forward_tangent_signals_dense_multi(self._h, _ptr(state0), _ptr(state0_dots), p, K, _ptr(ts), T, _ptr(st_times),
                                                                     nst.ctypes.data_as(C.POINTER(C.c_int64)), st_times.shape[1], *targs,
                                                                     _ptr(signals), _ptr(signals_dots), C.byref(st)),
                    "dfx_forward_tangent_signals_dense_multi")
        return signals, signals_dots, _stats(st)

    def adaptive_step_counts(self):
        """(batch, T-1) accepted steps of the last forward_adaptive per member and output interval."""
        out = np.zeros((self.batch, max(self.n_timepoints - 1, 0)), dtype=np.int32)
        self._check(self.lib.dfx_adaptive_step_counts(self._h, out.ctypes.data_as(_ip)), "dfx_adaptive_step_counts")
        return out

    def adaptive_step_times(self, member=0):
        """End times of the steps one member accepted in the last forward_adaptive."""
        n = C.c_int64(0)
        self._check(self.lib.dfx_adaptive_step_times(self._h, int(member), None, 0, C.byref(n)), "dfx_adaptive_step_times")
        out = np.empty(n.value)
        self._check(self.lib.dfx_adaptive_step_times(self._h, int(member), _ptr(out), n.value, C.byref(n)), "dfx_adaptive_step_times")
        return out

    def forward_adaptive(self, state0, timepoints, rtol, atol, max_attempts=10_000_000, keep_trajectory=False, want_fields=True):
        """Adaptive Dormand-Prince with the reference's odeint semantics.  ``keep_trajectory``: the accepted steps are kept for the
        reverse sweep (``adjoint`` / ``kinetic_value_and_grad`` afterwards: the dense-output discrete adjoint of this very solve)."""
        B, nb = self.batch, self.n_blocks
        state0 = _f64(state0, (B, 2, nb, 3)) if state0 is not None else None        # None: every member starts at rest
        ts = _f64(timepoints)
        T = len(ts)
        fields = np.empty((B, T, 2, nb, 3)) if want_fields else None
        st = dfx_stats()
        if keep_trajectory or not want_fields:
            if not self.can_keep_adaptive:
                raise RuntimeError("this library has no dfx_forward_adaptive_keep")
            self._check(self.lib.dfx_forward_adaptive_keep(self._h, _ptr(state0), _ptr(ts), T, float(rtol), float(atol), int(max_attempts),
                                                           1 if keep_trajectory else 0, _ptr(fields), C.byref(st)), "dfx_forward_adaptive_keep")
        else:
            self._check(self.lib.dfx_forward_adaptive(self._h, _ptr(state0), _ptr(ts), T, float(rtol), float(atol),
                                                      int(max_attempts), _ptr(fields), C.byref(st)), "dfx_forward_adaptive")
        self.n_timepoints = T
        return fields, _stats(st)

    def member_status(self):
        """(batch,) int32: 0 ok, 1 non-finite, 2 step size underflow, 3 step budget exceeded -- of the last forward pass."""
        st = np.zeros(self.batch, dtype=np.int32)
        self._check(self.lib.dfx_member_status(self._h, st.ctypes.data_as(_ip)), "dfx_member_status")
        return st

    def set_failure_policy(self, isolate):
        """isolate=True: a member that diverges is flagged (``member_status``; its outputs NaN) instead of failing the call for the whole
        ensemble -- what the reference's list of forward problems does (problems/quads_focusing_multi_input.py:66-77)."""
        self._check(self.lib.dfx_set_failure_policy(self._h, 1 if isolate else 0), "dfx_set_failure_policy")

    @property
    def can_keep_adaptive(self):
        return hasattr(self.lib, "dfx_forward_adaptive_keep")

    def _grad_names(self, which, centroids=False):
        """The names of ``which`` that exist on this lattice (``centroids``: block_centroids on every lattice -- the angular kind)."""
        return [n for n in which if not (n == "fn_params" and self.n_fns == 0) and not (n == "contact" and not self.contact)
                and not (n == "void_angle0" and self.contact != CONTACT_ANGLE)
                and not (n == "block_centroids" and self.contact != CONTACT_DISTANCE and not centroids)]

    def _grads(self, which):
        sh = self.shapes()
        g = dfx_grads()
        out = {n: np.zeros(sh[n]) for n in self._grad_names(which)}
        for name, a in out.items():
            setattr(g, name, _ptr(a))
        return g, out

    def _grad_request(self, which, centroids=False):
        """What a ``*_value_and_grad`` entry takes besides its own arguments: ``want`` (a non-null field per requested gradient), the
        ``views`` the library fills, the requested names and the stats."""
        want, views = dfx_grads(), dfx_grads()
        names = self._grad_names(which, centroids)
        for n in names:
            setattr(want, n, _ptr(_WANTED))
        return want, views, names, dfx_stats()

    def _grad_views(self, views, names, device):
        """The gradients the library left behind ``views``: ``DeviceArray`` handles, or read-only views of its pinned memory."""
        sh = self.shapes()
        if device:
            return {n: DeviceArray(self, C.cast(getattr(views, n), C.c_void_p).value, sh[n]) for n in names}
        out = {}
        for n in names:
            a = np.ctypeslib.as_array(getattr(views, n), shape=sh[n])
            a.flags.writeable = False
            out[n] = a
        return out

    def _time_weights(self, time_weights):
        if time_weights is None:
            return None
        tau = _f64(time_weights)
        if self.n_timepoints is not None and tau.shape != (self.n_timepoints,):
            raise ValueError(f"time_weights must be ({self.n_timepoints},), got {tau.shape}")
        return tau

    ALL_GRADS = tuple(_PARAM_FIELDS + ["state0", "block_centroids"])

    def adjoint(self, fields_bar, which=ALL_GRADS):
        B, nb = self.batch, self.n_blocks
        if self.n_timepoints is None:
            raise RuntimeError("dfx_adjoint failed: run forward with keep_trajectory=1 first")
        fb = _f64(fields_bar, (B, self.n_timepoints, 2, nb, 3))
        g, out = self._grads(which)
        st = dfx_stats()
        self._check(self.lib.dfx_adjoint(self._h, _ptr(fb), C.byref(g), C.byref(st)), "dfx_adjoint")
        return out, _stats(st)

    def objective_kinetic(self, target_blocks):
        tb = np.ascontiguousarray(target_blocks, dtype=np.int32)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_objective_kinetic(self._h, tb.ctypes.data_as(_ip), len(tb), _ptr(obj)),
                    "dfx_objective_kinetic")
        return obj

    def adjoint_kinetic(self, target_blocks, which=ALL_GRADS):
        tb = np.ascontiguousarray(target_blocks, dtype=np.int32)
        g, out = self._grads(which)
        st = dfx_stats()
        self._check(self.lib.dfx_adjoint_kinetic(self._h, tb.ctypes.data_as(_ip), len(tb), C.byref(g), C.byref(st)),
                    "dfx_adjoint_kinetic")
        return out, _stats(st)

    def kinetic_value_and_grad(self, target_blocks, which=ALL_GRADS, device=False):
        """objective (batch,) and the requested gradients in ONE call; the arrays are read-only views of library-owned pinned
        memory (valid until the next call on this engine: copy what must outlive it).  ``device=True`` leaves the gradients in HBM
        (HIP library only): the values are ``DeviceArray`` handles, ``.to_host()`` downloads one."""
        tb = np.ascontiguousarray(target_blocks, dtype=np.int32)
        want, views, names, st = self._grad_request(which)
        obj = np.zeros(self.batch)
        entry = "dfx_kinetic_value_and_grad_device" if device else "dfx_kinetic_value_and_grad"
        if device and not hasattr(self.lib, entry):
            raise RuntimeError("device-resident gradients need the HIP library")
        self._check(getattr(self.lib, entry)(self._h, tb.ctypes.data_as(_ip), len(tb), _ptr(obj), C.byref(want), C.byref(views), C.byref(st)), entry)
        return obj, self._grad_views(views, names, device), _stats(st)

    def forward_kinetic_value_and_grad(self, state0, timepoints, steps_per_interval, target_blocks, which=ALL_GRADS, device=False):
        """``forward(keep_trajectory=True, want_fields=False)`` + ``kinetic_value_and_grad`` as ONE library call (HIP library only): the host
        does not wait for the forward pass before it enqueues the reverse sweep.  Returns objective, gradients, forward stats, adjoint stats."""
        if not hasattr(self.lib, "dfx_forward_kinetic_value_and_grad"):
            raise RuntimeError("the fused call needs the HIP library")
        B, nb = self.batch, self.n_blocks
        state0 = _f64(state0, (B, 2, nb, 3)) if state0 is not None else None
        ts = _f64(timepoints)
        if ts.ndim != 1:
            raise ValueError("forward_kinetic_value_and_grad: one time grid for all members")
        T = len(ts)
        spis = np.ascontiguousarray(np.broadcast_to(steps_per_interval, (max(T - 1, 0),)), dtype=np.int32)
        tb = np.ascontiguousarray(target_blocks, dtype=np.int32)
        want, views, names, st_a = self._grad_request(which)
        obj = np.zeros(B)
        st_f = dfx_stats()
        self._check(self.lib.dfx_forward_kinetic_value_and_grad(self._h, _ptr(state0), _ptr(ts), T, spis.ctypes.data_as(_ip), tb.ctypes.data_as(_ip),
                                                                len(tb), _ptr(obj), C.byref(want), C.byref(views), int(bool(device)),
                                                                C.byref(st_f), C.byref(st_a)), "dfx_forward_kinetic_value_and_grad")
        self.n_timepoints = T
        return obj, self._grad_views(views, names, device), _stats(st_f), _stats(st_a)

    # -- weighted objectives on the device-resident history ----------------------------------------------
    @property
    def has_objective(self):
        return hasattr(self.lib, "dfx_objective_value_and_grad")

    def _objective_args(self, kind, block_weights, time_weights, lever0):
        """The array arguments of ``dfx_objective_value[_and_grad]``: weights (n_blocks,) or (batch, n_blocks), time weights (T,) or
        None, lever0 (n_blocks, 2) or (batch, n_blocks, 2) or None."""
        self._need("dfx_objective_value_and_grad", "device objectives", "the CPU port of the oracle has the kinetic entries only")
        B, nb = self.batch, self.n_blocks
        w = _f64(block_weights)
        if w.shape not in ((nb,), (B, nb)):
            raise ValueError(f"block_weights must be ({nb},) or ({B}, {nb}), got {w.shape}")
        tau = self._time_weights(time_weights)
        lev = None
        if lever0 is not None:
            lev = _f64(lever0)
            if lev.shape not in ((nb, 2), (B, nb, 2)):
                raise ValueError(f"lever0 must be ({nb}, 2) or ({B}, {nb}, 2), got {lev.shape}")
        return w, int(w.ndim == 2), tau, lev, int(lev is not None and lev.ndim == 3)

    def objective_value(self, kind, block_weights, time_weights=None, lever0=None):
        """(batch,) value of a weighted objective (``OBJ_KINETIC`` / ``OBJ_ANGULAR_MOMENTUM``, ``dfx_objective_value``) on the resident
        history of the last forward pass."""
        w, wpm, tau, lev, lpm = self._objective_args(kind, block_weights, time_weights, lever0)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_objective_value(self._h, int(kind), _ptr(w), wpm, _ptr(tau), _ptr(lev), lpm, _ptr(obj)), "dfx_objective_value")
        return obj

    def objective_value_and_grad(self, kind, block_weights, time_weights=None, lever0=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of a weighted objective in ONE call (``dfx_objective_value_and_grad``): the cotangent
        is formed on the device, the objective rides along with the reverse sweep, the explicit inertia / block-centroid terms are added
        behind it.  Results as :meth:`kinetic_value_and_grad`: read-only views of pinned memory, or ``DeviceArray`` handles with
        ``device=True``; ``block_centroids`` is available on every lattice for the angular kind."""
        w, wpm, tau, lev, lpm = self._objective_args(kind, block_weights, time_weights, lever0)
        want, views, names, st = self._grad_request(which, int(kind) == OBJ_ANGULAR_MOMENTUM)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_objective_value_and_grad(self._h, int(kind), _ptr(w), wpm, _ptr(tau), _ptr(lev), lpm, _ptr(obj), C.byref(want),
                                                          C.byref(views), int(bool(device)), C.byref(st)), "dfx_objective_value_and_grad")
        return obj, self._grad_views(views, names, device), _stats(st)

    # -- ligament strain-energy objective on the device-resident history ----------------------------------
    @property
    def has_strain_objective(self):
        return hasattr(self.lib, "dfx_strain_objective_value_and_grad")

    def _strain_objective_args(self, bond_weights, time_weights, parts):
        """The array arguments of ``dfx_strain_objective_value[_and_grad]``: bond weights (n_bonds,) or (batch, n_bonds), time weights (T,)
        or None, the four part coefficients (c_stretch, c_shear, c_bend, c_contact)."""
        self._need("dfx_strain_objective_value_and_grad", "strain-energy objective", self._STALE)
        B, nbd = self.batch, self.n_bonds
        w = _f64(bond_weights)
        if w.shape not in ((nbd,), (B, nbd)):
            raise ValueError(f"bond_weights must be ({nbd},) or ({B}, {nbd}), got {w.shape}")
        tau = self._time_weights(time_weights)
        c = _f64(parts)
        if c.shape != (4,):
            raise ValueError(f"parts must be (c_stretch, c_shear, c_bend, c_contact), got shape {c.shape}")
        return w, int(w.ndim == 2), tau, c

    def strain_objective_value(self, bond_weights, time_weights=None, parts=(1.0, 1.0, 1.0, 0.0)):
        """(batch,) weighted ligament strain energy (``dfx_strain_objective_value``) on the resident history of the last forward pass."""
        w, wpm, tau, c = self._strain_objective_args(bond_weights, time_weights, parts)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_strain_objective_value(self._h, _ptr(w), wpm, _ptr(tau), _ptr(c), _ptr(obj)), "dfx_strain_objective_value")
        return obj

    def strain_objective_value_and_grad(self, bond_weights, time_weights=None, parts=(1.0, 1.0, 1.0, 0.0), which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the weighted ligament strain energy in ONE call
        (``dfx_strain_objective_value_and_grad``): the ligament forces are formed on the device as the cotangent of the reverse sweep, the
        explicit node-vector / void-angle / per-ligament terms are added behind it.  Results as :meth:`objective_value_and_grad`."""
        w, wpm, tau, c = self._strain_objective_args(bond_weights, time_weights, parts)
        want, views, names, st = self._grad_request(which)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_strain_objective_value_and_grad(self._h, _ptr(w), wpm, _ptr(tau), _ptr(c), _ptr(obj), C.byref(want),
                                                                 C.byref(views), int(bool(device)), C.byref(st)),
                    "dfx_strain_objective_value_and_grad")
        return obj, self._grad_views(views, names, device), _stats(st)

    # -- peak ligament strain on the device-resident history --------------------------------------------------
    @property
    def has_strain_peak(self):
        return hasattr(self.lib, "dfx_strain_peak_value_and_grad")

    def _strain_peak_args(self, bond_coef, bond_weights, time_weights, aggregate, sharpness):
        """The arguments of ``dfx_strain_peak_value[_and_grad]``: coefficients (n_bonds, 3) or (batch, n_bonds, 3), bond weights
        (n_bonds,), (batch, n_bonds) or None = ones, time weights (T,) or None, the aggregate ("ks" / "pnorm" or DFX_PEAK_*), beta or p."""
        self._need("dfx_strain_peak_value_and_grad", "peak-strain objective", self._STALE)
        B, nbd = self.batch, self.n_bonds
        c = _f64(bond_coef)
        if c.shape not in ((nbd, 3), (B, nbd, 3)):
            raise ValueError(f"bond_coef must be ({nbd}, 3) or ({B}, {nbd}, 3), got {c.shape}")
        w = None
        if bond_weights is not None:
            w = _f64(bond_weights)
            if w.shape not in ((nbd,), (B, nbd)):
                raise ValueError(f"bond_weights must be ({nbd},) or ({B}, {nbd}), got {w.shape}")
        tau = self._time_weights(time_weights)
        agg = {"ks": PEAK_KS, "pnorm": PEAK_PNORM}.get(aggregate, aggregate)
        return c, int(c.ndim == 3), w, int(w is not None and w.ndim == 2), tau, int(agg), float(sharpness)

    def strain_peak_value(self, bond_coef, bond_weights=None, time_weights=None, aggregate="ks", sharpness=1.0):
        """(J, peak, peak_at): the smooth maximum (batch,), the hard maximum (batch,) and its (output, bond) (batch, 2) of the ligament strain
        measure (``dfx_strain_peak_value``) on the resident history of the last forward pass."""
        c, cpm, w, wpm, tau, agg, sharp = self._strain_peak_args(bond_coef, bond_weights, time_weights, aggregate, sharpness)
        obj, peak, at = np.zeros(self.batch), np.zeros(self.batch), np.zeros((self.batch, 2), dtype=np.int32)
        self._check(self.lib.dfx_strain_peak_value(self._h, _ptr(c), cpm, _ptr(w), wpm, _ptr(tau), agg, sharp, _ptr(obj), _ptr(peak),
                                                   at.ctypes.data_as(_ip)), "dfx_strain_peak_value")
        return obj, peak, at

    def strain_peak_value_and_grad(self, bond_coef, bond_weights=None, time_weights=None, aggregate="ks", sharpness=1.0, which=ALL_GRADS,
                                   device=False):
        """(J, peak, peak_at) and the requested gradients of J in ONE call (``dfx_strain_peak_value_and_grad``): maximum, softmax sum and
        the softmax-weighted ligament forces are formed on the device as the cotangent of the reverse sweep, the explicit node-vector /
        reference-vector terms are added behind it.  Results as :meth:`objective_value_and_grad`."""
        c, cpm, w, wpm, tau, agg, sharp = self._strain_peak_args(bond_coef, bond_weights, time_weights, aggregate, sharpness)
        want, views, names, st = self._grad_request(which)
        obj, peak, at = np.zeros(self.batch), np.zeros(self.batch), np.zeros((self.batch, 2), dtype=np.int32)
        self._check(self.lib.dfx_strain_peak_value_and_grad(self._h, _ptr(c), cpm, _ptr(w), wpm, _ptr(tau), agg, sharp, _ptr(obj), _ptr(peak),
                                                            at.ctypes.data_as(_ip), C.byref(want), C.byref(views), int(bool(device)),
                                                            C.byref(st)), "dfx_strain_peak_value_and_grad")
        return (obj, peak, at), self._grad_views(views, names, device), _stats(st)

    # -- signal misfit on the device-resident history ---------------------------------------------------------
    @property
    def has_signal_misfit(self):
        return hasattr(self.lib, "dfx_signal_misfit_value_and_grad")

    # ``hinge_channels = True`` opens the hinge components 9 + 3 node + dof to every entry that takes signal terms
    # (``dfx_signal_hinge_channels``); off, the default, they are refused as out of range, as before the hinge channels existed
    hinge_channels = False

    def _signal_terms(self, terms, n_signals):
        """The term arrays of ``dfx_signal_*``: ``terms`` is a sequence of (signal, block, component, coef)."""
        self._need("dfx_signal_misfit_value_and_grad", "signal misfit", self._STALE)
        if self.hinge_channels:
            self._need("dfx_signal_hinge_channels", "hinge-force signal channels", self._STALE)
        if hasattr(self.lib, "dfx_signal_hinge_channels"):
            self.lib.dfx_signal_hinge_channels(self._h, int(bool(self.hinge_channels)))
        t = np.asarray(terms, dtype=float).reshape(-1, 4)
        idx = [np.ascontiguousarray(t[:, i], dtype=np.int32) for i in range(3)]
        coef = np.ascontiguousarray(t[:, 3], dtype=np.float64)
        return (len(t), idx[0].ctypes.data_as(_ip), idx[1].ctypes.data_as(_ip), idx[2].ctypes.data_as(_ip), _ptr(coef), int(n_signals)), (idx, coef)

    def _signal_targets(self, n_signals, targets, signal_weights, time_weights):
        B, T, ns = self.batch, self.n_timepoints, int(n_signals)
        tg = _f64(targets)
        if tg.ndim not in (2, 3) or tg.shape[-1] != ns or (tg.ndim == 3 and tg.shape[0] != B) or (T is not None and tg.shape[-2] != T):
            raise ValueError(f"targets must be ({T}, {ns}) or ({B}, {T}, {ns}), got {tg.shape}")
        om = None
        if signal_weights is not None:
            om = _f64(signal_weights)
            if om.shape != (ns,):
                raise ValueError(f"signal_weights must be ({ns},), got {om.shape}")
        return tg, int(tg.ndim == 3), om, self._time_weights(time_weights)

    def signal_values(self, terms, n_signals):
        """(batch, T, n_signals) signals (``dfx_signal_values``) on the resident history of the last forward pass: linear combinations of
        displacement (components 0..2), velocity (3..5), elastic-force (6..8) and, with ``hinge_channels`` set, hinge-force (9 + 3 node + dof) components of blocks."""
        args, keep = self._signal_terms(terms, n_signals)
        out = np.zeros((self.batch, self.n_timepoints or 1, max(int(n_signals), 1)))       # (no forward pass yet: the library refuses before it writes)
        self._check(self.lib.dfx_signal_values(self._h, *args, _ptr(out)), "dfx_signal_values")
        return out

    def signal_misfit_value(self, terms, n_signals, targets, signal_weights=None, time_weights=None):
        """(batch,) least-squares misfit of the signals against ``targets`` (``dfx_signal_misfit_value``)."""
        args, keep = self._signal_terms(terms, n_signals)
        tg, tpm, om, tau = self._signal_targets(n_signals, targets, signal_weights, time_weights)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_signal_misfit_value(self._h, *args, _ptr(tg), tpm, _ptr(om), _ptr(tau), _ptr(obj)), "dfx_signal_misfit_value")
        return obj

    def signal_misfit_value_and_grad(self, terms, n_signals, targets, signal_weights=None, time_weights=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the signal misfit in ONE call (``dfx_signal_misfit_value_and_grad``): channels,
        signals and residual cotangents are formed on the device, force terms add the Hessian-vector product K w to the cotangent of the
        reverse sweep and their mixed second derivatives behind it.  Results as :meth:`objective_value_and_grad`."""
        args, keep = self._signal_terms(terms, n_signals)
        tg, tpm, om, tau = self._signal_targets(n_signals, targets, signal_weights, time_weights)
        want, views, names, st = self._grad_request(which)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_signal_misfit_value_and_grad(self._h, *args, _ptr(tg), tpm, _ptr(om), _ptr(tau), _ptr(obj), C.byref(want),
                                                              C.byref(views), int(bool(device)), C.byref(st)),
                    "dfx_signal_misfit_value_and_grad")
        return obj, self._grad_views(views, names, device), _stats(st)

    # -- signal projections on the device-resident history -----------------------------------------------------
    @property
    def has_signal_projection(self):
        return hasattr(self.lib, "dfx_signal_projection_value_and_grad")

    def _projection_args(self, n_signals, basis, row_weights=None, targets=None, weights=True):
        """The array arguments of ``dfx_signal_projection*``: basis (n_rows, T), row weights (n_signals, n_rows), targets (n_signals, n_rows)
        or (batch, n_signals, n_rows) or None = zeros."""
        self._need("dfx_signal_projection_value_and_grad", "signal projections", self._STALE)
        B, T, ns = self.batch, self.n_timepoints, int(n_signals)
        b = _f64(basis)
        if b.ndim != 2 or (T is not None and b.shape[1] != T):
            raise ValueError(f"basis must be (n_rows, {T}), got {b.shape}")
        nr = b.shape[0]
        if not weights:
            return b, nr, None, None, 0
        w = _f64(row_weights)
        if w.shape != (ns, nr):
            raise ValueError(f"row_weights must be ({ns}, {nr}), got {w.shape}")
        tg = None
        if targets is not None:
            tg = _f64(targets)
            if tg.shape not in ((ns, nr), (B, ns, nr)):
                raise ValueError(f"targets must be ({ns}, {nr}) or ({B}, {ns}, {nr}), got {tg.shape}")
        return b, nr, w, tg, int(tg is not None and tg.ndim == 3)

    def signal_projections(self, terms, n_signals, basis):
        """(batch, n_signals, n_rows) projections P = B S of the signals on the rows of ``basis`` (``dfx_signal_projections``) on the
        resident history of the last forward pass."""
        args, keep = self._signal_terms(terms, n_signals)
        b, nr, _, _, _ = self._projection_args(n_signals, basis, weights=False)
        out = np.zeros((self.batch, max(int(n_signals), 1), max(nr, 1)))       # (a refused call: the library refuses before it writes)
        self._check(self.lib.dfx_signal_projections(self._h, *args, _ptr(b), nr, _ptr(out)), "dfx_signal_projections")
        return out

    def signal_projection_value(self, terms, n_signals, basis, row_weights, targets=None):
        """(batch,) weighted quadratic form 1/2 sum W (P - Ptarget)^2 of the projections (``dfx_signal_projection_value``)."""
        args, keep = self._signal_terms(terms, n_signals)
        b, nr, w, tg, tpm = self._projection_args(n_signals, basis, row_weights, targets)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_signal_projection_value(self._h, *args, _ptr(b), nr, _ptr(w), _ptr(tg), tpm, _ptr(obj)), "dfx_signal_projection_value")
        return obj

    def signal_projection_value_and_grad(self, terms, n_signals, basis, row_weights, targets=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the projection objective in ONE call (``dfx_signal_projection_value_and_grad``):
        the time reduction and the cotangent on the signals are formed on the device, everything behind them is the signal misfit's.
        Results as :meth:`signal_misfit_value_and_grad`."""
        args, keep = self._signal_terms(terms, n_signals)
        b, nr, w, tg, tpm = self._projection_args(n_signals, basis, row_weights, targets)
        want, views, names, st = self._grad_request(which)
        obj = np.zeros(self.batch)
        self._check(self.lib.dfx_signal_projection_value_and_grad(self._h, *args, _ptr(b), nr, _ptr(w), _ptr(tg), tpm, _ptr(obj), C.byref(want),
                                                                  C.byref(views), int(bool(device)), C.byref(st)),
                    "dfx_signal_projection_value_and_grad")
        return obj, self._grad_views(views, names, device), _stats(st)

    # -- signal cross-correlation on the device-resident history ------------------------------------------------
    @property
    def has_signal_xcorr(self):
        return hasattr(self.lib, "dfx_signal_xcorr_value_and_grad")

    def _xcorr_args(self, n_signals, pairs, max_lag, templates, normalisation):
        """The pair, template, lag and normalisation arguments of ``dfx_signal_xcorr*``: ``pairs`` a sequence of (a, b), b < 0 naming
        column -1 - b of ``templates`` (T, n_templates) or (batch, T, n_templates); ``normalisation`` a name of ``XCORR_NORMS`` (or its
        number).  Returns (the C arguments, the arrays they point into)."""
        self._need("dfx_signal_xcorr_value_and_grad", "signal cross-correlation", self._STALE)
        B, T = self.batch, self.n_timepoints
        p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(p[:, 0], dtype=np.int32), np.ascontiguousarray(p[:, 1], dtype=np.int32)
        tp, nt = None, 0
        if templates is not None:
            tp = _f64(templates)
            if tp.ndim not in (2, 3) or (tp.ndim == 3 and tp.shape[0] != B) or (T is not None and tp.shape[-2] != T):
                raise ValueError(f"templates must be ({T}, n_templates) or ({B}, {T}, n_templates), got {tp.shape}")
            nt = tp.shape[-1]
        norm = XCORR_NORMS[normalisation] if isinstance(normalisation, str) else int(normalisation)
        return (len(p), pa.ctypes.data_as(_ip), pb.ctypes.data_as(_ip), _ptr(tp), nt, int(tp is not None and tp.ndim == 3), int(max_lag), norm), (pa, pb, tp)

    @staticmethod
    def _xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target):
        red = XCORR_REDUCES[reduce] if isinstance(reduce, str) else int(reduce)
        return (red, int(0 if lag is None else lag), float(1.0 if beta is None else beta), float(w_peak), float(w_delay), float(delay_target))

    def signal_xcorr(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference"):
        """(batch, 2 max_lag + 1) normalised cross-correlation rho of the signal pairs over the lags -max_lag .. max_lag in output indices
        (``dfx_signal_xcorr``; lag d at index d + max_lag, d > 0: side B lags side A) on the resident history of the last forward pass."""
        xa, keep2 = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        out = np.zeros((self.batch, 2 * max(int(max_lag), 0) + 1))
        self._check(self.lib.dfx_signal_xcorr(self._h, *args, *xa, _ptr(out)), "dfx_signal_xcorr")
        return out

    def signal_xcorr_value(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference", reduce="max", lag=None, beta=None,
                           w_peak=1.0, w_delay=0.0, delay_target=0.0):
        """(J, peak, delay), (batch,) each: J = w_peak M + 1/2 w_delay (delta - delay_target)^2 of the reduction ``reduce`` ("at" the lag
        ``lag``, "max", "softmax" with ``beta``) of the cross-correlation over the lags (``dfx_signal_xcorr_value``)."""
        xa, keep2 = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        va = self._xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target)
        obj, peak, delay = np.zeros(self.batch), np.zeros(self.batch), np.zeros(self.batch)
        self._check(self.lib.dfx_signal_xcorr_value(self._h, *args, *xa, *va, _ptr(obj), _ptr(peak), _ptr(delay)), "dfx_signal_xcorr_value")
        return obj, peak, delay

    def signal_xcorr_value_and_grad(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference", reduce="max", lag=None,
                                    beta=None, w_peak=1.0, w_delay=0.0, delay_target=0.0, which=ALL_GRADS, device=False):
        """(J, peak, delay) and the requested gradients of J in ONE call (``dfx_signal_xcorr_value_and_grad``): the correlation over the lags,
        its reduction and the cotangent on the signals are formed on the device, everything behind them is the signal misfit's.  Returns
        (J, peak, delay, gradients, stats), the gradients as :meth:`signal_misfit_value_and_grad`."""
        xa, keep2 = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        va = self._xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target)
        want, views, names, st = self._grad_request(which)
        obj, peak, delay = np.zeros(self.batch), np.zeros(self.batch), np.zeros(self.batch)
        self._check(self.lib.dfx_signal_xcorr_value_and_grad(self._h, *args, *xa, *va, _ptr(obj), _ptr(peak), _ptr(delay), C.byref(want),
                                                             C.byref(views), int(bool(device)), C.byref(st)),
                    "dfx_signal_xcorr_value_and_grad")
        return obj, peak, delay, self._grad_views(views, names, device), _stats(st)

    # -- the samples of a table drive as a differentiable leaf ------------------------------------------------
    @property
    def has_fn_table_grads(self):
        return hasattr(self.lib, "dfx_fn_table_grads")

    def _need_table(self, entry):
        self._need(entry, "table-sample gradients", self._STALE)

    def fn_table_values(self, fn, values):
        """New values of the table of time function ``fn`` (``dfx_fn_table_values``): (n_tab,) for all members or (batch, n_tab).  They
        hold for every later solve; the kept trajectory is dropped, as by :meth:`set_params`."""
        self._need_table("dfx_fn_table_values")
        n = self.fn_table_n[int(fn)] if 0 <= int(fn) < DFX_MAX_FNS else 0
        v = _f64(values)
        if v.shape not in ((n,), (self.batch, n)):
            raise ValueError(f"fn_table_values: values must be ({n},) or ({self.batch}, {n}), got {v.shape}")
        self._check(self.lib.dfx_fn_table_values(self._h, int(fn), _ptr(v), int(v.ndim == 2)), "dfx_fn_table_values")

    def fn_table_grads(self, enable=True):
        """Opt in (or out): every later reverse sweep keeps the cotangent of the drive per stage and reduces it onto the samples of the
        table functions (``dfx_fn_table_grads``)."""
        self._need_table("dfx_fn_table_grads")
        self._check(self.lib.dfx_fn_table_grads(self._h, int(bool(enable))), "dfx_fn_table_grads")

    def fn_table_grad(self, fn):
        """(batch, n_tab) gradient of the samples of table function ``fn`` from the last reverse sweep (``dfx_fn_table_grad``)."""
        self._need_table("dfx_fn_table_grad")
        out = np.zeros((self.batch, max(self.fn_table_n[int(fn)] if 0 <= int(fn) < DFX_MAX_FNS else 0, 1)))
        self._check(self.lib.dfx_fn_table_grad(self._h, int(fn), _ptr(out)), "dfx_fn_table_grad")
        return out

    def drive_cotangent(self, member=0):
        """(times (n,), gbar (n_fns, n)) of one member from the last reverse sweep (``dfx_drive_cotangent``): the stage times in order
        and the cotangent of every drive value g_f there."""
        self._need_table("dfx_drive_cotangent")
        n = C.c_int64(0)
        self._check(self.lib.dfx_drive_cotangent(self._h, int(member), None, None, 0, C.byref(n)), "dfx_drive_cotangent")
        times, gbar = np.zeros(n.value), np.zeros((max(self.n_fns, 1), n.value))
        self._check(self.lib.dfx_drive_cotangent(self._h, int(member), _ptr(times), _ptr(gbar), n.value, C.byref(n)), "dfx_drive_cotangent")
        return times, gbar[:self.n_fns]

    def fn_table_tangents(self, fn, values_dots):
        """Per-direction sample tangents (n_dirs, batch, n_tab) of table function ``fn`` for the forward-mode entries
        (``dfx_fn_table_tangents``); None clears them."""
        self._need_table("dfx_fn_table_tangents")
        if values_dots is None:
            self._check(self.lib.dfx_fn_table_tangents(self._h, int(fn), None, 0), "dfx_fn_table_tangents")
            return
        v = _f64(values_dots)
        n = self.fn_table_n[int(fn)] if 0 <= int(fn) < DFX_MAX_FNS else 0
        if v.ndim != 3 or v.shape[1:] != (self.batch, n):
            raise ValueError(f"fn_table_tangents: values_dots must be (n_dirs, {self.batch}, {n}), got {v.shape}")
        self._check(self.lib.dfx_fn_table_tangents(self._h, int(fn), _ptr(v), v.shape[0]), "dfx_fn_table_tangents")

    def response_data(self, strains=True, kinetic=True):
        """Per-ligament strain energies (batch, T, n_bonds) x 3 and per-block kinetic energy (batch, T, n_blocks) of the last
        forward solve, computed on the device from its resident history."""
        B, T = self.batch, self.n_timepoints
        out = {}
        if strains:
            for n in ("strain_energy_stretch", "strain_energy_shear", "strain_energy_bending"):
                out[n] = np.empty((B, T, self.n_bonds))
        if kinetic:
            out["kinetic_energy"] = np.empty((B, T, self.n_blocks))
        self._check(self.lib.dfx_response_data(self._h, _ptr(out.get("strain_energy_stretch")), _ptr(out.get("strain_energy_shear")),
                                               _ptr(out.get("strain_energy_bending")), _ptr(out.get("kinetic_energy"))), "dfx_response_data")
        return out

    # -- test hooks ---------------------------------------------------------------------------
    def rhs(self, y, t):
        B, nb = self.batch, self.n_blocks
        y = _f64(y, (B, 2, nb, 3))
        dy = np.empty_like(y)
        self._check(self.lib.dfx_rhs(self._h, _ptr(y), float(t), _ptr(dy)), "dfx_rhs")
        return dy

    def rhs_vjp(self, y, t, lam, which=tuple(_PARAM_FIELDS + ["block_centroids"])):
        B, nb = self.batch, self.n_blocks
        y, lam = _f64(y, (B, 2, nb, 3)), _f64(lam, (B, 2, nb, 3))
        y_bar = np.empty_like(y)
        g, out = self._grads(which)
        self._check(self.lib.dfx_rhs_vjp(self._h, _ptr(y), float(t), _ptr(lam), _ptr(y_bar), C.byref(g)), "dfx_rhs_vjp")
        return y_bar, out

    @property
    def has_rhs_jvp(self):
        return hasattr(self.lib, "dfx_rhs_jvp")

    def rhs_jvp(self, y, t, y_dots, params_dots, n_dirs):
        """Forward mode of :meth:`rhs` for ``n_dirs`` directions (``dfx_rhs_jvp``, the twin of :meth:`rhs_vjp`): ``y_dots``
        (batch, n_dirs, 2, nb, 3) or None, ``params_dots`` a list of ``n_dirs`` dicts of arrays by ``dfx_params`` field name (or None).
        Returns (dy (batch, 2, nb, 3), dy_dots (batch, n_dirs, 2, nb, 3)); rows of constrained DOFs are 0."""
        self._need("dfx_rhs_jvp")
        K = int(n_dirs)
        if params_dots is not None and len(params_dots) != K:
            raise ValueError(f"rhs_jvp: need one params_dot per direction (n_dirs={K})")
        B, nb = self.batch, self.n_blocks
        y = _f64(y, (B, 2, nb, 3))
        y_dots = self._state0_dots(y_dots, K) if K >= 1 else None
        p, keep = self._params_dots(params_dots, K) if K >= 1 else (None, [])
        dy, dy_dots = np.empty((B, 2, nb, 3)), np.empty((B, max(K, 0), 2, nb, 3))
        self._check(self.lib.dfx_rhs_jvp(self._h, _ptr(y), float(t), _ptr(y_dots), p, K, _ptr(dy), _ptr(dy_dots)), "dfx_rhs_jvp")
        return dy, dy_dots

    def energy(self, u):
        u = _f64(u, (self.batch, self.n_blocks, 3))
        e = np.zeros(self.batch)
        self._check(self.lib.dfx_energy(self._h, _ptr(u), _ptr(e)), "dfx_energy")
        return e


class DeviceArray:
    """A float64 array in the HBM of an engine's GPU (a pointer the library handed out, valid until the next call on that engine)."""

    def __init__(self, engine, ptr, shape):
        self.engine, self.ptr, self.shape = engine, ptr, tuple(shape)
        self.size = int(np.prod(self.shape))
        self.nbytes = 8 * self.size

    def to_host(self):
        out = np.empty(self.shape)
        self.engine._check(self.engine.lib.dfx_download(self.engine._h, _ptr(out), self.ptr, self.size), "dfx_download")
        return out


def _stats(st):
    return {"steps": st.steps, "rhs_evals": st.rhs_evals, "launches": st.launches, "kernel_ms": st.kernel_ms,
            "stage_kernel_us": st.stage_kernel_us, "streams": st.streams, "stage_checkpoint": st.stage_checkpoint,
            "checkpoint_records": st.checkpoint_records, "tile_kernels": st.tile_kernels}
