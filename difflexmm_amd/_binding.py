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
SPECTRUM_MEASURES = {"ratio": 0, "log": 1}                           # DFX_SPECTRUM_RATIO / _LOG
SPECTRUM_AGGREGATES = {"sum": 0, "ks": 1}                            # DFX_SPECTRUM_SUM / _KS
FN_ZERO, FN_PULSE, FN_HARMONIC, FN_RAMP, FN_SECH2TANH, FN_CONSTANT, FN_RAMP_CAP, FN_TABLE = range(8)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


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
                "dfx_signal_xcorr", "dfx_signal_xcorr_value", "dfx_signal_xcorr_value_and_grad", "dfx_signal_spectrum",
                "dfx_signal_spectrum_value", "dfx_signal_spectrum_value_and_grad", "dfx_strain_peak_value",
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


def _argtypes():
    """Entry name -> argument types for every entry point of include/dfx.h, from argument groups that are each written once."""
    P, H, i32, i64, f64 = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lp, stats, grads, params, dmap = P(i64), P(dfx_stats), P(dfx_grads), P(dfx_params), P(dfx_design_map)
    terms = [i32, _ip, _ip, _ip, _dp, i32]                       # n_terms, signal, block, component, coef, n_signals
    tail = [grads, grads, i32, stats]                            # want, views, device_views, stats of every *_value_and_grad
    corr = [i32, _ip, _ip, _dp, i32, i32, i32, i32]              # pairs, templates, max_lag, normalisation
    xval = [i32, i32, f64, f64, f64, f64, _dp, _dp, _dp]         # reduce, lag, beta, w_peak, w_delay, delay_target, J, peak, delay
    peak = [_dp, i32, _dp, i32, _dp, i32, f64, _dp, _dp, _ip]    # coef, weights, tau, aggregate, sharpness, J, peak, peak_at
    spec = [_dp, i32, i32, _dp, _dp, _dp, _dp, i32]              # basis, n_rows, n_groups, Wn, Wd, n0, d0, offsets_per_member
    sval = [i32, i32, f64, _dp, _dp, _dp]                        # measure, aggregate, beta, group_coef, J, measures
    grid = [H, _dp, _dp, i32, _ip, _dp, i32, _dp, stats]         # a fixed-grid forward pass
    kinetic = [H, _ip, i32, _dp, grads, grads, stats]
    adaptive = [H, _dp, _dp, i32, f64, f64, i64]                 # state0, timepoints, T, rtol, atol, max_attempts
    design = [dmap, _dp, i32, f64, _dp, _dp, _dp, _dp]           # the native design map: designs, count, density, four arrays
    fixed, dense = [_dp, i32, _ip, _dp, i32], [_dp, i32, _dp, lp, i64]      # timepoints and steps of the two kinds of tangent solve
    one, multi = [H, _dp, _dp, params], [H, _dp, _dp, params, i32]          # state0, its tangent(s), the parameter tangent(s)[, n_dirs]
    out = [_dp, _dp, stats]
    objective, strain = [H, i32, _dp, i32, _dp, _dp, i32, _dp], [H, _dp, i32, _dp, _dp, _dp]
    misfit, projection = [H] + terms + [_dp, i32, _dp, _dp, _dp], [H] + terms + [_dp, i32, _dp, _dp, i32, _dp]
    return {
        "dfx_create": [P(dfx_problem), P(H)],
        "dfx_destroy": [H],
        "dfx_share_checkpoint": [H, H],
        "dfx_last_error": [H],
        "dfx_set_params": [H, params],
        "dfx_reserve": [H, i64, i32, i32],
        "dfx_abi_layout": [_ip, i32],
        "dfx_forward": [H, _dp, _dp, i32, i32, i32, _dp, stats],
        "dfx_forward_grid": grid,
        "dfx_forward_grid_members": grid,
        "dfx_adaptive_step_counts": [H, _ip],
        "dfx_adaptive_step_times": [H, i32, _dp, i64, lp],
        "dfx_forward_adaptive": adaptive + [_dp, stats],
        "dfx_forward_adaptive_keep": adaptive + [i32, _dp, stats],
        "dfx_design_forward": design,
        "dfx_design_vjp": design + [_dp],
        "dfx_member_status": [H, _ip],
        "dfx_set_failure_policy": [H, i32],
        "dfx_test_set_spin_limit": [H, i32],
        "dfx_adjoint": [H, _dp, grads, stats],
        "dfx_objective_kinetic": [H, _ip, i32, _dp],
        "dfx_adjoint_kinetic": [H, _ip, i32, grads, stats],
        "dfx_kinetic_value_and_grad": kinetic,
        "dfx_kinetic_value_and_grad_device": kinetic,
        "dfx_forward_kinetic_value_and_grad": [H, _dp, _dp, i32, _ip, _ip, i32, _dp] + tail + [stats],
        "dfx_response_data": [H, _dp, _dp, _dp, _dp],
        "dfx_rhs": [H, _dp, f64, _dp],
        "dfx_rhs_vjp": [H, _dp, f64, _dp, _dp, grads],
        "dfx_rhs_jvp": [H, _dp, f64, _dp, params, i32, _dp, _dp],
        "dfx_energy": [H, _dp, _dp],
        "dfx_device_count": [],
        "dfx_version": [],
        "dfx_forward_tangent": one + fixed + out,
        "dfx_forward_tangent_dense": one + dense + out,
        "dfx_forward_tangent_multi": multi + fixed + out,
        "dfx_forward_tangent_dense_multi": multi + dense + out,
        "dfx_forward_tangent_signals_multi": multi + fixed + terms + out,
        "dfx_forward_tangent_signals_dense_multi": multi + dense + terms + out,
        "dfx_dense_output_map": [_dp, lp, i64, i32, _dp, i32, _ip, _dp],
        "dfx_objective_value": objective,
        "dfx_objective_value_and_grad": objective + tail,
        "dfx_strain_objective_value": strain,
        "dfx_strain_objective_value_and_grad": strain + tail,
        "dfx_strain_peak_value": [H] + peak,
        "dfx_strain_peak_value_and_grad": [H] + peak + tail,
        "dfx_signal_values": [H] + terms + [_dp],
        "dfx_signal_hinge_channels": [H, i32],
        "dfx_signal_misfit_value": misfit,
        "dfx_signal_misfit_value_and_grad": misfit + tail,
        "dfx_signal_projections": [H] + terms + [_dp, i32, _dp],
        "dfx_signal_projection_value": projection,
        "dfx_signal_projection_value_and_grad": projection + tail,
        "dfx_signal_xcorr": [H] + terms + corr + [_dp],
        "dfx_signal_xcorr_value": [H] + terms + corr + xval,
        "dfx_signal_xcorr_value_and_grad": [H] + terms + corr + xval + tail,
        "dfx_signal_spectrum": [H] + terms + spec + [i32, _dp],
        "dfx_signal_spectrum_value": [H] + terms + spec + sval,
        "dfx_signal_spectrum_value_and_grad": [H] + terms + spec + sval + tail,
        "dfx_fn_table_values": [H, i32, _dp, i32],
        "dfx_fn_table_grads": [H, i32],
        "dfx_fn_table_grad": [H, i32, _dp],
        "dfx_drive_cotangent": [H, i32, _dp, _dp, i64, lp],
        "dfx_fn_table_tangents": [H, i32, _dp, i32],
        "dfx_comm_unique_id": [C.c_char_p],
        "dfx_comm_init": [i32, i32, C.c_char_p, i32, P(H)],
        "dfx_comm_destroy": [H],
        "dfx_comm_rank": [H],
        "dfx_comm_size": [H],
        "dfx_comm_barrier": [H],
        "dfx_comm_rccl_version": [_ip, _ip],
        "dfx_gather_objectives": [H, _dp, i32, _dp],
        "dfx_reduce_grads": [H, _dp, i64],
        "dfx_comm_allreduce": [H, _dp, i64, i32],
        "dfx_comm_last_error": [],
        "dfx_mem_info": [i32, lp, lp],
        "dfx_device_synchronize": [i32],
        "dfx_download": [H, _dp, H, i64],
    }


_ARGTYPES = _argtypes()
_STRING_RETURNS = ("dfx_last_error", "dfx_version", "dfx_comm_last_error")


def declare(lib):
    """Attach argument / result types to every entry point of include/dfx.h that the library has (the CPU port of the oracle and a stale
    libdfx.so lack the later ones): no entry's types depend on another entry's presence."""
    check_abi_layout(lib)
    for name, argtypes in _ARGTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = C.c_char_p if name in _STRING_RETURNS else C.c_int
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


_POINTER_OF = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.int64): _lp}


def _c(a):
    """An array as the pointer of its element type (float64, int32 or int64); anything else -- a number, None, a pointer -- as it is."""
    if not isinstance(a, np.ndarray):
        return a
    if a.dtype not in _POINTER_OF or not a.flags.c_contiguous:
        raise TypeError(f"an array argument must be C-contiguous float64, int32 or int64, got {a.dtype}, C-contiguous: {a.flags.c_contiguous}")
    return a.ctypes.data_as(_POINTER_OF[a.dtype])


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
        # state0 None: at rest (no upload); timepoints (batch, T): every member its own output times and step boundaries, shared
        # step counts; step_times: caller-chosen step boundaries (every timepoint must be one of them)
        scalar = np.ndim(steps_per_interval) == 0 and step_times is None
        state0, ts, T, spis, step_times, per_member = self._fixed_grid_args(state0, timepoints, steps_per_interval, step_times)
        fields = np.empty((self.batch, T, 2, self.n_blocks, 3)) if want_fields else None
        st = dfx_stats()
        if scalar and not per_member:
            entry, steps = "dfx_forward", (int(steps_per_interval),)
        else:   # its own number of equal steps in every output interval
            entry, steps = "dfx_forward_grid_members" if per_member else "dfx_forward_grid", (_c(spis), _ptr(step_times))
        self._check(getattr(self.lib, entry)(self._h, _ptr(state0), _ptr(ts), T, *steps, int(bool(keep_trajectory)), _ptr(fields), C.byref(st)),
                    entry)
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

    def _forward_tangent(self, entry, state0, state0_dots, params_dots, n_dirs, timepoints, fixed=None, dense=None, signals=None):
        """The six forward-tangent entries: ``fixed = (steps_per_interval, step_times)`` or ``dense = (step_times, n_steps)``;
        ``n_dirs = None`` for the single-direction entries, which take one state0_dot / params_dot and no count; ``signals =
        (terms, n_signals)`` keeps the history on the device and returns the signals instead of the fields."""
        who = entry[len("dfx_"):]
        self._need(entry)
        K = 1 if n_dirs is None else int(n_dirs)
        if K < 1 or (n_dirs is not None and params_dots is not None and len(params_dots) != K):
            raise ValueError(f"{who}: need n_dirs >= 1 and one params_dot per direction (n_dirs={K})")
        B, nb = self.batch, self.n_blocks
        if dense is None:
            state0, ts, T, spis, step_times, per_member = self._fixed_grid_args(state0, timepoints, *fixed)
            grid = (_c(spis), _ptr(step_times), int(per_member))
        else:
            state0, ts, T, st_times, ns = self._dense_grid_args(who, state0, timepoints, *dense)
            grid = (_ptr(st_times), _c(ns), st_times.shape[1])
        if n_dirs is None:
            state0_dots = _f64(state0_dots, (B, 2, nb, 3)) if state0_dots is not None else None
            p, keep = self._params_dots([params_dots], 1)
            dirs = ()
        else:
            state0_dots = self._state0_dots(state0_dots, K)
            p, keep = self._params_dots(params_dots, K)
            dirs = (K,)
        if signals is None:
            targs = ()
            out, out_dots = np.empty((B, T, 2, nb, 3)), np.empty((B,) + dirs + (T, 2, nb, 3))
        else:
            targs, tkeep = self._signal_terms(*signals)
            n_sig = max(int(signals[1]), 1)
            out, out_dots = np.zeros((B, T, n_sig)), np.zeros((B, K, T, n_sig))      # (a refusal comes before the library writes)
        st = dfx_stats()
        self._check(getattr(self.lib, entry)(self._h, _ptr(state0), _ptr(state0_dots), p, *dirs, _ptr(ts), T, *grid, *targs, _ptr(out),
                                             _ptr(out_dots), C.byref(st)), entry)
        return out, out_dots, _stats(st)

    @property
    def has_forward_tangent(self):
        return hasattr(self.lib, "dfx_forward_tangent")

    def forward_tangent(self, state0, state0_dot, params_dot, timepoints, steps_per_interval, step_times=None):
        """Primal fields and their directional derivative along (state0_dot, params_dot) of the fixed-grid solve (``dfx_forward_tangent``)
        on the parameters of the last :meth:`set_params`.  ``params_dot``: arrays by ``dfx_params`` field name (a missing one: zero
        tangent); ``timepoints`` (T,) or (batch, T) (then every member its own grid, as :meth:`forward`).  Returns (fields, fields_dot, stats)."""
        return self._forward_tangent("dfx_forward_tangent", state0, state0_dot, params_dot, None, timepoints,
                                     fixed=(steps_per_interval, step_times))

    @property
    def has_forward_tangent_dense(self):
        return hasattr(self.lib, "dfx_forward_tangent_dense")

    def forward_tangent_dense(self, state0, state0_dot, params_dot, timepoints, step_times, n_steps):
        """Primal fields and their directional derivative of the ADAPTIVE solve's dense output on every member's own frozen accepted steps
        (``dfx_forward_tangent_dense``): ``step_times`` (batch, stride) rows ``t_0 .. t_{N_m}``, ``n_steps`` (batch,)
        (:func:`padded_step_times`), ``timepoints`` (T,).  Otherwise as :meth:`forward_tangent`.  Returns (fields, fields_dot, stats)."""
        return self._forward_tangent("dfx_forward_tangent_dense", state0, state0_dot, params_dot, None, timepoints, dense=(step_times, n_steps))

    @property
    def has_forward_tangent_multi(self):
        return hasattr(self.lib, "dfx_forward_tangent_multi")

    def forward_tangent_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, steps_per_interval, step_times=None):
        """:meth:`forward_tangent` for ``n_dirs`` directions per member with the primal evaluated once per stage
        (``dfx_forward_tangent_multi``): ``state0_dots`` (batch, n_dirs, 2, nb, 3) or None, ``params_dots`` a list of ``n_dirs`` dicts of
        arrays by ``dfx_params`` field name (or None).  Returns (fields (batch, T, ...), fields_dots (batch, n_dirs, T, ...), stats)."""
        return self._forward_tangent("dfx_forward_tangent_multi", state0, state0_dots, params_dots, n_dirs, timepoints,
                                     fixed=(steps_per_interval, step_times))

    @property
    def has_forward_tangent_dense_multi(self):
        return hasattr(self.lib, "dfx_forward_tangent_dense_multi")

    def forward_tangent_dense_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, step_times, n_steps):
        """:meth:`forward_tangent_dense` for ``n_dirs`` directions per member (``dfx_forward_tangent_dense_multi``); arguments as
        :meth:`forward_tangent_multi` and :meth:`forward_tangent_dense`.  Returns (fields, fields_dots (batch, n_dirs, T, ...), stats)."""
        return self._forward_tangent("dfx_forward_tangent_dense_multi", state0, state0_dots, params_dots, n_dirs, timepoints,
                                     dense=(step_times, n_steps))

    @property
    def has_forward_tangent_signals(self):
        return hasattr(self.lib, "dfx_forward_tangent_signals_multi")

    def forward_tangent_signals_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, steps_per_interval, terms, n_signals,
                                      step_times=None):
        """:meth:`forward_tangent_multi` with the history kept on the device (``dfx_forward_tangent_signals_multi``): the signals of
        ``terms`` (sequence of (signal, block, component, coef), as :meth:`signal_values`) and their tangents along the ``n_dirs``
        directions.  Returns (signals (batch, T, n_signals), signals_dots (batch, n_dirs, T, n_signals), stats)."""
        return self._forward_tangent("dfx_forward_tangent_signals_multi", state0, state0_dots, params_dots, n_dirs, timepoints,
                                     fixed=(steps_per_interval, step_times), signals=(terms, n_signals))

    def forward_tangent_signals_dense_multi(self, state0, state0_dots, params_dots, n_dirs, timepoints, step_times, n_steps, terms, n_signals):
        """:meth:`forward_tangent_dense_multi` with the history kept on the device (``dfx_forward_tangent_signals_dense_multi``);
        ``terms`` and the results as :meth:`forward_tangent_signals_multi`."""
        return self._forward_tangent("dfx_forward_tangent_signals_dense_multi", state0, state0_dots, params_dots, n_dirs, timepoints,
                                     dense=(step_times, n_steps), signals=(terms, n_signals))

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

    def _value(self, entry, lead, outs):
        """Run a value entry: ``lead`` its arguments behind the handle (arrays go as pointers), ``outs`` the arrays it fills."""
        self._check(getattr(self.lib, entry)(self._h, *map(_c, lead), *map(_c, outs)), entry)
        return outs

    def _value_and_grad(self, entry, lead, outs, which, device, centroids=False, device_flag=True, more_stats=()):
        """Run a ``*_value_and_grad`` entry: as :meth:`_value`, then the tail ``want, views[, device_views], stats`` (``device_flag=False``:
        the kinetic entries, whose name says where the gradients stay; ``more_stats``: structs that go before the sweep's).  Returns
        (gradients, stats of the reverse sweep)."""
        want, views, names, st = self._grad_request(which, centroids)
        tail = (int(bool(device)),) if device_flag else ()
        self._check(getattr(self.lib, entry)(self._h, *map(_c, lead), *map(_c, outs), C.byref(want), C.byref(views), *tail,
                                             *map(C.byref, more_stats), C.byref(st)), entry)
        return self._grad_views(views, names, device), _stats(st)

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
        obj = np.zeros(self.batch)
        entry = "dfx_kinetic_value_and_grad_device" if device else "dfx_kinetic_value_and_grad"
        if device and not hasattr(self.lib, entry):
            raise RuntimeError("device-resident gradients need the HIP library")
        return (obj,) + self._value_and_grad(entry, (tb, len(tb)), (obj,), which, device, device_flag=False)

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
        obj = np.zeros(B)
        st_f = dfx_stats()
        grads, st_a = self._value_and_grad("dfx_forward_kinetic_value_and_grad", (state0, ts, T, spis, tb, len(tb)), (obj,), which, device,
                                           more_stats=(st_f,))
        self.n_timepoints = T
        return obj, grads, _stats(st_f), st_a

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
        return int(kind), w, int(w.ndim == 2), tau, lev, int(lev is not None and lev.ndim == 3)

    def objective_value(self, kind, block_weights, time_weights=None, lever0=None):
        """(batch,) value of a weighted objective (``OBJ_KINETIC`` / ``OBJ_ANGULAR_MOMENTUM``, ``dfx_objective_value``) on the resident
        history of the last forward pass."""
        return self._value("dfx_objective_value", self._objective_args(kind, block_weights, time_weights, lever0), [np.zeros(self.batch)])[0]

    def objective_value_and_grad(self, kind, block_weights, time_weights=None, lever0=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of a weighted objective in ONE call (``dfx_objective_value_and_grad``): the cotangent
        is formed on the device, the objective rides along with the reverse sweep, the explicit inertia / block-centroid terms are added
        behind it.  Results as :meth:`kinetic_value_and_grad`: read-only views of pinned memory, or ``DeviceArray`` handles with
        ``device=True``; ``block_centroids`` is available on every lattice for the angular kind."""
        lead, obj = self._objective_args(kind, block_weights, time_weights, lever0), np.zeros(self.batch)
        return (obj,) + self._value_and_grad("dfx_objective_value_and_grad", lead, (obj,), which, device, centroids=lead[0] == OBJ_ANGULAR_MOMENTUM)

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
        return self._value("dfx_strain_objective_value", self._strain_objective_args(bond_weights, time_weights, parts), [np.zeros(self.batch)])[0]

    def strain_objective_value_and_grad(self, bond_weights, time_weights=None, parts=(1.0, 1.0, 1.0, 0.0), which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the weighted ligament strain energy in ONE call
        (``dfx_strain_objective_value_and_grad``): the ligament forces are formed on the device as the cotangent of the reverse sweep, the
        explicit node-vector / void-angle / per-ligament terms are added behind it.  Results as :meth:`objective_value_and_grad`."""
        lead, obj = self._strain_objective_args(bond_weights, time_weights, parts), np.zeros(self.batch)
        return (obj,) + self._value_and_grad("dfx_strain_objective_value_and_grad", lead, (obj,), which, device)

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

    def _peak_outs(self):
        return np.zeros(self.batch), np.zeros(self.batch), np.zeros((self.batch, 2), dtype=np.int32)          # J, peak, peak_at

    def strain_peak_value(self, bond_coef, bond_weights=None, time_weights=None, aggregate="ks", sharpness=1.0):
        """(J, peak, peak_at): the smooth maximum (batch,), the hard maximum (batch,) and its (output, bond) (batch, 2) of the ligament strain
        measure (``dfx_strain_peak_value``) on the resident history of the last forward pass."""
        lead = self._strain_peak_args(bond_coef, bond_weights, time_weights, aggregate, sharpness)
        return self._value("dfx_strain_peak_value", lead, self._peak_outs())

    def strain_peak_value_and_grad(self, bond_coef, bond_weights=None, time_weights=None, aggregate="ks", sharpness=1.0, which=ALL_GRADS,
                                   device=False):
        """(J, peak, peak_at) and the requested gradients of J in ONE call (``dfx_strain_peak_value_and_grad``): maximum, softmax sum and
        the softmax-weighted ligament forces are formed on the device as the cotangent of the reverse sweep, the explicit node-vector /
        reference-vector terms are added behind it.  Results as :meth:`objective_value_and_grad`."""
        lead, outs = self._strain_peak_args(bond_coef, bond_weights, time_weights, aggregate, sharpness), self._peak_outs()
        return (outs,) + self._value_and_grad("dfx_strain_peak_value_and_grad", lead, outs, which, device)

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
        return self._value("dfx_signal_values", args, [out])[0]

    def signal_misfit_value(self, terms, n_signals, targets, signal_weights=None, time_weights=None):
        """(batch,) least-squares misfit of the signals against ``targets`` (``dfx_signal_misfit_value``)."""
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + self._signal_targets(n_signals, targets, signal_weights, time_weights)
        return self._value("dfx_signal_misfit_value", lead, [np.zeros(self.batch)])[0]

    def signal_misfit_value_and_grad(self, terms, n_signals, targets, signal_weights=None, time_weights=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the signal misfit in ONE call (``dfx_signal_misfit_value_and_grad``): channels,
        signals and residual cotangents are formed on the device, force terms add the Hessian-vector product K w to the cotangent of the
        reverse sweep and their mixed second derivatives behind it.  Results as :meth:`objective_value_and_grad`."""
        args, keep = self._signal_terms(terms, n_signals)
        lead, obj = args + self._signal_targets(n_signals, targets, signal_weights, time_weights), np.zeros(self.batch)
        return (obj,) + self._value_and_grad("dfx_signal_misfit_value_and_grad", lead, (obj,), which, device)

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
        return self._value("dfx_signal_projections", args + (b, nr), [out])[0]

    def signal_projection_value(self, terms, n_signals, basis, row_weights, targets=None):
        """(batch,) weighted quadratic form 1/2 sum W (P - Ptarget)^2 of the projections (``dfx_signal_projection_value``)."""
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + self._projection_args(n_signals, basis, row_weights, targets)
        return self._value("dfx_signal_projection_value", lead, [np.zeros(self.batch)])[0]

    def signal_projection_value_and_grad(self, terms, n_signals, basis, row_weights, targets=None, which=ALL_GRADS, device=False):
        """Value (batch,) and the requested gradients of the projection objective in ONE call (``dfx_signal_projection_value_and_grad``):
        the time reduction and the cotangent on the signals are formed on the device, everything behind them is the signal misfit's.
        Results as :meth:`signal_misfit_value_and_grad`."""
        args, keep = self._signal_terms(terms, n_signals)
        lead, obj = args + self._projection_args(n_signals, basis, row_weights, targets), np.zeros(self.batch)
        return (obj,) + self._value_and_grad("dfx_signal_projection_value_and_grad", lead, (obj,), which, device)

    # -- signal cross-correlation on the device-resident history ------------------------------------------------
    @property
    def has_signal_xcorr(self):
        return hasattr(self.lib, "dfx_signal_xcorr_value_and_grad")

    def _xcorr_args(self, n_signals, pairs, max_lag, templates, normalisation):
        """The pair, template, lag and normalisation arguments of ``dfx_signal_xcorr*``: ``pairs`` a sequence of (a, b), b < 0 naming
        column -1 - b of ``templates`` (T, n_templates) or (batch, T, n_templates); ``normalisation`` a name of ``XCORR_NORMS`` (or its
        number)."""
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
        return len(p), pa, pb, tp, nt, int(tp is not None and tp.ndim == 3), int(max_lag), norm

    @staticmethod
    def _xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target):
        red = XCORR_REDUCES[reduce] if isinstance(reduce, str) else int(reduce)
        return (red, int(0 if lag is None else lag), float(1.0 if beta is None else beta), float(w_peak), float(w_delay), float(delay_target))

    def signal_xcorr(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference"):
        """(batch, 2 max_lag + 1) normalised cross-correlation rho of the signal pairs over the lags -max_lag .. max_lag in output indices
        (``dfx_signal_xcorr``; lag d at index d + max_lag, d > 0: side B lags side A) on the resident history of the last forward pass."""
        xa = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        return self._value("dfx_signal_xcorr", args + xa, [np.zeros((self.batch, 2 * max(int(max_lag), 0) + 1))])[0]

    def signal_xcorr_value(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference", reduce="max", lag=None, beta=None,
                           w_peak=1.0, w_delay=0.0, delay_target=0.0):
        """(J, peak, delay), (batch,) each: J = w_peak M + 1/2 w_delay (delta - delay_target)^2 of the reduction ``reduce`` ("at" the lag
        ``lag``, "max", "softmax" with ``beta``) of the cross-correlation over the lags (``dfx_signal_xcorr_value``)."""
        xa = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + xa + self._xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target)
        return self._value("dfx_signal_xcorr_value", lead, (np.zeros(self.batch), np.zeros(self.batch), np.zeros(self.batch)))

    def signal_xcorr_value_and_grad(self, terms, n_signals, pairs, max_lag, templates=None, normalisation="reference", reduce="max", lag=None,
                                    beta=None, w_peak=1.0, w_delay=0.0, delay_target=0.0, which=ALL_GRADS, device=False):
        """(J, peak, delay) and the requested gradients of J in ONE call (``dfx_signal_xcorr_value_and_grad``): the correlation over the lags,
        its reduction and the cotangent on the signals are formed on the device, everything behind them is the signal misfit's.  Returns
        (J, peak, delay, gradients, stats), the gradients as :meth:`signal_misfit_value_and_grad`."""
        xa = self._xcorr_args(n_signals, pairs, max_lag, templates, normalisation)
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + xa + self._xcorr_value_args(reduce, lag, beta, w_peak, w_delay, delay_target)
        outs = np.zeros(self.batch), np.zeros(self.batch), np.zeros(self.batch)          # J, peak, delay
        return outs + self._value_and_grad("dfx_signal_xcorr_value_and_grad", lead, outs, which, device)

    # -- signal spectral ratios on the device-resident history --------------------------------------------------
    @property
    def has_signal_spectrum(self):
        return hasattr(self.lib, "dfx_signal_spectrum_value_and_grad")

    def _spectrum_args(self, n_signals, basis, num_weights, den_weights, num_offset, den_offset):
        """The array arguments of ``dfx_signal_spectrum*``: basis (n_rows, T), group weights (G, n_signals, n_rows) each, offsets (G,) or
        (batch, G) or None = zeros (one per member as soon as either is)."""
        self._need("dfx_signal_spectrum_value_and_grad", "signal spectral ratios", self._STALE)
        B, T, ns = self.batch, self.n_timepoints, int(n_signals)
        b = _f64(basis)
        if b.ndim != 2 or (T is not None and b.shape[1] != T):
            raise ValueError(f"basis must be (n_rows, {T}), got {b.shape}")
        nr = b.shape[0]
        wn, wd = _f64(num_weights), _f64(den_weights)
        if wn.ndim != 3 or wn.shape[1:] != (ns, nr) or wd.shape != wn.shape:
            raise ValueError(f"num_weights and den_weights must be (G, {ns}, {nr}), got {wn.shape} and {wd.shape}")
        G = wn.shape[0]
        offs = [None if o is None else _f64(o) for o in (num_offset, den_offset)]
        for name, o in zip(("num_offset", "den_offset"), offs):
            if o is not None and o.shape not in ((G,), (B, G)):
                raise ValueError(f"{name} must be ({G},) or ({B}, {G}), got {o.shape}")
        per = any(o is not None and o.ndim == 2 for o in offs)
        if per:
            offs = [None if o is None else _f64(o, (B, G)) for o in offs]
        return b, nr, G, wn, wd, offs[0], offs[1], int(per)

    def _spectrum_value_args(self, G, measure, aggregate, beta, group_coef):
        a = _f64(np.ones(G) if group_coef is None else group_coef)
        if a.shape != (G,):
            raise ValueError(f"group_coef must be ({G},), got {a.shape}")
        mea = SPECTRUM_MEASURES[measure] if isinstance(measure, str) else int(measure)
        agg = SPECTRUM_AGGREGATES[aggregate] if isinstance(aggregate, str) else int(aggregate)
        return mea, agg, float(1.0 if beta is None else beta), a

    def signal_spectrum(self, terms, n_signals, basis, num_weights, den_weights, num_offset=None, den_offset=None, measure="log"):
        """(batch, G, 3) = N | D | l of the groups of a spectral-ratio objective (``dfx_signal_spectrum``), l the ``measure`` ("ratio" N / D
        or "log" ln N - ln D; NaN where it does not exist), on the resident history of the last forward pass."""
        sa = self._spectrum_args(n_signals, basis, num_weights, den_weights, num_offset, den_offset)
        args, keep = self._signal_terms(terms, n_signals)
        mea = SPECTRUM_MEASURES[measure] if isinstance(measure, str) else int(measure)
        return self._value("dfx_signal_spectrum", args + sa + (mea,), [np.zeros((self.batch, sa[2], 3))])[0]

    def signal_spectrum_value(self, terms, n_signals, basis, num_weights, den_weights, num_offset=None, den_offset=None, group_coef=None,
                              measure="log", aggregate="sum", beta=None):
        """(J, l): the aggregate (batch,) over the groups ("sum", or "ks" with ``beta``) of the measures l (batch, G) ("ratio" N / D or
        "log" ln N - ln D) of the band-power forms of the projections (``dfx_signal_spectrum_value``)."""
        sa = self._spectrum_args(n_signals, basis, num_weights, den_weights, num_offset, den_offset)
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + sa + self._spectrum_value_args(sa[2], measure, aggregate, beta, group_coef)
        return self._value("dfx_signal_spectrum_value", lead, (np.zeros(self.batch), np.zeros((self.batch, sa[2]))))

    def signal_spectrum_value_and_grad(self, terms, n_signals, basis, num_weights, den_weights, num_offset=None, den_offset=None,
                                       group_coef=None, measure="log", aggregate="sum", beta=None, which=ALL_GRADS, device=False):
        """(J, l) and the requested gradients of J in ONE call (``dfx_signal_spectrum_value_and_grad``): the forms, their reduction and
        the cotangent on the signals are formed on the device, everything behind them is the signal misfit's.  Returns
        (J, l, gradients, stats), the gradients as :meth:`signal_misfit_value_and_grad`."""
        sa = self._spectrum_args(n_signals, basis, num_weights, den_weights, num_offset, den_offset)
        args, keep = self._signal_terms(terms, n_signals)
        lead = args + sa + self._spectrum_value_args(sa[2], measure, aggregate, beta, group_coef)
        outs = np.zeros(self.batch), np.zeros((self.batch, sa[2]))          # J, l
        return outs + self._value_and_grad("dfx_signal_spectrum_value_and_grad", lead, outs, which, device)

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
