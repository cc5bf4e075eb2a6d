"""Cross-correlation measures between recorded signals -- the names of ``difflexmm/objective.py`` (post-processing of space-time
records in the notebooks; host code, SciPy where the reference uses ``jax.scipy.signal``) -- and the weighted objectives the engine
evaluates and differentiates on the device-resident history (``ObjectiveSpec``; ``include/dfx.h``: ``dfx_objective_value_and_grad``;
``StrainObjectiveSpec``: ``dfx_strain_objective_value_and_grad``; ``SignalSpec``: ``dfx_signal_misfit_value_and_grad``; ``ProjectionSpec``: ``dfx_signal_projection_value_and_grad``, with ``fourier_basis``
for its rows; ``CorrelationSpec``: ``dfx_signal_xcorr_value_and_grad`` -- the cross-correlation measures above as an objective on the
device, with ``xcorr_of_signals`` / ``host_xcorr_value_and_cotangent`` as its NumPy restatement; ``PeakStrainSpec``:
``dfx_strain_peak_value_and_grad`` -- a smooth maximum over output times and ligaments of a squared strain measure, with
``strain_limit_coefficients`` for its coefficients and ``host_peak_strain_value`` as its NumPy restatement)."""
from typing import Any, NamedTuple

import numpy as np
import scipy.signal

KINETIC, ANGULAR_MOMENTUM = 0, 1          # DFX_OBJ_*


def compute_xcorr2d(signal0, signal1, shift=(None, None)):
    """objective.py:10-39: full 2-D cross-correlation of two 2-D arrays divided by the peak of signal0's auto-correlation; with a shift
    along one axis (0 = no shift) the corresponding slice, with both the single value."""
    signal0, signal1 = np.asarray(signal0, dtype=float), np.asarray(signal1, dtype=float)
    xcorr2d = scipy.signal.correlate2d(signal0, signal1) / scipy.signal.correlate2d(signal0, signal0).max()
    s0, s1 = shift
    if s0 is None and s1 is None:
        return xcorr2d
    if s1 is None:
        return xcorr2d[signal1.shape[0] - 1 + s0, :]
    if s0 is None:
        return xcorr2d[:, signal1.shape[1] - 1 + s1]
    return xcorr2d[signal1.shape[0] - 1 + s0, signal1.shape[1] - 1 + s1]


def compute_xcorr(signal0, signal1, shift=None):
    """objective.py:42-57: the 1-D counterpart."""
    signal0, signal1 = np.asarray(signal0, dtype=float), np.asarray(signal1, dtype=float)
    xcorr = scipy.signal.correlate(signal0, signal1) / scipy.signal.correlate(signal0, signal0).max()
    return xcorr if shift is None else xcorr[signal1.shape[0] - 1 + shift]


def compute_max_xcorr2d_at_shift(signal0, signal1, shift, shift_axis=0):
    """objective.py:60-75: (maximum of the slice at ``shift`` along ``shift_axis``, delay along the other axis; delay > 0: signal1 lags)."""
    signal1 = np.asarray(signal1)
    sl = compute_xcorr2d(signal0, signal1, shift=(shift, None) if shift_axis == 0 else (None, shift))
    return sl.max(), -(int(sl.argmax()) + 1 - signal1.shape[1 if shift_axis == 0 else 0])


def compute_space_time_xcorr(space_time0, space_time1):
    """objective.py:78-89: space on axis 0, time on axis 1 -> (largest cross-correlation at zero space shift, its time delay)."""
    return compute_max_xcorr2d_at_shift(space_time0, space_time1, shift=0, shift_axis=0)


# ---- weighted objectives on the device-resident history -----------------------------------------------------------------------------
class ObjectiveSpec(NamedTuple):
    """A weighted sum over blocks and output times (``include/dfx.h``, DFX_OBJ_*):

        KINETIC            J_m = sum_k tau_k sum_b w_mb sum_d p_mbd v_mkbd^2 / 2
        ANGULAR_MOMENTUM   J_m = sum_k tau_k sum_b w_mb [ (a_x + u_x) m_y v_y - (a_y + u_y) m_x v_x + J omega ]

    ``block_weights`` (n_blocks,) or (batch, n_blocks); ``time_weights`` (T,) or None = all ones; ``lever0`` = block centroid - spin
    centre, (n_blocks, 2) or (batch, n_blocks, 2), angular kind only; p = (m_x, m_y, J) the inertia, (u, v) the fields."""
    kind: int
    block_weights: Any
    time_weights: Any = None
    lever0: Any = None

    def engine_call(self):
        """How ``DynamicSolver.value`` / ``value_and_raw`` reach the engine with a spec, stated once per spec class: (family -- the
        methods are ``Engine.<family>_value`` and ``<family>_value_and_grad`` --, the ``SignalSpec`` whose terms lead the arguments or
        None, the positional arguments, the keyword arguments)."""
        return "objective", None, (self.kind, self.block_weights, self.time_weights, self.lever0), {}

    @property
    def needs_centroids(self):
        """the levers of the angular kind contain the block centroids: their gradient exists on every lattice (no other spec has this)"""
        return self.kind == ANGULAR_MOMENTUM


def block_weights_from_targets(n_blocks, target_blocks_list, weights):
    """Weights of target regions -> weights of blocks.  ``target_blocks_list``: one array of block ids per target; ``weights``: one row
    (n_targets,) -> (n_blocks,), or one row per member (batch, n_targets) -> (batch, n_blocks).  Overlapping targets add."""
    w = np.asarray(weights, dtype=float)
    if w.shape[-1:] != (len(target_blocks_list),) or w.ndim not in (1, 2):
        raise ValueError(f"weights must be ({len(target_blocks_list)},) or (batch, {len(target_blocks_list)}), got {w.shape}")
    out = np.zeros(w.shape[:-1] + (int(n_blocks),))
    for i, tb in enumerate(target_blocks_list):
        tb = np.asarray(tb, dtype=np.int64).reshape(-1)
        if tb.size and (tb.min() < 0 or tb.max() >= n_blocks):
            raise ValueError(f"target {i}: block out of range [0, {n_blocks})")
        np.add.at(out, (Ellipsis, tb), w[..., i:i + 1])
    return out


def host_value_and_cotangent(spec, fields, inertia):
    """NumPy restatement of the two formulas: ``fields`` (batch, T, 2, n_blocks, 3) or (T, 2, n_blocks, 3), ``inertia`` (batch, n_blocks, 3)
    or (n_blocks, 3).  Returns (value, fields_bar, inertia_bar, centroid_bar): the value per member, its cotangent on the fields (what
    ``vjp`` / ``dfx_adjoint`` take), and the explicit terms d J / d inertia (.., n_blocks, 3) and d J / d block_centroids = d J / d lever0
    (.., n_blocks, 2; zeros for the kinetic kind) -- with the member axis of ``fields``."""
    f = np.asarray(fields, dtype=float)
    single = f.ndim == 4
    if single:
        f = f[None]
    B, T, _, nb, _ = f.shape
    p = np.broadcast_to(np.asarray(inertia, dtype=float), (B, nb, 3))
    w = np.broadcast_to(np.asarray(spec.block_weights, dtype=float), (B, nb))
    tau = np.ones(T) if spec.time_weights is None else np.asarray(spec.time_weights, dtype=float)
    if tau.shape != (T,):
        raise ValueError(f"time_weights must be ({T},), got {tau.shape}")
    tw = tau[None, :, None] * w[:, None, :]                     # (B, T, nb)
    u, v = f[:, :, 0], f[:, :, 1]
    fb = np.zeros_like(f)
    cen_bar = np.zeros((B, nb, 2))
    if spec.kind == KINETIC:
        value = np.sum(tw[..., None] * p[:, None] * v ** 2 / 2, axis=(1, 2, 3))
        fb[:, :, 1] = tw[..., None] * p[:, None] * v
        m_bar = np.sum(tw[..., None] * v ** 2 / 2, axis=1)
    elif spec.kind == ANGULAR_MOMENTUM:
        if spec.lever0 is None:
            raise ValueError("the angular-momentum objective needs lever0")
        a = np.broadcast_to(np.asarray(spec.lever0, dtype=float), (B, nb, 2))
        rx, ry = a[:, None, :, 0] + u[..., 0], a[:, None, :, 1] + u[..., 1]
        mx, my, J = p[:, None, :, 0], p[:, None, :, 1], p[:, None, :, 2]
        value = np.sum(tw * (rx * my * v[..., 1] - ry * mx * v[..., 0] + J * v[..., 2]), axis=(1, 2))
        fb[:, :, 0, :, 0] = tw * my * v[..., 1]
        fb[:, :, 0, :, 1] = -tw * mx * v[..., 0]
        fb[:, :, 1, :, 0] = -tw * ry * mx
        fb[:, :, 1, :, 1] = tw * rx * my
        fb[:, :, 1, :, 2] = tw * J
        m_bar = np.stack([-(tw * ry * v[..., 0]).sum(1), (tw * rx * v[..., 1]).sum(1), (tw * v[..., 2]).sum(1)], axis=-1)
        cen_bar = np.stack([(tw * my * v[..., 1]).sum(1), -(tw * mx * v[..., 0]).sum(1)], axis=-1)
    else:
        raise ValueError(f"unknown objective kind {spec.kind!r}")
    if single:
        return float(value[0]), fb[0], m_bar[0], cen_bar[0]
    return value, fb, m_bar, cen_bar


# ---- ligament strain energy on the device-resident history ---------------------------------------------------------------------------
class StrainObjectiveSpec:
    """The elastic energy stored in weighted ligaments (``include/dfx.h``: ``dfx_strain_objective_value[_and_grad]``):

        J_m = sum_k tau_k sum_bonds w_mb [ c_stretch E_stretch + c_shear E_shear + c_bend E_bend + c_contact E_contact ](bond; u_k, params_m)

    ``bond_weights`` (n_bonds,) or (batch, n_bonds), in the order of the problem's bond list; ``time_weights`` (T,) or None = all ones;
    ``parts`` = (c_stretch, c_shear, c_bend, c_contact).  The arrays are converted and their shapes checked here (``ValueError``); their
    lengths against a solve are checked where the spec is used."""
    __slots__ = ("bond_weights", "time_weights", "parts")

    def __init__(self, bond_weights, time_weights=None, parts=(1.0, 1.0, 1.0, 0.0)):
        w = np.array(bond_weights, dtype=float)
        if w.ndim not in (1, 2) or w.shape[-1] == 0:
            raise ValueError(f"bond_weights must be (n_bonds,) or (batch, n_bonds), got {w.shape}")
        tau = None
        if time_weights is not None:
            tau = np.array(time_weights, dtype=float)
            if tau.ndim != 1:
                raise ValueError(f"time_weights must be (T,), got {tau.shape}")
        c = np.array(parts, dtype=float)
        if c.shape != (4,) or not np.isfinite(c).all():
            raise ValueError(f"parts must be four finite numbers (c_stretch, c_shear, c_bend, c_contact), got {parts!r}")
        self.bond_weights, self.time_weights, self.parts = w, tau, tuple(float(x) for x in c)

    def __repr__(self):
        return f"StrainObjectiveSpec(bond_weights={self.bond_weights.shape}, time_weights={self.time_weights!r}, parts={self.parts})"

    def engine_call(self):
        return "strain_objective", None, (self.bond_weights, self.time_weights, self.parts), {}


def bond_weights_from_blocks(bond_connectivity, n_nodes_per_block, target_blocks_list, weights, ends="both"):
    """Weights of target regions -> weights of bonds.  A bond belongs to a target when both (``ends="both"``) or any (``ends="any"``) of its
    end blocks are in it; ``bond_connectivity`` (n_bonds, 2) node ids, node n on block n // n_nodes_per_block.  ``weights``: one row
    (n_targets,) -> (n_bonds,), or one row per member (batch, n_targets) -> (batch, n_bonds).  Overlapping targets add, as in
    ``block_weights_from_targets``."""
    if ends not in ("both", "any"):
        raise ValueError(f"ends must be 'both' or 'any', got {ends!r}")
    bonds = np.asarray(bond_connectivity, dtype=np.int64).reshape(-1, 2)
    blocks = bonds // int(n_nodes_per_block)
    n_blocks = int(blocks.max()) + 1 if blocks.size else 0
    w = np.asarray(weights, dtype=float)
    if w.shape[-1:] != (len(target_blocks_list),) or w.ndim not in (1, 2):
        raise ValueError(f"weights must be ({len(target_blocks_list)},) or (batch, {len(target_blocks_list)}), got {w.shape}")
    out = np.zeros(w.shape[:-1] + (len(bonds),))
    for i, tb in enumerate(target_blocks_list):
        tb = np.asarray(tb, dtype=np.int64).reshape(-1)
        if tb.size and (tb.min() < 0 or tb.max() >= n_blocks):
            raise ValueError(f"target {i}: block out of range [0, {n_blocks})")
        inside = np.isin(blocks, tb)
        member = inside.all(1) if ends == "both" else inside.any(1)
        out[..., member] += w[..., i:i + 1]
    return out


def host_strain_value(spec, fields, centroid_node_vectors, bond_connectivity, reference_bond_vectors, k_stretch, k_shear, k_rot):
    """NumPy value of the three ligament parts of a ``StrainObjectiveSpec`` for nonlinear ligaments, from the strains of
    ``energy.compute_ligament_strains_history`` as ``compute_response_data`` forms them: 1/2 k (strain |l0|)^2 for the axial and shear
    strain, 1/2 k_rot (theta_2 - theta_1)^2.  ``fields`` (batch, T, 2, n_blocks, 3) or (T, 2, n_blocks, 3); ``centroid_node_vectors`` with
    or without the member axis; stiffnesses scalars or (n_bonds,).  The contact part has no host formula here: ``parts[3]`` must be 0.
    Returns (batch,) or a float."""
    from .energy import compute_ligament_strains_history
    f = np.asarray(fields, dtype=float)
    single = f.ndim == 4
    if single:
        f = f[None]
    B, T = f.shape[:2]
    c = np.asarray(spec.parts, dtype=float)
    if c.shape != (4,):
        raise ValueError(f"parts must be (c_stretch, c_shear, c_bend, c_contact), got {spec.parts!r}")
    if c[3] != 0.0:
        raise ValueError("host_strain_value: the contact part is evaluated on the device only (parts[3] must be 0)")
    refv = np.asarray(reference_bond_vectors, dtype=float)
    nbd = len(np.asarray(bond_connectivity))
    w = np.asarray(spec.bond_weights, dtype=float)
    if w.shape not in ((nbd,), (B, nbd)):
        raise ValueError(f"bond_weights must be ({nbd},) or ({B}, {nbd}), got {w.shape}")
    w = np.broadcast_to(w, (B, nbd))
    tau = np.ones(T) if spec.time_weights is None else np.asarray(spec.time_weights, dtype=float)
    if tau.shape != (T,):
        raise ValueError(f"time_weights must be ({T},), got {tau.shape}")
    cnv = np.asarray(centroid_node_vectors, dtype=float)
    cnv = np.broadcast_to(cnv, (B,) + cnv.shape[-3:])
    l0 = np.linalg.norm(np.broadcast_to(refv, (nbd, 2)), axis=-1)
    out = np.zeros(B)
    for m in range(B):
        axial, shear, bending = compute_ligament_strains_history(f[m, :, 0], cnv[m], bond_connectivity, refv)
        e = c[0] * 0.5 * k_stretch * (axial * l0) ** 2 + c[1] * 0.5 * k_shear * (shear * l0) ** 2 + c[2] * 0.5 * k_rot * bending ** 2
        out[m] = tau @ (e @ w[m])
    return float(out[0]) if single else out


# ---- peak ligament strain on the device-resident history ------------------------------------------------------------------------------
PEAK_AGGREGATES = ("ks", "pnorm")          # DFX_PEAK_KS, DFX_PEAK_PNORM


class PeakStrainSpec:
    """A smooth maximum over output times and ligaments of a squared strain measure (``include/dfx.h``:
    ``dfx_strain_peak_value[_and_grad]``):

        q_mkb = a_mb (l0 eps)^2 + s_mb (l0 gamma)^2 + r_mb kappa^2        W_mkb = tau_k omega_mb
        "ks"     J_m = q_hat_m + log( sum W exp(beta (q - q_hat_m)) ) / beta        (sharpness = beta > 0)
        "pnorm"  J_m = q_hat_m ( sum W (q / q_hat_m)^p )^(1/p)                      (sharpness = p >= 1)

    with q_hat the hard maximum over the pairs with W > 0.  ``bond_coef`` (n_bonds, 3) or (batch, n_bonds, 3): (a, s, r) per ligament, in
    the order of the problem's bond list (``strain_limit_coefficients`` turns strain limits into them: q is then the squared utilisation
    and J <= 1 a strain limit); ``bond_weights`` omega (n_bonds,), (batch, n_bonds) or None = ones; ``time_weights`` tau (T,) or None = ones.
    Coefficients and weights are non-negative and finite; a zero weight excludes the pair.  The coefficients are CONSTANTS of the spec: the
    ``reference_vector`` gradient of J does not see how a helper derived them from l0.  Shapes, signs and finiteness are checked here
    (``ValueError``); lengths against a solve are checked where the spec is used."""
    __slots__ = ("bond_coef", "bond_weights", "time_weights", "aggregate", "sharpness")

    def __init__(self, bond_coef, bond_weights=None, time_weights=None, aggregate="ks", sharpness=20.0):
        c = np.array(bond_coef, dtype=float)
        if c.ndim not in (2, 3) or c.shape[-1] != 3 or c.shape[-2] == 0:
            raise ValueError(f"bond_coef must be (n_bonds, 3) or (batch, n_bonds, 3), got {c.shape}")
        if not np.isfinite(c).all() or (c < 0).any():
            raise ValueError("bond_coef must be finite and non-negative")
        w = None
        if bond_weights is not None:
            w = np.array(bond_weights, dtype=float)
            if w.ndim not in (1, 2) or w.shape[-1] != c.shape[-2]:
                raise ValueError(f"bond_weights must be ({c.shape[-2]},) or (batch, {c.shape[-2]}), got {w.shape}")
            if not np.isfinite(w).all() or (w < 0).any():
                raise ValueError("bond_weights must be finite and non-negative")
            if not (w > 0).any(-1).all():
                raise ValueError("bond_weights: all weights are zero for some member")
        tau = None
        if time_weights is not None:
            tau = np.array(time_weights, dtype=float)
            if tau.ndim != 1:
                raise ValueError(f"time_weights must be (T,), got {tau.shape}")
            if not np.isfinite(tau).all() or (tau < 0).any():
                raise ValueError("time_weights must be finite and non-negative")
            if not (tau > 0).any():
                raise ValueError("time_weights: all weights are zero")
        if aggregate not in PEAK_AGGREGATES:
            raise ValueError(f"aggregate must be one of {PEAK_AGGREGATES}, got {aggregate!r}")
        s = float(sharpness)
        if not np.isfinite(s) or (aggregate == "ks" and not s > 0.0) or (aggregate == "pnorm" and not s >= 1.0):
            raise ValueError(f"sharpness must be finite, beta > 0 for 'ks' and p >= 1 for 'pnorm', got {sharpness!r}")
        self.bond_coef, self.bond_weights, self.time_weights, self.aggregate, self.sharpness = c, w, tau, aggregate, s

    def __repr__(self):
        return (f"PeakStrainSpec(bond_coef={self.bond_coef.shape}, bond_weights={None if self.bond_weights is None else self.bond_weights.shape}, "
                f"time_weights={self.time_weights!r}, aggregate={self.aggregate!r}, sharpness={self.sharpness})")

    def engine_call(self):
        return "strain_peak", None, (self.bond_coef, self.bond_weights, self.time_weights, self.aggregate, self.sharpness), {}


def strain_limit_coefficients(reference_bond_vectors, eps_lim=None, gamma_lim=None, kappa_lim=None):
    """(n_bonds, 3) coefficients (a, s, r) = (1 / (l0 eps_lim)^2, 1 / (l0 gamma_lim)^2, 1 / kappa_lim^2) of a ``PeakStrainSpec`` from strain
    limits: q is then the squared utilisation of a ligament.  ``reference_bond_vectors`` (n_bonds, 2), l0 its row norms; every limit a
    positive scalar or (n_bonds,); a limit of None or inf gives coefficient 0 (that part is not limited)."""
    refv = np.asarray(reference_bond_vectors, dtype=float)
    if refv.ndim != 2 or refv.shape[1] != 2:
        raise ValueError(f"reference_bond_vectors must be (n_bonds, 2), got {refv.shape}")
    l0 = np.linalg.norm(refv, axis=-1)
    out = np.zeros((len(refv), 3))
    for i, (lim, scale) in enumerate(((eps_lim, l0), (gamma_lim, l0), (kappa_lim, np.ones_like(l0)))):
        if lim is None:
            continue
        lim = np.broadcast_to(np.asarray(lim, dtype=float), l0.shape)
        if np.isnan(lim).any() or (lim <= 0).any():
            raise ValueError("strain limits must be positive (None or inf: no limit)")
        out[:, i] = np.where(np.isinf(lim), 0.0, 1.0 / (scale * np.where(np.isinf(lim), 1.0, lim)) ** 2)
    return out


def host_strain_measure(bond_coef, fields, centroid_node_vectors, bond_connectivity, reference_bond_vectors, model="nonlinear"):
    """NumPy restatement of the squared strain measure q of a ``PeakStrainSpec`` for the ligament models (``model`` = "nonlinear" or
    "linearized"), from the strains of ``energy.ligament_strains[_linearized]``:  q = a (eps l0)^2 + s (gamma l0)^2 + r kappa^2.  ``fields``
    (batch, T, 2, n_blocks, 3) -> (batch, T, n_bonds), or (T, 2, n_blocks, 3) -> (T, n_bonds); ``bond_coef`` and ``centroid_node_vectors``
    with or without the member axis."""
    from .energy import block_to_node_kinematics, ligament_strains, ligament_strains_linearized
    strains = {"nonlinear": ligament_strains, "linearized": ligament_strains_linearized}.get(model)
    if strains is None:
        raise ValueError(f"host_strain_measure: model must be 'nonlinear' or 'linearized', got {model!r}")
    f = np.asarray(fields, dtype=float)
    single = f.ndim == 4
    if single:
        f = f[None]
    B, T = f.shape[:2]
    bonds = np.asarray(bond_connectivity)
    nbd = len(bonds)
    coef = np.asarray(bond_coef, dtype=float)
    if coef.shape not in ((nbd, 3), (B, nbd, 3)):
        raise ValueError(f"bond_coef must be ({nbd}, 3) or ({B}, {nbd}, 3), got {coef.shape}")
    coef = np.broadcast_to(coef, (B, nbd, 3))
    cnv = np.asarray(centroid_node_vectors, dtype=float)
    cnv = np.broadcast_to(cnv, (B,) + cnv.shape[-3:])
    refv = np.broadcast_to(np.asarray(reference_bond_vectors, dtype=float), (nbd, 2))
    l0 = np.linalg.norm(refv, axis=-1)
    q = np.zeros((B, T, nbd))
    for m in range(B):
        for k in range(T):
            nd = block_to_node_kinematics(f[m, k, 0], cnv[m]).reshape(-1, 3)
            axial, shear, bend = strains(nd[bonds[:, 0]], nd[bonds[:, 1]], reference_vector=refv)
            q[m, k] = coef[m, :, 0] * (axial * l0) ** 2 + coef[m, :, 1] * (shear * l0) ** 2 + coef[m, :, 2] * bend ** 2
    return q[0] if single else q


def peak_of_measure(spec, q):
    """(J, peak, peak_at) of a ``PeakStrainSpec`` from the measure ``q`` (batch, T, n_bonds): the formulas of the class in NumPy.  peak_at =
    (output, bond) of the hard maximum over the pairs with W > 0; on ties the lowest output, then the lowest bond."""
    q = np.asarray(q, dtype=float)
    B, T, nbd = q.shape
    w = np.ones(nbd) if spec.bond_weights is None else np.asarray(spec.bond_weights, dtype=float)
    if w.shape not in ((nbd,), (B, nbd)):
        raise ValueError(f"bond_weights must be ({nbd},) or ({B}, {nbd}), got {w.shape}")
    w = np.broadcast_to(w, (B, nbd))
    tau = np.ones(T) if spec.time_weights is None else np.asarray(spec.time_weights, dtype=float)
    if tau.shape != (T,):
        raise ValueError(f"time_weights must be ({T},), got {tau.shape}")
    J, peak, at = np.zeros(B), np.zeros(B), np.zeros((B, 2), dtype=np.int32)
    for m in range(B):
        W = tau[:, None] * w[m][None, :]
        on = W > 0
        if not on.any():
            raise ValueError(f"all weights are zero for member {m}")
        flat = int(np.argmax(np.where(on, q[m], -np.inf)))          # row-major: the lowest output, then the lowest bond
        qh = q[m].reshape(-1)[flat]
        peak[m], at[m] = qh, (flat // nbd, flat % nbd)
        if spec.aggregate == "ks":
            J[m] = qh + np.log(np.sum(W[on] * np.exp(spec.sharpness * (q[m][on] - qh)))) / spec.sharpness
        else:
            J[m] = qh * np.sum(W[on] * (q[m][on] / qh) ** spec.sharpness) ** (1.0 / spec.sharpness) if qh > 0 else 0.0
    return J, peak, at


def host_peak_strain_value(spec, fields, centroid_node_vectors, bond_connectivity, reference_bond_vectors, model="nonlinear"):
    """NumPy restatement of a ``PeakStrainSpec`` beside ``host_strain_value``, for the ligament models (``model`` = "nonlinear" or
    "linearized"): (J, peak, peak_at) with the member axis of ``fields`` ((batch, T, 2, n_blocks, 3) -> (batch,), (batch,), (batch, 2); (T, 2,
    n_blocks, 3) -> float, float, (2,)).  ``host_strain_measure`` gives q, ``peak_of_measure`` the reduction."""
    single = np.asarray(fields).ndim == 4
    q = host_strain_measure(spec.bond_coef, fields, centroid_node_vectors, bond_connectivity, reference_bond_vectors, model)
    J, peak, at = peak_of_measure(spec, q[None] if single else q)
    if single:
        return float(J[0]), float(peak[0]), at[0]
    return J, peak, at


# ---- signal misfit on the device-resident history -------------------------------------------------------------------------------------
DISPLACEMENT, VELOCITY, FORCE = 0, 3, 6          # first component of each kind: + 0, 1, 2 for x, y, theta
HINGE = 9                                        # first hinge component: + 3 * node + (0, 1, 2 for x, y, theta)
MAX_NODES_PER_BLOCK = 4


def hinge_component(node, dof):
    """The component of the force that ONE hinge carries: 9 + 3 node + dof, the part dE_h/d(x, y, theta) that the ligament on ``node``
    of a block (with its two void-angle penalties on a lattice with the angle contact) contributes to the block's components 6..8."""
    if int(node) != node or int(dof) != dof or not 0 <= node < MAX_NODES_PER_BLOCK or not 0 <= dof <= 2:
        raise ValueError(f"hinge_component: node must be in 0..{MAX_NODES_PER_BLOCK - 1} and dof in 0..2, got ({node!r}, {dof!r})")
    return HINGE + 3 * int(node) + int(dof)


def bonds_across(bond_connectivity, n_nodes_per_block, blocks_inside):
    """The hinges that cross the boundary of a region, seen from inside: the (block, node) pairs, in ascending order, of the bond ends that
    sit on a block of ``blocks_inside`` while the bond's other end sits on a block outside it.  ``bond_connectivity`` (n_bonds, 2) node
    ids, node n on block n // n_nodes_per_block -- the arguments of ``bond_weights_from_blocks``.  The sum of these hinges' force
    components is the force the region's surroundings transmit into it through the ligaments (``SignalSpec.cut_force``)."""
    npb = int(n_nodes_per_block)
    bonds = np.asarray(bond_connectivity, dtype=np.int64).reshape(-1, 2)
    inside = np.unique(np.asarray(blocks_inside, dtype=np.int64).reshape(-1))
    if inside.size == 0 or inside.min() < 0:
        raise ValueError("blocks_inside must be a non-empty sequence of block numbers >= 0")
    blocks = bonds // npb
    isin = np.isin(blocks, inside)
    out = [(int(blocks[i, e]), int(bonds[i, e] % npb)) for i in range(len(bonds)) for e in (0, 1) if isin[i, e] and not isin[i, 1 - e]]
    return sorted(out)


class SignalSpec:
    """A least-squares misfit between target histories and signals that are linear combinations of displacement, velocity and elastic-force
    components of blocks (``include/dfx.h``: ``dfx_signal_values``, ``dfx_signal_misfit_value[_and_grad]``):

        S_mks = sum over the terms of signal s: coef * channel(block, component; fields_mk, params_m)
        J_m   = 1/2 sum_k tau_k sum_s omega_s (S_mks - Starget_mks)^2

    ``terms``: a sequence of (signal, block, component, coef); component 0..2 displacement x, y, theta, 3..5 velocity, 6..8 the elastic force
    dE/d(x, y, theta) on the block, 9 + 3 node + dof (``hinge_component``) the part of that force that the ligament on one node of the block
    carries -- same sign and units, so the force the hinge exerts on the block is minus the channel, and a block's hinge channels add up to its
    components 6..8 -- accepted with ``hinge_channels=True`` only (the constructors ``hinge_force`` and ``cut_force`` set it; without it
    component 9 and above are out of range, as before these channels existed, and the engine refuses them likewise); a signal adds its
    terms in list order.  ``targets`` (T, n_signals) shared or (batch, T, n_signals), or
    None for a spec that only evaluates signals; ``omega`` (n_signals,) or None = ones; ``tau`` (T,) or None = ones.  Shapes are checked here
    (``ValueError``); block numbers and lengths against a solve are checked where the spec is used."""
    __slots__ = ("terms", "n_signals", "targets", "omega", "tau", "hinge_channels")

    def __init__(self, terms, n_signals=None, targets=None, omega=None, tau=None, hinge_channels=False):
        t = np.array(terms, dtype=float)
        if t.ndim != 2 or t.shape[1] != 4 or len(t) == 0:
            raise ValueError(f"terms must be a non-empty sequence of (signal, block, component, coef), got shape {t.shape}")
        if not np.isfinite(t).all() or (t[:, :3] != np.round(t[:, :3])).any():
            raise ValueError("terms: signal, block and component must be integers and every coefficient finite")
        top = HINGE + 3 * MAX_NODES_PER_BLOCK - 1 if hinge_channels else HINGE - 1
        if (t[:, :3] < 0).any() or (t[:, 2] > top).any():
            raise ValueError(f"terms: signal and block must be >= 0 and component in 0..{top} (0..2 displacement, 3..5 velocity, 6..8 force" +
                             (", 9 + 3 node + dof hinge force)" if hinge_channels else "; 9 + 3 node + dof hinge force with hinge_channels=True)"))
        ns = int(t[:, 0].max()) + 1 if n_signals is None else int(n_signals)
        if ns <= 0 or t[:, 0].max() >= ns:
            raise ValueError(f"terms name signal {int(t[:, 0].max())} but n_signals = {ns}")
        empty = sorted(set(range(ns)) - set(int(x) for x in t[:, 0]))
        if empty:
            raise ValueError(f"signals without terms: {empty}")
        tg = None
        if targets is not None:
            tg = np.array(targets, dtype=float)
            if tg.ndim not in (2, 3) or tg.shape[-1] != ns:
                raise ValueError(f"targets must be (T, {ns}) or (batch, T, {ns}), got {tg.shape}")
        om = None
        if omega is not None:
            om = np.array(omega, dtype=float)
            if om.shape != (ns,):
                raise ValueError(f"omega must be ({ns},), got {om.shape}")
        ta = None
        if tau is not None:
            ta = np.array(tau, dtype=float)
            if ta.ndim != 1 or (tg is not None and ta.shape[0] != tg.shape[-2]):
                raise ValueError(f"tau must be (T,){'' if tg is None else f' with T = {tg.shape[-2]}'}, got {ta.shape}")
        self.terms = [(int(a), int(b), int(c), float(d)) for a, b, c, d in t]
        self.n_signals, self.targets, self.omega, self.tau, self.hinge_channels = ns, tg, om, ta, bool(hinge_channels)

    def __repr__(self):
        return (f"SignalSpec({len(self.terms)} terms, n_signals={self.n_signals}, targets={None if self.targets is None else self.targets.shape}, "
                f"omega={self.omega!r}, tau={self.tau!r})")

    def engine_call(self):
        return "signal_misfit", self, (self.targets, self.omega, self.tau), {}

    @property
    def has_force(self):
        """a block-force or hinge-force term: evaluated on the device only"""
        return any(c >= FORCE for _, _, c, _ in self.terms)

    @classmethod
    def fields_of(cls, block_dofs, kind="displacement", targets=None, omega=None, tau=None):
        """One signal per (block, dof) of the displacement (``kind="displacement"``) or velocity (``"velocity"``) history: tracked block
        motions.  ``block_dofs``: a sequence of (block, dof), dof 0, 1, 2 = x, y, theta."""
        if kind not in ("displacement", "velocity"):
            raise ValueError(f"kind must be 'displacement' or 'velocity', got {kind!r}")
        base = DISPLACEMENT if kind == "displacement" else VELOCITY
        bd = np.array(block_dofs, dtype=np.int64).reshape(-1, 2)
        if len(bd) == 0 or (bd[:, 1] < 0).any() or (bd[:, 1] > 2).any():
            raise ValueError("block_dofs must be a non-empty sequence of (block, dof) with dof in 0..2")
        return cls([(s, int(b), base + int(d), 1.0) for s, (b, d) in enumerate(bd)], len(bd), targets, omega, tau)

    @classmethod
    def force_sum(cls, block_dofs, scale=1.0, targets=None, omega=None, tau=None):
        """ONE signal: ``scale`` times the sum of the elastic force on the listed (block, dof) pairs -- the reaction force on a set of driven
        DOFs (``hinge_characterization.py``: force_multiplier * sum of the reaction on the driven DOFs)."""
        bd = np.array(block_dofs, dtype=np.int64).reshape(-1, 2)
        if len(bd) == 0 or (bd[:, 1] < 0).any() or (bd[:, 1] > 2).any():
            raise ValueError("block_dofs must be a non-empty sequence of (block, dof) with dof in 0..2")
        return cls([(0, int(b), FORCE + int(d), float(scale)) for b, d in bd], 1, targets, omega, tau)

    @classmethod
    def hinge_force(cls, block_node_dofs, targets=None, omega=None, tau=None):
        """One signal per (block, node, dof): the force component dof (0, 1, 2 = x, y, moment) that the hinge on ``node`` of ``block``
        carries -- a ligament against a load cell or a strain gauge."""
        bnd = np.array(block_node_dofs, dtype=np.int64).reshape(-1, 3)
        if len(bnd) == 0 or (bnd[:, 0] < 0).any():
            raise ValueError("block_node_dofs must be a non-empty sequence of (block, node, dof) with block >= 0")
        return cls([(s, int(b), hinge_component(n, d), 1.0) for s, (b, n, d) in enumerate(bnd)], len(bnd), targets, omega, tau, True)

    @classmethod
    def cut_force(cls, hinges, dofs=(0, 1), scale=1.0, targets=None, omega=None, tau=None):
        """One signal per dof of ``dofs``: ``scale`` times the sum of that force component over ``hinges``, a sequence of (block, node) --
        the resultant through a line of hinges (``bonds_across``: the force transmitted into a region)."""
        hg = np.array(hinges, dtype=np.int64).reshape(-1, 2)
        dofs = [int(d) for d in np.atleast_1d(dofs)]
        if len(hg) == 0 or (hg[:, 0] < 0).any() or not dofs or len(set(dofs)) != len(dofs):
            raise ValueError("hinges must be a non-empty sequence of (block, node) with block >= 0 and dofs a non-empty sequence of distinct dofs")
        return cls([(s, int(b), hinge_component(n, d), float(scale)) for s, d in enumerate(dofs) for b, n in hg], len(dofs), targets, omega, tau, True)

    def with_targets(self, targets, omega=None, tau=None):
        """The same terms against other targets and weights."""
        return SignalSpec(self.terms, self.n_signals, targets, omega, tau, self.hinge_channels)


def host_signal_values(spec, fields):
    """NumPy restatement of the signals of a ``SignalSpec`` whose terms are field components (displacement, velocity): ``fields``
    (batch, T, 2, n_blocks, 3) -> (batch, T, n_signals), or (T, 2, n_blocks, 3) -> (T, n_signals).  Force and hinge-force components have
    no host path (``ValueError``): they are evaluated on the device, that is the point of ``DynamicSolver.signal_values``."""
    f = np.asarray(fields, dtype=float)
    if f.ndim not in (4, 5) or f.shape[-3] != 2 or f.shape[-1] != 3:
        raise ValueError(f"fields must be (batch, T, 2, n_blocks, 3) or (T, 2, n_blocks, 3), got {f.shape}")
    if spec.has_force:
        raise ValueError("host_signal_values: force and hinge-force components are evaluated on the device only (DynamicSolver.signal_values)")
    out = np.zeros(f.shape[:-3] + (spec.n_signals,))
    for s, b, c, coef in spec.terms:
        if b >= f.shape[-2]:
            raise ValueError(f"block {b} out of range [0, {f.shape[-2]})")
        out[..., s] += coef * f[..., c // 3, b, c % 3]
    return out


# ---- signal projections on the device-resident history --------------------------------------------------------------------------------
class ProjectionSpec:
    """The signals of a ``SignalSpec`` projected on the rows of a time basis, and a weighted quadratic form of the coefficients
    (``include/dfx.h``: ``dfx_signal_projections``, ``dfx_signal_projection_value[_and_grad]``):

        P_msj = sum_k B_jk S_mks
        J_m   = 1/2 sum_s sum_j W_sj (P_msj - Ptarget_msj)^2

    ``signal_spec``: the terms (its own targets, omega and tau play no part; targets, when present, fix T); ``basis`` (n_rows, T), shared by
    the members -- quadrature weights and windows are baked into the rows (``fourier_basis``); ``row_weights`` (n_signals, n_rows), any
    sign; ``targets`` (n_signals, n_rows) shared or (batch, n_signals, n_rows), None = zeros.  Band power at f: a cos and a sin row with
    equal weights; a matched filter: one row holding the shifted template.  Shapes and finiteness are checked here (``ValueError``);
    T against a solve where the spec is used."""
    __slots__ = ("signal_spec", "basis", "row_weights", "targets")

    def __init__(self, signal_spec, basis, row_weights, targets=None):
        ns = signal_spec.n_signals
        b = np.array(basis, dtype=float)
        if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1:
            raise ValueError(f"basis must be (n_rows, T) with n_rows >= 1, got {b.shape}")
        if signal_spec.targets is not None and signal_spec.targets.shape[-2] != b.shape[1]:
            raise ValueError(f"basis has T = {b.shape[1]} but the targets of the signal spec have T = {signal_spec.targets.shape[-2]}")
        if signal_spec.tau is not None and signal_spec.tau.shape[0] != b.shape[1]:
            raise ValueError(f"basis has T = {b.shape[1]} but tau of the signal spec has T = {signal_spec.tau.shape[0]}")
        w = np.array(row_weights, dtype=float)
        if w.shape != (ns, b.shape[0]):
            raise ValueError(f"row_weights must be ({ns}, {b.shape[0]}), got {w.shape}")
        tg = None
        if targets is not None:
            tg = np.array(targets, dtype=float)
            if tg.ndim not in (2, 3) or tg.shape[-2:] != (ns, b.shape[0]):
                raise ValueError(f"targets must be ({ns}, {b.shape[0]}) or (batch, {ns}, {b.shape[0]}), got {tg.shape}")
        for name, a in (("basis", b), ("row_weights", w), ("targets", tg)):
            if a is not None and not np.isfinite(a).all():
                raise ValueError(f"{name}: non-finite entry")
        self.signal_spec, self.basis, self.row_weights, self.targets = signal_spec, b, w, tg

    def __repr__(self):
        return (f"ProjectionSpec({self.signal_spec!r}, basis={self.basis.shape}, row_weights={self.row_weights.shape}, "
                f"targets={None if self.targets is None else self.targets.shape})")

    def engine_call(self):
        return "signal_projection", self.signal_spec, (self.basis, self.row_weights, self.targets), {}

    @property
    def n_rows(self):
        return self.basis.shape[0]

    def with_targets(self, targets):
        """The same signals, basis and weights against other targets."""
        return ProjectionSpec(self.signal_spec, self.basis, self.row_weights, targets)


def fourier_basis(timepoints, frequencies, window=None, quadrature="trapezoid"):
    """(2 * len(frequencies), T) rows of a ``ProjectionSpec`` basis: per frequency f the row q_k w_k cos(2 pi f t_k), then the row
    q_k w_k sin(2 pi f t_k), so that P_cos - i P_sin approximates the integral of s(t) w(t) exp(-2 pi i f t) dt over the output times.
    ``quadrature``: "trapezoid" weights of the (possibly non-uniform) grid, or "rectangle" = t_{k+1} - t_k with the last spacing repeated
    (on a uniform grid: dt times the discrete Fourier sum).  ``window``: None, "hann" (0.5 - 0.5 cos(2 pi (t - t_0) / (t_{T-1} - t_0)))
    or an explicit (T,) array."""
    t = np.asarray(timepoints, dtype=float)
    f = np.atleast_1d(np.asarray(frequencies, dtype=float))
    if t.ndim != 1 or len(t) < 2 or not np.isfinite(t).all() or (np.diff(t) <= 0).any():
        raise ValueError(f"timepoints must be (T,) with T >= 2, finite and increasing, got shape {t.shape}")
    if f.ndim != 1 or len(f) == 0 or not np.isfinite(f).all():
        raise ValueError(f"frequencies must be a non-empty sequence of finite numbers, got shape {f.shape}")
    dt = np.diff(t)
    if quadrature == "trapezoid":
        q = np.zeros_like(t)
        q[:-1] += 0.5 * dt
        q[1:] += 0.5 * dt
    elif quadrature == "rectangle":
        q = np.append(dt, dt[-1])
    else:
        raise ValueError(f"quadrature must be 'trapezoid' or 'rectangle', got {quadrature!r}")
    if window is None:
        w = np.ones_like(t)
    elif isinstance(window, str):
        if window != "hann":
            raise ValueError(f"window must be None, 'hann' or a (T,) array, got {window!r}")
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (t - t[0]) / (t[-1] - t[0]))
    else:
        w = np.asarray(window, dtype=float)
        if w.shape != t.shape or not np.isfinite(w).all():
            raise ValueError(f"window must be ({len(t)},) and finite, got shape {w.shape}")
    phase = 2.0 * np.pi * f[:, None] * t[None, :]
    out = np.empty((2 * len(f), len(t)))
    out[0::2] = q * w * np.cos(phase)
    out[1::2] = q * w * np.sin(phase)
    return out


def project_signals(spec, S):
    """The time reduction of a ``ProjectionSpec`` on signals that are already formed: ``S`` (..., T, n_signals) -> (..., n_signals,
    n_rows), ``P_sj = sum_k B_jk S_ks``.  It is linear, so the same call on the tangent columns of ``DynamicSolver.signal_jvp_multi``
    gives the tangents of the projections, ``P_dot = B S_dot``."""
    S = np.asarray(S, dtype=float)
    if S.ndim < 2 or S.shape[-2] != spec.basis.shape[1]:
        raise ValueError(f"basis has T = {spec.basis.shape[1]} but the signals have shape {S.shape} (..., T, n_signals)")
    return np.einsum("jk,...ks->...sj", spec.basis, S)


def host_projection_values(spec, fields):
    """NumPy restatement of the projections of a ``ProjectionSpec`` whose terms are field components: ``fields`` (batch, T, 2, n_blocks, 3)
    -> (batch, n_signals, n_rows), or (T, 2, n_blocks, 3) -> (n_signals, n_rows).  Force components raise, as in ``host_signal_values``."""
    S = host_signal_values(spec.signal_spec, fields)
    if S.shape[-2] != spec.basis.shape[1]:
        raise ValueError(f"basis has T = {spec.basis.shape[1]} but the fields have T = {S.shape[-2]}")
    return project_signals(spec, S)


def host_projection_value_and_cotangent(spec, fields):
    """(value, fields_bar) of a ``ProjectionSpec`` whose terms are field components: J = 1/2 sum W (P - Ptarget)^2 per member and its
    cotangent on the fields (what ``vjp`` / ``dfx_adjoint`` take), coef * c_ks on the row of every term with
    c_ks = sum_j W_sj (P_sj - Ptarget_sj) B_jk.  ``fields`` with or without the member axis; the value is (batch,) or a float."""
    f = np.asarray(fields, dtype=float)
    P = host_projection_values(spec, f)
    tg = 0.0 if spec.targets is None else spec.targets
    if f.ndim == 4 and np.ndim(tg) == 3:
        raise ValueError("per-member targets against the fields of one member")
    r = P - tg
    d = spec.row_weights * r
    value = 0.5 * np.sum(d * r, axis=(-2, -1))
    c = np.einsum("...sj,jk->...ks", d, spec.basis)
    fb = np.zeros_like(f)
    for s, b, comp, coef in spec.signal_spec.terms:
        fb[..., comp // 3, b, comp % 3] += coef * c[..., s]
    return (float(value) if f.ndim == 4 else value), fb


# ---- signal cross-correlation on the device-resident history ---------------------------------------------------------------------------
NORMALISATIONS = ("reference", "coefficient", "none")
REDUCTIONS = ("at", "max", "softmax")


class CorrelationSpec:
    """The normalised cross-correlation of pairs of signals of a ``SignalSpec`` over time lags, its peak and the delay of the peak
    (``include/dfx.h``: ``dfx_signal_xcorr``, ``dfx_signal_xcorr_value[_and_grad]``) -- ``compute_xcorr*`` / ``compute_space_time_xcorr``
    above as an objective, the pairs being the space rows at zero space shift:

        R[d]   = sum_p sum_k A_p[k] B_p[k + d]      d = -max_lag .. max_lag in output indices; d > 0: B lags A
        rho[d] = R[d] / N     N = sum A^2 ("reference"), sqrt(sum A^2 sum B^2) ("coefficient"), 1 ("none")
        J      = w_peak M + 1/2 w_delay (delta - delay_target)^2

    ``pairs``: a sequence of (a, b); a a signal index, b >= 0 a signal index, b < 0 column -1 - b of ``templates`` (T, n_templates) shared
    or (batch, T, n_templates).  ``reduce``: "at" (M = rho[lag], delta = lag), "max" (the maximum and its argmax; on ties the lowest lag)
    or "softmax" (M = log sum exp(beta rho) / beta, delta = sum d softmax(beta rho)_d; ``beta`` > 0).  A delay term (``w_delay`` != 0)
    needs "softmax".  ``signal_spec``: the terms (its own targets, omega and tau play no part).  Shapes, finiteness and these rules are
    checked here (``ValueError``); T against a solve where the spec is used."""
    __slots__ = ("signal_spec", "pairs", "max_lag", "templates", "normalisation", "reduce", "lag", "beta", "w_peak", "w_delay", "delay_target")

    def __init__(self, signal_spec, pairs, max_lag, templates=None, normalisation="reference", reduce="max", lag=None, beta=None, w_peak=1.0,
                 w_delay=0.0, delay_target=0.0):
        ns = signal_spec.n_signals
        p = np.array(pairs, dtype=float)
        if p.ndim != 2 or p.shape[1] != 2 or len(p) == 0:
            raise ValueError(f"pairs must be a non-empty sequence of (a, b), got shape {p.shape}")
        if not np.isfinite(p).all() or (p != np.round(p)).any():
            raise ValueError("pairs: a and b must be integers")
        p = p.astype(np.int64)
        if (p[:, 0] < 0).any() or (p >= ns).any():
            raise ValueError(f"pairs name a signal out of range [0, {ns})")
        tp = None
        if templates is not None:
            tp = np.array(templates, dtype=float)
            if tp.ndim not in (2, 3) or tp.shape[-1] < 1 or tp.shape[-2] < 1:
                raise ValueError(f"templates must be (T, n_templates) or (batch, T, n_templates), got {tp.shape}")
            if not np.isfinite(tp).all():
                raise ValueError("templates: non-finite entry")
        if (p[:, 1] < 0).any():
            if tp is None:
                raise ValueError("pairs name a template column but templates is None")
            if (-1 - p[:, 1]).max() >= tp.shape[-1]:
                raise ValueError(f"pairs name template column {int((-1 - p[:, 1]).max())} but templates has {tp.shape[-1]} columns")
        if int(max_lag) != max_lag or max_lag < 0:
            raise ValueError(f"max_lag must be a non-negative integer, got {max_lag!r}")
        T = tp.shape[-2] if tp is not None else (signal_spec.targets.shape[-2] if signal_spec.targets is not None else None)
        if T is not None and max_lag > T - 1:
            raise ValueError(f"max_lag = {max_lag} outside [0, T - 1] with T = {T}")
        if normalisation not in NORMALISATIONS:
            raise ValueError(f"normalisation must be one of {NORMALISATIONS}, got {normalisation!r}")
        if reduce not in REDUCTIONS:
            raise ValueError(f"reduce must be one of {REDUCTIONS}, got {reduce!r}")
        if reduce == "at":
            lag = 0 if lag is None else lag
            if int(lag) != lag or abs(lag) > max_lag:
                raise ValueError(f"lag must be an integer in [-{max_lag}, {max_lag}], got {lag!r}")
            lag = int(lag)
        if reduce == "softmax" and (beta is None or not np.isfinite(beta) or beta <= 0):
            raise ValueError(f"the softmax reduction needs a finite beta > 0, got {beta!r}")
        for name, v in (("w_peak", w_peak), ("w_delay", w_delay), ("delay_target", delay_target)):
            if not np.isfinite(v):
                raise ValueError(f"{name}: non-finite")
        if w_delay != 0 and reduce != "softmax":
            raise ValueError("w_delay != 0 needs reduce='softmax' (the delay of a maximum has no derivative)")
        self.signal_spec, self.pairs, self.max_lag, self.templates = signal_spec, [(int(a), int(b)) for a, b in p], int(max_lag), tp
        self.normalisation, self.reduce, self.lag, self.beta = normalisation, reduce, lag, None if beta is None else float(beta)
        self.w_peak, self.w_delay, self.delay_target = float(w_peak), float(w_delay), float(delay_target)

    def __repr__(self):
        return (f"CorrelationSpec({self.signal_spec!r}, {len(self.pairs)} pairs, max_lag={self.max_lag}, "
                f"templates={None if self.templates is None else self.templates.shape}, normalisation={self.normalisation!r}, "
                f"reduce={self.reduce!r}, lag={self.lag!r}, beta={self.beta!r}, w_peak={self.w_peak}, w_delay={self.w_delay}, "
                f"delay_target={self.delay_target})")

    def engine_call(self):
        return "signal_xcorr", self.signal_spec, (self.pairs, self.max_lag), dict(
            templates=self.templates, normalisation=self.normalisation, reduce=self.reduce, lag=self.lag, beta=self.beta, w_peak=self.w_peak,
            w_delay=self.w_delay, delay_target=self.delay_target)

    @property
    def n_lags(self):
        return 2 * self.max_lag + 1

    def with_templates(self, templates):
        """The same signals, pairs, lags and reduction against other templates."""
        return CorrelationSpec(self.signal_spec, self.pairs, self.max_lag, templates, self.normalisation, self.reduce, self.lag, self.beta,
                               self.w_peak, self.w_delay, self.delay_target)


def _xcorr_sides(spec, S):
    """A, B (..., n_pairs, T) of the pairs of a ``CorrelationSpec`` on signals ``S`` (..., T, n_signals)."""
    S = np.asarray(S, dtype=float)
    if S.ndim < 2 or S.shape[-1] != spec.signal_spec.n_signals:
        raise ValueError(f"the signals must be (..., T, {spec.signal_spec.n_signals}), got {S.shape}")
    T = S.shape[-2]
    if spec.max_lag > T - 1:
        raise ValueError(f"max_lag = {spec.max_lag} outside [0, T - 1] with T = {T}")
    tp = spec.templates
    if tp is not None:
        if tp.shape[-2] != T:
            raise ValueError(f"templates have T = {tp.shape[-2]} but the signals have T = {T}")
        if tp.ndim == 3 and (S.ndim < 3 or S.shape[-3] != tp.shape[0]):
            raise ValueError(f"per-member templates {tp.shape} against signals of shape {S.shape}")
        tp = np.broadcast_to(tp, S.shape[:-1] + tp.shape[-1:])
    A = np.stack([S[..., a] for a, _ in spec.pairs], axis=-2)
    B = np.stack([S[..., b] if b >= 0 else tp[..., -1 - b] for _, b in spec.pairs], axis=-2)
    return A, B


def _xcorr_norm(spec, A, B):
    EA, EB = np.sum(A * A, axis=(-2, -1)), np.sum(B * B, axis=(-2, -1))
    N = EA if spec.normalisation == "reference" else np.sqrt(EA * EB) if spec.normalisation == "coefficient" else np.ones_like(EA)
    return EA, EB, N


def xcorr_of_signals(spec, S):
    """The cross-correlation of a ``CorrelationSpec`` on signals that are already formed: ``S`` (..., T, n_signals) -> rho
    (..., 2 max_lag + 1), lag d at index d + max_lag.  A member whose normalisation N is 0 gets NaN."""
    A, B = _xcorr_sides(spec, S)
    T, D = A.shape[-1], spec.max_lag
    R = np.stack([np.sum(A[..., max(0, -d):T - max(0, d)] * B[..., max(0, d):T - max(0, -d)], axis=(-2, -1)) for d in range(-D, D + 1)], axis=-1)
    _, _, N = _xcorr_norm(spec, A, B)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(N[..., None] == 0, np.nan, R / N[..., None])


def xcorr_reduce(spec, rho):
    """(J, peak, delay, g) of the reduction of a ``CorrelationSpec`` on rho (..., 2 max_lag + 1): g = dJ / d rho."""
    rho = np.asarray(rho, dtype=float)
    D = spec.max_lag
    lags = np.arange(-D, D + 1, dtype=float)
    g = np.zeros_like(rho)
    if spec.reduce == "softmax":
        mx = rho.max(-1, keepdims=True)
        e = np.exp(spec.beta * (rho - mx))
        Z = e.sum(-1, keepdims=True)
        pi = e / Z
        M = (mx + np.log(Z) / spec.beta)[..., 0]
        delta = (pi * lags).sum(-1)
        g = spec.w_peak * pi + spec.w_delay * (delta - spec.delay_target)[..., None] * spec.beta * pi * (lags - delta[..., None])
    else:
        at = np.argmax(rho, axis=-1) if spec.reduce == "max" else np.full(rho.shape[:-1], spec.lag + D, dtype=np.int64)
        M = np.take_along_axis(rho, at[..., None], -1)[..., 0]
        delta = at.astype(float) - D
        np.put_along_axis(g, at[..., None], spec.w_peak, -1)
    J = spec.w_peak * M + 0.5 * spec.w_delay * (delta - spec.delay_target) ** 2
    return J, M, delta, g


def xcorr_value_and_signal_cotangent(spec, S):
    """(J, peak, delay, c) of a ``CorrelationSpec`` on signals ``S`` (..., T, n_signals): the value, the peak M, the delay delta and
    the cotangent c = dJ/dS, the formulas of ``include/dfx.h``.  A member whose N is 0 gets NaN values and c = 0."""
    A, B = _xcorr_sides(spec, S)
    T, D = A.shape[-1], spec.max_lag
    EA, EB, N = _xcorr_norm(spec, A, B)
    dead = N == 0
    Ns = np.where(dead, 1.0, N)
    rho = xcorr_of_signals(spec, S)
    J, M, delta, g = xcorr_reduce(spec, np.where(dead[..., None], 0.0, rho))
    Rbar = np.where(dead[..., None], 0.0, g / Ns[..., None])
    Nbar = np.where(dead, 0.0, -np.sum(g * np.where(dead[..., None], 0.0, rho), -1) / Ns)
    if spec.normalisation == "reference":
        eA, eB = Nbar, np.zeros_like(Nbar)
    elif spec.normalisation == "coefficient":
        eA, eB = Nbar * Ns / (2 * np.where(dead, 1.0, EA)), Nbar * Ns / (2 * np.where(dead, 1.0, EB))
    else:
        eA, eB = np.zeros_like(Nbar), np.zeros_like(Nbar)
    Abar, Bbar = 2 * eA[..., None, None] * A, 2 * eB[..., None, None] * B
    for i, d in enumerate(range(-D, D + 1)):
        ka, kb = slice(max(0, -d), T - max(0, d)), slice(max(0, d), T - max(0, -d))
        Abar[..., ka] += Rbar[..., i, None, None] * B[..., kb]
        Bbar[..., kb] += Rbar[..., i, None, None] * A[..., ka]
    c = np.zeros(np.shape(S), dtype=float)
    for p, (a, b) in enumerate(spec.pairs):
        c[..., a] += Abar[..., p, :]
        if b >= 0:
            c[..., b] += Bbar[..., p, :]
    nan = np.where(dead, np.nan, 0.0)
    return J + nan, M + nan, delta + nan, c


def host_xcorr_value_and_cotangent(spec, fields):
    """(J, peak, delay, fields_bar) of a ``CorrelationSpec`` whose terms are field components: the value, the peak and the delay per
    member and the cotangent of J on the fields (what ``vjp`` / ``dfx_adjoint`` take), coef * c_ks on the row of every term.  ``fields``
    with or without the member axis; the values are (batch,) or floats.  Force components raise, as in ``host_signal_values``."""
    f = np.asarray(fields, dtype=float)
    S = host_signal_values(spec.signal_spec, f)
    if f.ndim == 4 and spec.templates is not None and spec.templates.ndim == 3:
        raise ValueError("per-member templates against the fields of one member")
    J, M, delta, c = xcorr_value_and_signal_cotangent(spec, S)
    fb = np.zeros_like(f)
    for s, b, comp, coef in spec.signal_spec.terms:
        fb[..., comp // 3, b, comp % 3] += coef * c[..., s]
    if f.ndim == 4:
        return float(J), float(M), float(delta), fb
    return J, M, delta, fb


# ---- signal spectral ratios on the device-resident history ------------------------------------------------------------------------------
MEASURES = ("ratio", "log")
AGGREGATES = ("sum", "ks")


class SpectrumSpec:
    """Ratios of band powers of the projections of a ``ProjectionSpec``-like basis (``include/dfx.h``: ``dfx_signal_spectrum``,
    ``dfx_signal_spectrum_value[_and_grad]``) -- transmissibility, a band gap, harmonic generation.  G groups, per member:

        N_g = n0_g + sum_s sum_j Wn_gsj P_sj^2        D_g = d0_g + sum_s sum_j Wd_gsj P_sj^2        P_sj = sum_k B_jk S_ks
        l_g = N_g / D_g ("ratio")  or  ln N_g - ln D_g ("log"; dB = 10 / ln 10 * l)
        J   = sum_g a_g l_g ("sum")  or  M + ln(sum_g exp(beta (a_g l_g - M))) / beta with M = max_g a_g l_g ("ks", ``beta`` > 0)

    ``signal_spec``: the terms (its own targets, omega and tau play no part; targets, when present, fix T); ``basis`` (n_rows, T), shared
    by the members; ``num_weights``, ``den_weights`` (G, n_signals, n_rows), entries >= 0; ``num_offset``, ``den_offset`` (G,) shared or
    (batch, G), entries >= 0, None = zeros -- ``den_offset`` > 0 with zero ``den_weights`` normalises by a known constant; ``group_coef``
    (G,) of any sign, None = ones.  A group whose numerator is empty (no weight, zero offset) is refused.  A member with some D_g <= 0
    ("log": or N_g <= 0; "ks": or a non-finite l_g) gets J = NaN and a zero gradient.  Shapes, signs and finiteness are checked here
    (``ValueError``); T against a solve where the spec is used."""
    __slots__ = ("signal_spec", "basis", "num_weights", "den_weights", "num_offset", "den_offset", "group_coef", "measure", "aggregate", "beta")

    def __init__(self, signal_spec, basis, num_weights, den_weights, num_offset=None, den_offset=None, group_coef=None, measure="log",
                 aggregate="sum", beta=None):
        ns = signal_spec.n_signals
        b = np.array(basis, dtype=float)
        if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1:
            raise ValueError(f"basis must be (n_rows, T) with n_rows >= 1, got {b.shape}")
        if signal_spec.targets is not None and signal_spec.targets.shape[-2] != b.shape[1]:
            raise ValueError(f"basis has T = {b.shape[1]} but the targets of the signal spec have T = {signal_spec.targets.shape[-2]}")
        if signal_spec.tau is not None and signal_spec.tau.shape[0] != b.shape[1]:
            raise ValueError(f"basis has T = {b.shape[1]} but tau of the signal spec has T = {signal_spec.tau.shape[0]}")
        wn, wd = np.array(num_weights, dtype=float), np.array(den_weights, dtype=float)
        if wn.ndim != 3 or wn.shape[0] < 1 or wn.shape[1:] != (ns, b.shape[0]) or wd.shape != wn.shape:
            raise ValueError(f"num_weights and den_weights must be (G, {ns}, {b.shape[0]}) with G >= 1, got {wn.shape} and {wd.shape}")
        G = wn.shape[0]
        offs = []
        for name, o in (("num_offset", num_offset), ("den_offset", den_offset)):
            o = None if o is None else np.array(o, dtype=float)
            if o is not None and (o.ndim not in (1, 2) or o.shape[-1] != G):
                raise ValueError(f"{name} must be ({G},) or (batch, {G}), got {o.shape}")
            offs.append(o)
        if offs[0] is not None and offs[1] is not None and offs[0].ndim == 2 and offs[1].ndim == 2 and len(offs[0]) != len(offs[1]):
            raise ValueError(f"num_offset is for {len(offs[0])} members and den_offset for {len(offs[1])}")
        a = np.ones(G) if group_coef is None else np.array(group_coef, dtype=float)
        if a.shape != (G,):
            raise ValueError(f"group_coef must be ({G},), got {a.shape}")
        for name, v, nonneg in (("basis", b, False), ("num_weights", wn, True), ("den_weights", wd, True), ("num_offset", offs[0], True),
                                ("den_offset", offs[1], True), ("group_coef", a, False)):
            if v is not None and not np.isfinite(v).all():
                raise ValueError(f"{name}: non-finite entry")
            if v is not None and nonneg and (v < 0).any():
                raise ValueError(f"{name}: negative entry")
        n0 = np.zeros(G) if offs[0] is None else offs[0]
        empty = [g for g in range(G) if not (wn[g] > 0).any() and (np.atleast_2d(n0)[:, g] == 0).any()]
        if empty:
            raise ValueError(f"groups with an empty numerator (no weight and a zero offset): {empty}")
        if measure not in MEASURES:
            raise ValueError(f"measure must be one of {MEASURES}, got {measure!r}")
        if aggregate not in AGGREGATES:
            raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
        if aggregate == "ks" and (beta is None or not np.isfinite(beta) or beta <= 0):
            raise ValueError(f"the ks aggregate needs a finite beta > 0, got {beta!r}")
        self.signal_spec, self.basis, self.num_weights, self.den_weights = signal_spec, b, wn, wd
        self.num_offset, self.den_offset, self.group_coef = offs[0], offs[1], a
        self.measure, self.aggregate, self.beta = measure, aggregate, None if beta is None else float(beta)

    def __repr__(self):
        return (f"SpectrumSpec({self.signal_spec!r}, basis={self.basis.shape}, groups={self.n_groups}, measure={self.measure!r}, "
                f"aggregate={self.aggregate!r}, beta={self.beta!r})")

    def engine_call(self):
        return "signal_spectrum", self.signal_spec, (self.basis, self.num_weights, self.den_weights), dict(
            num_offset=self.num_offset, den_offset=self.den_offset, group_coef=self.group_coef, measure=self.measure,
            aggregate=self.aggregate, beta=self.beta)

    @property
    def n_rows(self):
        return self.basis.shape[0]

    @property
    def n_groups(self):
        return self.num_weights.shape[0]

    def with_offsets(self, num_offset, den_offset):
        """The same signals, basis, weights and reduction with other offsets."""
        return SpectrumSpec(self.signal_spec, self.basis, self.num_weights, self.den_weights, num_offset, den_offset, self.group_coef,
                            self.measure, self.aggregate, self.beta)


def band_groups(n_signals, n_frequencies, numerator, denominator):
    """(Wn, Wd), each (G, n_signals, 2 n_frequencies), of a ``SpectrumSpec`` on a ``fourier_basis``: group g has unit weight on the cos and
    the sin row (they weigh alike, as in ``TargetBandPower``) of every (signal, frequency index) of ``numerator[g]`` in Wn and of
    ``denominator[g]`` in Wd.  A pair listed twice in one list counts once; an empty denominator list leaves the row of Wd zero (normalise
    by ``den_offset``)."""
    ns, nf = int(n_signals), int(n_frequencies)
    if ns < 1 or nf < 1:
        raise ValueError(f"n_signals and n_frequencies must be positive, got {n_signals!r} and {n_frequencies!r}")
    if len(numerator) != len(denominator) or len(numerator) == 0:
        raise ValueError(f"numerator and denominator must list the same number (>= 1) of groups, got {len(numerator)} and {len(denominator)}")
    out = np.zeros((2, len(numerator), ns, 2 * nf))
    for side, groups in enumerate((numerator, denominator)):
        for g, pairs in enumerate(groups):
            for s, f in np.array(pairs, dtype=np.int64).reshape(-1, 2):
                if not (0 <= s < ns and 0 <= f < nf):
                    raise ValueError(f"group {g}: (signal, frequency) = ({s}, {f}) out of range ({ns} signals, {nf} frequencies)")
                out[side, g, s, 2 * f] = out[side, g, s, 2 * f + 1] = 1.0
    return out[0], out[1]


def _spectrum_offsets(spec, lead):
    """n0, d0 of a ``SpectrumSpec`` broadcast against projections whose leading axes are ``lead``"""
    G, out = spec.n_groups, []
    for o in (spec.num_offset, spec.den_offset):
        o = np.zeros(G) if o is None else o
        if o.ndim == 2 and (len(lead) == 0 or lead[-1] != len(o)):
            raise ValueError(f"per-member offsets for {len(o)} members against projections with leading axes {lead}")
        out.append(np.broadcast_to(o, lead + (G,)))
    return out


def spectrum_of_projections(spec, P):
    """(N, D, l) of a ``SpectrumSpec`` from projections ``P`` (..., n_signals, n_rows): the forms and the measures (..., G), the formulas
    of the class in NumPy.  A group with D <= 0 ("log": or N <= 0) gets l = NaN."""
    P = np.asarray(P, dtype=float)
    if P.shape[-2:] != spec.num_weights.shape[1:]:
        raise ValueError(f"the projections must be (..., {spec.num_weights.shape[1]}, {spec.num_weights.shape[2]}), got {P.shape}")
    n0, d0 = _spectrum_offsets(spec, P.shape[:-2])
    N = n0 + np.einsum("gsj,...sj->...g", spec.num_weights, P * P)
    D = d0 + np.einsum("gsj,...sj->...g", spec.den_weights, P * P)
    ok = (D > 0) & ((N > 0) | (spec.measure != "log"))
    Ns, Ds = np.where(ok, N, 1.0), np.where(ok, D, 1.0)
    l = np.where(ok, np.log(Ns) - np.log(Ds) if spec.measure == "log" else Ns / Ds, np.nan)
    return N, D, l


def spectrum_value_and_projection_cotangent(spec, P):
    """(J, l, Pbar) of a ``SpectrumSpec`` on projections ``P`` (..., n_signals, n_rows): the value (...), the measures (..., G) and
    dJ/dP = Weff P.  A member with a NaN measure ("ks": or a non-finite one) gets J = NaN and Pbar = 0."""
    P = np.asarray(P, dtype=float)
    N, D, l = spectrum_of_projections(spec, P)
    if spec.aggregate == "ks":
        l = np.where(np.isfinite(l), l, np.nan)
    dead = np.isnan(l).any(-1)
    ls = np.where(dead[..., None], 0.0, l)
    Ns, Ds = np.where(dead[..., None], 1.0, N), np.where(dead[..., None], 1.0, D)
    a = spec.group_coef
    if spec.aggregate == "ks":
        z = a * ls
        M = z.max(-1, keepdims=True)
        e = np.exp(spec.beta * (z - M))
        Z = e.sum(-1, keepdims=True)
        J = (M + np.log(Z) / spec.beta)[..., 0]
        lam = a * e / Z
    else:
        J = (a * ls).sum(-1)
        lam = np.broadcast_to(a, ls.shape)
    dN, dD = (1.0 / Ns, -1.0 / Ds) if spec.measure == "log" else (1.0 / Ds, -Ns / Ds ** 2)
    Weff = 2.0 * (np.einsum("...g,gsj->...sj", lam * dN, spec.num_weights) + np.einsum("...g,gsj->...sj", lam * dD, spec.den_weights))
    Weff = np.where(dead[..., None, None], 0.0, Weff)
    return np.where(dead, np.nan, J), l, Weff * P


def host_spectrum_value_and_cotangent(spec, fields):
    """(J, l, fields_bar) of a ``SpectrumSpec`` whose terms are field components: the value and the measures per member and the cotangent
    of J on the fields (what ``vjp`` / ``dfx_adjoint`` take), coef * c_ks on the row of every term with c_ks = sum_j Weff_sj P_sj B_jk.
    ``fields`` with or without the member axis; the value is (batch,) or a float.  Force components raise, as in ``host_signal_values``."""
    f = np.asarray(fields, dtype=float)
    S = host_signal_values(spec.signal_spec, f)
    if S.shape[-2] != spec.basis.shape[1]:
        raise ValueError(f"basis has T = {spec.basis.shape[1]} but the fields have T = {S.shape[-2]}")
    if f.ndim == 4 and any(o is not None and o.ndim == 2 for o in (spec.num_offset, spec.den_offset)):
        raise ValueError("per-member offsets against the fields of one member")
    P = np.einsum("jk,...ks->...sj", spec.basis, S)
    J, l, Pbar = spectrum_value_and_projection_cotangent(spec, P)
    c = np.einsum("...sj,jk->...ks", Pbar, spec.basis)
    fb = np.zeros_like(f)
    for s, b, comp, coef in spec.signal_spec.terms:
        fb[..., comp // 3, b, comp % 3] += coef * c[..., s]
    return (float(J) if f.ndim == 4 else J), l, fb
