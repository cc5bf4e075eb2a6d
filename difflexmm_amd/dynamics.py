"""``setup_dynamic_solver`` with the reference's signature (``difflexmm/dynamics.py:60-186``) on top of the HIP
engine.  The returned ``solve_dynamics(state0, timepoints, control_params)`` has the reference's shapes,
``(T, 2, n_blocks, 3)``, and additionally ``solve_dynamics.vjp(fields_bar)`` -- the counterpart of taking
``jax.grad`` through the reference solver -- returning a ``ControlParams``-shaped gradient tree.

Differences that are inherent to running inside hand-written kernels (all keyword-only, all with defaults):
  * by default the forward solve is the reference's own scheme: adaptive Dormand-Prince 5(4) controlled by ``rtol`` /
    ``atol`` with dense output at ``timepoints`` (jax.experimental.ode.odeint semantics, every member its own step).
    With ``steps_per_interval=k`` (an int, or one int per output interval) the same tableau runs on k equal steps
    between consecutive ``timepoints`` (``step_times=`` gives the step boundaries explicitly).  ``keep_trajectory=True`` (needed by ``vjp``: the reverse sweep is the exact
    discrete adjoint of a FIXED grid) without a grid first runs the adaptive controller and then freezes ITS grid: the
    step boundaries it accepted (for the member that needed the most steps) plus the output times, so the
    differentiated solve has the accuracy rtol / atol ask for;
  * ``energy_fn``, ``loading_fn`` and ``constrained_DOFs_fn`` must come from ``difflexmm_amd.energy`` /
    ``difflexmm_amd.loading`` (declarative specs), otherwise ``TypeError`` at setup;
  * ``batch=B`` integrates B members (list of B ``ControlParams``) side by side.
"""
import os
from typing import Optional

import numpy as np

from . import _binding as _b
from .energy import _EnergyFn
from .geometry import (DOFsInfo, compute_inertia, compute_inertia_jvp, compute_inertia_vjp, void_angles0, void_angles0_jvp,
                       void_angles0_vjp)
from .loading import as_time_function, zero
from .utils import (ContactParams, ControlParams, GeometricalParams, MechanicalParams, _frozen)


_FLAT_CACHE = {}      # id(centroid_node_vectors) -> (weakref, bonds, density, inertia, void_angle0)


def remember_flat(cnv, bonds, density, inertia, void_angle0):
    """What a solver derives from a design's node vectors, computed elsewhere (the native design map, problems.prefetch_designs): kept for
    ``DynamicSolver._flatten`` under the identity of the (read-only) array, like the entries it makes itself."""
    import weakref
    key = id(cnv)
    if len(_FLAT_CACHE) > 1024:
        _FLAT_CACHE.clear()
    _FLAT_CACHE[key] = (weakref.ref(cnv, lambda _r, k=key: _FLAT_CACHE.pop(k, None)), bonds, np.array(density, copy=True), inertia, void_angle0)


def _leaf_key(x):
    """What ``DynamicSolver._memo`` keeps of a ControlParams leaf to recognise it: a frozen array by identity, a Python / NumPy scalar by
    value, a tuple element by element, anything else (writeable arrays, 0-d arrays, lists) by a private copy of its content."""
    if isinstance(x, tuple):
        return ("t", tuple(_leaf_key(v) for v in x))
    if x is None:
        return ("n",)
    if isinstance(x, np.ndarray):
        return ("f", x) if _frozen(x) else ("c", np.array(x, copy=True))
    if isinstance(x, (int, float, np.generic)):
        return ("s", x)
    try:
        return ("c", np.array(x, copy=True))
    except (TypeError, ValueError):
        return ("x",)


def _leaf_unchanged(key, x):
    kind = key[0]
    if kind == "t":
        return isinstance(x, tuple) and len(x) == len(key[1]) and all(_leaf_unchanged(k, v) for k, v in zip(key[1], x))
    if kind == "n":
        return x is None
    if kind == "f":
        return key[1] is x
    if kind == "s":
        return isinstance(x, (int, float, np.generic)) and type(x) is type(key[1]) and x == key[1]
    if kind == "c":
        if x is None or isinstance(x, tuple):
            return False
        try:
            a = np.asarray(x)
        except (TypeError, ValueError):
            return False
        return a.shape == key[1].shape and a.dtype == key[1].dtype and np.array_equal(a, key[1])
    return False


def _bcast(x, n):
    return np.broadcast_to(np.asarray(x, dtype=float), (n,)).copy()


JACFWD_LEAVES = ("k_stretch", "k_shear", "k_rot", "density", "damping", "min_angle", "cutoff_angle", "k_contact")


def _sample_leaf(who, control_params, name):
    """``(name, j)``: sample j of the 1-D array ``name`` of ``constraint_params`` / ``loading_params`` (the values of a named
    ``loading.Table``).  Returns (field of ControlParams, key, j, length); ``ValueError`` on anything else."""
    if len(name) != 2 or not isinstance(name[0], str):
        raise ValueError(f"{who}: a sample of an array leaf is addressed as (name, j), got {name!r}")
    key, j = name
    in_con = key in (control_params.constraint_params or {})
    in_load = key in (control_params.loading_params or {})
    if in_con and in_load:
        raise ValueError(f"{who}: {key!r} is a key of both constraint_params and loading_params: seed it with jvp_multi")
    if not (in_con or in_load):
        raise ValueError(f"{who}: {key!r} is not a key of constraint_params / loading_params")
    field = "constraint_params" if in_con else "loading_params"
    arr = np.asarray(getattr(control_params, field)[key])
    if arr.ndim != 1:
        raise ValueError(f"{who}: {key!r} is not a 1-D array leaf (shape {arr.shape})")
    if not isinstance(j, (int, np.integer)) or not 0 <= int(j) < len(arr):
        raise ValueError(f"{who}: sample {j!r} of {key!r} is out of range (it has {len(arr)} samples)")
    return field, key, int(j), len(arr)


def unit_tangent(control_params: ControlParams, name):
    """The ``ControlParams``-shaped tangent tree that is 1 on the scalar leaf ``name`` and zero (None) elsewhere -- one column of
    :meth:`DynamicSolver.jacfwd`.  ``name``: one of ``JACFWD_LEAVES`` (stiffnesses of ``bond_params``, ``density`` / ``damping`` of
    ``mechanical_params``, the contact constants) or a key of ``constraint_params`` / ``loading_params``.  The leaf must be ONE number: a
    Python / 0-d scalar, or an array that holds one value broadcast over bonds or blocks -- that one gets an all-ones tangent of its
    shape.  ``ValueError``: an unknown name, a name both dicts hold, a leaf that is missing or holds different values."""
    mp = control_params.mechanical_params
    if isinstance(name, tuple):
        field, key, j, n = _sample_leaf("unit_tangent", control_params, name)
        e = np.zeros(n)
        e[j] = 1.0
        return ControlParams(GeometricalParams(None, None), MechanicalParams(None, None), **{field: {key: e}})

    def ones(leaf, where):
        if leaf is None:
            raise ValueError(f"unit_tangent: {where} is not set in these ControlParams")
        a = np.asarray(leaf, dtype=float)
        if a.ndim and (a.size == 0 or np.any(a != a.reshape(-1)[0])):
            raise ValueError(f"unit_tangent: {where} is not a scalar leaf (shape {a.shape}, different values): seed it with jvp_multi")
        return np.ones(a.shape) if a.ndim else 1.0
    geo0 = GeometricalParams(None, None)
    if name in ("k_stretch", "k_shear", "k_rot"):
        bp = mp.bond_params
        if not hasattr(bp, name):
            raise ValueError(f"unit_tangent: these bond parameters have no {name}")
        bd = type(bp)(**{f: (ones(getattr(bp, f), f"bond_params.{name}") if f == name else None) for f in bp._fields})
        return ControlParams(geo0, MechanicalParams(bd, None))
    if name in ("density", "damping"):
        return ControlParams(geo0, MechanicalParams(None, None)._replace(**{name: ones(getattr(mp, name), f"mechanical_params.{name}")}))
    if name in ("min_angle", "cutoff_angle", "k_contact"):
        c = mp.contact_params
        if c is None:
            raise ValueError(f"unit_tangent: {name}: these ControlParams have no contact_params")
        cd = ContactParams(**{f: (ones(getattr(c, f), f"contact_params.{name}") if f == name else None) for f in c._fields})
        return ControlParams(geo0, MechanicalParams(None, None, contact_params=cd))
    in_con = name in (control_params.constraint_params or {})
    in_load = name in (control_params.loading_params or {})
    if in_con and in_load:
        raise ValueError(f"unit_tangent: {name!r} is a key of both constraint_params and loading_params: seed it with jvp_multi")
    if in_con or in_load:
        src = control_params.constraint_params if in_con else control_params.loading_params
        if np.ndim(src[name]) != 0:
            raise ValueError(f"unit_tangent: {name!r} is not a scalar leaf (shape {np.shape(src[name])})")
        return ControlParams(geo0, MechanicalParams(None, None), **{"constraint_params" if in_con else "loading_params": {name: 1.0}})
    raise ValueError(f"unit_tangent: unknown leaf {name!r} (one of {', '.join(JACFWD_LEAVES)}, a key of constraint_params / loading_params, "
                     "or (key, j): sample j of an array held there)")


def with_leaf(control_params: ControlParams, name, value):
    """The setter beside :func:`unit_tangent`: a copy of ``control_params`` with the scalar leaf ``name`` set to ``value`` -- the same
    names (``JACFWD_LEAVES``, keys of ``constraint_params`` / ``loading_params``) and the same "scalar leaf" rule: a Python / 0-d scalar
    is replaced, an array that holds one value is filled with ``value`` in its shape.  ``ValueError``: what :func:`unit_tangent` raises."""
    if isinstance(name, tuple):
        field, key, j, _ = _sample_leaf("with_leaf", control_params, name)
        arr = np.array(getattr(control_params, field)[key], dtype=float)
        arr[j] = float(value)
        return control_params._replace(**{field: dict(getattr(control_params, field), **{key: arr})})
    shape = unit_tangent(control_params, name)          # (the checks; the tree itself tells where the leaf sits and its shape)
    value = float(value)
    mp = control_params.mechanical_params

    def filled(ones):
        return np.full(np.shape(ones), value) if np.ndim(ones) else value
    if name in ("k_stretch", "k_shear", "k_rot"):
        bp = mp.bond_params
        return control_params._replace(mechanical_params=mp._replace(bond_params=bp._replace(
            **{name: filled(getattr(shape.mechanical_params.bond_params, name))})))
    if name in ("density", "damping"):
        return control_params._replace(mechanical_params=mp._replace(**{name: filled(getattr(shape.mechanical_params, name))}))
    if name in ("min_angle", "cutoff_angle", "k_contact"):
        return control_params._replace(mechanical_params=mp._replace(contact_params=mp.contact_params._replace(
            **{name: filled(getattr(shape.mechanical_params.contact_params, name))})))
    field = "constraint_params" if name in (control_params.constraint_params or {}) else "loading_params"
    return control_params._replace(**{field: dict(getattr(control_params, field), **{name: value})})


class DynamicSolver:
    """Callable returned by :func:`setup_dynamic_solver`."""

    def __init__(self, geometry, energy_fn, loaded_block_DOF_pairs, loading_fn, constrained_block_DOF_pairs,
                 constrained_DOFs_fn, damped_blocks, rtol, atol, integrator, steps_per_interval, batch, device, lib, streams=0, grid_refine=1):
        if not isinstance(energy_fn, _EnergyFn) or energy_fn.spec.bond_model is None:
            raise TypeError("energy_fn must be built with difflexmm_amd.energy.build_strain_energy "
                            "(optionally combined with build_contact_energy)")
        self.geometry = geometry
        self.spec = energy_fn.spec
        self.n_blocks, self.n_npb = geometry.n_blocks, geometry.n_npb
        self.bonds = self.spec.bond_connectivity
        self.rtol, self.atol = rtol, atol
        self.steps_per_interval = steps_per_interval
        if int(grid_refine) < 1:
            raise ValueError("grid_refine must be >= 1")
        self.grid_refine = int(grid_refine)
        self.max_attempts = 10_000_000          # budget of the adaptive controller (attempted steps per member): jax's mxstep is unbounded
        self.batch = int(batch)
        self.damped_blocks = None if damped_blocks is None else np.asarray(damped_blocks, dtype=np.int64)
        self.constrained_pairs = np.asarray(constrained_block_DOF_pairs, dtype=np.int64).reshape(-1, 2)
        self.free_DOF_ids, self.constrained_DOF_ids, _ = DOFsInfo(self.n_blocks, self.constrained_pairs)
        self.constraint_fn = as_time_function(constrained_DOFs_fn, "constrained_DOFs_fn")
        if loaded_block_DOF_pairs is not None and loading_fn is not None:
            self.loaded_pairs = np.asarray(loaded_block_DOF_pairs, dtype=np.int64).reshape(-1, 2)
            self.loading_fn = as_time_function(loading_fn, "loading_fn")
        else:
            self.loaded_pairs = np.zeros((0, 2), dtype=np.int64)
            self.loading_fn = zero
        # time-function slots: constraint terms first, then loading terms
        self.con_terms, self.load_terms = self.constraint_fn.terms, self.loading_fn.terms
        n_fns = len(self.con_terms) + len(self.load_terms)
        if n_fns > _b.DFX_MAX_FNS:
            raise ValueError(f"at most {_b.DFX_MAX_FNS} time functions (constraint + loading terms) are supported")
        fn_types = [f.type_id for f in self.con_terms + self.load_terms]
        # blocks with constrained or loaded DOFs
        special = {}

        def entry(block):
            return special.setdefault(int(block), [0, np.zeros((3, _b.DFX_MAX_FNS)), np.zeros((3, _b.DFX_MAX_FNS))])

        n_con = len(self.constrained_pairs)
        for j, (blk, d) in enumerate(self.constrained_pairs):
            e = entry(blk)
            e[0] |= 1 << int(d)
            for f, term in enumerate(self.con_terms):
                e[1][d, f] = _bcast(term.vector, n_con)[j]
        n_load = len(self.loaded_pairs)
        for j, (blk, d) in enumerate(self.loaded_pairs):
            e = entry(blk)
            for f, term in enumerate(self.load_terms):
                e[2][d, len(self.con_terms) + f] = _bcast(term.vector, n_load)[j]
        self._special = [(blk, e[0], e[1], e[2]) for blk, e in sorted(special.items())]
        self.engine = _b.Engine(self.n_blocks, self.n_npb, self.bonds, self.spec.bond_model,
                                int(self.spec.contact or 0), self._special, fn_types,
                                batch=self.batch, tableau=integrator, device=device, lib=lib,
                                fn_tables=[getattr(f, "table", None) for f in self.con_terms + self.load_terms], streams=streams)
        # table drives whose samples are a leaf of the params dict (loading.Table with named values): (function slot, term, field of
        # ControlParams).  Their values go to the device with every prepare, and every reverse sweep of this solver keeps the
        # drive-cotangent trace that gives their gradient (dfx_fn_table_grads: stage launches, never the persistent loops)
        nc = len(self.con_terms)
        self._table_leaves = [(f, t, "constraint_params") for f, t in enumerate(self.con_terms) if getattr(t, "values_name", None)] + \
                             [(nc + f, t, "loading_params") for f, t in enumerate(self.load_terms) if getattr(t, "values_name", None)]
        if self._table_leaves:
            if not self.engine.has_fn_table_grads:
                raise NotImplementedError(f"loading.Table with named values: the library {getattr(self.engine.lib, '_name', self.engine.lib)!r} has no "
                                          "dfx_fn_table_grads (a stale libdfx.so, or the CPU port of the oracle; build the HIP engine)")
            self.engine.fn_table_grads(True)
        self._last = None
        self._memo_pass = None
        self.solve_count = 0          # forward solves run so far (what the engine's resident history belongs to)

    # -- ControlParams -> engine arrays -------------------------------------------------------------
    def _memo(self, name, source, build):
        """The flattened form of a ControlParams leaf that rarely changes between members and evaluations (stiffnesses, reference vectors,
        damping): rebuilt unless the leaf cannot have changed since (the same frozen array, the same scalar values) or still holds the
        content it had (an array that may have been written in place in between is compared against a private copy -- once per
        ``prepare`` for the members that share it)."""
        cache = self.__dict__.setdefault("_memo_cache", {})
        hit = cache.get(name)
        if hit is not None:
            key, arr, seen_in, seen = hit
            if (seen_in is not None and seen_in is self._memo_pass and seen is source) or _leaf_unchanged(key, source):
                cache[name] = (key, arr, self._memo_pass, source)
                return arr
        arr = build()
        arr.flags.writeable = False
        cache[name] = (_leaf_key(source), arr, self._memo_pass, source)
        return arr

    def _stack(self, flats):
        """The members' flattened arrays as batch-leading arrays in buffers this solver keeps: a row is copied only when its source is
        another object than last time (the static leaves above, and designs that did not change, cost nothing)."""
        bufs = self.__dict__.setdefault("_batch_bufs", {})
        out = {}
        for k in flats[0]:
            rows = [f[k] for f in flats]
            shape = (len(rows),) + np.shape(rows[0])
            buf = bufs.get(k)
            if buf is None or buf[0].shape != shape:
                buf = bufs[k] = [np.empty(shape), [None] * len(rows)]
            for m, r in enumerate(rows):
                if buf[1][m] is not r or not _frozen(r):
                    buf[0][m] = r
                    buf[1][m] = r if _frozen(r) else None     # (only frozen arrays are trusted to be unchanged)
            out[k] = buf[0]
        return out

    def _flatten(self, cp: ControlParams):
        gp, mp = cp.geometrical_params, cp.mechanical_params
        cnv = np.asarray(gp.centroid_node_vectors, dtype=float)
        nbd = len(self.bonds)
        bp = mp.bond_params
        # the spring models read a subset of (k_stretch, k_shear, k_rot, reference_vector) (energy.py:30-67): what a model does not
        # read is passed as 0 / a unit dummy vector and comes back with a zero gradient
        zero = np.zeros(nbd)
        out = {
            "centroid_node_vectors": cnv,
            "reference_vector": self._memo("reference_vector", getattr(bp, "reference_vector", None), lambda: np.ascontiguousarray(np.broadcast_to(
                np.asarray(getattr(bp, "reference_vector", np.array([1.0, 0.0])), dtype=float), (nbd, 2)))),
            "k_bond": self._memo("k_bond", (bp.k_stretch, getattr(bp, "k_shear", None), getattr(bp, "k_rot", None)), lambda: np.stack(
                [_bcast(bp.k_stretch, nbd),
                 _bcast(bp.k_shear, nbd) if self.spec.bond_model in (_b.BOND_LINEARIZED, _b.BOND_NONLINEAR) else zero,
                 _bcast(bp.k_rot, nbd) if self.spec.bond_model != _b.BOND_SIMPLE_SPRING else zero], 1)),
        }
        cached = _FLAT_CACHE.get(id(cnv)) if mp.inertia is None else None
        if cached is not None and cached[0]() is cnv and _frozen(cnv) and (cached[1] is self.bonds or np.array_equal(cached[1], self.bonds)) and np.array_equal(cached[2], mp.density):
            out["inertia"] = cached[3]        # same design seen through another solver (multi-input problems): reuse
            if self.spec.contact == _b.CONTACT_ANGLE and cached[4] is not None:
                out["void_angle0"] = cached[4]
        elif mp.inertia is None:   # dynamics.py:157-163
            out["inertia"] = compute_inertia(cnv, mp.density)
        else:
            out["inertia"] = np.asarray(mp.inertia, dtype=float).reshape(self.n_blocks, 3)
        def _damping():
            damping = np.zeros((self.n_blocks, 3))
            if self.damped_blocks is not None:   # loading.py:71-106
                damping[self.damped_blocks] = np.broadcast_to(np.asarray(mp.damping, dtype=float), (len(self.damped_blocks), 3))
            return damping
        out["damping"] = self._memo("damping", mp.damping, _damping)
        if self.spec.contact:
            c = mp.contact_params
            if self.spec.contact == _b.CONTACT_DISTANCE:      # energy.py:397-404: absolute node positions enter
                out["block_centroids"] = np.asarray(gp.block_centroids, dtype=float).reshape(self.n_blocks, 2)
                out.pop("void_angle0", None)
            elif "void_angle0" not in out:
                out["void_angle0"] = void_angles0(cnv, self.bonds)
            out["contact"] = np.array([c.min_angle, c.cutoff_angle, c.k_contact], dtype=float)
        if mp.inertia is None and cached is None and _frozen(cnv):
            # geometry arrays that come out of the design cache are frozen and shared: remember what was derived from them
            import weakref
            key = id(cnv)
            if len(_FLAT_CACHE) > 1024:
                _FLAT_CACHE.clear()
            _FLAT_CACHE[key] = (weakref.ref(cnv, lambda _r, k=key: _FLAT_CACHE.pop(k, None)), self.bonds, np.array(mp.density, copy=True),
                                out["inertia"], out.get("void_angle0"))
        fnp = [f.resolve(cp.constraint_params) for f in self.con_terms] + [f.resolve(cp.loading_params) for f in self.load_terms]
        if fnp:
            out["fn_params"] = np.stack(fnp)
        return out

    def _flatten_tangent(self, cp: ControlParams, cp_dot):
        """The tangent of :meth:`_flatten` at ``cp`` along ``cp_dot`` (a ``ControlParams``-shaped tree of tangents; a leaf of None, a
        missing sub-tree or a missing dict key is a zero tangent): the same arrays, the same broadcasts (scalar stiffnesses, damping on
        ``damped_blocks`` only), the same zeroing of what a spring model does not read, and the exact host derivatives of the derived
        leaves -- inertia through compute_inertia (when ``mechanical_params.inertia`` is None), void angles through void_angles0,
        time-function parameters through each term's ``resolve``.  Linear in ``cp_dot``."""
        gp, mp = cp.geometrical_params, cp.mechanical_params
        gd = getattr(cp_dot, "geometrical_params", None)
        md = getattr(cp_dot, "mechanical_params", None)

        def leaf(tree, name):
            v = getattr(tree, name, None) if tree is not None else None
            return 0.0 if v is None else v
        cnv = np.asarray(gp.centroid_node_vectors, dtype=float)
        cnv_dot = np.broadcast_to(np.asarray(leaf(gd, "centroid_node_vectors"), dtype=float), cnv.shape).copy()
        nbd = len(self.bonds)
        bp = mp.bond_params
        bd = getattr(md, "bond_params", None)
        zero = np.zeros(nbd)
        refv_dot = leaf(bd, "reference_vector") if hasattr(bp, "reference_vector") else 0.0
        out = {
            "centroid_node_vectors": cnv_dot,
            "reference_vector": np.broadcast_to(np.asarray(refv_dot, dtype=float), (nbd, 2)).copy(),
            "k_bond": np.stack([_bcast(leaf(bd, "k_stretch"), nbd),
                                _bcast(leaf(bd, "k_shear"), nbd) if self.spec.bond_model in (_b.BOND_LINEARIZED, _b.BOND_NONLINEAR) else zero,
                                _bcast(leaf(bd, "k_rot"), nbd) if self.spec.bond_model != _b.BOND_SIMPLE_SPRING else zero], 1),
        }
        if mp.inertia is None:
            out["inertia"] = compute_inertia_jvp(cnv, mp.density, cnv_dot, leaf(md, "density"))
        else:
            out["inertia"] = np.broadcast_to(np.asarray(leaf(md, "inertia"), dtype=float).reshape(-1), (self.n_blocks * 3,)).reshape(
                self.n_blocks, 3).copy()
        damping = np.zeros((self.n_blocks, 3))
        if self.damped_blocks is not None:
            damping[self.damped_blocks] = np.broadcast_to(np.asarray(leaf(md, "damping"), dtype=float), (len(self.damped_blocks), 3))
        out["damping"] = damping
        if self.spec.contact:
            cd = getattr(md, "contact_params", None)
            if self.spec.contact == _b.CONTACT_DISTANCE:
                out["block_centroids"] = np.broadcast_to(np.asarray(leaf(gd, "block_centroids"), dtype=float).reshape(-1),
                                                         (self.n_blocks * 2,)).reshape(self.n_blocks, 2).copy()
            else:
                out["void_angle0"] = void_angles0_jvp(cnv, self.bonds, cnv_dot)
            out["contact"] = np.array([leaf(cd, "min_angle"), leaf(cd, "cutoff_angle"), leaf(cd, "k_contact")], dtype=float)
        con_dot = getattr(cp_dot, "constraint_params", None)
        load_dot = getattr(cp_dot, "loading_params", None)
        fnp = [f.resolve_jvp(cp.constraint_params, con_dot) for f in self.con_terms] + \
              [f.resolve_jvp(cp.loading_params, load_dot) for f in self.load_terms]
        if fnp:
            out["fn_params"] = np.stack(fnp)
        return out

    def _members(self, control_params):
        cps = list(control_params) if isinstance(control_params, (list, tuple)) and not isinstance(control_params, ControlParams) \
            else [control_params]
        if len(cps) == 1 and self.batch > 1:
            cps = cps * self.batch
        if len(cps) != self.batch:
            raise ValueError(f"expected {self.batch} ControlParams, got {len(cps)}")
        return cps

    def estimate_steps_per_interval(self, flat, timepoints):
        """Fixed grid from a Gershgorin-type bound on the largest natural frequency: h * omega_max <= 0.5."""
        inertia, k, cnv = flat["inertia"], flat["k_bond"], flat["centroid_node_vectors"]
        l02 = (flat["reference_vector"] ** 2).sum(1)
        n_b = np.zeros(self.n_blocks)
        kt = np.zeros(self.n_blocks); kr = np.zeros(self.n_blocks)
        r2 = (cnv ** 2).sum(-1).max(1)
        for end in (0, 1):
            blk = self.bonds[:, end] // self.n_npb
            np.add.at(kt, blk, 2 * (k[:, 0] + k[:, 1]))
            np.add.at(kr, blk, 2 * ((k[:, 0] + k[:, 1]) * r2[blk] + k[:, 2] + k[:, 1] * l02 / 4))
            np.add.at(n_b, blk, 1)
        w2 = max((kt / inertia[:, 0]).max(), (kr / inertia[:, 2]).max())
        dt = 0.5 / np.sqrt(w2)
        span = np.diff(np.asarray(timepoints, dtype=float)).max() if len(timepoints) > 1 else 0.0
        return max(1, int(np.ceil(span / dt)))

    def adaptive_grid(self, state0, timepoints, flats, refine=None):
        """(steps per output interval, step boundaries) frozen from a forward-only adaptive solve of the same problem
        (parameters already on the device): the step boundaries the controller accepted for the member that needed
        the most steps, merged with the output times (the controller steps across them and interpolates; a fixed grid
        has to land on them).  Accepted boundaries closer to an output time than 1 % of the neighbouring step are dropped.

        ``refine = k`` (default: the solver's ``grid_refine``, 1) splits every step of the frozen grid into k equal ones.  Why one
        would: the discrete adjoint differentiates the fixed-grid solve exactly, but at loose tolerances (the paper's atol = 1e-4) that
        solve -- on steps the controller sized for ITS error estimate -- is further from the exact gradient than the reference's
        continuous adjoint, which re-integrates the adjoint equations with its own controller (6.9e-3 against 1.7e-3 on the paper
        lattice; with k = 2 the frozen-grid gradient is the closer one, at twice the steps: python -m tests.adjoint_semantics)."""
        ts = np.asarray(timepoints, dtype=float)
        if len(ts) < 2:
            return np.zeros(0, dtype=np.int32), None
        _, st = self.engine.forward_adaptive(state0, ts, self.rtol, self.atol, max_attempts=self.max_attempts)
        self.adaptive_stats = st
        counts = self.engine.adaptive_step_counts()
        acc = self.engine.adaptive_step_times(int(counts.sum(1).argmax()))
        acc = acc[(acc > ts[0]) & (acc < ts[-1])]
        if len(acc):
            step = np.diff(np.concatenate([[ts[0]], acc]))
            near = np.abs(acc[:, None] - ts[None, :]).min(1)
            acc = acc[near > 0.01 * step]
        grid = np.union1d(ts, acc)
        k = self.grid_refine if refine is None else int(refine)
        if k > 1:
            fr = np.arange(k) / k
            grid = np.concatenate([(grid[:-1, None] + np.diff(grid)[:, None] * fr[None, :]).reshape(-1), grid[-1:]])
            grid[::k] = np.union1d(ts, acc)          # the original boundaries exactly (output times must be hit bit for bit)
        spis = np.array([np.count_nonzero((grid >= a) & (grid < b)) for a, b in zip(ts[:-1], ts[1:])], dtype=np.int32)
        return spis, grid

    # -- solve -----------------------------------------------------------------------------------------
    def prepare(self, control_params):
        """Host side of a solve: ``ControlParams`` -> flattened arrays -> device (``dfx_set_params``).  After it the inputs of
        :meth:`solve_resident` are resident in HBM."""
        cps = self._members(control_params)
        self._memo_pass = object()          # (the members of one prepare share their leaves' content checks)
        try:
            flats = [self._flatten(cp) for cp in cps]
        finally:
            self._memo_pass = None
        self.engine.set_params(**self._stack(flats))
        for f, term, field in self._table_leaves:
            self.engine.fn_table_values(f, np.stack([term.resolve_values(getattr(cp, field)) for cp in cps]))
        self._prepared = (cps, flats)
        return cps, flats

    def __call__(self, state0, timepoints, control_params, keep_trajectory=False, steps_per_interval=None, step_times=None,
                 want_fields=True):
        self.prepare(control_params)
        fields = self.solve_resident(state0, timepoints, keep_trajectory=keep_trajectory, steps_per_interval=steps_per_interval,
                                     step_times=step_times, want_fields=want_fields)
        if fields is None:
            return None
        # one ControlParams (not a list) and batch 1 -> no leading member axis
        return fields[0] if self.batch == 1 and not isinstance(control_params, (list,)) else fields

    def solve_resident(self, state0, timepoints, keep_trajectory=False, steps_per_interval=None, step_times=None, want_fields=True):
        """The solve on the parameters :meth:`prepare` left on the device; returns the fields with their leading member axis (or None)."""
        cps, flats = self._prepared
        self.solve_count += 1
        spi = steps_per_interval if steps_per_interval is not None else self.steps_per_interval
        if np.ndim(timepoints) == 2:
            # one row of output times per member (same number of outputs and of steps per interval: the members advance in the same
            # launches, each on its own time grid) -- forward inputs whose static phases differ in length, static-tuning problem
            if spi is None:
                raise ValueError("per-member timepoints need steps_per_interval (the adaptive controller chooses one grid per call)")
            s0 = None if state0 is None else np.asarray(state0, dtype=float)
            if s0 is not None and s0.ndim == 3:
                s0 = np.broadcast_to(s0, (self.batch,) + s0.shape)
            fields, stats = self.engine.forward(s0, timepoints, spi, keep_trajectory=keep_trajectory, step_times=step_times, want_fields=want_fields)
            self._last = (cps, flats, np.asarray(timepoints, dtype=float))
            self._last_fields = fields
            self.stats = dict(stats, steps_per_interval=spi, step_times=step_times, step_control="fixed")
            return fields
        state0 = np.asarray(state0, dtype=float)
        if state0.ndim == 3:
            state0 = np.broadcast_to(state0, (self.batch,) + state0.shape)
        if spi is None and not keep_trajectory:
            # reference behaviour: adaptive Dormand-Prince controlled by rtol / atol (dynamics.py:166)
            fields, stats = self.engine.forward_adaptive(state0, timepoints, self.rtol, self.atol, max_attempts=self.max_attempts)
            self._last = None
            self.stats = dict(stats, steps_per_interval=None, step_control="adaptive")
            return fields
        control = "fixed"
        if spi is None and self.grid_refine == 1 and self.engine.can_keep_adaptive and os.environ.get("DFX_ADAPTIVE_RECORDS", "1") != "0":
            # the reference's call, differentiable as it stands: the adaptive pass keeps its accepted steps and the reverse sweep is their
            # exact discrete adjoint, output cotangents entering through the dense output -- one forward pass, one reverse sweep, and the
            # gradient belongs to exactly the fields returned (dfx_forward_adaptive_keep; DFX_ADAPTIVE_RECORDS=0: the frozen grid below)
            try:
                fields, stats = self.engine.forward_adaptive(state0, timepoints, self.rtol, self.atol, max_attempts=self.max_attempts,
                                                             keep_trajectory=True, want_fields=want_fields)
            except RuntimeError as e:
                if "forward_adaptive_keep:" not in str(e):
                    raise
                fields = stats = None        # the kept steps do not fit the device (or this physics keeps the two-pass form): frozen grid below
            if stats is not None:
                self._last = (cps, flats, np.asarray(timepoints, dtype=float))
                self._last_fields = fields
                self.stats = dict(stats, steps_per_interval=None, step_times=None, step_control="adaptive-records")
                return fields
        if spi is None:   # the reverse sweep needs a fixed grid: freeze the one the adaptive controller chooses
            spi, step_times = self.adaptive_grid(state0, timepoints, flats)
            control = "adaptive-grid"
        # want_fields=False: the histories stay on the device (objectives evaluated there do not need them on the host)
        fields, stats = self.engine.forward(state0, timepoints, spi, keep_trajectory=keep_trajectory, step_times=step_times,
                                            want_fields=want_fields)
        self._last = (cps, flats, np.asarray(timepoints, dtype=float))
        self._last_fields = fields
        self.stats = dict(stats, steps_per_interval=spi, step_times=step_times, step_control=control)
        return fields

    # -- forward mode ------------------------------------------------------------------------------------
    def jvp(self, state0, timepoints, control_params, state0_dot, control_params_dot, steps_per_interval=None, step_times=None,
            adaptive=False):
        """Forward-mode derivative of the FIXED-GRID solve (``adaptive=True``: of the adaptive solve itself, see below):
        ``fields, fields_dot = jvp(state0, timepoints, control_params, state0_dot, control_params_dot)``,
        ``fields_dot = d fields / d(state0, control_params) . (state0_dot, control_params_dot)`` with the steps frozen
        (one stage launch per Runge-Kutta stage computes the primal and the tangent together: the kernels of :meth:`jvp_multi` at one
        direction, and this call is ``jvp_multi`` with ``tangents=[(state0_dot, control_params_dot)]``, column 0).  This is the map
        :meth:`vjp` transposes: on the same grid  ``sum(fields_bar * fields_dot) == <vjp(fields_bar), tangent>``.

        * ``control_params_dot``: a ``ControlParams``-shaped tree of tangents (the shape :meth:`vjp` returns), or a list of them, one per
          member; a leaf of None, a missing sub-tree or a missing key of ``constraint_params`` / ``loading_params`` is a zero tangent.
          ``state0_dot`` (None: zero) has the shape of ``state0``.  One direction per member here; several directions per member (a
          ``jacfwd`` over k leaves, on a solver of any batch) are :meth:`jvp_multi`.  Tangents of derived leaves are exact host derivatives:
          inertia (through compute_inertia when ``mechanical_params.inertia`` is None), void angles, time-function parameters.
        * ``fields`` is the primal history of the same call; on the same grid it equals ``solve_dynamics(..., steps_per_interval=...,
          step_times=...)`` to rounding.
        * ``steps_per_interval=None`` (and no default grid set at setup): the grid the adaptive controller chooses is frozen first
          (:meth:`adaptive_grid`, as the ``"adaptive-grid"`` path of a differentiable solve) and the tangent pass runs on it.  These
          ``fields`` are then the frozen-grid RE-INTEGRATION, not the adaptive solve's dense output: they differ from what
          ``solve_dynamics(state0, timepoints, control_params)`` returns by O(tolerance).  ``self.stats`` reports the grid.
        * ``adaptive=True`` (no grid of any kind: not with ``steps_per_interval``, ``step_times``, a default grid set at setup,
          ``grid_refine > 1`` or per-member ``timepoints`` -- ``ValueError``): the map differentiated is the reference's call,
          ``solve_dynamics(state0, timepoints, control_params)``.  The adaptive pass runs first (keeping its accepted steps where the
          library and the physics allow it), then the tangent pass takes every member over ITS OWN accepted steps, frozen, and forms the
          outputs and their tangents inside the steps by the controller's quartic dense output (``dfx_forward_tangent_dense_multi``).
          ``fields`` are the fields of that call to rounding, and ``fields_dot`` is the transpose of what :meth:`vjp` computes on the
          ``"adaptive-records"`` path: when the steps were kept (``self.stats["kept_trajectory"]``), ``vjp`` may follow this call directly
          and differentiates the same solve.  Step sizes and accept / reject decisions are not differentiated.  ``self.stats`` reports
          ``step_control="adaptive-dense"`` and ``steps_per_member``.
        * rows of PRESCRIBED DOFs in ``fields_dot`` are  sum_f coef (dg_f/dp . dp, dg_f'/dp . dp)  from each term's ``param_partials``,
          as :meth:`vjp` computes their cotangents -- a central difference, accurate to ~1e-9 relative, not to rounding.  The samples
          of a ``loading.Table`` with named values are the exception: value and rate are linear in them, and their share of these rows
          (an array tangent under the table's key) is the analytic hat weights ``Table.hat_weights`` / ``rate_weights``, to rounding.
        * not supported (``RuntimeError`` from the engine): lattices whose nodes carry more than one ligament.  The CPU port of the
          oracle has no forward mode (``NotImplementedError``).

        The solver's trajectory checkpoint is not kept by this call (``adaptive=True`` apart): a ``vjp`` must follow a solve with
        ``keep_trajectory=True``."""
        fields, fields_dot = self.jvp_multi(state0, timepoints, control_params, [(state0_dot, control_params_dot)],
                                            steps_per_interval=steps_per_interval, step_times=step_times, adaptive=adaptive, _who="jvp")
        return fields, (fields_dot[0] if fields_dot.ndim == 5 else fields_dot[:, 0])

    def _prescribed_tangent_rows(self, fields_dot_m, cp, cd, ts_m):
        """The rows of PRESCRIBED DOFs of one member's ``fields_dot`` (T, 2, nb, 3) along one direction ``cd``, in place:
        sum_f coef (dg_f/dp . dp, dg_f'/dp . dp) at the member's output times (:meth:`jvp`, :meth:`jvp_multi`)."""
        if not (len(self.constrained_pairs) and self.con_terms):
            return
        n_con = len(self.constrained_pairs)
        dofs = self.constrained_pairs[:, 0] * 3 + self.constrained_pairs[:, 1]
        fdm = fields_dot_m.reshape(len(ts_m), 2, -1)
        fdm[:, :, dofs] = 0.0
        for term in self.con_terms:
            dp = term.resolve_jvp(cp.constraint_params, getattr(cd, "constraint_params", None))
            dy = self._table_tangent(term, getattr(cd, "constraint_params", None))
            if not np.any(dp) and dy is None:
                continue
            p = term.resolve(cp.constraint_params)
            bound = term.bind(cp.constraint_params)
            vec = _bcast(term.vector, n_con)
            for k, t in enumerate(ts_m):
                if np.any(dp):
                    fdm[k, 0, dofs] += vec * float(bound.param_partials(float(t), p, "value") @ dp)
                    fdm[k, 1, dofs] += vec * float(bound.param_partials(float(t), p, "rate") @ dp)
                if dy is not None:          # the samples of a named table: analytic hat weights
                    fdm[k, 0, dofs] += vec * p[0] * float(term.hat_weights(float(t) - p[1]) @ dy)
                    fdm[k, 1, dofs] += vec * p[0] * float(term.rate_weights(float(t) - p[1]) @ dy)

    @staticmethod
    def _table_tangent(term, params_dot):
        """The (n_tab,) tangent of a named table's values in a tangent dict, or None (no such leaf, no entry, an all-zero entry)."""
        name = getattr(term, "values_name", None)
        v = None if (name is None or params_dot is None) else params_dot.get(name)
        if v is None:
            return None
        v = np.asarray(v, dtype=float)
        if v.shape != term.times.shape:
            raise ValueError(f"tangent of '{name}' must have shape {term.times.shape}, got {v.shape}")
        return v if np.any(v) else None

    def _set_table_tangents(self, dots, K):
        """The sample tangents of every named table, [direction][member], on the device for the next forward-mode call of K directions."""
        for f, term, field in self._table_leaves:
            arr = np.zeros((K, self.batch, len(term.times)))
            for k in range(K):
                for m in range(self.batch):
                    v = self._table_tangent(term, getattr(dots[k][m], field, None))
                    if v is not None:
                        arr[k, m] = v
            self.engine.fn_table_tangents(f, arr)

    def _clear_table_tangents(self):
        for f, _, _ in self._table_leaves:
            self.engine.fn_table_tangents(f, None)

    def _member_tangents(self, control_params_dot):
        """``control_params_dot`` of one direction as a list of one tangent tree per member (:meth:`jvp`'s rules)."""
        dots = list(control_params_dot) if isinstance(control_params_dot, (list, tuple)) and not isinstance(control_params_dot, ControlParams) \
            else [control_params_dot]
        if len(dots) == 1 and self.batch > 1:
            dots = dots * self.batch
        if len(dots) != self.batch:
            raise ValueError(f"expected {self.batch} tangents, got {len(dots)}")
        return dots

    def _tangent_solve(self, _who, state0, timepoints, control_params, tangents, steps_per_interval, step_times, adaptive, spec=None):
        """What :meth:`jvp_multi` and :meth:`signal_jvp_multi` share: the checks, the flattened parameters and tangents, the grid (given,
        chosen by the adaptive controller and frozen, or the adaptive solve's own accepted steps), ``self.stats`` and the engine call.
        ``spec=None``: (fields, fields_dot) of all members as the engine returns them (rows of prescribed DOFs not yet assembled);
        an ``objective.SignalSpec``: (signals, signals_dot) through the signal entries.  Also returns the per-member parameters, the
        tangent trees [direction][member] and the timepoints."""
        who = f"DynamicSolver.{_who}"
        if adaptive:
            grids = [name for name, on in (("steps_per_interval", steps_per_interval is not None), ("step_times", step_times is not None),
                                           ("a default grid of the solver", self.steps_per_interval is not None),
                                           ("grid_refine > 1", self.grid_refine > 1), ("per-member timepoints", np.ndim(timepoints) == 2)) if on]
            if grids:
                raise ValueError(f"{who}: adaptive=True differentiates the adaptive solve on its own accepted steps and takes "
                                 f"no grid (got {', '.join(grids)})")
        tangents = list(tangents) if tangents is not None else []
        if not tangents:
            raise ValueError(f"{who}: need at least one (state0_dot, control_params_dot) pair")
        for tg in tangents:
            if not (isinstance(tg, (tuple, list)) and not isinstance(tg, ControlParams) and len(tg) == 2):
                raise ValueError(f"{who}: every tangent is a pair (state0_dot, control_params_dot)")
        K = len(tangents)
        dots = [self._member_tangents(cd) for _, cd in tangents]            # [direction][member]
        engine = self.engine
        if spec is not None and not engine.has_forward_tangent_signals:
            raise NotImplementedError(f"{who}: the library {getattr(engine.lib, '_name', engine.lib)!r} has no dfx_forward_tangent_signals_multi "
                                      "(a stale libdfx.so, or the CPU port of the oracle; build the HIP engine)")
        if spec is None:
            fixed, dense = engine.forward_tangent_multi, engine.forward_tangent_dense_multi
        else:       # the same two solves with the history kept on the device: signals and their tangents come back
            def fixed(*a, step_times=None):
                return engine.forward_tangent_signals_multi(*a, *self._terms(spec), step_times=step_times)

            def dense(*a):
                return engine.forward_tangent_signals_dense_multi(*a, *self._terms(spec))
        if not engine.has_forward_tangent_multi or (adaptive and not engine.has_forward_tangent_dense_multi):
            lib = engine.lib
            raise NotImplementedError(f"{who}: the library {getattr(lib, '_name', lib)!r} has no dfx_forward_tangent{'' if _who == 'jvp' else '_multi'} "
                                      "(forward mode runs on the HIP engine only; the CPU port of the oracle is reverse mode only)")
        cps, flats = self.prepare(control_params)
        self._last = None                   # (dfx_set_params dropped the handle's checkpoint)
        params_dots = []
        for k in range(K):
            tflats = [self._flatten_tangent(cp, cd) for cp, cd in zip(cps, dots[k])]
            params_dots.append({name: np.stack([f[name] for f in tflats]) for name in tflats[0]})
        ts = np.asarray(timepoints, dtype=float)
        B, nb = self.batch, self.n_blocks

        def members(x):
            if x is None:
                return None
            x = np.asarray(x, dtype=float)
            return np.broadcast_to(x, (B,) + x.shape) if x.ndim == 3 else x
        s0 = members(state0)
        s0ds = None
        if any(sd is not None for sd, _ in tangents):
            s0ds = np.zeros((B, K, 2, nb, 3))
            for k, (sd, _) in enumerate(tangents):
                if sd is not None:
                    s0ds[:, k] = members(sd)
        spi = steps_per_interval if steps_per_interval is not None else self.steps_per_interval
        control = "fixed"
        if adaptive:
            # What the tangent pass refuses (extra ligaments, a tableau without dense output) is refused before the adaptive pass is paid
            # for: the same entry point on the initial state alone, one timepoint and no step.  Then the adaptive pass, its accepted steps
            # kept for a vjp of the same solve where the kept-steps path serves the physics, and the tangent pass over every member's own
            # step boundaries.
            dense(s0, None, None, 1, ts[:1], np.full((B, 1), ts[0]), np.zeros(B, dtype=np.int64))
            kept, primal, astats = False, None, None
            if engine.can_keep_adaptive and os.environ.get("DFX_ADAPTIVE_RECORDS", "1") != "0":
                try:
                    primal, astats = engine.forward_adaptive(s0, ts, self.rtol, self.atol, max_attempts=self.max_attempts, keep_trajectory=True)
                    kept = True
                except RuntimeError as e:
                    if "forward_adaptive_keep:" not in str(e):
                        raise
            if not kept:
                primal, astats = engine.forward_adaptive(s0, ts, self.rtol, self.atol, max_attempts=self.max_attempts)
            self.adaptive_stats = astats
            grid, n_steps = _b.padded_step_times([engine.adaptive_step_times(m) for m in range(B)], ts[0])
            self._set_table_tangents(dots, K)
            try:
                fields, fields_dot, stats = dense(s0, s0ds, params_dots, K, ts, grid, n_steps)
            finally:
                self._clear_table_tangents()
            if kept:        # as a differentiable solve leaves it: vjp reverses the adaptive pass above
                self._last = (cps, flats, ts)
                self._last_fields = primal
            self.stats = dict(stats, steps_per_interval=None, step_times=grid, step_control="adaptive-dense",
                              steps_per_member=[int(n) for n in n_steps], kept_trajectory=kept)
        else:
            if spi is None:
                if ts.ndim == 2:
                    raise ValueError("per-member timepoints need steps_per_interval (the adaptive controller chooses one grid per call)")
                # (the refusals before the adaptive pass that chooses the grid is paid for)
                fixed(s0, None, None, 1, ts[:1], 1)
                spi, step_times = self.adaptive_grid(np.zeros((B, 2, nb, 3)) if s0 is None else s0, ts, flats)
                control = "adaptive-grid"
            self._set_table_tangents(dots, K)
            try:
                fields, fields_dot, stats = fixed(s0, s0ds, params_dots, K, ts, spi, step_times=step_times)
            finally:
                self._clear_table_tangents()
            self.stats = dict(stats, steps_per_interval=spi, step_times=step_times, step_control=control)
        return fields, fields_dot, cps, dots, ts

    def jvp_multi(self, state0, timepoints, control_params, tangents, steps_per_interval=None, step_times=None, adaptive=False,
                  _who="jvp_multi"):
        """:meth:`jvp` along K directions in one pass: ``fields, fields_dot = jvp_multi(state0, timepoints, control_params, tangents)``
        with ``tangents`` a list of K pairs ``(state0_dot, control_params_dot)`` (either element may be None: zero; ``control_params_dot``
        follows :meth:`jvp`'s rules -- None leaves, missing keys, a list of one tree per member when batch > 1).  The stage kernel carries
        one value and several epsilon parts (``dfx_forward_tangent_multi`` / ``dfx_forward_tangent_dense_multi``), so the primal chain --
        records, transcendentals, branch decisions, parameter loads -- is paid once per chunk of directions instead of once per
        direction, and a solver of batch 1 returns a whole Jacobian over a few leaves.  ``fields`` is what :meth:`jvp` returns;
        ``fields_dot`` has a direction axis in front of T: (K, T, 2, nb, 3) for a single design, (batch, K, T, 2, nb, 3) otherwise, and
        ``fields_dot[..., k, :, :, :, :]`` is :meth:`jvp` along ``tangents[k]`` to rounding.  Grid semantics, ``adaptive=True`` (a
        ``ValueError`` with a grid of any kind), ``self.stats`` and "``vjp`` may follow on the kept solve" are :meth:`jvp`'s.
        (``_who``: the public method the call came through, for the error texts.)"""
        fields, fields_dot, cps, dots, ts = self._tangent_solve(_who, state0, timepoints, control_params, tangents, steps_per_interval,
                                                                step_times, adaptive)
        for m, cp in enumerate(cps):
            for k in range(len(dots)):
                self._prescribed_tangent_rows(fields_dot[m, k], cp, dots[k][m], ts[m] if ts.ndim == 2 else ts)
        if self.batch == 1 and not isinstance(control_params, list):
            return fields[0], fields_dot[0]
        return fields, fields_dot

    def signal_jvp_multi(self, state0, timepoints, control_params, tangents, spec, steps_per_interval=None, step_times=None, adaptive=False):
        """The signals of an ``objective.SignalSpec`` and their tangents along K directions, with the history kept on the device:
        ``signals, signals_dot = signal_jvp_multi(state0, timepoints, control_params, tangents, spec)`` -- (T, ns) and (K, T, ns) for
        one design, (batch, T, ns) and (batch, K, T, ns) otherwise.  It is :meth:`jvp_multi` followed by the signals of ``fields`` and of
        every ``fields_dot[k]`` -- the same solve, the same kernels, the same passes -- but what crosses PCIe is (batch, K, T, ns)
        instead of two histories, and force components (which have no host path) are differentiated where the solve ran: one dual-number
        evaluation of the ligament gradient per listed slot and output time (``dfx_forward_tangent_signals_multi`` / ``_dense_multi``).
        Column k is the derivative of :meth:`signal_values` along ``tangents[k]``; on the same grid it is the transpose of
        :meth:`signal_misfit_value_and_raw`.  ``tangents``, the grid semantics, ``adaptive=True``, ``self.stats`` and "a ``vjp`` may follow
        on the kept adaptive solve" are :meth:`jvp_multi`'s; targets and weights of ``spec`` are not read.  For a term on the VELOCITY of
        a prescribed DOF the engine's column holds 0 and ``coef * vector * (dg'/dp . dp)`` is added here from the ``"rate"`` partials of
        the constraint's time functions, as :meth:`jvp_multi` assembles those rows (a handful of numbers per solve)."""
        S, Sd, cps, dots, ts = self._tangent_solve("signal_jvp_multi", state0, timepoints, control_params, tangents, steps_per_interval,
                                                   step_times, adaptive, spec=spec)
        if len(self.constrained_pairs) and self.con_terms:
            n_con = len(self.constrained_pairs)
            row = {(int(b), int(d)): i for i, (b, d) in enumerate(self.constrained_pairs)}
            driven = [(s_, row[(b, c - 3)], coef) for s_, b, c, coef in spec.terms if 3 <= c < 6 and (b, c - 3) in row]
            for m, cp in enumerate(cps if driven else []):
                ts_m = ts[m] if ts.ndim == 2 else ts
                for k in range(len(dots)):
                    for term in self.con_terms:
                        dp = term.resolve_jvp(cp.constraint_params, getattr(dots[k][m], "constraint_params", None))
                        dy = self._table_tangent(term, getattr(dots[k][m], "constraint_params", None))
                        if not np.any(dp) and dy is None:
                            continue
                        p = term.resolve(cp.constraint_params)
                        bound = term.bind(cp.constraint_params)
                        vec = _bcast(term.vector, n_con)
                        rate = np.zeros(len(ts_m))
                        if np.any(dp):
                            rate += np.array([float(bound.param_partials(float(t), p, "rate") @ dp) for t in ts_m])
                        if dy is not None:
                            rate += np.array([p[0] * float(term.rate_weights(float(t) - p[1]) @ dy) for t in ts_m])
                        for s_, i, coef in driven:
                            Sd[m, k, :, s_] += coef * vec[i] * rate
        if self.batch == 1 and not isinstance(control_params, list):
            return S[0], Sd[0]
        return S, Sd

    def signal_jacfwd(self, state0, timepoints, control_params, wrt, spec, **grid_kwargs):
        """Columns of the Jacobian of the signals of ``spec`` with respect to scalar leaves, by :meth:`signal_jvp_multi` on one unit
        tangent per name (:func:`unit_tangent`): ``signals, {name: d signals / d name} = signal_jacfwd(state0, timepoints,
        control_params, wrt, spec)``; names, ``grid_kwargs`` and the batch rule are :meth:`jacfwd`'s."""
        wrt = list(wrt)
        if isinstance(control_params, (list, tuple)) and not isinstance(control_params, ControlParams):
            trees = [[unit_tangent(cp, name) for cp in control_params] for name in wrt]
        else:
            trees = [unit_tangent(control_params, name) for name in wrt]
        S, Sd = self.signal_jvp_multi(state0, timepoints, control_params, [(None, t) for t in trees], spec, **grid_kwargs)
        single = Sd.ndim == 3
        return S, {name: (Sd[k] if single else Sd[:, k]) for k, name in enumerate(wrt)}

    def jacfwd(self, state0, timepoints, control_params, wrt, **grid_kwargs):
        """Columns of the Jacobian of the fields with respect to scalar leaves, by :meth:`jvp_multi` on one unit tangent per name
        (:func:`unit_tangent`): ``fields, {name: fields_dot} = jacfwd(state0, timepoints, control_params, wrt)``.  ``wrt``: names from
        ``JACFWD_LEAVES`` and keys of ``constraint_params`` / ``loading_params``; ``grid_kwargs``: ``steps_per_interval``, ``step_times``,
        ``adaptive``.  With batch > 1 every member's leaf of that name is seeded (a list of ``ControlParams``: one tree per member)."""
        wrt = list(wrt)
        if isinstance(control_params, (list, tuple)) and not isinstance(control_params, ControlParams):
            trees = [[unit_tangent(cp, name) for cp in control_params] for name in wrt]
        else:
            trees = [unit_tangent(control_params, name) for name in wrt]
        fields, fields_dot = self.jvp_multi(state0, timepoints, control_params, [(None, t) for t in trees], **grid_kwargs)
        single = fields_dot.ndim == 5
        return fields, {name: (fields_dot[k] if single else fields_dot[:, k]) for k, name in enumerate(wrt)}

    # -- reverse mode ------------------------------------------------------------------------------------
    def vjp(self, fields_bar):
        """Gradient of sum(fields_bar * fields) w.r.t. every ControlParams leaf and state0.
        Requires the last call to have used ``keep_trajectory=True``.  Returns (ControlParams tree(s), state0_bar)."""
        if self._last is None:
            raise RuntimeError("vjp: call the solver with keep_trajectory=True first")
        fb = np.asarray(fields_bar, dtype=float)
        if fb.ndim == 4:
            fb = fb[None]
        grads, stats = self.engine.adjoint(fb)
        self.adjoint_stats = stats
        trees, s0 = self._unflatten_grads(grads, fb)
        self._last_state0_bar = s0
        # cotangents on the OUTPUTS of prescribed DOFs feed the constraint parameters directly:
        # fields[k, 0, dof] = c_dof(t_k; p), fields[k, 1, dof] = dc_dof/dt(t_k; p)   (dynamics.py:132-134, 169-182)
        if len(self.constrained_pairs) and self.con_terms:
            cps, flats, ts = self._last
            tl = trees if isinstance(trees, list) else [trees]
            n_con = len(self.constrained_pairs)
            dofs = self.constrained_pairs[:, 0] * 3 + self.constrained_pairs[:, 1]
            for m, (cp, tree) in enumerate(zip(cps, tl)):
                fbm = fb[m].reshape(ts.shape[-1], 2, -1)
                for term in self.con_terms:
                    vec = _bcast(term.vector, n_con)
                    wq = fbm[:, 0, dofs] @ vec          # (T,) weights of g(t_k)
                    wv = fbm[:, 1, dofs] @ vec          # (T,) weights of g'(t_k)
                    if not (np.any(wq) or np.any(wv)):
                        continue
                    p = term.resolve(cp.constraint_params)
                    bound = term.bind(cp.constraint_params)
                    leaf = getattr(term, "values_name", None)
                    g5 = np.zeros(_b.DFX_FN_PARAMS)
                    for k, t in enumerate(ts[m] if ts.ndim == 2 else ts):
                        if wq[k]:
                            g5 += wq[k] * bound.param_partials(float(t), p, "value")
                        if wv[k]:
                            g5 += wv[k] * bound.param_partials(float(t), p, "rate")
                        if leaf and (wq[k] or wv[k]):      # the samples: value and rate are linear in them, analytic hat weights
                            tree.constraint_params[leaf] = tree.constraint_params[leaf] + p[0] * (
                                wq[k] * term.hat_weights(float(t) - p[1]) + wv[k] * term.rate_weights(float(t) - p[1]))
                    term.scatter_grad(g5, tree.constraint_params, cp.constraint_params)
        return trees, s0

    def timepoints_vjp(self, fields_bar):
        """Cotangent of ``timepoints`` for the cotangent ``fields_bar`` of the last solve -- what ``jax.grad`` through the reference's
        ``solve_dynamics`` returns for its ``timepoints`` argument (dynamics.py:138-148; jax.experimental.ode._odeint_rev, restated in
        oracle/ref_adjoint.py).  Call after ``vjp(fields_bar)`` (its state0 cotangent is used).  With f = (v, a) the right-hand side on the
        free DOFs and (c', c'') the rates of the prescribed ones:

            ts_bar[i] = fields_bar[i] . d fields[i] / d t_i = g_i . f(y_i, t_i)        i >= 1   (moving a measurement time)
            ts_bar[0] = -lambda(t_0+) . f(y_0, t_0)  (+ g_0 . (c', c'') on prescribed DOFs),  lambda(t_0+) = state0_bar - g_0 on the free DOFs

        (the second line is the closed form of _odeint_rev's ``t0_bar``: d/dt (lambda . f) = lambda . df/dt between outputs and lambda jumps by
        g_i at t_i, so  -sum_i g_i . f_i + int lambda . df/dt dt = -lambda(t_0+) . f_0).  These are the derivatives of the CONTINUOUS solution:
        on a fixed grid they differ from the derivative of the discrete map by the integrator's truncation error, like the reference's own.
        One right-hand-side evaluation per output time (the engine's ``dfx_rhs`` hook).  Returns (T,) or (batch, T)."""
        if self._last is None or getattr(self, "_last_fields", None) is None or getattr(self, "_last_state0_bar", None) is None:
            raise RuntimeError("timepoints_vjp: solve with keep_trajectory=True (fields returned), then call vjp(fields_bar) first")
        cps, flats, ts = self._last
        B, nb = self.batch, self.n_blocks
        fb = np.asarray(fields_bar, dtype=float).reshape(B, -1, 2, nb * 3)
        fields = np.asarray(self._last_fields, dtype=float).reshape(B, -1, 2, nb * 3)
        s0b = np.asarray(self._last_state0_bar, dtype=float).reshape(B, 2, nb * 3)
        T = fields.shape[1]
        tsm = np.broadcast_to(ts, (B, T)) if ts.ndim == 1 else ts
        con = self.constrained_pairs[:, 0] * 3 + self.constrained_pairs[:, 1] if len(self.constrained_pairs) else np.zeros(0, dtype=np.int64)
        n_con = len(con)
        out = np.zeros((B, T))
        for i in range(T):
            # members that share this output time are evaluated in one call (one time for all of them unless timepoints has a row per member)
            for t in np.unique(tsm[:, i]):
                rows = np.nonzero(tsm[:, i] == t)[0]
                dy = self.engine.rhs(fields[:, i].reshape(B, 2, nb, 3), float(t)).reshape(B, 2, nb * 3)
                for m in rows:
                    rate = dy[m].copy()                           # (v, a) on the free DOFs, zeros on the prescribed ones
                    if n_con:
                        rate[0, con] = fields[m, i, 1, con]       # c'(t): the prescribed velocity is what the output holds
                        acc = np.zeros(n_con)
                        for term in self.con_terms:
                            p = term.resolve(cps[m].constraint_params)
                            h = 1e-4 * max(float(np.ptp(tsm[m])), 1e-300)      # (central difference of the rate, in the scale of the horizon)
                            bt = term.bind(cps[m].constraint_params)
                            acc += _bcast(term.vector, n_con) * (bt.rate(float(t) + h, p) - bt.rate(float(t) - h, p)) / (2 * h)
                        rate[1, con] = acc                        # c''(t)
                    g = fb[m, i]
                    if i == 0:
                        lam = s0b[m] - g
                        lam[:, con] = 0.0
                        out[m, 0] = -float(np.vdot(lam, rate))
                        if n_con:
                            out[m, 0] += float(np.vdot(g[:, con], rate[:, con]))
                    else:
                        out[m, i] = float(np.vdot(g, rate))
        return out[0] if (B == 1 and ts.ndim == 1) else out

    def _raw_which(self, which, centroids=False):
        """The parameter groups a raw-gradient call asks the engine for: no ``void_angle0`` without the angle contact, ``block_centroids``
        added with the distance contact (``centroids``: on every lattice -- the angular-momentum objective)."""
        which = tuple(w for w in which if not (w == "void_angle0" and self.spec.contact != _b.CONTACT_ANGLE))
        if (self.spec.contact == _b.CONTACT_DISTANCE or centroids) and "block_centroids" not in which:
            which = which + ("block_centroids",)
        return which

    def _take_stats(self, result):
        """An engine result that ends with the stats of its reverse sweep: those kept as ``adjoint_stats``, the rest returned."""
        self.adjoint_stats = result[-1]
        if self._table_leaves:      # the sample gradients of named tables, by function slot: {slot: (batch, n_tab)}
            for r in result[:-1]:
                if isinstance(r, dict):
                    r["fn_table_values"] = self._fn_table_grads()
        return result[:-1]

    def _fn_table_grads(self):
        """{function slot: (batch, n_tab)} sample gradients of the named tables from the last reverse sweep."""
        return {f: self.engine.fn_table_grad(f) for f, _, _ in self._table_leaves}

    def drive_cotangent(self, member=0):
        """``(times (n,), gbar (n_fns, n))`` of one member from the last reverse sweep of a solver with a named ``loading.Table``: the
        stage times in order and the cotangent dL/dg_f of every drive value there (function slots: constraint terms first, then loading
        terms).  For any parameter p of function f the sweep's part of dL/dp is ``sum(gbar[f] * dg_f/dp(times))`` -- the adjoint
        sensitivity of the objective to the drive itself."""
        return self.engine.drive_cotangent(member)

    def vjp_raw(self, fields_bar, which=("centroid_node_vectors", "void_angle0", "inertia")):
        """Reverse sweep for a cotangent of the fields, returning the engine's raw gradient arrays (batch-leading) of the requested
        parameter groups only -- by default what a design reaches.  Asking for every ControlParams leaf (``vjp``) runs the reverse
        stage in its build that also accumulates per-ligament and damping gradients, at up to twice the time per launch."""
        if self._last is None:
            raise RuntimeError("vjp_raw: call the solver with keep_trajectory=True first")
        fb = np.asarray(fields_bar, dtype=float)
        if fb.ndim == 4:
            fb = fb[None]
        which = self._raw_which(which)
        return self._take_stats(self.engine.adjoint(fb, which=which))[0]

    def kinetic_energy_value_and_vjp(self, target_blocks):
        """objective = sum_t sum_{b in target} m v^2/2 (energy.py:494-499 over problems/quads_focusing.py:461-467),
        evaluated and differentiated on the device (one engine call: the objective rides along with the reverse sweep)."""
        obj, grads = self._take_stats(self.engine.kinetic_value_and_grad(target_blocks))
        grads = {k: np.array(v) for k, v in grads.items()}      # the gradient tree outlives the engine's result area
        trees, s0 = self._unflatten_grads(grads, None)
        return (obj[0] if self.batch == 1 else obj), trees, s0

    def kinetic_energy_value_and_raw(self, target_blocks, which=("centroid_node_vectors", "void_angle0", "inertia")):
        """Same objective; returns the engine's raw gradient arrays (batch-leading) for the requested parameter groups only:
        read-only views of the engine's pinned result area, valid until the next call on this solver.
        The maps from these to a design (void-angle and inertia chain rules, lattice map) are linear in the cotangent, so a
        caller that sums several solves of ONE design (multi-input problems) applies them once to the sum."""
        which = self._raw_which(which)
        return self._take_stats(self.engine.kinetic_value_and_grad(target_blocks, which=which))

    def _engine_call(self, spec, suffix, **kwargs):
        """``Engine.<family><suffix>`` on the arguments ``spec.engine_call()`` states; the terms of its ``SignalSpec``, if any, lead them."""
        family, signal_spec, args, spec_kwargs = spec.engine_call()
        terms = () if signal_spec is None else self._terms(signal_spec)
        return getattr(self.engine, family + suffix)(*terms, *args, **spec_kwargs, **kwargs)

    def value(self, spec):
        """The value of any spec of ``objective`` on the device-resident history of the last solve (any forward pass): (batch,), or
        (J, peak, peak_at) / (J, peak, delay) for the peak-strain and cross-correlation specs."""
        return self._engine_call(spec, "_value")

    def value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """``(value, raw)`` of any spec of ``objective`` on the last kept solve: ``value`` as :meth:`value` returns it, ``raw`` the raw
        gradients of the parameter groups ``which`` as :meth:`kinetic_energy_value_and_raw` (``device=True``: ``DeviceArray`` handles)."""
        which = self._raw_which(which, centroids=getattr(spec, "needs_centroids", False))
        *out, raw = self._take_stats(self._engine_call(spec, "_value_and_grad", which=which, device=device))
        return (out[0] if len(out) == 1 else tuple(out)), raw

    def objective_value(self, spec):
        """(batch,) value of a weighted objective (``objective.ObjectiveSpec``) on the device-resident history of the last solve."""
        return self.value(spec)

    def objective_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """A weighted kinetic-energy / angular-momentum objective (``objective.ObjectiveSpec``) of the last kept solve, evaluated and
        differentiated on the device like :meth:`kinetic_energy_value_and_raw`: the history stays in HBM, the cotangent is formed there,
        and the explicit inertia / block-centroid terms are already in the raw gradients returned (``block_centroids`` is added to
        ``which`` for the angular kind: its levers contain the centroids)."""
        return self.value_and_raw(spec, which, device)

    def strain_objective_value(self, spec):
        """(batch,) value of a weighted ligament strain-energy objective (``objective.StrainObjectiveSpec``) on the device-resident history
        of the last solve (any forward pass: no kept trajectory needed)."""
        return self.value(spec)

    def strain_objective_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The weighted ligament strain energy (``objective.StrainObjectiveSpec``) of the last kept solve, evaluated and differentiated on
        the device beside :meth:`objective_value_and_raw`: the history stays in HBM, the ligament forces are formed there as the cotangent
        of the reverse sweep, and the explicit node-vector, void-angle and (when ``which`` names ``reference_vector`` / ``k_bond`` /
        ``contact``) per-ligament terms are already in the raw gradients returned.  As with :meth:`vjp_raw`, ``fn_params`` holds what the
        sweep accumulates: the direct dependence of a prescribed output DOF on its drive is not in it."""
        return self.value_and_raw(spec, which, device)

    def peak_strain_value(self, spec):
        """(J, peak, peak_at) of a peak ligament-strain measure (``objective.PeakStrainSpec``) on the device-resident history of the last
        solve (any forward pass: no kept trajectory needed): the smooth maximum (batch,), the hard maximum (batch,) and its (output, bond)
        (batch, 2)."""
        return self.value(spec)

    def peak_strain_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The peak ligament strain (``objective.PeakStrainSpec``) of the last kept solve, evaluated and differentiated on the device beside
        :meth:`strain_objective_value_and_raw`: ((J, peak, peak_at), raw gradients of J).  The softmax-weighted ligament forces are formed on
        the device as the cotangent of the reverse sweep; the explicit node-vector and (when ``which`` names ``reference_vector``) reference-
        vector terms are already in the raw gradients returned.  The coefficients of the spec are constants: the ``reference_vector``
        gradient does not see how ``objective.strain_limit_coefficients`` derived them from l0.  As with :meth:`vjp_raw`, ``fn_params``
        holds what the sweep accumulates: the direct dependence of a prescribed output DOF on its drive is not in it."""
        return self.value_and_raw(spec, which, device)

    def _terms(self, spec):
        """(terms, n_signals) of an ``objective.SignalSpec`` for the engine, whose hinge components are switched on or off as the spec says
        (``dfx_signal_hinge_channels``: off, component 9 and above are refused as out of range)"""
        self.engine.hinge_channels = spec.hinge_channels
        return spec.terms, spec.n_signals

    def signal_values(self, spec):
        """(batch, T, n_signals) signals of an ``objective.SignalSpec`` on the device-resident history of the last solve (any forward
        pass): field components are read from the history, force components are the elastic force dE/d(x, y, theta) on the block
        and hinge components the part of it that one ligament carries, evaluated there -- no second handle, no upload of states."""
        return self.engine.signal_values(*self._terms(spec))

    def signal_misfit_value(self, spec):
        """(batch,) least-squares misfit of an ``objective.SignalSpec`` against its targets on the device-resident history."""
        return self.value(spec)

    def signal_misfit_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The signal misfit (``objective.SignalSpec``) of the last kept solve, evaluated and differentiated on the device beside
        :meth:`strain_objective_value_and_raw`: the residual cotangent and, for force terms, the Hessian-vector product that carries it
        onto the fields are formed in HBM; the mixed second derivatives of the force terms (node vectors, void angles and, when ``which``
        names them, ``reference_vector`` / ``k_bond`` / ``contact``) are already in the raw gradients returned.  As with :meth:`vjp_raw`,
        ``fn_params`` holds what the sweep accumulates: the direct dependence of a prescribed output DOF on its drive is not in it."""
        return self.value_and_raw(spec, which, device)

    def signal_projections(self, spec):
        """(batch, n_signals, n_rows) projections of the signals of an ``objective.ProjectionSpec`` on the rows of its time basis, on the
        device-resident history of the last solve (any forward pass)."""
        return self.engine.signal_projections(*self._terms(spec.signal_spec), spec.basis)

    def signal_projection_value(self, spec):
        """(batch,) weighted quadratic form of the projections of an ``objective.ProjectionSpec`` on the device-resident history."""
        return self.value(spec)

    def signal_projection_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The projection objective (``objective.ProjectionSpec``) of the last kept solve, evaluated and differentiated on the device
        beside :meth:`signal_misfit_value_and_raw`: the time reduction and the cotangent on the signals are formed in HBM; what follows
        (the Hessian-vector product of force terms, their mixed second derivatives, what ``fn_params`` holds) is that method's."""
        return self.value_and_raw(spec, which, device)

    def signal_xcorr(self, spec):
        """(batch, 2 max_lag + 1) normalised cross-correlation of the signal pairs of an ``objective.CorrelationSpec`` over its lags (lag d
        at index d + max_lag), on the device-resident history of the last solve (any forward pass)."""
        return self.engine.signal_xcorr(*self._terms(spec.signal_spec), spec.pairs, spec.max_lag, spec.templates,
                                        spec.normalisation)

    def signal_xcorr_value(self, spec):
        """(J, peak, delay), (batch,) each, of an ``objective.CorrelationSpec`` on the device-resident history."""
        return self.value(spec)

    def signal_xcorr_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The cross-correlation objective (``objective.CorrelationSpec``) of the last kept solve, evaluated and differentiated on the
        device beside :meth:`signal_projection_value_and_raw`: the correlation over the lags, its reduction to a peak and a delay and the
        cotangent on the signals are formed in HBM; what follows is :meth:`signal_misfit_value_and_raw`'s.  Returns
        ((J, peak, delay), raw gradients)."""
        return self.value_and_raw(spec, which, device)

    def signal_spectrum(self, spec):
        """(N, D, l), (batch, G) each: the numerator and denominator forms of the groups of an ``objective.SpectrumSpec`` and their measures
        (N / D or ln N - ln D as the spec says; NaN where the measure does not exist), on the device-resident history of the last solve
        (any forward pass)."""
        out = self.engine.signal_spectrum(*self._terms(spec.signal_spec), spec.basis, spec.num_weights, spec.den_weights, spec.num_offset,
                                          spec.den_offset, spec.measure)
        return out[..., 0], out[..., 1], out[..., 2]

    def signal_spectrum_value(self, spec):
        """(J, l): the value (batch,) and the measures (batch, G) of an ``objective.SpectrumSpec`` on the device-resident history."""
        return self.value(spec)

    def signal_spectrum_value_and_raw(self, spec, which=("centroid_node_vectors", "void_angle0", "inertia"), device=False):
        """The spectral-ratio objective (``objective.SpectrumSpec``) of the last kept solve, evaluated and differentiated on the device
        beside :meth:`signal_projection_value_and_raw`: the band-power forms, their ratios, the aggregate over the groups and the cotangent
        on the signals are formed in HBM; what follows is :meth:`signal_misfit_value_and_raw`'s.  Returns ((J, l), raw gradients)."""
        return self.value_and_raw(spec, which, device)

    @staticmethod
    def _bond_params_bar(bp, kb, refv_bar, like):
        """Gradient tree with the structure of the bond parameters that were passed in (LigamentParams /
        StretchingTorsionalSpringParams / any NamedTuple with a subset of their fields)."""
        cols = {"k_stretch": 0, "k_shear": 1, "k_rot": 2}
        vals = {}
        for name in bp._fields:
            if name in cols:
                vals[name] = like(getattr(bp, name), kb[:, cols[name]])
            elif name == "reference_vector":
                vals[name] = refv_bar
            else:
                vals[name] = None
        return type(bp)(**vals)

    def _unflatten_grads(self, g, fields_bar):
        cps, flats, ts = self._last
        trees = []
        tab = (g.get("fn_table_values") or self._fn_table_grads()) if self._table_leaves else {}
        for m, (cp, flat) in enumerate(zip(cps, flats)):
            gp, mp = cp.geometrical_params, cp.mechanical_params
            cnv = flat["centroid_node_vectors"]
            cnv_bar = g["centroid_node_vectors"][m].copy()
            if self.spec.contact == _b.CONTACT_ANGLE:
                cnv_bar += void_angles0_vjp(cnv, self.bonds, g["void_angle0"][m])
            density_bar, inertia_bar = None, None
            if mp.inertia is None:
                vb, density_bar = compute_inertia_vjp(cnv, mp.density, g["inertia"][m])
                cnv_bar += vb
            else:
                inertia_bar = g["inertia"][m].reshape(np.shape(mp.inertia))
            kb = g["k_bond"][m]

            def like(x, full):
                return full.sum() if np.ndim(x) == 0 else full
            damping_bar = 0.0
            if self.damped_blocks is not None:
                rows = g["damping"][m][self.damped_blocks]
                damping_bar = rows.sum() if np.ndim(mp.damping) == 0 else rows.reshape(np.shape(mp.damping)) \
                    if np.shape(mp.damping) == rows.shape else rows.sum(0)
            contact_bar = None
            if self.spec.contact:
                c = g["contact"][m]
                contact_bar = ContactParams(min_angle=c[0], cutoff_angle=c[1], k_contact=c[2])
            con_bar, load_bar = {}, {}
            for f, term in enumerate(self.con_terms):
                term.scatter_grad(g["fn_params"][m][f], con_bar, cp.constraint_params)
            for f, term in enumerate(self.load_terms):
                term.scatter_grad(g["fn_params"][m][len(self.con_terms) + f], load_bar, cp.loading_params)
            for f, term, field in self._table_leaves:
                bar = con_bar if field == "constraint_params" else load_bar
                bar[term.values_name] = bar.get(term.values_name, 0.0) + tab[f][m]
            trees.append(ControlParams(
                geometrical_params=GeometricalParams(
                    block_centroids=(np.array(g["block_centroids"][m]).reshape(np.shape(gp.block_centroids)) if "block_centroids" in g
                                     else np.zeros_like(np.asarray(gp.block_centroids, dtype=float))),
                    centroid_node_vectors=cnv_bar),
                mechanical_params=MechanicalParams(
                    bond_params=self._bond_params_bar(mp.bond_params, kb, g["reference_vector"][m], like),
                    density=density_bar, inertia=inertia_bar, damping=damping_bar, contact_params=contact_bar),
                loading_params=load_bar, constraint_params=con_bar))
        state0_bar = g["state0"]
        if self.batch == 1:
            return trees[0], state0_bar[0]
        return trees, state0_bar


def setup_dynamic_solver(geometry, energy_fn, loaded_block_DOF_pairs=None, loading_fn=None,
                         constrained_block_DOF_pairs=np.array([]), constrained_DOFs_fn=zero,
                         damped_blocks=None, rtol: float = 1e-8, atol: float = 1e-8, *,
                         integrator: str = "dopri5", steps_per_interval: Optional[int] = None,
                         batch: int = 1, device: int = 0, streams: int = 0, grid_refine: int = 1, _lib=None):
    """Same positional/keyword arguments as ``difflexmm.dynamics.setup_dynamic_solver`` (dynamics.py:60-69).
    Keyword-only extras of this engine: ``steps_per_interval`` (fixed grid), ``batch``, ``device``, ``streams``, and ``grid_refine``:
    with ``keep_trajectory=True`` and no explicit grid the adaptive controller's accepted steps are frozen into the grid the reverse
    sweep differentiates; ``grid_refine = k`` splits each of them into k (accuracy knob of the gradient, see ``adaptive_grid``)."""
    return DynamicSolver(geometry, energy_fn, loaded_block_DOF_pairs, loading_fn, constrained_block_DOF_pairs,
                         constrained_DOFs_fn, damped_blocks, rtol, atol, integrator, steps_per_interval, batch, device, _lib, streams, grid_refine)


def linear_mode_analysis(displacement, geometry, energy_fn, control_params: ControlParams,
                         constrained_block_DOF_pairs=np.array([]), *, device: int = 0, _lib=None, return_stiffness=False):
    """Eigenvalues (squared angular frequencies) and eigenmodes of ``K q = w^2 M q`` around ``displacement`` -- same arguments and
    results as ``difflexmm.dynamics.linear_mode_analysis`` (dynamics.py:189-245): ``(eigenvalues (n_free,), modes (n_free, n_blocks, 3))``,
    every mode scaled to unit Euclidean norm, constrained DOFs zero.

    The reference takes ``jax.hessian`` of the constrained energy; here the stiffness matrix is assembled on the device from the
    engine's Hessian-vector hook (``dfx_rhs_vjp``): with no damping and no loading the acceleration is ``a = -M^-1 grad E``, so the
    cotangent ``e_j`` on acceleration ``j`` returns ``-K[j, :] / m_j`` in the position part -- ``batch`` rows per call.  The dense
    generalised eigenproblem then goes to ``scipy.linalg.eigh`` on the host, as in the reference."""
    import scipy.linalg
    pairs = np.asarray(constrained_block_DOF_pairs, dtype=np.int64).reshape(-1, 2)
    n = geometry.n_blocks
    free, _, _ = DOFsInfo(n, pairs)
    nf = len(free)
    B = int(min(64, max(nf, 1)))
    solver = setup_dynamic_solver(geometry, energy_fn, constrained_block_DOF_pairs=pairs, batch=B, device=device, _lib=_lib)
    flat = solver._flatten(control_params)
    solver.engine.set_params(**{k: np.broadcast_to(v, (B,) + np.shape(v)).copy() for k, v in flat.items()})
    inertia = np.asarray(flat["inertia"], dtype=float).reshape(-1)
    u = np.asarray(displacement, dtype=float).reshape(n, 3)
    y = np.zeros((B, 2, n, 3))
    y[:, 0] = u
    y[:, 0].reshape(B, -1)[:, solver.constrained_DOF_ids] = 0.0          # the constrained kinematics hold them at c(0) = 0
    K = np.zeros((nf, nf))
    for j0 in range(0, nf, B):
        rows = free[j0:j0 + B]
        lam = np.zeros((B, 2, n, 3))
        lam[:, 1].reshape(B, -1)[np.arange(len(rows)), rows] = 1.0
        y_bar, _ = solver.engine.rhs_vjp(y, 0.0, lam, which=())
        K[j0:j0 + len(rows)] = -inertia[rows, None] * y_bar[:len(rows), 0].reshape(len(rows), -1)[:, free]
    K = 0.5 * (K + K.T)
    eigenvalues, vectors = scipy.linalg.eigh(K, np.diag(inertia[free]))
    vectors = (vectors / np.linalg.norm(vectors, axis=0)).T                # row-wise, unit norm
    modes = np.zeros((nf, n * 3))
    modes[:, free] = vectors
    out = (eigenvalues, modes.reshape(nf, n, 3))
    return out + (K,) if return_stiffness else out
