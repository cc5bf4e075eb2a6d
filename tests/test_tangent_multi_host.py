"""Multi-direction forward mode, host side (no GPU): the declarations, the interface's refusals, the unit-tangent builder of ``jacfwd``,
the prescribed-DOF assembly ``jvp`` and ``jvp_multi`` share, and a build-time guard on the widest stage kernel.  The kernel side is
tests/test_gpu_tangent_multi.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import difflexmm_amd as dm
from difflexmm_amd import _binding as b
from difflexmm_amd.dynamics import JACFWD_LEAVES, _bcast, unit_tangent

from .common import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FAST = dict(amplitude=7.5, loading_rate=3000.0, input_delay=1e-5)
ENTRIES = ("dfx_forward_tangent_multi", "dfx_forward_tangent_dense_multi")


def _cpu_case(cpu_lib, lattice="quads", batch=1):
    c = Case(lattice, 4, True, True, seed=3, lib=cpu_lib, cutoff_deg=125.0 if lattice == "kagome" else 42.0, batch=batch)
    c.cp = c.cp._replace(constraint_params=dict(FAST))
    return c


def test_header_declares_the_entries_and_the_binding_lists_them(cpu_lib, hip_lib):
    text = open(os.path.join(ROOT, "include", "dfx.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in b.COMM_EXPORTS and name in b.EXPORTS and hasattr(hip_lib, name)
        assert not hasattr(cpu_lib, name)
    assert len(hip_lib.dfx_forward_tangent_multi.argtypes) == 13 and len(hip_lib.dfx_forward_tangent_dense_multi.argtypes) == 13
    for prop in ("has_forward_tangent_multi", "has_forward_tangent_dense_multi"):
        assert isinstance(getattr(b.Engine, prop), property)


def test_cpu_port_has_no_multi_direction_forward_mode(cpu_lib):
    c = _cpu_case(cpu_lib)
    ts = np.linspace(0.0, 1e-4, 3)
    y0 = np.zeros((2, 16, 3))
    assert not c.solver.engine.has_forward_tangent_multi and not c.solver.engine.has_forward_tangent_dense_multi
    for kw in (dict(steps_per_interval=2), dict(adaptive=True)):
        with pytest.raises(NotImplementedError, match="dfx_forward_tangent_multi"):
            c.solver.jvp_multi(y0, ts, c.cp, [(None, c.cp), (y0, None)], **kw)
        with pytest.raises(NotImplementedError, match="dfx_forward_tangent_multi"):
            c.solver.jacfwd(y0, ts, c.cp, ["k_stretch", "amplitude"], **kw)
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent_multi"):
        c.solver.engine.forward_tangent_multi(None, None, None, 2, ts, 2)
    with pytest.raises(NotImplementedError, match="dfx_forward_tangent_dense_multi"):
        c.solver.engine.forward_tangent_dense_multi(None, None, None, 2, ts, np.zeros((1, 1)), np.zeros(1, dtype=np.int64))


def test_argument_validation(cpu_lib):
    c = _cpu_case(cpu_lib, batch=3)
    ts = np.linspace(0.0, 1e-4, 3)
    y0 = np.zeros((2, 16, 3))
    # refused before any library call (the engine is not even looked at)
    engine, c.solver.engine = c.solver.engine, None
    try:
        with pytest.raises(ValueError, match="at least one"):
            c.solver.jvp_multi(y0, ts, c.cp, [], steps_per_interval=2)
        with pytest.raises(ValueError, match="pair"):
            c.solver.jvp_multi(y0, ts, c.cp, [c.cp], steps_per_interval=2)
        with pytest.raises(ValueError, match="expected 3 tangents, got 2"):
            c.solver.jvp_multi(y0, ts, c.cp, [(None, c.cp), (None, [c.cp, c.cp])], steps_per_interval=2)
        for kw in (dict(steps_per_interval=2), dict(steps_per_interval=2, step_times=np.linspace(0.0, 1e-4, 5))):
            with pytest.raises(ValueError, match="adaptive=True"):
                c.solver.jvp_multi(y0, ts, c.cp, [(None, c.cp)], adaptive=True, **kw)
            with pytest.raises(ValueError, match="adaptive=True"):
                c.solver.jacfwd(y0, ts, c.cp, ["k_rot"], adaptive=True, **kw)
        with pytest.raises(ValueError, match="per-member timepoints"):
            c.solver.jvp_multi(y0, np.stack([ts] * 3), c.cp, [(None, c.cp)], adaptive=True)
        c.solver.grid_refine = 2
        with pytest.raises(ValueError, match="grid_refine"):
            c.solver.jvp_multi(y0, ts, c.cp, [(None, c.cp)], adaptive=True)
        c.solver.grid_refine = 1
        c.solver.steps_per_interval = 4
        with pytest.raises(ValueError, match="default grid"):
            c.solver.jvp_multi(y0, ts, c.cp, [(None, c.cp)], adaptive=True)
    finally:
        c.solver.engine, c.solver.steps_per_interval, c.solver.grid_refine = engine, None, 1


def _hand_tree(c, name):
    """The unit tangent of one accepted name, written out leaf by leaf."""
    G, M, L, CP = dm.GeometricalParams, dm.MechanicalParams, dm.LigamentParams, dm.ContactParams
    mp = c.cp.mechanical_params
    one = lambda x: np.ones(np.shape(x)) if np.ndim(x) else 1.0        # noqa: E731
    geo0 = G(None, None)
    if name == "k_stretch":
        return dm.ControlParams(geo0, M(L(one(mp.bond_params.k_stretch), None, None, None), None))
    if name == "k_shear":
        return dm.ControlParams(geo0, M(L(None, one(mp.bond_params.k_shear), None, None), None))
    if name == "k_rot":
        return dm.ControlParams(geo0, M(L(None, None, one(mp.bond_params.k_rot), None), None))
    if name == "density":
        return dm.ControlParams(geo0, M(None, 1.0))
    if name == "damping":
        return dm.ControlParams(geo0, M(None, None, None, one(mp.damping)))
    if name == "min_angle":
        return dm.ControlParams(geo0, M(None, None, None, 0.0, CP(1.0, None, None)))
    if name == "cutoff_angle":
        return dm.ControlParams(geo0, M(None, None, None, 0.0, CP(None, 1.0, None)))
    if name == "k_contact":
        return dm.ControlParams(geo0, M(None, None, None, 0.0, CP(None, None, 1.0)))
    return dm.ControlParams(geo0, M(None, None), constraint_params={name: 1.0})


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
def test_unit_tangents_flatten_like_hand_written_trees(lattice, cpu_lib):
    c = _cpu_case(cpu_lib, lattice)
    nbd = len(c.bonds)
    bp = c.cp.mechanical_params.bond_params
    # (the Case's damping holds one value per DOF: no scalar leaf)
    with pytest.raises(ValueError, match="not a scalar leaf"):
        unit_tangent(c.cp, "damping")
    scalar = c.cp._replace(mechanical_params=c.cp.mechanical_params._replace(damping=3e-5))
    # one value over the bonds / over the damped blocks
    spread = c.cp._replace(mechanical_params=c.cp.mechanical_params._replace(
        bond_params=bp._replace(k_shear=np.full(nbd, float(bp.k_shear))), damping=np.full((c.geo.n_blocks, 1), 3e-5)))
    for cp in (scalar, spread):
        c.cp = cp
        for name in JACFWD_LEAVES + tuple(FAST):
            got = c.solver._flatten_tangent(cp, unit_tangent(cp, name))
            want = c.solver._flatten_tangent(cp, _hand_tree(c, name))
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (name, k)
            assert any(np.any(v != 0.0) for v in got.values()), name          # (a zero tangent would compare equal, too)
    # what is no scalar leaf, and what is no leaf at all
    with pytest.raises(ValueError, match="unknown leaf"):
        unit_tangent(c.cp, "k_strech")
    with pytest.raises(ValueError, match="unknown leaf"):
        unit_tangent(c.cp, "reference_vector")
    varied = bp._replace(k_rot=np.linspace(1.0, 2.0, nbd))
    with pytest.raises(ValueError, match="not a scalar leaf"):
        unit_tangent(c.cp._replace(mechanical_params=c.cp.mechanical_params._replace(bond_params=varied)), "k_rot")
    with pytest.raises(ValueError, match="no contact_params"):
        unit_tangent(c.cp._replace(mechanical_params=c.cp.mechanical_params._replace(contact_params=None)), "k_contact")
    with pytest.raises(ValueError, match="both"):
        unit_tangent(c.cp._replace(loading_params=dict(amplitude=1.0)), "amplitude")


def test_prescribed_rows_equal_the_loop_jvp_had(cpu_lib):
    """``_prescribed_tangent_rows`` (factored out of ``jvp``) against a restatement of the loop ``jvp`` carried."""
    c = _cpu_case(cpu_lib)
    s = c.solver
    rng = np.random.default_rng(0)
    ts = np.linspace(0.0, 3e-4, 7)
    cd = dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None),
                          constraint_params=dict(amplitude=0.3, loading_rate=-20.0, input_delay=1e-6))
    assert len(s.constrained_pairs) and s.con_terms
    start = rng.normal(size=(len(ts), 2, c.geo.n_blocks, 3))
    got = start.copy()
    s._prescribed_tangent_rows(got, c.cp, cd, ts)
    want = start.copy()
    n_con = len(s.constrained_pairs)
    dofs = s.constrained_pairs[:, 0] * 3 + s.constrained_pairs[:, 1]
    fdm = want.reshape(len(ts), 2, -1)
    fdm[:, :, dofs] = 0.0
    for term in s.con_terms:
        dp = term.resolve_jvp(c.cp.constraint_params, cd.constraint_params)
        if not np.any(dp):
            continue
        p = term.resolve(c.cp.constraint_params)
        vec = _bcast(term.vector, n_con)
        for k, t in enumerate(ts):
            fdm[k, 0, dofs] += vec * float(term.param_partials(float(t), p, "value") @ dp)
            fdm[k, 1, dofs] += vec * float(term.param_partials(float(t), p, "rate") @ dp)
    assert np.array_equal(got, want)
    assert np.abs(got.reshape(len(ts), 2, -1)[:, :, dofs]).max() > 0.0
    free = np.setdiff1d(np.arange(c.geo.n_blocks * 3), dofs)
    assert np.array_equal(got.reshape(len(ts), 2, -1)[:, :, free], start.reshape(len(ts), 2, -1)[:, :, free])
    # a zero tangent of the constraint parameters leaves zeros
    got0 = start.copy()
    s._prescribed_tangent_rows(got0, c.cp, dm.ControlParams(dm.GeometricalParams(None, None), dm.MechanicalParams(None, None)), ts)
    assert np.all(got0.reshape(len(ts), 2, -1)[:, :, dofs] == 0.0)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_widest_stage_kernel_has_no_scratch_traffic(tmp_path):
    """The widest shipped k_tan_stage_multi<nonlinear, angle contact, 4, KC>: no scratch instruction, no scratch segment (the rule the
    shipped widths were chosen by: profiles/r09_tangent_multi.txt)."""
    csrc = os.path.join(ROOT, "difflexmm_amd", "csrc")
    src = open(os.path.join(csrc, "engine_tangent.hip")).read()
    widths = [int(w) for w in re.search(r"constexpr int kWidths\[\] = \{([^}]*)\}", src).group(1).split(",")]
    kc = max(widths)
    hdr = open(os.path.join(csrc, "dfx_tangent.h")).read()
    assert int(re.search(r"constexpr int kTanMaxWidth = (\d+);", hdr).group(1)) == kc
    out = tmp_path / "tangent_multi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-disable-machine-licm", "-S", "--cuda-device-only",
                           "-o", str(out), os.path.join(csrc, "engine_tangent.hip")], stderr=subprocess.DEVNULL)
    txt = out.read_text()
    name = f"_ZN3dfx17k_tan_stage_multiILi1ELi1ELi4ELi{kc}EEEvNS_6TanCtxENS_7TableauENS_9TanStageME"
    i = txt.index("\n" + name + ":")
    body = [l.strip() for l in txt[i:txt.index(".Lfunc_end", i)].split("\n")]
    instrs = [l for l in body if l and not l.startswith((";", ".", "_")) and not l.endswith(":")]
    assert len(instrs) > 1000
    assert not any(x.startswith("scratch_") for x in instrs), f"k_tan_stage_multi<nonlinear, angle contact, 4, {kc}> spills to scratch"
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\n.*?\.private_segment_fixed_size:\s+(\d+)", txt, re.S)
    assert m and int(m.group(1)) == 0, m
    # the angle-contact and contact-free builds of every shipped width are free of it as well
    for w in widths:
        for contact in (0, 1):
            for npb in (3, 4):
                n2 = f"_ZN3dfx17k_tan_stage_multiILi1ELi{contact}ELi{npb}ELi{w}EEE"
                j = txt.index("\n" + n2)
                assert "scratch_" not in txt[j:txt.index(".Lfunc_end", j)], n2
