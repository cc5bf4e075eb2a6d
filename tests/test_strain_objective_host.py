"""The host side of the ligament strain-energy objective (difflexmm_amd/objective.py): ``bond_weights_from_blocks``, the shape checks of
``StrainObjectiveSpec`` and the NumPy value ``host_strain_value`` against torch through ``oracle.ref_energy`` (tests/strain_yardstick.py) on
random fields of quads 4x4 and kagome 3x3.  Bar 1e-13 of the value: both sides are a few float64 operations per ligament and a sum of
~100 terms of one sign per part.  No engine involved."""
import numpy as np
import pytest

from difflexmm_amd import geometry as G
from difflexmm_amd import objective as O

from .strain_yardstick import T64, strain_objective

TOL = 1e-13


def _bonds_line():
    """three blocks of 4 nodes in a row: bonds 0-1, 1-2 and a second one 0-1"""
    return np.array([[1, 4], [5, 8], [2, 7]])


def test_bond_weights_both_and_any_ends():
    bonds = _bonds_line()
    both = O.bond_weights_from_blocks(bonds, 4, [[0, 1]], [2.0], ends="both")
    assert both.shape == (3,) and np.array_equal(both, [2.0, 0.0, 2.0])
    any_ = O.bond_weights_from_blocks(bonds, 4, [[0]], [2.0], ends="any")
    assert np.array_equal(any_, [2.0, 0.0, 2.0])
    assert np.array_equal(O.bond_weights_from_blocks(bonds, 4, [[0]], [2.0], ends="both"), [0.0, 0.0, 0.0])
    assert np.array_equal(O.bond_weights_from_blocks(bonds, 4, [[1]], [1.0], ends="any"), [1.0, 1.0, 1.0])
    assert np.array_equal(O.bond_weights_from_blocks(bonds, 4, [[0, 1]], [2.0]), both)          # "both" is the default


def test_bond_weights_overlapping_targets_add_and_members_stack():
    bonds = _bonds_line()
    w = O.bond_weights_from_blocks(bonds, 4, [[0, 1], [0, 1, 2]], [1.0, 0.5])
    assert np.array_equal(w, [1.5, 0.5, 1.5])
    wm = O.bond_weights_from_blocks(bonds, 4, [[0, 1], [1, 2]], [[1.0, 2.0], [-0.5, 0.25]])
    assert wm.shape == (2, 3) and np.array_equal(wm, [[1.0, 2.0, 1.0], [-0.5, 0.25, -0.5]])


def test_bond_weights_refusals():
    bonds = _bonds_line()
    with pytest.raises(ValueError, match="out of range"):
        O.bond_weights_from_blocks(bonds, 4, [[0, 3]], [1.0])
    with pytest.raises(ValueError, match="out of range"):
        O.bond_weights_from_blocks(bonds, 4, [[-1]], [1.0])
    with pytest.raises(ValueError, match="weights must be"):
        O.bond_weights_from_blocks(bonds, 4, [[0], [1]], [1.0])
    with pytest.raises(ValueError, match="ends must be"):
        O.bond_weights_from_blocks(bonds, 4, [[0]], [1.0], ends="either")


def test_spec_shape_errors():
    s = O.StrainObjectiveSpec([1.0, 0.0, 2.0])
    assert s.bond_weights.shape == (3,) and s.time_weights is None and s.parts == (1.0, 1.0, 1.0, 0.0)
    s = O.StrainObjectiveSpec(np.ones((2, 3)), [0.0, 1.0], (0, 0.5, 2, 1.5))
    assert s.bond_weights.shape == (2, 3) and s.time_weights.shape == (2,) and s.parts == (0.0, 0.5, 2.0, 1.5)
    with pytest.raises(ValueError, match="bond_weights"):
        O.StrainObjectiveSpec(np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match="bond_weights"):
        O.StrainObjectiveSpec(1.0)
    with pytest.raises(ValueError, match="time_weights"):
        O.StrainObjectiveSpec(np.ones(3), np.ones((2, 2)))
    with pytest.raises(ValueError, match="parts"):
        O.StrainObjectiveSpec(np.ones(3), None, (1, 1, 1))
    with pytest.raises(ValueError, match="parts"):
        O.StrainObjectiveSpec(np.ones(3), None, (1, 1, np.nan, 0))


def _lattice(name):
    rng = np.random.default_rng(5)
    if name == "quads":
        geo = G.QuadGeometry(4, 4, 15.0, 2.25)
        base = geo.get_design_from_rotated_square(25 * np.pi / 180)
        design = tuple(b + rng.uniform(-0.3, 0.3, b.shape) for b in base)
    else:
        basis = 20.0 * np.array([[1.0, 0.0], [np.cos(np.pi / 3), np.sin(np.pi / 3)]])
        geo = G.KagomeGeometry(3, 3, basis, 2.25)
        design = tuple(rng.uniform(-0.3, 0.3, s) for s in geo.design_shapes())
    return geo, geo.centroid_node_vectors(*design), geo.bond_connectivity(), geo.reference_bond_vectors()


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
@pytest.mark.parametrize("parts", [(1, 1, 1, 0), (1, 0, 0, 0), (0, 0.5, 2, 0)])
def test_host_value_against_torch_through_the_oracle(lattice, parts):
    geo, cnv, bonds, refv = _lattice(lattice)
    rng = np.random.default_rng(21)
    B, T, nb, nbd = 2, 4, geo.n_blocks, len(bonds)
    fields = rng.normal(size=(B, T, 2, nb, 3)) * np.array([0.4, 0.4, 0.15])
    w = rng.normal(size=(B, nbd)) * (rng.random((B, nbd)) < 0.4)
    tau = np.array([0.0, 1.0, 0.37, 2.0])
    ks, ksh = 120.0 * (1 + 0.1 * rng.uniform(-1, 1, nbd)), 1.19
    kr = 1.5 * (1 + 0.1 * rng.uniform(-1, 1, nbd))
    refv = np.broadcast_to(refv, (nbd, 2)) * (1 + 0.05 * rng.uniform(-1, 1, (nbd, 1)))
    spec = O.StrainObjectiveSpec(w, tau, parts)
    mine = O.host_strain_value(spec, fields, cnv, bonds, refv, ks, ksh, kr)
    assert mine.shape == (B,)
    ref = np.array([strain_objective(T64(fields[m, :, 0]), T64(cnv), bonds, T64(refv), T64(ks), T64(ksh), T64(kr), T64(w[m]), T64(tau), parts).item()
                    for m in range(B)])
    err = np.abs(mine - ref).max() / np.abs(ref).max()
    print(f"[strain objective] host value vs torch, {lattice} parts={parts}: {err:.2e}")
    assert np.abs(ref).min() > 0 and err <= TOL
    # one member without the member axis, shared weights, no time weights
    one = O.host_strain_value(O.StrainObjectiveSpec(w[0], None, parts), fields[1], cnv, bonds, refv, ks, ksh, kr)
    ref1 = strain_objective(T64(fields[1, :, 0]), T64(cnv), bonds, T64(refv), T64(ks), T64(ksh), T64(kr), T64(w[0]), T64(np.ones(T)), parts).item()
    assert isinstance(one, float) and abs(one - ref1) <= TOL * abs(ref1)


def test_host_value_refusals():
    geo, cnv, bonds, refv = _lattice("quads")
    fields = np.zeros((3, 2, geo.n_blocks, 3))
    with pytest.raises(ValueError, match="contact part"):
        O.host_strain_value(O.StrainObjectiveSpec(np.ones(len(bonds)), None, (1, 1, 1, 1)), fields, cnv, bonds, refv, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="bond_weights"):
        O.host_strain_value(O.StrainObjectiveSpec(np.ones(len(bonds) + 1)), fields, cnv, bonds, refv, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="time_weights"):
        O.host_strain_value(O.StrainObjectiveSpec(np.ones(len(bonds)), np.ones(4)), fields, cnv, bonds, refv, 1.0, 1.0, 1.0)


def test_the_entries_are_exports_of_the_hip_library(hip_lib):
    """HIP-library-only exports of include/dfx.h, like the other objective entries: an engine on a library without them says so."""
    import difflexmm_amd._binding as b
    for name in ("dfx_strain_objective_value", "dfx_strain_objective_value_and_grad"):
        assert name in b.COMM_EXPORTS and name in b.EXPORTS and hasattr(hip_lib, name)
