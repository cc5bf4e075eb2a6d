"""Forward mode on non-uniform parameter images, host side (no GPU): the reference helpers of tests/parity.py that
tests/test_gpu_tangent_param_shapes.py compares the tangent kernels with, pinned with the oracle alone, and the premises of those tests.

  * ``oracle_param_jvp`` along the directions of ``shape_tangents`` is the transpose of ``oracle_param_leaves``:
    <fields_bar, fields_dot> == sum over the leaves of <gradient, tangent leaf> + <state0 gradient, state0_dot>, to 1e-10 relative (both
    sides are torch.autograd through the same oracle solve, one forward over reverse, one reverse).  This pins the mapping from the
    helper's tangent trees to oracle leaves -- the shape of a per-block damping tangent, inertia as a leaf of its own, the node vectors
    reaching the void angles -- before a kernel is involved.
  * every non-uniform image of the GPU tests moves the oracle's fields away from those of its uniform twin by more than 1e-6 relative
    (1e4 times the bar on the fields): a kernel that read the uniform arm of the image could not pass."""
import numpy as np
import pytest

from .common import relerr
from .param_shapes import ShapeCase
from .parity import (RTOL_TRAJ, _fields_bar, oracle_param_fields, oracle_param_jvp, oracle_param_leaves, shape_leaf_names, shape_tangents,
                     tangent_tree_of, uniform_twin)
from .test_gpu_param_shapes import FIXED, SIZES, SPI, TS

TANGENT_SEED = 5
# (the identity below is exact on any grid: the first quarter of TS at the same step size, four Dopri5 steps, keeps the oracle calls short)
HOST_TS, HOST_SPI = np.linspace(0.0, TS[-1] / 4, 3), SPI // 4


@pytest.mark.parametrize("shape,lattice,n", [("k_per_bond", "quads", 7), ("damping_per_block", "kagome", 5), ("mixed_batch_17", "kagome", 5)])
def test_oracle_jvp_is_the_transpose_of_the_oracle_gradients(cpu_lib, shape, lattice, n):
    sc = ShapeCase(shape, lattice, n, lib=cpu_lib, seed=1)
    dirs = shape_tangents(sc, TANGENT_SEED)
    grads = oracle_param_leaves(sc, HOST_TS, spi=HOST_SPI, expanded=True)
    jv = oracle_param_jvp(sc, HOST_TS, dirs, spi=HOST_SPI)
    free = sc.c.solver.free_DOF_ids
    fb = _fields_bar(sc, len(HOST_TS)).reshape(len(sc.members), len(HOST_TS), 2, -1)[:, :, :, free]
    for m, p in enumerate(sc.members):
        # (the same solve twice; the node vectors come from the NumPy geometry here and from its torch twin there: RTOL_TRAJ)
        assert relerr(jv[m]["fields"], grads[m]["fields"]) < RTOL_TRAJ
        for name in ("all", "leaf"):
            y0d, tree, tan = dirs[m][name]
            lhs = float(np.sum(fb[m] * jv[m][name]))
            rhs = 0.0
            for k, v in tan.items():
                g = grads[m][k]
                v = np.asarray(v, dtype=float)
                if k == "state0":
                    v = v.reshape(2, -1)[:, free]
                assert np.shape(g) == v.shape, (k, np.shape(g), v.shape)
                rhs += float(np.sum(g * v))
            gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
            print(shape, "member", m, name, "lhs", lhs, "rhs", rhs, "gap", gap)
            assert gap < 1e-10, (m, name, lhs, rhs, gap)
            # the tree says what the dict says
            if name == "leaf":
                assert sorted(tan) == sorted(shape_leaf_names(shape)) and y0d is None
                assert tree.geometrical_params.centroid_node_vectors is None and tree.mechanical_params.inertia is None
            else:
                assert y0d is tan["state0"] and tree.mechanical_params.inertia is tan["inertia"]
                assert tree.geometrical_params.centroid_node_vectors is tan["cnv"]
                assert tree.mechanical_params.contact_params.cutoff_angle == tan["cutoff_angle"]
            assert tree.mechanical_params.damping is tan.get("damping") and tree.mechanical_params.bond_params.reference_vector is tan.get("refv")
        assert np.shape(dirs[m]["all"][2]["damping"]) == np.shape(p["damping"])
    if shape == "damping_per_block":
        assert np.shape(dirs[0]["leaf"][2]["damping"]) == (len(sc.c.damped), 3) and len(sc.c.damped) < sc.c.geo.n_blocks
        # what the separate direction is for: the damping-only column is far below the all-leaf column
        assert np.abs(jv[0]["leaf"]).max() < 0.1 * np.abs(jv[0]["all"]).max()
    for m in range(len(sc.members)):
        assert np.abs(jv[m]["leaf"]).max() > 0.0


def test_tangent_tree_follows_jvps_rules(cpu_lib):
    """The engine-side flattening of a helper tree (DynamicSolver._flatten_tangent) puts every leaf where the oracle dict says it is:
    damping rows on the damped blocks only, stiffness tangents per ligament on a member whose stiffnesses are scalars."""
    sc = ShapeCase("damping_per_block", "kagome", 5, lib=cpu_lib, seed=1)
    s = sc.c.solver
    for m, cp in enumerate(sc.cps):
        y0d, tree, tan = shape_tangents(sc, TANGENT_SEED)[m]["all"]
        flat = s._flatten_tangent(cp, tree)
        want = np.zeros((sc.c.geo.n_blocks, 3))
        want[sc.c.damped] = tan["damping"]
        assert np.array_equal(flat["damping"], want)
        assert np.array_equal(flat["k_bond"], np.stack([tan["ks"], tan["ksh"], tan["kr"]], 1))
        assert np.array_equal(flat["reference_vector"], tan["refv"]) and np.array_equal(flat["inertia"], tan["inertia"])
        assert np.array_equal(flat["contact"], [tan["min_angle"], tan["cutoff_angle"], tan["k_contact"]])
        assert np.array_equal(flat["fn_params"][0][:3], [tan["amplitude"], tan["loading_rate"], tan["input_delay"]])
        _, only, _ = shape_tangents(sc, TANGENT_SEED)[m]["leaf"]
        flat1 = s._flatten_tangent(cp, only)
        assert np.array_equal(flat1["damping"], want)
        assert not any(np.any(v) for k, v in flat1.items() if k != "damping")
    # and a tree of nothing is a zero tangent
    assert not any(np.any(v) for v in s._flatten_tangent(sc.cps[0], tangent_tree_of(sc, {})[1]).values())


@pytest.mark.parametrize("shape,lattice", [sl for sl in FIXED if sl[0] != "uniform"])
def test_every_nonuniform_image_moves_the_oracles_fields(cpu_lib, shape, lattice):
    """The premise of the GPU tests, at their sizes and seed: the image differs from its uniform twin (the leaf the shape is named after
    replaced by its mean, or by the lattice's reference vectors) by more than 1e-6 of the fields."""
    sc = ShapeCase(shape, lattice, SIZES[lattice], lib=cpu_lib, seed=1)
    checked = 0
    for m, p in enumerate(sc.members):
        twin = uniform_twin(sc, m)
        if all(np.array_equal(np.broadcast_to(v, np.shape(p[k])), p[k]) for k, v in twin.items()):
            continue                    # (a member of a mixed batch that holds the lattice's own vectors)
        e = relerr(oracle_param_fields(sc, TS, SPI, m), oracle_param_fields(sc, TS, SPI, m, **twin))
        print(shape, lattice, "member", m, "fields against the uniform twin", e)
        assert e > 1e-6, (shape, lattice, m, e)
        checked += 1
    assert checked == (1 if shape.startswith(("refv", "mixed")) else len(sc.members)), checked
