"""Every bond model x contact model (tests/model_matrix.py) through the CPU port of the engine: the twin of tests/test_gpu_model_matrix.py
without a GPU.  The port has one arm, no checkpoint levels and no build codes, and keeps the accepted adaptive steps for every physics
("adaptive-records"), so what is left is the harness itself -- the builder, its premises, the oracle twins of all 24 combinations and
every leaf of every model against torch.autograd -- and the port's own arithmetic for the pairs nothing else runs (linearised ligaments with
either contact, the springs with any contact)."""
import numpy as np
import pytest

from . import model_matrix as mm

TS = np.linspace(0.0, 3e-4, 3)
SPI = 8
TS_ADAPTIVE = np.linspace(0.0, 3e-4, 7)
GRID = [(lattice, model, contact) for lattice in ("quads", "kagome") for model in mm.MODELS for contact in mm.CONTACTS]
PAIRS = [(model, contact) for model in mm.MODELS for contact in mm.CONTACTS]
PER_BOND = [("quads", m, c) for m, c in mm.rotating_contacts(start=0)] + [("kagome", m, c) for m, c in mm.rotating_contacts(start=1)]
# (the oracle's replay of an adaptive solve is the slow part here: one case per model, contacts rotating; all 16 run in the GPU suite.
# Not torsion + distance on the kept steps, which only the port takes: the zero-length springs pull the hinges under the penalty's lower
# threshold, the cutoff gradient comes out at 2e-6 of the threshold's (a sum that cancels), and the ORACLE's own value moves by 1.8e-9 when state0 moves
# by 1e-15 -- RTOL_GRAD cannot be asked of that leaf there.  On the frozen grid, the path the HIP engine takes, it holds: 6.5e-11.)
ADAPTIVE = [("quads", 9, m, c) for m, c in mm.rotating_contacts(start=1)] + [("kagome", 5, "simple", "distance")]


def _ids(cases):
    return [mm.case_id(*c) if len(c) == 3 else mm.case_id(c[0], c[2], c[3]) for c in cases]


@pytest.mark.parametrize("lattice,model,contact", GRID, ids=_ids(GRID))
def test_fixed_grid_every_leaf_matches_the_oracle(cpu_lib, lattice, model, contact):
    mc = mm.ModelCase(lattice, model, contact, mm.SIZES[lattice], "uniform", lib=cpu_lib)
    mc.assert_partial_last_wave()
    errs = mm.compare(mc, mc.run_engine(TS, spi=SPI), mc.oracle(TS, spi=SPI))
    print("model_matrix: cpu port %s uniform: fields %.1e gradients %.1e" % ((mm.case_id(lattice, model, contact),) + mm.worst(errs)))


@pytest.mark.parametrize("lattice,model,contact", PER_BOND, ids=_ids(PER_BOND))
def test_per_ligament_stiffnesses_match_the_oracle(cpu_lib, lattice, model, contact):
    mc = mm.ModelCase(lattice, model, contact, mm.SIZES[lattice], "per_bond", lib=cpu_lib, seed=1)
    errs = mm.compare(mc, mc.run_engine(TS, spi=SPI), mc.oracle(TS, spi=SPI))
    print("model_matrix: cpu port %s per_bond: fields %.1e gradients %.1e" % ((mm.case_id(lattice, model, contact),) + mm.worst(errs)))


def test_per_bond_cases_cover_every_model_on_both_lattices_and_every_contact_twice():
    assert {(l, m) for l, m, _ in PER_BOND} == {(l, m) for l in ("quads", "kagome") for m in mm.MODELS}
    assert all(sum(c == contact for _, _, c in PER_BOND) >= 2 for contact in mm.CONTACTS)


@pytest.mark.parametrize("lattice", ["quads", "kagome"])
@pytest.mark.parametrize("model,contact", PAIRS, ids=[mm.case_id("e", m, c)[2:] for m, c in PAIRS])
def test_energy_matches_the_oracle(cpu_lib, lattice, model, contact):
    mm.ModelCase(lattice, model, contact, mm.SIZES[lattice], "uniform", lib=cpu_lib).check_energy()


@pytest.mark.parametrize("lattice,n,model,contact", ADAPTIVE, ids=_ids(ADAPTIVE))
def test_adaptive_call_matches_the_oracle(cpu_lib, lattice, n, model, contact):
    mc = mm.ModelCase(lattice, model, contact, n, "uniform", lib=cpu_lib, batch=1)
    e_plain, steps = mm.check_plain_adaptive(mc, TS_ADAPTIVE)
    eng, errs = mm.check_kept_adaptive(mc, TS_ADAPTIVE, "adaptive-records")
    print("model_matrix: cpu port %s adaptive: %d steps, plain fields %.1e; kept steps: fields %.1e gradients %.1e"
          % ((mm.case_id(lattice, model, contact), steps, e_plain) + mm.worst(errs)))
