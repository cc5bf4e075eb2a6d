"""The signal misfit without a GPU: ``objective.SignalSpec`` validation, ``objective.host_signal_values`` against plain indexing of a random
history, and the per-ligament dual-number evaluation of the force terms (``signal_lig_eps``, difflexmm_amd/csrc/dfx_signal.h -- the function
the kernels k_signal_cotangent / k_signal_explicit call) in a g++ harness around the headers the kernels are compiled from, as
tests/test_physics_hvp.py does.

The harness seeds a random direction (w_o, w_p) on the six DOFs of a ligament's two blocks and compares every epsilon part -- of dE/du (the
Hessian-vector product), dE/dr (node vector), dE/dl (reference vector), dE/dk (three stiffnesses), dE/dphi (two void angles) and the three
contact constants -- with
  * central differences of bond_grad<double> / contact_grad<double> along the same seeds, for all four bond models and the angle contact
    inside its window (both void angles between 0.1 and 0.9 of it on every draw).  The two steps h = 1e-4 and 2h are extrapolated,
    (4 D(h) - D(2h)) / 3, which leaves a truncation error of h^4 |f^(5)| / 30 and a rounding error of about 2e-16 |f| / h = 2e-12 |f|.
    The draws keep what bounds them: the deformed ligament keeps a length >= 1.3 (higher derivatives of 1 / L are bounded), the penalty
    stays 0.1 of its window away from its poles (each derivative costs a factor <= 10 / D ~ 20: f^(5) / f' ~ 1e7, truncation ~ 3e-11), and
    the seeds turn the two blocks against each other (every contact entry is proportional to d kappa / d eps; a direction that leaves
    kappa fixed has no scale to measure against).  Bar: 1e-6 of the largest entry of each group, the bar of the directional-derivative
    tests of this suite (test_gpu_strain_objective.py); central differences in double precision do not test to 1e-12, the next check does.
  * bond_hvp / contact_hvp (the hand-derived second derivatives of the reverse stage) where those exist -- the two ligament models:
    dE/du with the contact's share of the moment row, dE/dr; the contact: dE/dphi.  Bar: test_physics_hvp.py's own, 1e-12.
Worst cases seen: central differences 2.4e-9 (bonds), 1.4e-9 (contact); hand-derived 8.9e-14 (bonds), 6.8e-16 (contact)."""
import os
import subprocess

import numpy as np
import pytest

from difflexmm_amd import objective as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SignalSpec --------------------------------------------------------------------------------------------------------------------------
def test_signal_spec_checks_shapes():
    terms = [(0, 3, 6, 1.5), (0, 4, 7, -2.0), (1, 3, 0, 1.0)]
    s = O.SignalSpec(terms, targets=np.zeros((5, 2)), omega=[1.0, 2.0], tau=np.ones(5))
    assert s.n_signals == 2 and s.has_force and s.terms[1] == (0, 4, 7, -2.0) and s.targets.shape == (5, 2)
    assert O.SignalSpec(terms, targets=np.zeros((3, 5, 2))).targets.shape == (3, 5, 2)
    assert not O.SignalSpec([(0, 1, 2, 1.0)]).has_force
    for bad in ([], [(0, 1, 2)], [(0, 1, 9, 1.0)], [(0, -1, 2, 1.0)], [(0, 1, 2, np.nan)], [(0.5, 1, 2, 1.0)], [(1, 1, 2, 1.0)]):
        with pytest.raises(ValueError):
            O.SignalSpec(bad)
    with pytest.raises(ValueError, match="signals without terms"):
        O.SignalSpec(terms, n_signals=3)
    with pytest.raises(ValueError, match="n_signals"):
        O.SignalSpec(terms, n_signals=1)
    with pytest.raises(ValueError, match="targets"):
        O.SignalSpec(terms, targets=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="targets"):
        O.SignalSpec(terms, targets=np.zeros(5))
    with pytest.raises(ValueError, match="omega"):
        O.SignalSpec(terms, targets=np.zeros((5, 2)), omega=np.ones(3))
    with pytest.raises(ValueError, match="tau"):
        O.SignalSpec(terms, targets=np.zeros((5, 2)), tau=np.ones(4))
    with pytest.raises(ValueError, match="tau"):
        O.SignalSpec(terms, tau=np.ones((2, 2)))


def test_signal_spec_constructors():
    f = O.SignalSpec.fields_of([(3, 0), (3, 2), (7, 1)], "velocity", targets=np.zeros((4, 3)))
    assert f.n_signals == 3 and f.terms == [(0, 3, 3, 1.0), (1, 3, 5, 1.0), (2, 7, 4, 1.0)] and not f.has_force
    d = O.SignalSpec.fields_of([(2, 1)])
    assert d.terms == [(0, 2, 1, 1.0)] and d.targets is None
    r = O.SignalSpec.force_sum([(5, 0), (6, 0), (6, 2)], scale=-2.5)
    assert r.n_signals == 1 and r.terms == [(0, 5, 6, -2.5), (0, 6, 6, -2.5), (0, 6, 8, -2.5)] and r.has_force
    r2 = r.with_targets(np.ones((6, 1)), omega=[0.5])
    assert r2.terms == r.terms and r2.targets.shape == (6, 1) and r2.omega[0] == 0.5 and r.targets is None
    for bad in ([], [(1, 3)], [(1, -1)]):
        with pytest.raises(ValueError):
            O.SignalSpec.force_sum(bad)
        with pytest.raises(ValueError):
            O.SignalSpec.fields_of(bad)
    with pytest.raises(ValueError, match="kind"):
        O.SignalSpec.fields_of([(1, 1)], "force")


def test_host_signal_values_equal_indexing_of_the_history():
    rng = np.random.default_rng(5)
    f = rng.normal(size=(3, 6, 2, 7, 3))
    bd = [(0, 0), (6, 2), (3, 1), (3, 0)]
    for kind, plane in (("displacement", 0), ("velocity", 1)):
        got = O.host_signal_values(O.SignalSpec.fields_of(bd, kind), f)
        want = np.stack([f[:, :, plane, b, d] for b, d in bd], -1)
        assert got.shape == (3, 6, 4) and np.array_equal(got, want)
    mixed = O.SignalSpec([(0, 2, 1, 2.0), (0, 5, 4, -0.5), (1, 2, 1, 1.0), (0, 2, 2, 0.25)])
    got = O.host_signal_values(mixed, f)
    want0 = 2.0 * f[:, :, 0, 2, 1] - 0.5 * f[:, :, 1, 5, 1] + 0.25 * f[:, :, 0, 2, 2]
    worst = float(np.abs(got[..., 0] - want0).max())
    print(f"[signal misfit] host_signal_values, a signal of three terms against indexing: {worst:.2e}")
    assert worst <= 1e-15 and np.array_equal(got[..., 1], f[:, :, 0, 2, 1])
    assert np.array_equal(O.host_signal_values(mixed, f[1]), got[1])                  # one member, no member axis
    with pytest.raises(ValueError, match="device only"):
        O.host_signal_values(O.SignalSpec.force_sum([(1, 0)]), f)
    with pytest.raises(ValueError, match="out of range"):
        O.host_signal_values(O.SignalSpec.fields_of([(7, 0)]), f)
    with pytest.raises(ValueError, match="fields must be"):
        O.host_signal_values(mixed, f[0, 0])


# ---- the per-ligament dual-number evaluation ----------------------------------------------------------------------------------------------
HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include "dfx_signal.h"
using namespace dfx;
static double rnd(double a, double b) { return a + (b - a) * (double)rand() / RAND_MAX; }
static void pack(const SignalLigOut& o, double* v) {
  v[0] = o.hx; v[1] = o.hy; v[2] = o.hth; v[3] = o.rx; v[4] = o.ry; v[5] = o.p1; v[6] = o.p2;
  for (int i = 0; i < 8; ++i) v[7 + i] = o.q[i];
}
// the same entries of the plain gradient at the configuration moved by s along the seeds
template <int MODEL, int CONTACT> static void grad_at(SignalLigIn in, const double* wo, const double* wp, double s, double* v) {
  auto move = [&](BlockRec<double>& r, const double* w) { r.x += s * w[0]; r.y += s * w[1]; r.th += s * w[2]; r.sh = sin(0.5 * r.th); r.ch = cos(0.5 * r.th); };
  move(in.o, wo); move(in.p, wp);
  BondGrad<double> g;
  bond_grad<MODEL, double>(in.o, in.p, in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, in.l0, in.il0, in.ks, in.ksh, in.kr, in.sgn, g);
  ContactGrad<double> cg;
  cg.dkap = cg.p1 = cg.p2 = cg.am = cg.ac = cg.kc = cg.e = 0.0;
  if (CONTACT) contact_grad<double>(in.sgn * (in.o.th - in.p.th), in.phi1, in.phi2, in.am, in.ac, in.kc, cg);
  const double q[15] = {g.fx, g.fy, g.fth + in.sgn * cg.dkap, g.rx, g.ry, cg.p1, cg.p2, g.lx, g.ly, g.ks, g.ksh, g.kr, cg.am, cg.ac, cg.kc};
  for (int i = 0; i < 15; ++i) v[i] = q[i];
}
// central differences with the steps h and 2h, extrapolated: (4 D(h) - D(2h)) / 3
template <int MODEL, int CONTACT> static void central(const SignalLigIn& in, const double* wo, const double* wp, double* d) {
  const double h = 1e-4;
  double a[15], b[15], c[15], e[15];
  grad_at<MODEL, CONTACT>(in, wo, wp, h, a); grad_at<MODEL, CONTACT>(in, wo, wp, -h, b);
  grad_at<MODEL, CONTACT>(in, wo, wp, 2 * h, c); grad_at<MODEL, CONTACT>(in, wo, wp, -2 * h, e);
  for (int i = 0; i < 15; ++i) d[i] = (4.0 * (a[i] - b[i]) / (2 * h) - (c[i] - e[i]) / (4 * h)) / 3.0;
}
// worst[0]: central differences, bond entries; [1]: central differences, contact entries; [2]: bond_hvp; [3]: contact_hvp; [4]: draws with the
// penalty active on both void angles
template <int MODEL> static void run(int n, double* worst) {
  for (int it = 0; it < n; ++it) {
    SignalLigIn in;
    auto fill = [&](BlockRec<double>& r) { r.x = rnd(-0.2, 0.2); r.y = rnd(-0.2, 0.2); r.th = rnd(-0.2, 0.2); r.sh = sin(0.5 * r.th); r.ch = cos(0.5 * r.th); };
    fill(in.o); fill(in.p);
    // node vectors of length <= 2.9 and rotations <= 0.2 move a node by <= 0.57, the blocks by <= 0.29 each: |dU| <= 1.7 against a ligament
    // of length >= 3, so the deformed ligament keeps a length >= 1.3 (a ligament shrunk to a point has unbounded higher derivatives)
    in.rox = rnd(1, 2); in.roy = rnd(-2, 2); in.rpx = -rnd(1, 2); in.rpy = rnd(-2, 2);
    in.lx = rnd(3.0, 4.0); in.ly = rnd(-1.0, 1.0); in.l0 = sqrt(in.lx * in.lx + in.ly * in.ly); in.il0 = 1.0 / in.l0;
    in.ks = rnd(50, 200); in.ksh = rnd(0.5, 3); in.kr = rnd(0.5, 3); in.sgn = (it & 1) ? 1.0 : -1.0;
    // rotation seeds of opposite sign, |d kappa / d eps| >= 0.25: every contact entry is proportional to it, and a direction that leaves
    // kappa almost fixed would measure rounding noise against a vanishing scale
    const double sw = (it & 2) ? 1.0 : -1.0;
    const double wo[3] = {rnd(-1, 1), rnd(-1, 1), sw * rnd(0.25, 1)}, wp[3] = {rnd(-1, 1), rnd(-1, 1), -sw * rnd(0, 1)};
    // both void angles inside the window of the penalty, |x| in [0.1, 0.9] of it: a = am + (0.1 .. 0.9) (ac - am)
    const double kap = in.sgn * (in.o.th - in.p.th);
    in.am = -0.26; in.ac = rnd(0.3, 0.8); in.kc = rnd(0.5, 3);
    in.phi1 = in.am + rnd(0.1, 0.9) * (in.ac - in.am) + kap;
    in.phi2 = in.am + rnd(0.1, 0.9) * (in.ac - in.am) - kap;
    SignalLigOut out;
    signal_lig_eps<MODEL, 1>(in, wo, wp, out);
    double got[15], fd[15], fdb[15], g0[15];
    pack(out, got);
    central<MODEL, 1>(in, wo, wp, fd); grad_at<MODEL, 1>(in, wo, wp, 0.0, g0);
    if (g0[5] != 0.0 && g0[6] != 0.0) worst[4] += 1.0;
    // without the contact: the bond entries alone (hth then holds no contact part)
    SignalLigOut ob;
    signal_lig_eps<MODEL, 0>(in, wo, wp, ob);
    double gotb[15];
    pack(ob, gotb);
    central<MODEL, 0>(in, wo, wp, fdb);
    const int bond_ids[10] = {0, 1, 2, 3, 4, 7, 8, 9, 10, 11}, contact_ids[5] = {5, 6, 12, 13, 14};
    double sb = 1e-300, sc = 1e-300;
    for (int i : bond_ids) sb = std::max(sb, fabs(gotb[i]));
    for (int i : bond_ids) worst[0] = std::max(worst[0], fabs(fdb[i] - gotb[i]) / sb);
    // the contact entries, and the contact's share of the moment row
    double cth = got[2] - gotb[2], cth_fd = fd[2] - fdb[2];
    for (int i : contact_ids) sc = std::max(sc, fabs(got[i]));
    sc = std::max(sc, fabs(cth));
    for (int i : contact_ids) worst[1] = std::max(worst[1], fabs(fd[i] - got[i]) / sc);
    worst[1] = std::max(worst[1], fabs(cth_fd - cth) / sc);
    if (MODEL == kNonlinear || MODEL == kLinearized) {
      BondHvp hv;
      constexpr int HM = (MODEL == kNonlinear || MODEL == kLinearized) ? MODEL : (int)kNonlinear;
      bond_hvp<HM>(in.o, in.p, wo[0], wo[1], wo[2], wp[0], wp[1], wp[2], in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, in.l0, in.il0, in.ks, in.ksh,
                   in.kr, in.sgn, hv);
      const double ref[5] = {hv.hx, hv.hy, hv.hth, hv.rx, hv.ry};
      double s = 1e-300;
      for (int i = 0; i < 5; ++i) s = std::max(s, fabs(ref[i]));
      for (int i = 0; i < 5; ++i) worst[2] = std::max(worst[2], fabs(gotb[i] - ref[i]) / s);
      // the moment row with the contact's share in it, on the scale of the bond entries (taking the difference of the two evaluations
      // instead would measure the cancellation of that difference)
      double dk, dke, p1e, p2e;
      contact_hvp(kap, in.sgn * (wo[2] - wp[2]), in.phi1, in.phi2, in.am, in.ac, in.kc, dk, dke, p1e, p2e);
      worst[2] = std::max(worst[2], fabs(got[2] - (hv.hth + in.sgn * dke)) / s);
    }
    double dk, dke, p1e, p2e;
    contact_hvp(kap, in.sgn * (wo[2] - wp[2]), in.phi1, in.phi2, in.am, in.ac, in.kc, dk, dke, p1e, p2e);
    const double cref[2] = {p1e, p2e}, cgot[2] = {got[5], got[6]};
    double s = 1e-300;
    for (int i = 0; i < 2; ++i) s = std::max(s, fabs(cref[i]));
    for (int i = 0; i < 2; ++i) worst[3] = std::max(worst[3], fabs(cgot[i] - cref[i]) / s);
  }
}
int main() {
  srand(11);
  const int n = 20000;
  double w[4][5] = {{0}};
  run<kLinearized>(n, w[0]); run<kNonlinear>(n, w[1]); run<kSimpleSpring>(n, w[2]); run<kStretchTorsion>(n, w[3]);
  for (int m = 0; m < 4; ++m) printf("%.3e %.3e %.3e %.3e %.0f\n", w[m][0], w[m][1], w[m][2], w[m][3], w[m][4]);
  return 0;
}
"""


def test_dual_number_ligament_evaluation_against_central_differences_and_the_hand_derived_hvp(tmp_path):
    src = tmp_path / "signal_lig.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "signal_lig"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "difflexmm_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    rows = [[float(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).strip().splitlines()]
    assert len(rows) == 4
    for name, (fd_bond, fd_contact, hvp_bond, hvp_contact, active) in zip(("linearized", "nonlinear", "simple_spring", "stretch_torsion"), rows):
        print(f"[signal misfit] {name}: central differences bonds {fd_bond:.2e} contact {fd_contact:.2e}; hand-derived hvp bonds {hvp_bond:.2e} "
              f"contact {hvp_contact:.2e}; draws with the penalty active {active:.0f}")
        assert active == 20000                         # the angle contact inside its window on every draw
        assert 0.0 < fd_bond < 1e-6 and 0.0 < fd_contact < 1e-6, (name, fd_bond, fd_contact)
        assert hvp_contact < 1e-12, (name, hvp_contact)
        if name in ("linearized", "nonlinear"):
            assert 0.0 < hvp_bond < 1e-12, (name, hvp_bond)
