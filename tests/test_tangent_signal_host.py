"""The forward-mode signals without a GPU: the per-ligament evaluation ``tan_signal_lig`` (difflexmm_amd/csrc/dfx_tangent_signal.h -- the
function the kernel k_tan_signal_channels calls) in a g++ harness around the headers the kernels are compiled from, as
tests/test_signal_misfit_host.py does for the reverse-mode twin ``signal_lig_eps``.

All four bond models, with and without the angle contact; both void angles between 0.1 and 0.9 of the window of the penalty on every
draw (the draws of test_signal_misfit_host.py).  Per draw:
  1. the value part equals ``signal_lig_force``: 1e-15 of the largest entry (the same expressions on the same numbers);
  2. parameter tangents zero: ``w . dF(du) == du . (K w)`` with ``K w`` from ``signal_lig_eps`` -- the own rows from the own end of the
     ligament seeded with w, the partner rows from the partner's end (blocks and node vectors swapped, sgn flipped) seeded with w on its
     partner.  Two evaluations of the same second derivatives: 1e-12 (the bar of test_physics_hvp.py);
  3. du = 0 and one parameter tangent t at a time (own and partner node vector, reference vector, three stiffnesses, two void angles,
     three contact constants): ``w . dF == (mixed derivative of signal_lig_eps) * t``: 1e-12;
  4. the columns of the 2- and 4-wide evaluation, every tangent non-zero, equal the 1-wide evaluation of each direction: 1e-12 (the bar
     the suite holds K-wide columns to against the 1-wide kernel).
Scales: 1 and 4 the largest entry of the compared triple; 2 compares two dot products on the scale sum |a_i b_i| of the products that
were added (what the rounding error of a dot product is proportional to); 3 likewise, the scale taken over the group of parameters --
bond parameters, contact parameters -- as test_signal_misfit_host.py takes the largest entry of each group: the column of a node
vector of the linearized model is a difference of terms ~ k_stretch |r| that nearly cancel (1e-5 of them), and its rounding error is
proportional to those terms, not to what is left of them.
Worst cases seen (20000 draws per model and contact): value 0; symmetry 7.1e-16; parameters 1.7e-14; columns 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include "dfx_signal.h"
#include "dfx_tangent_signal.h"
using namespace dfx;
static double rnd(double a, double b) { return a + (b - a) * (double)rand() / RAND_MAX; }

// the same ligament seen from its other end
static SignalLigIn other_end(const SignalLigIn& in) {
  SignalLigIn q = in;
  q.o = in.p; q.p = in.o; q.rox = in.rpx; q.roy = in.rpy; q.rpx = in.rox; q.rpy = in.roy; q.sgn = -in.sgn;
  return q;
}
// parameter j of a TanSignalLigIn: own node vector, partner node vector, reference vector, stiffnesses, void angles, contact constants
template <int KC> static DualN<KC>& par(TanSignalLigIn<KC>& t, int j) {
  DualN<KC>* a[14] = {&t.rox, &t.roy, &t.rpx, &t.rpy, &t.lx, &t.ly, &t.ks, &t.ksh, &t.kr, &t.phi1, &t.phi2, &t.am, &t.ac, &t.kc};
  return *a[j];
}
template <int KC> static TanSignalLigIn<KC> lift(const SignalLigIn& in) {
  TanSignalLigIn<KC> t;
  t.o = in.o; t.p = in.p; t.sgn = in.sgn;
  for (int k = 0; k < KC; ++k) t.dox[k] = t.doy[k] = t.doth[k] = t.dpx[k] = t.dpy[k] = t.dpth[k] = 0.0;
  const double v[14] = {in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, in.ks, in.ksh, in.kr, in.phi1, in.phi2, in.am, in.ac, in.kc};
  for (int j = 0; j < 14; ++j) par<KC>(t, j) = DualN<KC>(v[j]);
  return t;
}
// one direction: tangents of the six DOFs and of the fourteen parameters
struct Dir { double du[6], dp[14]; };
template <int KC> static void seed(TanSignalLigIn<KC>& t, int k, const Dir& d) {
  t.dox[k] = d.du[0]; t.doy[k] = d.du[1]; t.doth[k] = d.du[2]; t.dpx[k] = d.du[3]; t.dpy[k] = d.du[4]; t.dpth[k] = d.du[5];
  for (int j = 0; j < 14; ++j) par<KC>(t, j).e[k] = d.dp[j];
}
template <int MODEL, int CONTACT> static void column(const SignalLigIn& in, const Dir& d, double* val, double* col) {
  TanSignalLigIn<1> t = lift<1>(in);
  seed<1>(t, 0, d);
  DualN<1> fx, fy, fth;
  tan_signal_lig<MODEL, CONTACT, 1>(t, fx, fy, fth);
  val[0] = fx.v; val[1] = fy.v; val[2] = fth.v; col[0] = fx.e[0]; col[1] = fy.e[0]; col[2] = fth.e[0];
}
template <int MODEL, int CONTACT, int KC> static double wide(const SignalLigIn& in, const Dir* dirs) {
  TanSignalLigIn<KC> t = lift<KC>(in);
  for (int k = 0; k < KC; ++k) seed<KC>(t, k, dirs[k]);
  DualN<KC> f[3];
  tan_signal_lig<MODEL, CONTACT, KC>(t, f[0], f[1], f[2]);
  double worst = 0.0;
  for (int k = 0; k < KC; ++k) {
    double val[3], col[3], s = 1e-300;
    column<MODEL, CONTACT>(in, dirs[k], val, col);
    for (int i = 0; i < 3; ++i) s = std::max(s, fabs(col[i]));
    for (int i = 0; i < 3; ++i) worst = std::max(worst, fabs(f[i].e[k] - col[i]) / s);
    for (int i = 0; i < 3; ++i) worst = std::max(worst, fabs(f[i].v - val[i]) / std::max(1e-300, fabs(val[i])));
  }
  return worst;
}
static double dot3(const double* a, const double* b, double& scale) {
  double s = 0.0;
  for (int i = 0; i < 3; ++i) { s += a[i] * b[i]; scale += fabs(a[i] * b[i]); }
  return s;
}
// worst[0]: value; [1]: symmetry; [2]: parameters; [3]: columns; [4]: draws with the penalty active on both void angles
template <int MODEL, int CONTACT> static void run(int n, double* worst) {
  for (int it = 0; it < n; ++it) {
    SignalLigIn in;
    auto fill = [&](BlockRec<double>& r) { r.x = rnd(-0.2, 0.2); r.y = rnd(-0.2, 0.2); r.th = rnd(-0.2, 0.2); r.sh = sin(0.5 * r.th); r.ch = cos(0.5 * r.th); };
    fill(in.o); fill(in.p);
    in.rox = rnd(1, 2); in.roy = rnd(-2, 2); in.rpx = -rnd(1, 2); in.rpy = rnd(-2, 2);
    in.lx = rnd(3.0, 4.0); in.ly = rnd(-1.0, 1.0); in.l0 = sqrt(in.lx * in.lx + in.ly * in.ly); in.il0 = 1.0 / in.l0;
    in.ks = rnd(50, 200); in.ksh = rnd(0.5, 3); in.kr = rnd(0.5, 3); in.sgn = (it & 1) ? 1.0 : -1.0;
    // both void angles inside the window of the penalty, |x| in [0.1, 0.9] of it: a = am + (0.1 .. 0.9) (ac - am)
    const double kap = in.sgn * (in.o.th - in.p.th);
    in.am = -0.26; in.ac = rnd(0.3, 0.8); in.kc = rnd(0.5, 3);
    in.phi1 = in.am + rnd(0.1, 0.9) * (in.ac - in.am) + kap;
    in.phi2 = in.am + rnd(0.1, 0.9) * (in.ac - in.am) - kap;
    {
      ContactGrad<double> cg;
      contact_grad<double>(kap, in.phi1, in.phi2, in.am, in.ac, in.kc, cg);
      if (cg.p1 != 0.0 && cg.p2 != 0.0) worst[4] += 1.0;
    }
    const double w[3] = {rnd(-1, 1), rnd(-1, 1), rnd(-1, 1)}, zero[3] = {0.0, 0.0, 0.0};
    // 1. the value part
    double ref[3];
    signal_lig_force<MODEL, CONTACT>(in, ref[0], ref[1], ref[2]);
    Dir d0 = {};
    double val[3], col[3], s = 1e-300;
    column<MODEL, CONTACT>(in, d0, val, col);
    for (int i = 0; i < 3; ++i) s = std::max(s, fabs(ref[i]));
    for (int i = 0; i < 3; ++i) worst[0] = std::max(worst[0], fabs(val[i] - ref[i]) / s);
    // K w: the own rows from this end, the partner rows from the other end
    SignalLigOut own, oth;
    signal_lig_eps<MODEL, CONTACT>(in, w, zero, own);
    signal_lig_eps<MODEL, CONTACT>(other_end(in), zero, w, oth);
    // 2. symmetry of the Hessian
    Dir d = {};
    for (int i = 0; i < 6; ++i) d.du[i] = rnd(-1, 1);
    column<MODEL, CONTACT>(in, d, val, col);
    double sc = 1e-300;
    const double lhs = dot3(w, col, sc);
    const double kwo[3] = {own.hx, own.hy, own.hth}, kwp[3] = {oth.hx, oth.hy, oth.hth};
    const double rhs = dot3(d.du, kwo, sc) + dot3(d.du + 3, kwp, sc);
    worst[1] = std::max(worst[1], fabs(lhs - rhs) / sc);
    // 3. one parameter tangent at a time
    const double mixed[14] = {own.rx, own.ry, oth.rx, oth.ry, own.q[0], own.q[1], own.q[2], own.q[3], own.q[4], own.p1, own.p2, own.q[5], own.q[6], own.q[7]};
    double lj[14], rj[14], sg[2] = {1e-300, 1e-300};
    for (int j = 0; j < (CONTACT ? 14 : 9); ++j) {
      Dir dj = {};
      dj.dp[j] = rnd(0.5, 1.5) * ((it + j) & 1 ? 1.0 : -1.0);
      column<MODEL, CONTACT>(in, dj, val, col);
      lj[j] = dot3(w, col, sg[j >= 9]);
      rj[j] = mixed[j] * dj.dp[j];
    }
    for (int j = 0; j < (CONTACT ? 14 : 9); ++j) worst[2] = std::max(worst[2], fabs(lj[j] - rj[j]) / sg[j >= 9]);
    // 4. wide columns: every tangent non-zero
    Dir dirs[4];
    for (int k = 0; k < 4; ++k) {
      for (int i = 0; i < 6; ++i) dirs[k].du[i] = rnd(-1, 1);
      for (int j = 0; j < 14; ++j) dirs[k].dp[j] = rnd(-0.1, 0.1);
    }
    worst[3] = std::max(worst[3], wide<MODEL, CONTACT, 2>(in, dirs));
    worst[3] = std::max(worst[3], wide<MODEL, CONTACT, 4>(in, dirs));
  }
}
template <int MODEL> static void both(int n) {
  double w[2][5] = {{0}};
  run<MODEL, 0>(n, w[0]); run<MODEL, 1>(n, w[1]);
  for (int c = 0; c < 2; ++c) printf("%d %d %.3e %.3e %.3e %.3e %.0f\n", MODEL, c, w[c][0], w[c][1], w[c][2], w[c][3], w[c][4]);
}
int main() {
  srand(17);
  const int n = 20000;
  both<kLinearized>(n); both<kNonlinear>(n); both<kSimpleSpring>(n); both<kStretchTorsion>(n);
  return 0;
}
"""

NAMES = ("linearized", "nonlinear", "simple_spring", "stretch_torsion")


def test_dual_number_force_tangent_against_the_reverse_mode_evaluation(tmp_path):
    src = tmp_path / "tan_signal_lig.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "tan_signal_lig"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "difflexmm_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    rows = [line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines()]
    assert len(rows) == 8
    for row in rows:
        model, contact = NAMES[int(row[0])], int(row[1])
        value, symmetry, params, columns, active = (float(x) for x in row[2:])
        print(f"[signal tangent] {model}, angle contact {contact}: value {value:.2e}, symmetry {symmetry:.2e}, parameter tangents "
              f"{params:.2e}, wide columns {columns:.2e}; draws with the penalty active {active:.0f}")
        assert active == 20000                         # the angle contact inside its window on every draw
        assert value <= 1e-15, (model, contact, value)
        assert 0.0 < symmetry < 1e-12, (model, contact, symmetry)
        assert 0.0 < params < 1e-12, (model, contact, params)
        assert columns < 1e-12, (model, contact, columns)
