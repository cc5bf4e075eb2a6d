// dfx_signal.h -- the per-ligament evaluation of the signal misfit (include/dfx.h: dfx_signal_misfit_value_and_grad; kernels in
// dfx_objective.h).  A force channel of a signal is dE/d(x, y, theta) of a listed block, so the cotangent of the misfit on the fields is a
// Hessian-vector product K(u_k) w and its explicit parameter terms are the mixed derivatives d(w . grad_u E)/dp, with w the direction
// sum coef * c supported on the listed force DOFs.  Both are the epsilon parts of ONE evaluation of bond_grad / contact_grad on Dual
// records seeded with w (dfx_physics.h), as the reverse stage takes them for its own direction.
// Host and device: nothing here needs the GPU, so the function below is checked by a host program (tests/test_signal_misfit_host.py).
#pragma once
#include "dfx_physics.h"

namespace dfx {

// what one side of a ligament reads: the two block records, node vectors, reference vector, stiffnesses, void angles, contact constants
struct SignalLigIn {
  BlockRec<double> o, p;
  double rox, roy, rpx, rpy, lx, ly, l0, il0, ks, ksh, kr, phi1, phi2, am, ac, kc, sgn;
};

// epsilon parts along (wo, wp) of everything the OWN end of the ligament owns
struct SignalLigOut {
  double hx, hy, hth;    // (K w) on the own block's DOFs: d/d eps of dE/d(x, y, theta)
  double rx, ry;         // d/d eps of dE/d(own node vector)
  double p1, p2;         // d/d eps of dE/d(phi1, phi2)
  double q[8];           // d/d eps of dE/d(lx, ly, k_stretch, k_shear, k_rot, min_angle, cutoff_angle, k_contact)
};

// seeds in (wo on the own block's x, y, theta; wp on the partner's), epsilon parts out; CONTACT == 1: the angle contact is part of E
template <int MODEL, int CONTACT>
DFX_HD void signal_lig_eps(const SignalLigIn& in, const double* wo, const double* wp, SignalLigOut& out) {
  const BlockRec<Dual> od = seed_rec(in.o, wo[0], wo[1], wo[2]), pd = seed_rec(in.p, wp[0], wp[1], wp[2]);
  BondGrad<Dual> g;
  bond_grad<MODEL, Dual>(od, pd, in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, in.l0, in.il0, in.ks, in.ksh, in.kr, in.sgn, g);
  out.hx = g.fx.e; out.hy = g.fy.e; out.hth = g.fth.e;
  out.rx = g.rx.e; out.ry = g.ry.e;
  out.q[0] = g.lx.e; out.q[1] = g.ly.e; out.q[2] = g.ks.e; out.q[3] = g.ksh.e; out.q[4] = g.kr.e;
  out.p1 = out.p2 = out.q[5] = out.q[6] = out.q[7] = 0.0;
  if (CONTACT == 1) {
    ContactGrad<Dual> cg;
    contact_grad<Dual>(in.sgn * (od.th - pd.th), in.phi1, in.phi2, in.am, in.ac, in.kc, cg);
    out.hth += in.sgn * cg.dkap.e;
    out.p1 = cg.p1.e; out.p2 = cg.p2.e;
    out.q[5] = cg.am.e; out.q[6] = cg.ac.e; out.q[7] = cg.kc.e;
  }
}

// the value side of the same ligament: dE/d(x, y, theta) of the own block (a force channel is the sum of these over the block's slots)
template <int MODEL, int CONTACT>
DFX_HD void signal_lig_force(const SignalLigIn& in, double& fx, double& fy, double& fth) {
  BondGrad<double> g;
  bond_grad<MODEL, double>(in.o, in.p, in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, in.l0, in.il0, in.ks, in.ksh, in.kr, in.sgn, g);
  fx = g.fx; fy = g.fy; fth = g.fth;
  if (CONTACT == 1) {
    ContactGrad<double> cg;
    contact_grad<double>(in.sgn * (in.o.th - in.p.th), in.phi1, in.phi2, in.am, in.ac, in.kc, cg);
    fth += in.sgn * cg.dkap;
  }
}

}  // namespace dfx
