// dfx_tangent_signal.h -- the per-ligament evaluation of the forward-mode signals (include/dfx.h: dfx_forward_tangent_signals_multi; kernels
// in dfx_tangent.h).  A force channel of a signal is dE/d(x, y, theta) of a listed block, so its tangent along a direction of the solve is
// K(u) du + (d grad_u E / dp) dp: the epsilon parts of ONE evaluation of bond_grad_p / contact_grad on DualN<KC> records seeded with the
// tangent history, with every parameter of the ligament carrying its tangents -- the arithmetic the tangent stage kernel runs for its own
// force, at an output time instead of a stage.
// Host and device: nothing here needs the GPU, so the function below is checked by a host program (tests/test_tangent_signal_host.py).
#pragma once
#include "dfx_dualn.h"

namespace dfx {

// what one side of a ligament reads: the two primal block records (half-angles as signal_load forms them), their KC tangents, and every
// parameter with its KC tangents: node vectors, reference vector, stiffnesses, void angles, contact constants
template <int KC>
struct TanSignalLigIn {
  BlockRec<double> o, p;
  double dox[KC], doy[KC], doth[KC], dpx[KC], dpy[KC], dpth[KC];
  DualN<KC> rox, roy, rpx, rpy, lx, ly, ks, ksh, kr, phi1, phi2, am, ac, kc;
  double sgn;
};

// value and KC epsilon parts of dE/d(x, y, theta) on the OWN block (a force channel is the sum of these over the block's slots);
// CONTACT == 1: the angle contact is part of E.  |l0| and 1 / |l0| follow the reference vector, as in the tangent stage.
template <int MODEL, int CONTACT, int KC>
DFX_HD void tan_signal_lig(const TanSignalLigIn<KC>& in, DualN<KC>& fx, DualN<KC>& fy, DualN<KC>& fth) {
  using D = DualN<KC>;
  const BlockRec<D> o = seed_rec<KC>(in.o, in.dox, in.doy, in.doth), p = seed_rec<KC>(in.p, in.dpx, in.dpy, in.dpth);
  const D l0 = tsqrt(in.lx * in.lx + in.ly * in.ly);
  const D il0 = 1.0 / l0;
  BondGrad<D> g;
  bond_grad_p<MODEL, D, D>(o, p, in.rox, in.roy, in.rpx, in.rpy, in.lx, in.ly, l0, il0, in.ks, in.ksh, in.kr, in.sgn, g);
  fx = g.fx; fy = g.fy; fth = g.fth;
  if (CONTACT == 1) {
    ContactGrad<D> cg;
    const D kap = in.sgn * (o.th - p.th);
    contact_grad<D, D>(kap, in.phi1, in.phi2, in.am, in.ac, in.kc, cg);
    fth = fth + in.sgn * cg.dkap;
  }
}

}  // namespace dfx
