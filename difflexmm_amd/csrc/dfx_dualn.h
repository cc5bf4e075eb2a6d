// dfx_dualn.h -- the first-order forward-mode number with K epsilon parts that the tangent solve (dfx_tangent.h) and the per-ligament
// evaluation of the signal tangents (dfx_tangent_signal.h) instantiate the physics templates of dfx_physics.h with.  Host and device:
// nothing here needs the GPU.  DFX_DN_EACH (a loop over the K epsilon parts of the enclosing scope) stays defined for the headers that
// include this one; dfx_tangent.h drops it at its end.
#pragma once
#include "dfx_physics.h"

namespace dfx {

// ---------------------------------------------------------------------------------------
// first-order forward-mode number with K epsilon parts
// ---------------------------------------------------------------------------------------
template <int K>
struct DualN {
  double v, e[K];
  DFX_HD DualN() : v(0.0) {
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = 0.0;
  }
  DFX_HD DualN(double a) : v(a) {
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = 0.0;
  }
};
#define DFX_DN_EACH _Pragma("unroll") for (int k = 0; k < K; ++k)
template <int K> DFX_HD DualN<K> operator+(DualN<K> a, DualN<K> b) { DualN<K> r; r.v = a.v + b.v; DFX_DN_EACH r.e[k] = a.e[k] + b.e[k]; return r; }
template <int K> DFX_HD DualN<K> operator-(DualN<K> a, DualN<K> b) { DualN<K> r; r.v = a.v - b.v; DFX_DN_EACH r.e[k] = a.e[k] - b.e[k]; return r; }
template <int K> DFX_HD DualN<K> operator-(DualN<K> a) { DualN<K> r; r.v = -a.v; DFX_DN_EACH r.e[k] = -a.e[k]; return r; }
template <int K> DFX_HD DualN<K> operator*(DualN<K> a, DualN<K> b) {
  DualN<K> r; r.v = a.v * b.v; DFX_DN_EACH r.e[k] = a.v * b.e[k] + a.e[k] * b.v; return r;
}
template <int K> DFX_HD DualN<K> operator*(double a, DualN<K> b) { DualN<K> r; r.v = a * b.v; DFX_DN_EACH r.e[k] = a * b.e[k]; return r; }
template <int K> DFX_HD DualN<K> operator*(DualN<K> a, double b) { DualN<K> r; r.v = a.v * b; DFX_DN_EACH r.e[k] = a.e[k] * b; return r; }
template <int K> DFX_HD DualN<K> operator+(DualN<K> a, double b) { a.v = a.v + b; return a; }
template <int K> DFX_HD DualN<K> operator+(double a, DualN<K> b) { b.v = a + b.v; return b; }
template <int K> DFX_HD DualN<K> operator-(DualN<K> a, double b) { a.v = a.v - b; return a; }
template <int K> DFX_HD DualN<K> operator-(double a, DualN<K> b) { DualN<K> r; r.v = a - b.v; DFX_DN_EACH r.e[k] = -b.e[k]; return r; }
template <int K> DFX_HD DualN<K> operator/(DualN<K> a, DualN<K> b) {
  const double r = 1.0 / b.v, q = a.v * r;
  DualN<K> o; o.v = q; DFX_DN_EACH o.e[k] = (a.e[k] - q * b.e[k]) * r; return o;
}
template <int K> DFX_HD DualN<K> operator/(double a, DualN<K> b) {
  const double r = 1.0 / b.v, q = a * r;
  DualN<K> o; o.v = q; DFX_DN_EACH o.e[k] = -q * b.e[k] * r; return o;
}

// what the physics templates look up by argument type
template <int K> DFX_HD double val(DualN<K> a) { return a.v; }
template <int K> DFX_HD double eps(DualN<K> a, int k) { return a.e[k]; }
template <int K> DFX_HD DualN<K> trcp(DualN<K> a) {
  const double r = trcp(a.v);
  DualN<K> o; o.v = r; DFX_DN_EACH o.e[k] = -a.e[k] * r * r; return o;
}
template <int K> DFX_HD DualN<K> tsqrt(DualN<K> a) {
  const double s = sqrt(a.v);
  DualN<K> o; o.v = s; DFX_DN_EACH o.e[k] = 0.5 * a.e[k] / s; return o;
}
template <int K> DFX_HD DualN<K> trsqrt(DualN<K> a) {
  const double r = trsqrt(a.v);
  DualN<K> o; o.v = r; DFX_DN_EACH o.e[k] = -0.5 * a.e[k] * r * r * r; return o;
}
template <int K> DFX_HD DualN<K> tatan2(DualN<K> y, DualN<K> x) {
  const double w = trcp(x.v * x.v + y.v * y.v);
  DualN<K> o; o.v = fast_atan2(y.v, x.v); DFX_DN_EACH o.e[k] = (x.v * y.e[k] - y.v * x.e[k]) * w; return o;
}
template <int K> DFX_HD DualN<K> twrap(DualN<K> a) { a.v = twrap(a.v); return a; }

// seed_rec for K directions: the half-angle pair follows theta in every one
template <int K>
DFX_HD BlockRec<DualN<K>> seed_rec(const BlockRec<double>& r, const double (&wx)[K], const double (&wy)[K], const double (&wth)[K]) {
  BlockRec<DualN<K>> d;
  d.x.v = r.x; d.y.v = r.y; d.th.v = r.th; d.ch.v = r.ch; d.sh.v = r.sh;
  DFX_DN_EACH {
    d.x.e[k] = wx[k]; d.y.e[k] = wy[k]; d.th.e[k] = wth[k];
    d.ch.e[k] = -0.5 * r.sh * wth[k];
    d.sh.e[k] = 0.5 * r.ch * wth[k];
  }
  return d;
}

}  // namespace dfx
