// Host build of rpg_monocular_pose_estimator_amd/csrc/mpe_ddmath.h (test scaffolding, CPU tier): the device source of
// the libstdc++ / glibc restatement, against THIS image's libm / libstdc++ — the arithmetic the CPU oracle runs on.
// The "mine" side of every entry goes through ddm::eval (csrc/mpe_ddmath_eval.h), the function k_ddmath_batch runs
// per lane on the device.
#include <complex>
#include <cstddef>
#include "mpe_ddmath_eval.h"
using namespace mpe::ddm;

// every selector of mpe_ddmath_eval.h: out = n x (out0, out1), as mpe_ddmath_batch lays it out
extern "C" int ddm_eval_count() { return EV_COUNT; }
extern "C" void ddm_eval(int which, const double* a, const double* b, int n, double* out) {
  for (int i = 0; i < n; ++i) eval(which, a[i], b[i], out[2 * i], out[2 * i + 1]);
}

// which: 0 log, 1 log1p, 2 exp, 3 sin, 4 cos, 5 hypot(x, y), 6 atan2(y = a, x = b), 7 pow(a, b), 8 log1p restated literally
// out_mine / out_libm: n doubles each
extern "C" void ddm_compare(int which, const double* a, const double* b, int n, double* mine, double* libm) {
  if (which < 0 || which > 8) which = 7;
  for (int i = 0; i < n; ++i) {
    double unused;
    eval(which, a[i], b[i], mine[i], unused);
    switch (which) {
      case 0: libm[i] = std::log(a[i]); break;
      case 1: libm[i] = std::log1p(a[i]); break;
      case 2: libm[i] = std::exp(a[i]); break;
      case 3: libm[i] = std::sin(a[i]); break;
      case 4: libm[i] = std::cos(a[i]); break;
      case 5: libm[i] = std::hypot(a[i], b[i]); break;
      case 6: libm[i] = std::atan2(a[i], b[i]); break;
      case 8: libm[i] = std::log1p(a[i]); break;
      default: libm[i] = std::pow(a[i], b[i]); break;
    }
  }
}
// clog and pow(complex, double): mine / lib hold (re, im) pairs
extern "C" void ddm_clog(const double* re, const double* im, int n, double* mine, double* lib) {
  for (int i = 0; i < n; ++i) {
    eval(EV_CLOG_G, re[i], im[i], mine[2 * i], mine[2 * i + 1]);
    const std::complex<double> l = std::log(std::complex<double>(re[i], im[i]));
    lib[2 * i] = l.real();
    lib[2 * i + 1] = l.imag();
  }
}
// y: 1 / 3., 2.0 or 3.0 (the three exponents of p3p.cpp:262-268, one selector each)
extern "C" void ddm_cpow(const double* re, const double* im, double y, int n, double* mine, double* lib) {
  // (y reaches std::pow through a volatile, as a run-time value: the library call the oracle's TU makes)
  volatile double yv = y;
  const int which = y == 2.0 ? EV_CPOW_2 : y == 3.0 ? EV_CPOW_3 : EV_CPOW_THIRD;
  for (int i = 0; i < n; ++i) {
    eval(which, re[i], im[i], mine[2 * i], mine[2 * i + 1]);
    const double yy = yv;
    const std::complex<double> p = std::pow(std::complex<double>(re[i], im[i]), yy);
    lib[2 * i] = p.real();
    lib[2 * i + 1] = p.imag();
  }
}
