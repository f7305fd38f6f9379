// mpe_ddmath_eval.h — ONE statement of "evaluate primitive `which` of mpe_ddmath.h at (a, b)".
//
// The kernel k_ddmath_batch (mpe_k3.hip, entry mpe_ddmath_batch) and the host scaffold of the CPU tier
// (tests/host/ddmath_host.cpp, through tests/host/stub) both call ddm::eval, so what the device runs and what the
// host tests pin cannot drift apart.  mpe_ddmath.h is a sequence of IEEE + - * / sqrt fma and exact scalings: two
// correct compilations agree bit for bit, and tests/test_ddmath_device.py holds the amdgcn build to the x86 build's
// bits.  The final rounding of the correctly rounded primitives hides a wrong last bit underneath it (a contracted
// a * b + c changes hypot_g, log1p_g, clog_g, cpow_g on 0.03 - 0.25 % of random arguments and log_cr .. pow_cr on none):
// the selectors therefore reach the literal restatements AND the unrounded double-double pairs.
#pragma once
#include "mpe_p3p.h"  // (csqrt_<true>; includes mpe_ddmath.h)

namespace mpe {
namespace ddm {

// Selectors.  Every one maps (a, b) to (out0, out1); a function of one argument ignores b, a function with one result
// leaves out1 = 0.  0 - 8 are numbered as ddm_compare of tests/host/ddmath_host.cpp always numbered them.
enum {
  EV_LOG = 0,        // log_cr(a)
  EV_LOG1P_CR = 1,   // log1p_cr(a)
  EV_EXP = 2,        // exp_cr(a)
  EV_SIN = 3,        // sincos_cr(a): the sine
  EV_COS = 4,        //               the cosine
  EV_HYPOT_G = 5,    // hypot_g(a, b)
  EV_ATAN2 = 6,      // atan2_cr(y = a, x = b)
  EV_POW = 7,        // pow_cr(a, b)
  EV_LOG1P_G = 8,    // log1p_g(a)
  EV_CLOG_G = 9,     // clog_g(re = a, im = b): (re, im)
  EV_CPOW_THIRD = 10,  // cpow_g(re = a, im = b, 1 / 3.): (re, im)
  EV_CPOW_2 = 11,    // cpow_g(.., 2.0)
  EV_CPOW_3 = 12,    // cpow_g(.., 3.0)
  EV_CSQRT_G = 13,   // csqrt_<true>({a, b}) of mpe_p3p.h: (re, im)
  EV_X2Y2M1_G = 14,  // x2y2m1_g(a, b)
  // the unrounded pairs (hi, lo).  Double-double operands are made of the two arguments by error-free transformations:
  // x = two_prod(a, b) (the exact product), y = two_sum(a, b) (the exact sum)
  EV_TWO_PROD = 15,  // x
  EV_ADD_DD = 16,    // add(x, y)
  EV_MUL_DD = 17,    // mul(x, y)
  EV_DIV_DD = 18,    // div(x, y)
  EV_SQRT_DD = 19,   // sqrt_dd(x), a b > 0
  EV_LOG_DD = 20,    // log_dd(x), a b > 0 and normal
  EV_EXP_DD = 21,    // exp_dd(x), |a b| < 700
  EV_ATAN_DD = 22,   // atan_dd(x), a b in [0, 1]
  EV_SIN_DD = 23,    // sincos_dd(a): the sine before to_double, |a| <= pi
  EV_COS_DD = 24,    //               the cosine
  EV_COUNT = 25
};

__device__ __forceinline__ void eval(int which, double a, double b, double& o0, double& o1) {
  o0 = o1 = 0.0;
  double s, c;
  dd r;
  switch (which) {
    case EV_LOG: o0 = log_cr(a); return;
    case EV_LOG1P_CR: o0 = log1p_cr(a); return;
    case EV_EXP: o0 = exp_cr(a); return;
    case EV_SIN: sincos_cr(a, s, c); o0 = s; return;
    case EV_COS: sincos_cr(a, s, c); o0 = c; return;
    case EV_HYPOT_G: o0 = hypot_g(a, b); return;
    case EV_ATAN2: o0 = atan2_cr(a, b); return;
    case EV_POW: o0 = pow_cr(a, b); return;
    case EV_LOG1P_G: o0 = log1p_g(a); return;
    case EV_CLOG_G: clog_g(a, b, o0, o1); return;
    case EV_CPOW_THIRD: cpow_g(a, b, 1.0 / 3.0, o0, o1); return;
    case EV_CPOW_2: cpow_g(a, b, 2.0, o0, o1); return;
    case EV_CPOW_3: cpow_g(a, b, 3.0, o0, o1); return;
    case EV_CSQRT_G: {
      const C2 z = csqrt_<true>(C2{a, b});
      o0 = z.re;
      o1 = z.im;
      return;
    }
    case EV_X2Y2M1_G: o0 = x2y2m1_g(a, b); return;
    case EV_TWO_PROD: r = two_prod(a, b); break;
    case EV_ADD_DD: r = add(two_prod(a, b), two_sum(a, b)); break;
    case EV_MUL_DD: r = mul(two_prod(a, b), two_sum(a, b)); break;
    case EV_DIV_DD: r = div(two_prod(a, b), two_sum(a, b)); break;
    case EV_SQRT_DD: r = sqrt_dd(two_prod(a, b)); break;
    case EV_LOG_DD: r = log_dd(two_prod(a, b)); break;
    case EV_EXP_DD: r = exp_dd(two_prod(a, b)); break;
    case EV_ATAN_DD: r = atan_dd(two_prod(a, b)); break;
    case EV_SIN_DD:
    case EV_COS_DD: {
      dd sd, cd;
      sincos_dd(a, sd, cd);
      r = which == EV_SIN_DD ? sd : cd;
      break;
    }
    default: return;
  }
  o0 = r.hi;
  o1 = r.lo;
}

}  // namespace ddm
}  // namespace mpe
