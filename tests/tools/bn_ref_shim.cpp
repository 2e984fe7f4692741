// TEST INFRASTRUCTURE: a plain-int door to check_bn_ref of csrc/bn_ref_check.hpp for tests/test_bn_ref_cpu.py
// (c++ -O1 -shared -fPIC, no offload: the header is host code).  Returns 0, or MOPOE_ERR_ARG and the message the library
// would hand to mopoe_last_error().
#include "../../mopoe-mimic_amd/csrc/bn_ref_check.hpp"

// null_ref != 0: the reference itself is NULL.  present: bit 0 sums, 1 gamma, 2 beta, 3 rmean, 4 rvar (a set bit = a non-NULL
// pointer; nothing is read through it)
extern "C" int shim_check_bn_ref(int null_ref, int mode, int present, double inv_count, int C, int expected_C, int allow_mode3,
                                 const char* who, char* msg, int msg_n) {
  static const double d[1] = {0.0};
  static const float f[1] = {0.f};
  mopoe_bn_ref b;
  b.sums = (present & 1) ? d : nullptr;
  b.gamma = (present & 2) ? f : nullptr;
  b.beta = (present & 4) ? f : nullptr;
  b.rmean = (present & 8) ? f : nullptr;
  b.rvar = (present & 16) ? f : nullptr;
  b.inv_count = inv_count;
  b.eps = 1e-5f;
  b.C = C;
  b.mode = mode;
  return mopoe::check_bn_ref(null_ref ? nullptr : &b, expected_C, allow_mode3 != 0, who, msg, (size_t)msg_n);
}
