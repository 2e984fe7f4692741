// Host-side validation of a mopoe_bn_ref, called by every entry point that takes one before anything is enqueued.
//
// Plain C++17 host code without a HIP type in it, as conv_launch.hpp: the host compiler builds it alone, and
// tests/test_bn_ref_cpu.py holds it against a restatement in Python on a machine without a GPU.  A kernel dereferences the
// pointers its mode names (common.hpp, bn_coef) without a check of its own, so a reference that would make it read through
// NULL has to come back as MOPOE_ERR_ARG here, not as a memory fault on the device.
#ifndef MOPOE_BN_REF_CHECK_HPP   // (guards rather than #pragma once: the header is also compiled alone)
#define MOPOE_BN_REF_CHECK_HPP
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/mopoe_hip.h"

namespace mopoe {

// `who`: entry point and argument ("mopoe_conv_fwd: bn_in").  NULL or mode 0 is "absent" and passes: an entry point that
// needs a BatchNorm refuses mode 0 itself.  Mode 3 (the activation form, mopoe_hip.h) passes only where `allow_mode3`.
inline int check_bn_ref(const mopoe_bn_ref* b, int C, bool allow_mode3, const char* who, char* msg, size_t n) {
  if (!b || b->mode == 0) return MOPOE_OK;
  const char* field = nullptr;
  if (b->mode < 0 || b->mode > 3) {
    snprintf(msg, n, "%s: mode %d is none of 0..3", who, b->mode);
    return MOPOE_ERR_ARG;
  }
  if (b->mode == 3 && !allow_mode3) {
    snprintf(msg, n, "%s: mode 3 (activation form) is accepted as relu_bn of mopoe_conv_dgrad* only", who);
    return MOPOE_ERR_ARG;
  }
  if (!b->gamma) field = "gamma";
  else if (!b->beta) field = "beta";
  else if (b->C != C) {
    snprintf(msg, n, "%s: C = %d, expected %d channels", who, b->C, C);
    return MOPOE_ERR_ARG;
  } else if (b->mode == 1) {
    if (!b->sums) field = "sums";
    else if (!(isfinite(b->inv_count) && b->inv_count > 0.0)) {
      snprintf(msg, n, "%s: mode 1 needs a finite inv_count > 0 (got %g)", who, b->inv_count);
      return MOPOE_ERR_ARG;
    }
  } else if (b->mode == 2) {
    if (!b->rmean) field = "rmean";
    else if (!b->rvar) field = "rvar";
  }
  if (field) {
    snprintf(msg, n, "%s: mode %d needs %s", who, b->mode, field);
    return MOPOE_ERR_ARG;
  }
  return MOPOE_OK;
}

}  // namespace mopoe
#endif
