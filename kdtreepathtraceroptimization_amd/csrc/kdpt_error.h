// kdpt_error.h -- the library's one error channel (host only).  Every non-OK return of an extern "C"
// entry point goes through fail(): it stores the message that kdpt_last_error() (include/kdpt.h) hands
// back to the calling thread, and returns the code.  The slot is a function-local thread_local in
// csrc/scene_host.cpp, the one translation unit every build of the library links, so the g++ and hipcc
// objects share it through fail() and kdpt_last_error(), never through a variable.
#pragma once
#include <string>

#include "../../include/kdpt.h"

namespace kdpt {
int fail(int code, const std::string& msg);
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

// A translation unit may name its stage before including this header (csrc/kd_build.hip does).
#ifndef KDPT_HIP_STAGE
#define KDPT_HIP_STAGE ""
#endif

namespace kdpt {
// KDPT_ERR_HIP with "<what>: <HIP's reason>"
inline int hip_fail(const char* what, hipError_t e) {
  return fail(KDPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace kdpt

#define HIP_TRY(expr)                                                  \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess) return ::kdpt::hip_fail(KDPT_HIP_STAGE #expr, e_); \
  } while (0)
#endif
