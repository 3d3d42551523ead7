// rnnt_host.h -- host-only helpers of the extern "C" entry points (rnnt*_entrypoint.hip): the status of a HIP error and the
// pointer alignment checks.  No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/rnnt.h"

static rnntStatus_t from_hip(hipError_t e) {
    if (e == hipSuccess) return RNNT_STATUS_SUCCESS;
    if (e == hipErrorInvalidValue) return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_EXECUTION_FAILED;
}

static bool aligned4(const void *p) { return (((uintptr_t)p) & 3) == 0; }
static bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
