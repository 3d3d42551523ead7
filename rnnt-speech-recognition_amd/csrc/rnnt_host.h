// rnnt_host.h -- host-only helpers of the extern "C" entry points (rnnt*_entrypoint.hip): the status of a HIP error and the
// pointer alignment checks, and the vocabulary size the aligners' _path entry points hand to their shared checks.  No device code.
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

// A vocabulary size that holds `blank` and passes the V >= 2 check, for the _path entry points, which take no alphabet_size.  No
// such int exists from INT_MAX - 1 up: the blank itself comes back, which the blank < V check refuses.
static int vocab_holding(int blank) { return blank < 0x7ffffffe ? blank + 2 : blank; }
