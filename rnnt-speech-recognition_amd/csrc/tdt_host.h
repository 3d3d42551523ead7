// tdt_host.h -- the host-side rules of the token-and-duration (TDT) transducer that the extern "C" boundaries of all seven TDT
// libraries share (loss, fused joint, aligner, greedy, greedy stream, beam, beam stream): the limits on the duration set, the
// duration set's own rule, the decoders' rule for the two heads and the checks of the batched greedy decoder.  A device header
// that sizes an array by a constant of its own holds it against the limit here with a static_assert.  No device code; a library
// that links no tdt_greedy_kernels.hip may include this (an unused static inline names no launcher).
#pragma once
#include "rnnt_decode_host.h"

constexpr int kTdtHostMaxD = 8;         // durations per set (include/rnnt_tdt.h)
constexpr int kTdtHostMaxDuration = 8;  // the largest duration (include/rnnt_tdt.h)

namespace rnnt {
// tdt_greedy_kernels.hip
hipError_t tdt_greedy_workspace_bytes(int T, int B, int J, int Vt, int D, int joint_dtype, size_t *bytes);
}  // namespace rnnt

// strictly increasing, durations[0] in {0, 1}, some d > 0, the largest <= 8 (num_durations: checked by the caller, 1 .. 8)
static inline bool tdt_durations_ok(const int *durations, int num_durations) {
    if (durations[0] != 0 && durations[0] != 1) return false;
    for (int i = 1; i < num_durations; ++i)
        if (durations[i] <= durations[i - 1]) return false;
    return durations[num_durations - 1] > 0 && durations[num_durations - 1] <= kTdtHostMaxDuration;
}

// The decoders alone (the loss takes any alphabet): 2 <= V <= 2^24, 1 <= D <= 8, so V + D cannot overflow (and the decoders take
// no alphabet beyond 8192)
static inline bool tdt_heads_ok(int alphabet_size, int num_durations) {
    return alphabet_size >= 2 && alphabet_size <= (1 << 24) && num_durations >= 1 && num_durations <= kTdtHostMaxD;
}

// the checks of the greedy decoder at alphabet_size = R, then the blank inside the token head and the workspace's own layout
static inline rnntStatus_t check_tdt_greedy(int maxT, int joint_size, int alphabet_size, int num_durations, int minibatch,
                                            int joint_dtype, const rnntOptions &o) {
    if (!tdt_heads_ok(alphabet_size, num_durations)) return RNNT_STATUS_INVALID_VALUE;
    const rnntStatus_t st = check_greedy(maxT, joint_size, alphabet_size + num_durations, minibatch, joint_dtype, o);
    if (st != RNNT_STATUS_SUCCESS) return st;
    if (o.blank_label >= alphabet_size) return RNNT_STATUS_INVALID_VALUE;
    size_t n = 0;
    if (rnnt::tdt_greedy_workspace_bytes(maxT, minibatch, joint_size, alphabet_size, num_durations, joint_dtype, &n) != hipSuccess)
        return RNNT_STATUS_INVALID_VALUE;
    return RNNT_STATUS_SUCCESS;
}
