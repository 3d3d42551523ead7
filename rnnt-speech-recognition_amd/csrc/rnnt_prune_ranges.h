// rnnt_prune_ranges.h -- the band positions of the pruned loss (include/rnnt_prune_ranges.h): parameters and launchers of
// rnnt_prune_ranges_kernels.hip.  No workspace: the window pass writes raw[b, t] of the live frames into s_begin, the scan pass
// finishes the rule in place and writes every other element.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rnnt {

constexpr int kPruneRangesMaxU = 8192;
constexpr int kPruneRangesMaxS = 64;

struct PruneRangesParams {
    const float *occupancy;    // [B][T][U]
    const int *input_lengths;  // [B]
    const int *label_lengths;  // [B]
    int *s_begin;              // [B][T]
    int B, T, U, S;
};

hipError_t launch_prune_ranges_windows(const PruneRangesParams &p, hipStream_t s);
hipError_t launch_prune_ranges_scan(const PruneRangesParams &p, hipStream_t s);

}  // namespace rnnt
