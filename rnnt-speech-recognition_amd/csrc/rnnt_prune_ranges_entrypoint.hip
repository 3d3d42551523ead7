// rnnt_prune_ranges_entrypoint.hip -- the extern "C" boundary of libwarprnnt_pruneranges.so (declared in
// include/rnnt_prune_ranges.h): the band positions of the pruned loss.  build.py links this translation unit with
// rnnt_prune_ranges_kernels.hip alone, and rnnt_prune_ranges.map keeps everything but the entry point local.  Everything is checked
// before anything is enqueued, nothing is allocated, both launches go to the caller's stream.
#include "../../include/rnnt_prune_ranges.h"
#include "rnnt_prune_ranges.h"
#include "rnnt_host.h"

using namespace rnnt;

extern "C" {

rnntStatus_t compute_rnnt_prune_ranges(const float *occupancy, const int *input_lengths, const int *label_lengths,
                                       int minibatch, int s_range, int *s_begin, rnntOptions options) {
    if (!occupancy || !input_lengths || !label_lengths || !s_begin) return RNNT_STATUS_INVALID_VALUE;
    if (options.loc != RNNT_GPU) return RNNT_STATUS_INVALID_VALUE;  // device-only library: no CPU fallback
    if (minibatch < 1 || options.maxT < 1) return RNNT_STATUS_INVALID_VALUE;
    if (options.maxU < 1 || options.maxU > kPruneRangesMaxU) return RNNT_STATUS_INVALID_VALUE;
    if (s_range < 1 || s_range > kPruneRangesMaxS) return RNNT_STATUS_INVALID_VALUE;
    if ((long long)minibatch * options.maxT * options.maxU >= (1ll << 31)) return RNNT_STATUS_INVALID_VALUE;
    PruneRangesParams p{};
    p.occupancy = occupancy, p.input_lengths = input_lengths, p.label_lengths = label_lengths, p.s_begin = s_begin;
    p.B = minibatch, p.T = options.maxT, p.U = options.maxU, p.S = s_range;
    hipStream_t s = (hipStream_t)options.stream;
    hipError_t e = launch_prune_ranges_windows(p, s);
    if (e != hipSuccess) return from_hip(e);
    return from_hip(launch_prune_ranges_scan(p, s));
}

}  // extern "C"
