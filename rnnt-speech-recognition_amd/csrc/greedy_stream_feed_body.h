// greedy_stream_feed_body.h -- the feed kernel of the greedy stream (greedy_kernels.hip), included there once per instantiation:
// GREEDY_STREAM_FEED_KERNEL is the kernel's name, GREEDY_STREAM_FEED_TIMED 0 / 1 whether it keeps frame_base
// (greedy_stream_feed_kernel and greedy_stream_feed_timed_kernel).  As beam_select_body.h: both are compiled as kernels, so the
// untimed one comes out of the compiler as it did before the timed one existed.  No include guard on purpose.
// the per-frame range flags of the chunk's frames; workgroup 0 also moves every slot's state on to the chunk.  TIMED: and the
// slot's frame_base on by the frames of the chunk it leaves (a reset: to 0), so that base + t is the frame since the reset
__global__ __launch_bounds__(256) void GREEDY_STREAM_FEED_KERNEL(const GreedyStreamArgs a) {
    constexpr bool TIMED = GREEDY_STREAM_FEED_TIMED;
    const int rows = a.S * a.Te;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {  // (block-uniform trip count and skip: the barrier below is safe)
        const int s = r / a.Te, t = r - s * a.Te;
        if (t >= gs_frames(a, s)) continue;
        const size_t base = ((size_t)s * a.T + t) * a.J;
        bool big = false;
        for (int j = threadIdx.x; j < a.J; j += 256) big |= exp_tab_out_of_range(a.encraw[base + j]);  // also catches NaN
        big = __syncthreads_or(big);
        if (threadIdx.x == 0) a.rowflag[(size_t)s * a.T + t] = big ? 1 : 0;
    }
    if (blockIdx.x != 0) return;
    bool running = false;
    for (int b = threadIdx.x; b < a.S; b += 256) {
        GreedyState s = a.st[b];
        if (TIMED) a.frame_base[b] = (a.reset && a.reset[b] != 0) ? 0 : a.frame_base[b] + s.Tb;
        if (a.reset && a.reset[b] != 0) {
            s.n = 0, s.fin = 0, s.score = 0.0;
            s.maxsym = a.max_symbols ? max(a.max_symbols[b], 0) : INT_MAX;
            s.cap = a.max_per_frame;
        }
        s.t = 0, s.nf = 0;
        if (s.fin || s.n >= s.maxsym) {  // finished: nothing more until a reset
            s.fin = 1, s.Tb = 0;
        } else {
            s.Tb = gs_frames(a, b);
            if (a.final_ && a.final_[b] != 0) s.fin = 1;  // (after this chunk)
        }
        s.done = s.Tb == 0 ? 1 : 0;
        a.st[b] = s;
        a.hyp_lengths[b] = s.n;
        a.scores[b] = (float)s.score;
        running |= !s.done;
    }
    running = __syncthreads_or(running);
    if (threadIdx.x == 0) a.all_done[0] = running ? 0 : 1;  // (a full hyps buffer: the next step reports 2)
}
