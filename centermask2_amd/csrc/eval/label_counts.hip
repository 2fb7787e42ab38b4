// Overlap counts of Cityscapes instance evaluation on the device (evaluation/cityscapes_evaluation.py:47-130 writes every predicted mask
// as a PNG and hands the files to cityscapesscripts, whose hot loop compares each with the ground-truth image once per ground-truth
// instance).  What the score needs is, per prediction, how many of its pixels fall on each ground-truth region.  Here the predictions
// are packed masks (mask_iou.hip: bit p % 64 of 64-bit word p / 64 is the row-major pixel p) and the ground truth is one label image of
// uint16 columns; table[n*C + c] = #{p : bit p of mask n set, cols[p] == c}.
//
//   counts: label_counts_kernel — a workgroup is ONE wave and owns LC_WORDS consecutive words of one mask.  It loads them (lane l holds
//                                 words l, l + 64, ..), and leaves if all are zero: an instance covers about 1 % of a frame, so most
//                                 workgroups end here, before any LDS or label traffic.  Otherwise it zeroes a C-entry int32 histogram
//                                 in LDS (dynamic, 4*C bytes) and walks its non-zero words (a ballot per 64 words, one bit per word).
//                                 For one word, lane l is pixel 64*word + l: the 64 labels are one coalesced 128-byte load, read for
//                                 non-zero words only, the loads of LC_BATCH words in flight together (one load at a time left the
//                                 wave that holds a large instance waiting one memory latency per word: the kernel's tail).  Set
//                                 pixels of a word nearly always share a column, so the wave aggregates first: the first live
//                                 lane's column is broadcast, a ballot counts the live lanes that have it, that
//                                 lane alone adds the count to the histogram, and the lanes counted retire; the loop runs once per
//                                 distinct column under the word's set pixels.  At the end every non-zero counter goes to `table`
//                                 with one global integer atomic; the entry zeroes `table` on the stream first.
// A pixel whose column is >= C, or a bit at a position >= H*W, is never live: it indexes neither the histogram nor the table.
// Integer results throughout; every store is an ordinary vector store, the atomics are vector atomics.
#include "cmk_common.hpp"

namespace cmk {

constexpr int LC_ROUNDS = 4;                 // words per lane
constexpr int LC_WORDS = 64 * LC_ROUNDS;     // words per workgroup (one wave): 16384 pixels
constexpr int LC_BATCH = 8;                  // non-zero words whose label loads a wave keeps in flight

// grid = (ceil(nw / LC_WORDS), N), 64 threads, 4*C bytes of dynamic LDS; table zeroed before the launch
__global__ __launch_bounds__(64) void label_counts_kernel(const unsigned long long* __restrict__ words, int nw, const uint16_t* __restrict__ cols,
                                                          int HW, int C, int32_t* __restrict__ table) {
    extern __shared__ int32_t lc_hist[];
    const int lane = threadIdx.x;
    const int w0 = blockIdx.x * LC_WORDS;
    const unsigned long long* mask = words + (long)blockIdx.y * nw;
    unsigned long long mine[LC_ROUNDS];
    unsigned long long any = 0;
#pragma unroll
    for (int r = 0; r < LC_ROUNDS; ++r) {
        const int w = w0 + r * 64 + lane;
        mine[r] = w < nw ? mask[w] : 0ull;
        any |= mine[r];
    }
    if (__ballot(any != 0) == 0) return;                               // wave-uniform: nothing of this mask in these words
    for (int c = lane; c < C; c += 64) lc_hist[c] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LC_ROUNDS; ++r) {
        unsigned long long todo = __ballot(mine[r] != 0);              // bit k: word w0 + r*64 + k is non-zero
        while (todo) {
            int col[LC_BATCH];                                         // the labels of up to LC_BATCH words, their loads in flight together
#pragma unroll
            for (int b = 0; b < LC_BATCH; ++b) {
                col[b] = C;
                if (todo) {                                            // wave-uniform
                    const int k = __ffsll(todo) - 1;
                    todo &= todo - 1;
                    const unsigned long long word = __shfl(mine[r], k, 64);
                    const long p = (long)(w0 + r * 64 + k) * 64 + lane;
                    if (((word >> lane) & 1ull) && p < HW) col[b] = cols[p];
                }
            }
#pragma unroll
            for (int b = 0; b < LC_BATCH; ++b) {
                unsigned long long live = __ballot(col[b] < C);
                while (live) {
                    const int leader = __ffsll(live) - 1;
                    const int c0 = __shfl(col[b], leader, 64);
                    const unsigned long long same = __ballot(col[b] == c0) & live;
                    if (lane == leader) atomicAdd(&lc_hist[c0], __popcll(same));
                    live &= ~same;
                }
            }
        }
    }
    __syncthreads();
    int32_t* row = table + (long)blockIdx.y * C;
    for (int c = lane; c < C; c += 64) {
        const int v = lc_hist[c];
        if (v) atomicAdd(row + c, v);
    }
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_mask_label_counts(const uint64_t* words, int N, const uint16_t* cols, int H, int W, int C, int32_t* table, void* stream) {
    if (N < 0 || N > 65535) return fail(CMK_EINVAL, "%s: mask count %ld outside [0, 65535]", "mask_label_counts", N);
    if (H < 1 || W < 1) return fail(CMK_EINVAL, "%s: H = %ld, W = %ld must be at least 1", "mask_label_counts", H, W);
    if ((int64_t)H * W >= 0x7fffffffLL) return fail(CMK_EINVAL, "%s: H*W of %ld x %ld does not leave int32 positions and areas", "mask_label_counts", H, W);
    if (C < 1 || C > CMK_LABEL_MAX_COLS) return fail(CMK_EINVAL, "%s: %ld columns outside [1, %ld]", "mask_label_counts", C, CMK_LABEL_MAX_COLS);
    if (!words || !cols || !table) return fail(CMK_EINVAL, "%s: null pointer", "mask_label_counts");
    if (N == 0) return CMK_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nw = (int)(((int64_t)H * W + 63) / 64);
    if (hipMemsetAsync(table, 0, sizeof(int32_t) * (size_t)N * C, st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CMK_ELAUNCH, "%s: zeroing the output failed", "mask_label_counts");
    }
    hipLaunchKernelGGL(label_counts_kernel, dim3(cdiv(nw, LC_WORDS), N), dim3(64), sizeof(int32_t) * (size_t)C, st,
                       (const unsigned long long*)words, nw, cols, H * W, C, table);
    return check_launch("mask_label_counts");
}
