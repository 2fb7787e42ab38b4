// Mask IoU counts of COCO evaluation on the device (evaluation/coco_evaluation.py:543-591 hands results and annotations to pycocotools,
// whose hot loop is the IoU of every detection mask with every ground-truth mask of the image).  Here a mask is HW bits: bit p % 64 of
// 64-bit word p / 64 is the row-major pixel p = y*W + x, ceil(HW / 64) words per mask, the unused high bits of the last word zero.
//
//   pack  : mask_pack_kernel       — (R,H,W) bytes 0/1 -> words.  One lane per pixel, one ballot of "my byte is non-zero" per word,
//                                    MIOU_WPW words per wave with their byte loads in flight together.  A mask is HW contiguous bytes,
//                                    so the rows' alignment does not matter: the loads are bytes.
//   decode: rle_decode_pack_kernel — COCO runs (column-major, position x*H + y, zeros first) -> the same words and, on request, the
//                                    (M,H,W) bytes.  One lane per row-major pixel: its column-major position q lies in run
//                                    i = #{prefix sums <= q} (binary search over the mask's inclusive prefix sums; a zero-length run
//                                    repeats a prefix sum and is passed over), the pixel is i & 1, one ballot packs the word.
//   areas : words_area_kernel      — popcount of a mask's words, one workgroup per mask (both of the above end with it).
//   inter : mask_inter_kernel      — inter[n][m] = popcount(det[n] & gt[m]).  A workgroup owns MIOU_CW words of every mask and MIOU_DN
//                                    detections: it reads their words once into registers, stages the same words of up to MIOU_TM
//                                    ground truths in LDS (64 KiB), and every thread ANDs its detection words with its LDS column for
//                                    each ground truth; a wave reduction and one integer atomic per (wave, n, m) with a non-zero sum
//                                    add up in `inter`, which the entry zeroes on the stream first.  With M > MIOU_TM the next tile of
//                                    ground truths is staged over the first while the detection words stay in registers: one pass over
//                                    a detection serves every ground truth.
// Integer results throughout; every store is an ordinary vector store, the atomics are vector atomics.
#include "cmk_common.hpp"

namespace cmk {

constexpr int MIOU_WPW = 8;      // pack/decode: words per wave (byte loads a lane keeps in flight)
constexpr int MIOU_CW = 512;     // inter: words per workgroup, 2 per thread
constexpr int MIOU_DN = 16;      // inter: detections per workgroup, their words in 64 VGPRs
constexpr int MIOU_TM = 16;      // inter: ground truths per LDS tile, 16 * 512 * 8 B = 64 KiB

__device__ inline int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// first word of this wave's MIOU_WPW; false past the last word (wave-uniform)
__device__ inline bool miou_wave_words(int nw, int& w0) {
    const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u * MIOU_WPW >= nw) return false;
    w0 = (int)(u * MIOU_WPW);
    return true;
}

// lane k < MIOU_WPW stores word k of the wave: 64 contiguous bytes
__device__ inline void miou_store_words(unsigned long long* __restrict__ out, int w0, int nw, const unsigned long long (&b)[MIOU_WPW]) {
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < MIOU_WPW; ++k)
        if (lane == k) mine = b[k];
    if (lane < MIOU_WPW && w0 + lane < nw) out[w0 + lane] = mine;
}

// grid = (ceil(nw / (4 * MIOU_WPW)), R), 4 independent waves per workgroup
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* __restrict__ masks, int HW, int nw, unsigned long long* __restrict__ words) {
    int w0;
    if (!miou_wave_words(nw, w0)) return;
    const int lane = threadIdx.x & 63;
    const uint8_t* img = masks + (long)blockIdx.y * HW;
    uint8_t v[MIOU_WPW];
#pragma unroll
    for (int k = 0; k < MIOU_WPW; ++k) {
        const long p = (long)(w0 + k) * 64 + lane;
        v[k] = p < HW ? img[p] : (uint8_t)0;
    }
    unsigned long long b[MIOU_WPW];
#pragma unroll
    for (int k = 0; k < MIOU_WPW; ++k) b[k] = __ballot(v[k] != 0);
    miou_store_words(words + (long)blockIdx.y * nw, w0, nw, b);
}

// grid as mask_pack_kernel with M for R.  cum: inclusive prefix sums of the runs of all masks, off[m] .. off[m+1] those of mask m, the
// last one HW (checked by the caller).  bitmasks may be null.
__global__ __launch_bounds__(256) void rle_decode_pack_kernel(const int32_t* __restrict__ cum, const long long* __restrict__ off, int H, int W, int nw,
                                                             unsigned long long* __restrict__ words, uint8_t* __restrict__ bitmasks) {
    int w0;
    if (!miou_wave_words(nw, w0)) return;
    const int lane = threadIdx.x & 63;
    const int HW = H * W;
    const long long base = off[blockIdx.y];
    const int n = (int)(off[blockIdx.y + 1] - base);
    const int32_t* c = cum + base;
    unsigned long long b[MIOU_WPW];
#pragma unroll
    for (int k = 0; k < MIOU_WPW; ++k) {
        const long p = (long)(w0 + k) * 64 + lane;
        bool one = false;
        if (p < HW) {
            const int y = (int)(p / W), x = (int)(p - (long)y * W);
            const int q = x * H + y;
            int lo = 0, hi = n;                          // first i in [0, n) with c[i] > q; c[n-1] = HW > q
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (c[mid] <= q) lo = mid + 1; else hi = mid;
            }
            one = lo & 1;
            if (bitmasks) bitmasks[(long)blockIdx.y * HW + p] = (uint8_t)one;
        }
        b[k] = __ballot(one);
    }
    miou_store_words(words + (long)blockIdx.y * nw, w0, nw, b);
}

// grid = R masks
__global__ __launch_bounds__(256) void words_area_kernel(const unsigned long long* __restrict__ words, int nw, int32_t* __restrict__ areas) {
    __shared__ int lds[4];
    const unsigned long long* w = words + (long)blockIdx.x * nw;
    int s = 0;
    for (int i = threadIdx.x; i < nw; i += 256) s += __popcll(w[i]);
    s = wave_sum_i32(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) areas[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

// grid = (ceil(nw / MIOU_CW), ceil(N / MIOU_DN)); inter zeroed before the launch
__global__ __launch_bounds__(256) void mask_inter_kernel(const unsigned long long* __restrict__ det, int N, const unsigned long long* __restrict__ gt, int M,
                                                        int nw, int32_t* __restrict__ inter) {
    __shared__ unsigned long long tile[MIOU_TM][MIOU_CW];
    const int t = threadIdx.x;
    const int wa = blockIdx.x * MIOU_CW + t, wb = wa + 256;           // this thread's two words
    const int n0 = blockIdx.y * MIOU_DN;
    unsigned long long da[MIOU_DN], db[MIOU_DN];
#pragma unroll
    for (int i = 0; i < MIOU_DN; ++i) {
        const bool have = n0 + i < N;
        const unsigned long long* d = det + (long)(n0 + i) * nw;
        da[i] = (have && wa < nw) ? d[wa] : 0ull;
        db[i] = (have && wb < nw) ? d[wb] : 0ull;
    }
    for (int m0 = 0; m0 < M; m0 += MIOU_TM) {
        const int tm = min(MIOU_TM, M - m0);
        if (m0) __syncthreads();                                       // the tile before this one has been read
        for (int m = 0; m < tm; ++m) {
            const unsigned long long* g = gt + (long)(m0 + m) * nw;
            tile[m][t] = wa < nw ? g[wa] : 0ull;
            tile[m][t + 256] = wb < nw ? g[wb] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MIOU_DN; ++i) {
            if (n0 + i >= N) break;                                    // uniform over the workgroup
            for (int m = 0; m < tm; ++m) {
                int s = __popcll(da[i] & tile[m][t]) + __popcll(db[i] & tile[m][t + 256]);
                s = wave_sum_i32(s);
                if ((t & 63) == 0 && s) atomicAdd(inter + (long)(n0 + i) * M + m0 + m, s);
            }
        }
    }
}

inline int miou_nw(int H, int W) { return (int)(((int64_t)H * W + 63) / 64); }

// shared argument check; the messages name the entry
inline int miou_check(const char* what, int H, int W, bool any_null) {
    if (H < 1 || W < 1) return fail(CMK_EINVAL, "%s: H = %ld, W = %ld must be at least 1", what, H, W);
    if ((int64_t)H * W >= 0x7fffffffLL) return fail(CMK_EINVAL, "%s: H*W of %ld x %ld does not leave int32 positions and areas", what, H, W);
    if (any_null) return fail(CMK_EINVAL, "%s: null pointer", what);
    return CMK_OK;
}

inline int miou_count_check(const char* what, int v) {
    if (v < 0 || v > 65535) return fail(CMK_EINVAL, "%s: mask count %ld outside [0, 65535]", what, v);
    return CMK_OK;
}

inline dim3 miou_word_grid(int R, int nw) { return dim3(cdiv(cdiv(nw, MIOU_WPW), 4), R); }

// the entries zero what their kernels add into
inline int miou_zero(const char* what, void* p, size_t bytes, hipStream_t st) {
    if (hipMemsetAsync(p, 0, bytes, st) == hipSuccess) return CMK_OK;
    (void)hipGetLastError();
    return fail(CMK_ELAUNCH, "%s: zeroing the output failed", what);
}

}  // namespace cmk

using namespace cmk;

extern "C" int cmk_mask_pack_bits(const uint8_t* masks, int R, int H, int W, uint64_t* words, int32_t* areas, void* stream) {
    if (R == 0) return CMK_OK;
    if (int rc = miou_count_check("mask_pack_bits", R)) return rc;
    if (int rc = miou_check("mask_pack_bits", H, W, !masks || !words || !areas)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nw = miou_nw(H, W);
    hipLaunchKernelGGL(mask_pack_kernel, miou_word_grid(R, nw), dim3(256), 0, st, masks, H * W, nw, (unsigned long long*)words);
    hipLaunchKernelGGL(words_area_kernel, dim3(R), dim3(256), 0, st, (const unsigned long long*)words, nw, areas);
    return check_launch("mask_pack_bits");
}

extern "C" int cmk_rle_decode_pack(const int32_t* cum, const int64_t* off, int M, int H, int W, uint64_t* words, int32_t* areas, uint8_t* bitmasks,
                                   void* stream) {
    if (M == 0) return CMK_OK;
    if (int rc = miou_count_check("rle_decode_pack", M)) return rc;
    if (int rc = miou_check("rle_decode_pack", H, W, !cum || !off || !words || !areas)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nw = miou_nw(H, W);
    hipLaunchKernelGGL(rle_decode_pack_kernel, miou_word_grid(M, nw), dim3(256), 0, st, cum, (const long long*)off, H, W, nw, (unsigned long long*)words,
                       bitmasks);
    hipLaunchKernelGGL(words_area_kernel, dim3(M), dim3(256), 0, st, (const unsigned long long*)words, nw, areas);
    return check_launch("rle_decode_pack");
}

extern "C" int cmk_mask_intersections(const uint64_t* det, int N, const uint64_t* gt, int M, int H, int W, int32_t* inter, void* stream) {
    if (N == 0 || M == 0) return CMK_OK;
    if (int rc = miou_count_check("mask_intersections", N)) return rc;
    if (int rc = miou_count_check("mask_intersections", M)) return rc;
    if (int rc = miou_check("mask_intersections", H, W, !det || !gt || !inter)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nw = miou_nw(H, W);
    if (int rc = miou_zero("mask_intersections", inter, sizeof(int32_t) * (size_t)N * M, st)) return rc;
    hipLaunchKernelGGL(mask_inter_kernel, dim3(cdiv(nw, MIOU_CW), cdiv(N, MIOU_DN)), dim3(256), 0, st, (const unsigned long long*)det, N,
                       (const unsigned long long*)gt, M, nw, inter);
    return check_launch("mask_intersections");
}
