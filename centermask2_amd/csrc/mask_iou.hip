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
//   bound : mask_boundary_kernel   — boundary(m) = m & ~eroded(m) of Boundary IoU on the packed words, eroded = the (2d+1)x(2d+1) square
//                                    erosion with everything outside the image background.  A workgroup owns a tile of rows x 64-pixel
//                                    columns of one mask.  It loads the tile with a halo of d rows and ceil(d/64) words from the linear bit
//                                    stream into LDS RE-ALIGNED, every row starting on a word, bits past W and rows and words outside the
//                                    image zero (which is the border rule).  Horizontal pass: per word, the AND of d+1 pixels to the right
//                                    and of d+1 to the left, each by doubling funnel shifts over three words.  Vertical pass: word ANDs
//                                    down 2d+1 aligned rows, no shifts; skipped where the mask word is zero, left when the AND is zero.
//                                    m & ~e goes back into the linear layout shifted, as at most two 64-bit OR atomics per non-zero word
//                                    (a linear word holds pixels of several rows or tiles), and its popcount is added to the mask's area,
//                                    one integer atomic per wave; the entry zeroes bwords and bareas on the stream first.
//   unpack: mask_unpack_kernel     — words -> (R,H,W) bytes 0/1, one lane per pixel.
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

// ---- boundary ----------------------------------------------------------------------------------------------------------------------
constexpr int MB_LDS_WORDS = 8192;      // 64 KiB of LDS per workgroup: two workgroups on a CU
constexpr int MB_MAX_Q = 2;             // halo words per side, ceil(CMK_BOUNDARY_MAX_D / 64)
constexpr int MB_THREADS = 1024;        // threads of a workgroup
constexpr int MB_LOADS = 4;             // load phase: words per thread whose global loads are in flight together
constexpr int MB_ROWS = 8;              // vertical pass: rows read from LDS between two tests of "already zero"
static_assert(CMK_BOUNDARY_MAX_D <= 64 * MB_MAX_Q, "the horizontal pass looks MB_MAX_Q words to each side");

struct MbGeo {
    int H, W, nw, d;
    int q;        // halo words per side, ceil(d / 64)
    int TR, TW;   // tile: output rows, output words per row
    int nxt;      // tiles across a row
};

// word c of row y in the aligned layout: pixels (y, 64c .. 64c+63), zero outside the image
__host__ __device__ inline unsigned long long mb_aligned_word(const unsigned long long* __restrict__ w, const MbGeo& g, int y, int c) {
    const int nvalid = g.W - 64 * c;
    if (y < 0 || y >= g.H || c < 0 || nvalid <= 0) return 0ull;
    const long p0 = (long)y * g.W + 64L * c;
    const int wi = (int)(p0 >> 6), sh = (int)(p0 & 63);
    unsigned long long v = w[wi] >> sh;
    if (sh && wi + 1 < g.nw) v |= w[wi + 1] << (64 - sh);
    if (nvalid < 64) v &= (1ull << nvalid) - 1ull;
    return v;
}

// bit x of the result = AND of pixels x .. x+d of the stream a0, a1, a2 (a0 the word asked for, a1 and a2 the words after it).
// Doubling: after a step every bit holds the AND of n pixels; n goes 1, 2, 4, .. and the last step is shortened to land on d + 1.  With
// d <= 128 no step is longer than 64.
__host__ __device__ inline unsigned long long mb_and_right(unsigned long long a0, unsigned long long a1, unsigned long long a2, int d) {
    for (int n = 1; n < d + 1;) {
        const int s = min(n, d + 1 - n);
        if (s == 64) {
            a0 &= a1; a1 &= a2; a2 = 0ull;
        } else {
            a0 &= (a0 >> s) | (a1 << (64 - s));
            a1 &= (a1 >> s) | (a2 << (64 - s));
            a2 &= a2 >> s;
        }
        n += s;
    }
    return a0;
}

// the mirror image: AND of pixels x-d .. x, a1 and a2 the words before a0
__host__ __device__ inline unsigned long long mb_and_left(unsigned long long a0, unsigned long long a1, unsigned long long a2, int d) {
    for (int n = 1; n < d + 1;) {
        const int s = min(n, d + 1 - n);
        if (s == 64) {
            a0 &= a1; a1 &= a2; a2 = 0ull;
        } else {
            a0 &= (a0 << s) | (a1 >> (64 - s));
            a1 &= (a1 << s) | (a2 >> (64 - s));
            a2 &= a2 << s;
        }
        n += s;
    }
    return a0;
}

// The three phases of a tile for thread t of nt, a barrier between them.  lds: raw[(rows+2d)][TW+2q] then hero[(rows+2d)][TW].
struct MbTile {
    int y0, c0, rows, RS, rin;
    unsigned long long *raw, *hero;
};

__host__ __device__ inline MbTile mb_tile(const MbGeo& g, int tile, unsigned long long* lds) {
    MbTile k;
    k.y0 = (tile / g.nxt) * g.TR;
    k.c0 = (tile % g.nxt) * g.TW;
    k.rows = min(g.TR, g.H - k.y0);
    k.RS = g.TW + 2 * g.q;
    k.rin = k.rows + 2 * g.d;
    k.raw = lds;
    k.hero = lds + (long)(g.TR + 2 * g.d) * k.RS;
    return k;
}

__host__ __device__ inline void mb_load(const MbGeo& g, const MbTile& k, const unsigned long long* __restrict__ w, int t, int nt) {
    const int n = k.rin * k.RS;
    for (int i0 = t; i0 < n; i0 += MB_LOADS * nt) {                         // MB_LOADS words' global loads in flight per thread
        unsigned long long v[MB_LOADS];
#pragma unroll
        for (int u = 0; u < MB_LOADS; ++u) {
            const int i = i0 + u * nt;
            const int r = i / k.RS, j = i - r * k.RS;
            v[u] = i < n ? mb_aligned_word(w, g, k.y0 - g.d + r, k.c0 - g.q + j) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < MB_LOADS; ++u)
            if (i0 + u * nt < n) k.raw[i0 + u * nt] = v[u];
    }
}

__host__ __device__ inline void mb_horizontal(const MbGeo& g, const MbTile& k, int t, int nt) {
    for (int i = t; i < k.rin * g.TW; i += nt) {
        const int r = i / g.TW, j = i - r * g.TW;
        const unsigned long long* a = k.raw + r * k.RS + j + g.q;           // the halo of q words lies on both sides of a[0]
        unsigned long long e = a[0];
        if (e) {
            e = mb_and_right(a[0], a[1], g.q > 1 ? a[2] : 0ull, g.d);
            if (e) e &= mb_and_left(a[0], a[-1], g.q > 1 ? a[-2] : 0ull, g.d);
        }
        k.hero[i] = e;
    }
}

// -> the boundary pixels this thread found
__host__ __device__ inline int mb_vertical_store(const MbGeo& g, const MbTile& k, unsigned long long* __restrict__ out, int t, int nt) {
    int area = 0;
    for (int i = t; i < k.rows * g.TW; i += nt) {
        const int r = i / g.TW, j = i - r * g.TW;
        const unsigned long long m = k.raw[(r + g.d) * k.RS + j + g.q];
        if (!m) continue;                                                   // zero too where c0 + j is past the row's last word
        unsigned long long e = ~0ull;
        const unsigned long long* h = k.hero + r * g.TW + j;                // output row r is rows r .. r+2d of the halo'd tile
        for (int dy = 0; dy <= 2 * g.d && e; dy += MB_ROWS) {               // MB_ROWS independent LDS reads, then one test
            unsigned long long a = ~0ull;
#pragma unroll
            for (int u = 0; u < MB_ROWS; ++u)
                if (dy + u <= 2 * g.d) a &= h[(dy + u) * g.TW];
            e &= a;
        }
        const unsigned long long b = m & ~e;
        if (!b) continue;
        area += __builtin_popcountll(b);
        const long p0 = (long)(k.y0 + r) * g.W + 64L * (k.c0 + j);
        const int wi = (int)(p0 >> 6), sh = (int)(p0 & 63);
        // b has no bit past W, so a non-zero high part lies inside the mask's H*W bits: wi + 1 < nw there
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(out + wi, b << sh);
        if (sh && (b >> (64 - sh))) atomicOr(out + wi + 1, b >> (64 - sh));
#else
        out[wi] |= b << sh;
        if (sh && (b >> (64 - sh))) out[wi + 1] |= b >> (64 - sh);
#endif
    }
    return area;
}

// grid = (tiles of a mask, R), MB_THREADS threads: a tile is a few thousand words, and what a workgroup takes is the latency of a
// thread's share of them, so the share is kept small.  Dynamic LDS (TR + 2d) * (2 TW + 2q) words; bwords and bareas zeroed before the launch.
__global__ __launch_bounds__(MB_THREADS) void mask_boundary_kernel(const unsigned long long* __restrict__ words, MbGeo g,
                                                                 unsigned long long* __restrict__ bwords, int32_t* __restrict__ bareas) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long mb_lds[];
    const MbTile k = mb_tile(g, blockIdx.x, mb_lds);
    const unsigned long long* w = words + (long)blockIdx.y * g.nw;
    mb_load(g, k, w, threadIdx.x, MB_THREADS);
    __syncthreads();
    mb_horizontal(g, k, threadIdx.x, MB_THREADS);
    __syncthreads();
    const int area = wave_sum_i32(mb_vertical_store(g, k, bwords + (long)blockIdx.y * g.nw, threadIdx.x, MB_THREADS));
    if ((threadIdx.x & 63) == 0 && area) atomicAdd(bareas + blockIdx.y, area);
}

// The tile: as many words across as fit with at least min(H, 2d) output rows (the halo then costs at most as much as the tile), else
// the narrowest.  CMK_BOUNDARY_MAX_D leaves rows at TW = 8: 8192 / (2*8 + 2*2) - 2*128 = 153.
inline MbGeo mb_geometry(int H, int W, int d) {
    MbGeo g;
    g.H = H; g.W = W; g.d = d;
    g.nw = (int)(((int64_t)H * W + 63) / 64);
    g.q = (d + 63) / 64;
    const int RW = cdiv(W, 64);
    int fit = 0;
    for (int tw = 32; tw >= 8; tw >>= 1) {
        g.TW = min(RW, tw);
        fit = MB_LDS_WORDS / (2 * g.TW + 2 * g.q) - 2 * d;
        if (fit >= min(H, 2 * d)) break;
    }
    g.TR = min(min(fit, H), max(4 * d, 64));                                // no taller than that: the halo adds at most half, and a mask
    g.TR = cdiv(H, cdiv(H, g.TR));                                          // is many workgroups; bands of equal height
    g.nxt = cdiv(RW, g.TW);
    return g;
}

// grid as mask_pack_kernel
__global__ __launch_bounds__(256) void mask_unpack_kernel(const unsigned long long* __restrict__ words, int HW, int nw, uint8_t* __restrict__ masks) {
    int w0;
    if (!miou_wave_words(nw, w0)) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long* w = words + (long)blockIdx.y * nw;
    uint8_t* img = masks + (long)blockIdx.y * HW;
#pragma unroll
    for (int k = 0; k < MIOU_WPW; ++k) {
        const long p = (long)(w0 + k) * 64 + lane;
        if (p < HW) img[p] = (uint8_t)((w[w0 + k] >> lane) & 1ull);
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

extern "C" int cmk_mask_boundary_bits(const uint64_t* words, int R, int H, int W, int d, uint64_t* bwords, int32_t* bareas, void* stream) {
    if (R == 0) return CMK_OK;
    if (int rc = miou_count_check("mask_boundary_bits", R)) return rc;
    if (int rc = miou_check("mask_boundary_bits", H, W, !words || !bwords || !bareas)) return rc;
    if (d < 1) return fail(CMK_EINVAL, "%s: erosion distance d = %ld must be at least 1", "mask_boundary_bits", d);
    const bool fits = 2 * (int64_t)d + 1 <= (H < W ? H : W);                // else no square fits in the image: the boundary is the mask
    if (fits && d > CMK_BOUNDARY_MAX_D)
        return fail(CMK_EINVAL, "%s: erosion distance d = %ld is above CMK_BOUNDARY_MAX_D = %ld", "mask_boundary_bits", d, CMK_BOUNDARY_MAX_D);
    hipStream_t st = (hipStream_t)stream;
    const int nw = miou_nw(H, W);
    const size_t bytes = sizeof(uint64_t) * (size_t)R * nw;
    const char* lo = (const char*)words;
    const char* bo = (const char*)bwords;
    if (lo < bo + bytes && bo < lo + bytes) return fail(CMK_EINVAL, "%s: bwords overlaps words (out of place only)", "mask_boundary_bits");
    if (!fits) {
        if (hipMemcpyAsync(bwords, words, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            (void)hipGetLastError();
            return fail(CMK_ELAUNCH, "%s: copying the masks failed", "mask_boundary_bits");
        }
        hipLaunchKernelGGL(words_area_kernel, dim3(R), dim3(256), 0, st, (const unsigned long long*)bwords, nw, bareas);
    } else {                                                                // the kernel ORs into bwords and adds into bareas
        if (int rc = miou_zero("mask_boundary_bits", bwords, bytes, st)) return rc;
        if (int rc = miou_zero("mask_boundary_bits", bareas, sizeof(int32_t) * (size_t)R, st)) return rc;
        const MbGeo g = mb_geometry(H, W, d);
        const size_t lds = sizeof(uint64_t) * (size_t)(g.TR + 2 * d) * (2 * g.TW + 2 * g.q);
        hipLaunchKernelGGL(mask_boundary_kernel, dim3(g.nxt * cdiv(H, g.TR), R), dim3(MB_THREADS), lds, st, (const unsigned long long*)words, g,
                           (unsigned long long*)bwords, bareas);
    }
    return check_launch("mask_boundary_bits");
}

extern "C" int cmk_mask_unpack_bits(const uint64_t* words, int R, int H, int W, uint8_t* masks, void* stream) {
    if (R == 0) return CMK_OK;
    if (int rc = miou_count_check("mask_unpack_bits", R)) return rc;
    if (int rc = miou_check("mask_unpack_bits", H, W, !words || !masks)) return rc;
    const int nw = miou_nw(H, W);
    hipLaunchKernelGGL(mask_unpack_kernel, miou_word_grid(R, nw), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)words, H * W, nw, masks);
    return check_launch("mask_unpack_bits");
}
