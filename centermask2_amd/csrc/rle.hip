// COCO run-length encoding of pasted bitmasks on the device (evaluation/coco_evaluation.py:362-427: the "segmentation" of a result is
// the compressed RLE of the (H,W) bitmask).  Format as in wire.py: runs of the column-major flattening (position p = x*H + y) starting
// with a zeros run, every count as 5-bit groups with a continuation bit, counts delta-coded against the count two back from the
// fourth on.
//
// Two phases around one host read of the run totals (the caller sizes the outputs exactly from them):
//   count : rle_count_kernel  — transitions per segment (mask, 64-row chunk, column), stored [mask][chunk][column]
//           rle_scan_kernel   — per mask, exclusive scan of the segments in column-major order (column, then chunk), in place;
//                               n_runs = 1 + transitions
//           rle_offsets_kernel— exclusive scan of n_runs over the masks (int64): where each mask's runs start in the packed outputs
//   encode: rle_starts_kernel — the count kernel's walk again; every transition writes its position at its scanned offset
//           rle_string_kernel — per mask: run lengths from neighbouring starts, characters per count, scan, bytes
// Each bitmap byte is read twice (count, starts); there are no atomics, and every store is an ordinary vector store.
//
// Memory is row-major and the runs are column-major, so a wave walks rows with its lanes on adjacent columns, 4 columns per lane in
// one dword.  W is arbitrary, so a row starts at any byte alignment: unless every row is aligned, a lane reads the two aligned dwords
// around its 4 bytes and funnel-shifts them (v_alignbyte); a wave for which one of those dwords would leave the buffer (the first
// bytes of an unaligned buffer, the last bytes of the last row) reads its columns byte by byte instead.
// A transition at (y, x) is m[y][x] != m[y-1][x]; at y = 0 the neighbour is m[H-1][x-1], so a run that goes on from the bottom of a
// column into the top of the next stays one run; (0, 0) compares with 0, which gives the zero-length first run of a mask that starts
// with a one.
#include "cmk_common.hpp"

namespace cmk {

constexpr int RLE_CH = 64;    // rows per segment; the 4 per-column counters of a lane are the bytes of one dword, so at most 255
constexpr int RLE_TW = 256;   // columns per wave: 4 per lane
constexpr int RLE_ROWS = 8;   // row loads a lane keeps in flight (16 measured the same at twice the registers)

// wave of this thread -> (chunk, first of the lane's 4 columns); false past the last unit (wave-uniform)
__device__ inline bool rle_unit(int W, int nchunks, int& c, int& x0) {
    const int ntiles = cdiv(W, RLE_TW);
    const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= (long)nchunks * ntiles) return false;
    c = (int)(u / ntiles);
    x0 = (int)(u % ntiles) * RLE_TW + (threadIdx.x & 63) * 4;
    return true;
}

// 0x01 in byte j where column x0 + j exists
__device__ inline uint32_t rle_colmask(int x0, int W) {
    const int n = W - x0;
    return n >= 4 ? 0x01010101u : (n == 3 ? 0x00010101u : (n == 2 ? 0x00000101u : 0x00000001u));
}

// how a wave reads its rows (the same for all its lanes)
enum { RLE_ALIGNED = 0, RLE_FUNNEL = 1, RLE_BYTES = 2 };

// the 4 bytes at a as one dword (byte j = column x0 + j; with RLE_ALIGNED / RLE_FUNNEL the bytes of columns >= W are whatever follows)
template <int MODE>
__device__ inline uint32_t rle_load4(const uint8_t* __restrict__ a, int ncols) {
    if (MODE == RLE_ALIGNED) return *(const uint32_t*)a;
    if (MODE == RLE_FUNNEL) {
        const uint32_t k = (uint32_t)((uintptr_t)a & 3);
        const uint32_t* d = (const uint32_t*)(a - k);
        return __builtin_amdgcn_alignbyte(d[1], d[0], k);
    }
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < ncols) v |= (uint32_t)a[j] << (8 * j);
    return v;
}

// what row 0 compares with: byte j = m[H-1][x0+j-1], 0 for column 0
__device__ inline uint32_t rle_wrap_prev(const uint8_t* __restrict__ img, int H, int W, int x0) {
    const uint8_t* last = img + (long)(H - 1) * W;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x > 0 && x < W) v |= (uint32_t)last[x - 1] << (8 * j);
    }
    return v;
}

// rows [y0, y1) of the lane's 4 columns, RLE_ROWS row loads in flight; f(y, t) gets 0x01 in byte j of t where (y, x0 + j) starts a run
template <int MODE, typename F>
__device__ inline void rle_walk_rows(const uint8_t* __restrict__ col, int W, int y0, int y1, uint32_t cm, int ncols, uint32_t prev, F& f) {
    int y = y0;
    for (; y + RLE_ROWS <= y1; y += RLE_ROWS) {
        uint32_t v[RLE_ROWS];
#pragma unroll
        for (int u = 0; u < RLE_ROWS; ++u) v[u] = rle_load4<MODE>(col + (long)(y + u) * W, ncols);
#pragma unroll
        for (int u = 0; u < RLE_ROWS; ++u) {
            f(y + u, (v[u] ^ prev) & cm);
            prev = v[u];
        }
    }
    for (; y < y1; ++y) {
        const uint32_t v = rle_load4<MODE>(col + (long)y * W, ncols);
        f(y, (v ^ prev) & cm);
        prev = v;
    }
}

// The walk both passes share.  Aligned rows (W % 4 == 0 on a 4-byte aligned buffer) take one dword per lane and row; other rows the
// two aligned dwords around the lane's bytes, if every lane of the wave finds them inside the buffer on all its rows; else bytes.
template <typename F>
__device__ inline void rle_walk(const uint8_t* __restrict__ masks, int R, int r, int H, int W, int c, int x0, F f) {
    const uint8_t* end = masks + (long)R * H * W;
    const uint8_t* img = masks + (long)r * H * W;
    const uint8_t* col = img + x0;
    const int ncols = min(4, W - x0);
    const uint32_t cm = rle_colmask(x0, W);
    const int y0 = c * RLE_CH, y1 = min(H, y0 + RLE_CH), yp = max(y0 - 1, 0);
    const uintptr_t first = (uintptr_t)(col + (long)yp * W) & ~(uintptr_t)3, last = (uintptr_t)(col + (long)(y1 - 1) * W) & ~(uintptr_t)3;
    const bool aligned = (W & 3) == 0 && ((uintptr_t)masks & 3) == 0;
    const bool inside = __all(first >= (uintptr_t)masks && last + 8 <= (uintptr_t)end);
    if (aligned) {
        const uint32_t prev = y0 ? rle_load4<RLE_ALIGNED>(col + (long)yp * W, ncols) : rle_wrap_prev(img, H, W, x0);
        rle_walk_rows<RLE_ALIGNED>(col, W, y0, y1, cm, ncols, prev, f);
    } else if (inside) {
        const uint32_t prev = y0 ? rle_load4<RLE_FUNNEL>(col + (long)yp * W, ncols) : rle_wrap_prev(img, H, W, x0);
        rle_walk_rows<RLE_FUNNEL>(col, W, y0, y1, cm, ncols, prev, f);
    } else {
        const uint32_t prev = y0 ? rle_load4<RLE_BYTES>(col + (long)yp * W, ncols) : rle_wrap_prev(img, H, W, x0);
        rle_walk_rows<RLE_BYTES>(col, W, y0, y1, cm, ncols, prev, f);
    }
}

// grid = (ceil(nchunks * ceil(W/256) / 4), R), 4 independent waves per workgroup
__global__ __launch_bounds__(256) void rle_count_kernel(const uint8_t* __restrict__ masks, int H, int W, int nchunks, int32_t* __restrict__ seg) {
    int c, x0;
    if (!rle_unit(W, nchunks, c, x0) || x0 >= W) return;
    const int r = blockIdx.y;
    uint32_t acc = 0;                                     // 4 byte counters, each <= RLE_CH
    rle_walk(masks, gridDim.y, r, H, W, c, x0, [&](int, uint32_t t) { acc += t; });
    int32_t* s = seg + ((long)r * nchunks + c) * W + x0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < W) s[j] = (int32_t)((acc >> (8 * j)) & 255u);
}

// exclusive scan over the 1024 threads of a workgroup; total = the sum of all.  lds: 17 words, free again on return.
template <typename T>
__device__ inline T rle_block_scan(T v, T* lds, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    if (w == 0) {
        const T s = lane < 16 ? lds[lane] : (T)0;
        T si = s;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const T t = __shfl_up(si, o, 64);
            if (lane >= o) si += t;
        }
        if (lane < 16) lds[lane] = si - s;
        if (lane == 15) lds[16] = si;
    }
    __syncthreads();
    const T res = lds[w] + inc - v;
    total = lds[16];
    __syncthreads();
    return res;
}

// grid = R.  seg[mask][chunk][column] counts -> exclusive offsets in (column, chunk) order; n_runs[mask] = 1 + transitions.
__global__ __launch_bounds__(1024) void rle_scan_kernel(int32_t* __restrict__ seg, int W, int nchunks, int32_t* __restrict__ n_runs) {
    __shared__ int32_t lds[17];
    int32_t* s = seg + (long)blockIdx.x * nchunks * W;
    int32_t carry = 0;
    for (long xb = 0; xb < W; xb += 1024) {
        const long x = xb + threadIdx.x;
        int32_t tot = 0;
        if (x < W) {
#pragma unroll 4
            for (int c = 0; c < nchunks; ++c) tot += s[(long)c * W + x];
        }
        int32_t total;
        int32_t ex = rle_block_scan(tot, lds, total) + carry;
        if (x < W) {
#pragma unroll 4
            for (int c = 0; c < nchunks; ++c) {
                const long i = (long)c * W + x;
                const int32_t t = s[i];
                s[i] = ex;
                ex += t;
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) n_runs[blockIdx.x] = carry + 1;
}

// one workgroup: run_off[r] = n_runs[0] + .. + n_runs[r-1], run_off[R] = all runs of the batch
__global__ __launch_bounds__(1024) void rle_offsets_kernel(const int32_t* __restrict__ n_runs, int R, long long* __restrict__ run_off) {
    __shared__ long long lds[17];
    long long carry = 0;
    for (int rb = 0; rb < R; rb += 1024) {
        const int r = rb + threadIdx.x;
        long long total;
        const long long ex = rle_block_scan<long long>(r < R ? (long long)n_runs[r] : 0, lds, total) + carry;
        if (r < R) run_off[r] = ex;
        carry += total;
    }
    if (threadIdx.x == 0) run_off[R] = carry;
}

// grid as rle_count_kernel.  starts[run_off[r] + i] = position where run i of mask r begins, for i in [1, n_runs); slot 0 is unused
// (run 0 begins at 0).
__global__ __launch_bounds__(256) void rle_starts_kernel(const uint8_t* __restrict__ masks, int H, int W, int nchunks, const int32_t* __restrict__ seg,
                                                        const long long* __restrict__ run_off, int32_t* __restrict__ starts) {
    int c, x0;
    if (!rle_unit(W, nchunks, c, x0) || x0 >= W) return;
    const int r = blockIdx.y;
    const int32_t* s = seg + ((long)r * nchunks + c) * W + x0;
    int32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (x0 + j < W) ? s[j] : 0;
    int32_t* st = starts + run_off[r] + 1;
    rle_walk(masks, gridDim.y, r, H, W, c, x0, [&](int y, uint32_t t) {
        if (t) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((t >> (8 * j)) & 1u) st[o[j]++] = (x0 + j) * H + y;
        }
    });
}

// grid = R.  counts[run_off[r] + i] = length of run i; bytes[7 * run_off[r] ..) = the compressed string, lens[r] characters.
__global__ __launch_bounds__(1024) void rle_string_kernel(const int32_t* __restrict__ starts, const int32_t* __restrict__ n_runs,
                                                         const long long* __restrict__ run_off, int HW, int32_t* __restrict__ counts,
                                                         uint8_t* __restrict__ bytes, long long* __restrict__ lens) {
    __shared__ int32_t lds[17];
    const int r = blockIdx.x;
    const int n = n_runs[r];
    const long long base = run_off[r];
    const int32_t* st = starts + base;
    int32_t* cn = counts + base;
    uint8_t* out = bytes + 7 * base;
    auto start_of = [&](int i) -> int32_t { return i <= 0 ? 0 : (i >= n ? HW : st[i]); };
    long long carry = 0;
    for (long ib = 0; ib < n; ib += 1024) {
        const long il = ib + threadIdx.x;
        const int i = (int)il;
        int32_t v = 0, nch = 0;
        if (il < n) {
            const int32_t len = start_of(i + 1) - start_of(i);
            cn[i] = len;
            v = len - (i > 2 ? start_of(i - 1) - start_of(i - 2) : 0);
            int32_t x = v;
            bool more;
            do {                                           // rle_to_string: stop when the shifted rest is all sign bits
                const int32_t ch = x & 31;
                x >>= 5;
                more = (ch & 16) ? (x != -1) : (x != 0);
                ++nch;
            } while (more);
        }
        int32_t total;
        const int32_t ex = rle_block_scan(nch, lds, total);
        if (il < n) {
            uint8_t* p = out + carry + ex;
            int32_t x = v;
            for (int k = 0; k < nch; ++k) {
                int32_t ch = x & 31;
                x >>= 5;
                if (k + 1 < nch) ch |= 32;
                p[k] = (uint8_t)(ch + 48);
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) lens[r] = carry;
}

inline int rle_nchunks(int H) { return cdiv(H, RLE_CH); }

inline int64_t rle_ws_bytes(int R, int H, int W) { return 8 * ((int64_t)R + 1) + 4 * (int64_t)R * rle_nchunks(H) * W; }

// shared argument check of the two phases; the messages name the entry
inline int rle_check(const char* what, int R, int H, int W, const void* ws, int64_t ws_bytes, bool any_null) {
    if (R < 0 || R > 65535) return fail(CMK_EINVAL, "%s: R = %ld outside [0, 65535]", what, R);
    if (H < 1 || W < 1) return fail(CMK_EINVAL, "%s: H = %ld, W = %ld must be at least 1", what, H, W);
    if ((int64_t)H * W >= 0x7fffffffLL) return fail(CMK_EINVAL, "%s: H*W of %ld x %ld does not leave int32 positions and run totals", what, H, W);
    if (any_null) return fail(CMK_EINVAL, "%s: null pointer", what);
    if ((uintptr_t)ws & 7) return fail(CMK_EINVAL, "%s: workspace is not 8-byte aligned", what);
    if (ws_bytes < rle_ws_bytes(R, H, W)) return fail(CMK_EINVAL, "%s: workspace of %ld bytes, need %ld", what, (long)ws_bytes, (long)rle_ws_bytes(R, H, W));
    return CMK_OK;
}

inline dim3 rle_walk_grid(int R, int H, int W) { return dim3(cdiv(rle_nchunks(H) * cdiv(W, RLE_TW), 4), R); }

}  // namespace cmk

using namespace cmk;

extern "C" int64_t cmk_rle_ws_bytes(int R, int H, int W) {
    if (R < 0 || R > 65535 || H < 1 || W < 1 || (int64_t)H * W >= 0x7fffffffLL) return 0;
    return rle_ws_bytes(R, H, W);
}

extern "C" int cmk_rle_count(const uint8_t* masks, int R, int H, int W, void* ws, int64_t ws_bytes, int32_t* n_runs, void* stream) {
    if (R == 0) return CMK_OK;
    if (int rc = rle_check("rle_count", R, H, W, ws, ws_bytes, !masks || !ws || !n_runs)) return rc;
    hipStream_t st = (hipStream_t)stream;
    long long* run_off = (long long*)ws;
    int32_t* seg = (int32_t*)(run_off + R + 1);
    const int nchunks = rle_nchunks(H);
    hipLaunchKernelGGL(rle_count_kernel, rle_walk_grid(R, H, W), dim3(256), 0, st, masks, H, W, nchunks, seg);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(R), dim3(1024), 0, st, seg, W, nchunks, n_runs);
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)n_runs, R, run_off);
    return check_launch("rle_count");
}

extern "C" int cmk_rle_encode(const uint8_t* masks, int R, int H, int W, const void* ws, int64_t ws_bytes, const int32_t* n_runs, int32_t* starts,
                              int32_t* counts, uint8_t* bytes, int64_t* lens, void* stream) {
    if (R == 0) return CMK_OK;
    if (int rc = rle_check("rle_encode", R, H, W, ws, ws_bytes, !masks || !ws || !n_runs || !starts || !counts || !bytes || !lens)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long* run_off = (const long long*)ws;
    const int32_t* seg = (const int32_t*)(run_off + R + 1);
    hipLaunchKernelGGL(rle_starts_kernel, rle_walk_grid(R, H, W), dim3(256), 0, st, masks, H, W, rle_nchunks(H), seg, run_off, starts);
    hipLaunchKernelGGL(rle_string_kernel, dim3(R), dim3(1024), 0, st, (const int32_t*)starts, n_runs, run_off, H * W, counts, bytes, (long long*)lens);
    return check_launch("rle_encode");
}
