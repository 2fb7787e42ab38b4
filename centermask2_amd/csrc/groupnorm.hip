// GroupNorm(groups, C) of dense NHWC tensors (fcos.py:182-186), in place (+ ReLU) or as the per-(image, channel) (scale, shift) a consumer
// conv applies while staging its input.  Stage 1: per (level, image, pixel chunk) fp64 sum / sum-of-squares per group, fixed order, or the
// records a conv epilogue left behind (cmk_conv_desc.gn_ws).  Stage 2: sum the records in index order, (mean, rstd) in double, then
// normalise or write (scale, shift).  The *_multi kernels do all FPN levels of one tower conv in one launch each (the per-level kernels
// are launch-latency sized); they are the single-level kernels with x, HW, the workspace row and the outputs taken from a level table, and
// stay kernels of their own because the table costs the single-level entry points 0.3-1.6 us per call (profiles/gn_dwconv_ab.txt).
#include "cmk_common.hpp"

namespace cmk {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one group's chunk records {sum, sumsq}, summed in index order
__device__ inline void gn_sum_records(const double* __restrict__ w, int chunks, double& a, double& b) {
    a = 0.0; b = 0.0;
    for (int k = 0; k < chunks; ++k) { a += w[2 * k]; b += w[2 * k + 1]; }
}

// group totals over cnt elements -> (mean, rstd)
__device__ inline void gn_mean_rstd(double a, double b, double cnt, float eps, float& mean, float& rstd) {
    const double m = a / cnt;
    double var = b / cnt - m * m;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// one channel's (scale, shift) from its group's (mean, rstd): x * scale + shift == (x - mean) * rstd * gamma + beta
__device__ inline void gn_affine(float mean, float rstd, float gamma, float beta, float& scale, float& shift) {
    scale = rstd * gamma;
    shift = beta - mean * scale;
}

// grid (chunks, N); ws records ((image*groups + group)*chunks + chunk) x {sum, sumsq}
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, double* __restrict__ ws, int HW, int C, int groups,
                                                      int chunks) {
    __shared__ double rs[256], rss[256];
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int G = C >> 2;                    // float4 groups per pixel (<= 256 required)
    const int ppl = 256 / G;
    const int per = cdiv(HW, chunks);
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    const float* xn = x + (long)n * HW * C;
    double s = 0.0, ss = 0.0;
    const int g = threadIdx.x % G, pl = threadIdx.x / G;
    if (pl < ppl) {
        for (int p = p0 + pl; p < p1; p += ppl) {
            f32x4 v = *reinterpret_cast<const f32x4*>(xn + (long)p * C + g * 4);
            s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
            ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
    rs[threadIdx.x] = s;
    rss[threadIdx.x] = ss;
    __syncthreads();
    if (threadIdx.x < groups) {
        const int f4pg = (C / groups) >> 2;  // float4 groups per GN group
        double a = 0.0, b = 0.0;
        for (int l = 0; l < ppl; ++l)
            for (int k = 0; k < f4pg; ++k) {
                a += rs[l * G + threadIdx.x * f4pg + k];
                b += rss[l * G + threadIdx.x * f4pg + k];
            }
        double* o = ws + (((long)n * groups + threadIdx.x) * chunks + chunk) * 2;
        o[0] = a;
        o[1] = b;
    }
}

// RELU false: GroupNorm alone, stored unclamped, so a NaN makes its group NaN as in torch (a clamp fmaxf(v, -inf) would give -inf).
// RELU true: fmaxf(v, 0) maps NaN to 0, as the GroupNorm + ReLU the conv kernels fuse into their input staging does.
template <bool RELU>
__global__ __launch_bounds__(256) void gn_apply_kernel(float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const double* __restrict__ ws, int HW, int C, int groups, int chunks, float eps,
                                                      int blocks_per_image) {
    __shared__ float s_mean[64], s_rstd[64];
    const int n = blockIdx.y;
    if (threadIdx.x < groups) {
        double a, b;
        gn_sum_records(ws + ((long)n * groups + threadIdx.x) * chunks * 2, chunks, a, b);
        gn_mean_rstd(a, b, (double)HW * (C / groups), eps, s_mean[threadIdx.x], s_rstd[threadIdx.x]);
    }
    __syncthreads();
    const int C4 = C >> 2;
    const int cpg = C / groups;
    float* xn = x + (long)n * HW * C;
    long total = (long)HW * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)blocks_per_image * 256) {
        int c4 = (int)(i % C4);
        int c = c4 * 4;
        int grp = c / cpg;
        float mean = s_mean[grp], rstd = s_rstd[grp];
        f32x4 v = *reinterpret_cast<f32x4*>(xn + i * 4);
        f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c);
        f32x4 be = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 o;
        o.x = (v.x - mean) * rstd * ga.x + be.x;
        o.y = (v.y - mean) * rstd * ga.y + be.y;
        o.z = (v.z - mean) * rstd * ga.z + be.z;
        o.w = (v.w - mean) * rstd * ga.w + be.w;
        if (RELU) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        *reinterpret_cast<f32x4*>(xn + i * 4) = o;
    }
}

// finalize: per (image, channel) scale/shift of GroupNorm for a consumer that applies it while staging its input
__global__ __launch_bounds__(256) void gn_finalize_kernel(const double* __restrict__ ws, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ out_scale,
                                                         float* __restrict__ out_shift, int HW, int C, int groups, int chunks, float eps) {
    __shared__ float s_mean[64], s_rstd[64];
    const int n = blockIdx.x;
    if (threadIdx.x < groups) {
        double a, b;
        gn_sum_records(ws + ((long)n * groups + threadIdx.x) * chunks * 2, chunks, a, b);
        gn_mean_rstd(a, b, (double)HW * (C / groups), eps, s_mean[threadIdx.x], s_rstd[threadIdx.x]);
    }
    __syncthreads();
    const int cpg = C / groups;
    for (int c = threadIdx.x; c < C; c += 256)
        gn_affine(s_mean[c / cpg], s_rstd[c / cpg], gamma[c], beta[c], out_scale[(long)n * C + c], out_shift[(long)n * C + c]);
}

// All FPN levels of one tower conv in one launch each: gn_stats_kernel and gn_finalize_kernel with grid z | y = level.
constexpr int GN_MAXL = 5;
struct GnLevels {
    const float* x[GN_MAXL];
    float* out_scale[GN_MAXL];
    float* out_shift[GN_MAXL];
    int HW[GN_MAXL];
    int nlev;
};

__global__ __launch_bounds__(256) void gn_stats_multi_kernel(const GnLevels L, double* __restrict__ ws, int N, int C, int groups, int chunks) {
    __shared__ double rs[256], rss[256];
    const int chunk = blockIdx.x, n = blockIdx.y, l = blockIdx.z;
    const int HW = L.HW[l];
    const int G = C >> 2;
    const int ppl = 256 / G;
    const int per = cdiv(HW, chunks);
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    const float* xn = L.x[l] + (long)n * HW * C;
    double s = 0.0, ss = 0.0;
    const int g = threadIdx.x % G, pl = threadIdx.x / G;
    if (pl < ppl) {
        for (int p = p0 + pl; p < p1; p += ppl) {
            f32x4 v = *reinterpret_cast<const f32x4*>(xn + (long)p * C + g * 4);
            s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
            ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    }
    rs[threadIdx.x] = s;
    rss[threadIdx.x] = ss;
    __syncthreads();
    if (threadIdx.x < groups) {
        const int f4pg = (C / groups) >> 2;
        double a = 0.0, b = 0.0;
        for (int k = 0; k < ppl; ++k)
            for (int q = 0; q < f4pg; ++q) {
                a += rs[k * G + threadIdx.x * f4pg + q];
                b += rss[k * G + threadIdx.x * f4pg + q];
            }
        double* o = ws + ((((long)l * N + n) * groups + threadIdx.x) * chunks + chunk) * 2;
        o[0] = a;
        o[1] = b;
    }
}

__global__ __launch_bounds__(256) void gn_finalize_multi_kernel(const GnLevels L, const double* __restrict__ ws, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int N, int C, int groups, int chunks, float eps) {
    __shared__ float s_mean[64], s_rstd[64];
    const int n = blockIdx.x, l = blockIdx.y;
    if (threadIdx.x < groups) {
        double a, b;
        gn_sum_records(ws + (((long)l * N + n) * groups + threadIdx.x) * chunks * 2, chunks, a, b);
        gn_mean_rstd(a, b, (double)L.HW[l] * (C / groups), eps, s_mean[threadIdx.x], s_rstd[threadIdx.x]);
    }
    __syncthreads();
    const int cpg = C / groups;
    for (int c = threadIdx.x; c < C; c += 256)
        gn_affine(s_mean[c / cpg], s_rstd[c / cpg], gamma[c], beta[c], L.out_scale[l][(long)n * C + c], L.out_shift[l][(long)n * C + c]);
}

struct GnTileLevels {
    float* out_scale[GN_MAXL];
    float* out_shift[GN_MAXL];
    int HW[GN_MAXL], tile_begin[GN_MAXL], tiles[GN_MAXL];
};
// statistics written by the conv epilogue (cmk_conv_desc.gn_ws): records ((tile*2 + parity)*groups + group) x {sum, sumsq}
__global__ __launch_bounds__(256) void gn_finalize_tiles_kernel(const GnTileLevels L, const double* __restrict__ ws, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int N, int C, int groups, float eps) {
    __shared__ double rs[256], rss[256];
    __shared__ float s_mean[64], s_rstd[64];
    const int n = blockIdx.x, l = blockIdx.y;
    const int parts = 256 / groups;                       // thread = (part, group): consecutive threads read consecutive groups
    const int g = threadIdx.x % groups, part = threadIdx.x / groups;
    double a = 0.0, b = 0.0;
    if (part < parts) {
        const long r0 = (long)L.tile_begin[l] + (long)n * L.tiles[l];      // "tiles" here = records per image
        const int nrec = L.tiles[l];
        double a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0, a3 = 0.0, b3 = 0.0;      // four independent chains: the loads overlap
        int r = part;
        for (; r + 3 * parts < nrec; r += 4 * parts) {
            const double* w = ws + ((r0 + r) * groups + g) * 2;
            const long st = (long)parts * groups * 2;
            a += w[0]; b += w[1];
            a1 += w[st]; b1 += w[st + 1];
            a2 += w[2 * st]; b2 += w[2 * st + 1];
            a3 += w[3 * st]; b3 += w[3 * st + 1];
        }
        for (; r < nrec; r += parts) {
            const double* w = ws + ((r0 + r) * groups + g) * 2;
            a += w[0];
            b += w[1];
        }
        a += a1 + a2 + a3;
        b += b1 + b2 + b3;
    }
    rs[threadIdx.x] = a;
    rss[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x < groups) {
        a = 0.0; b = 0.0;
        for (int k = 0; k < parts; ++k) { a += rs[k * groups + threadIdx.x]; b += rss[k * groups + threadIdx.x]; }
        gn_mean_rstd(a, b, (double)L.HW[l] * (C / groups), eps, s_mean[threadIdx.x], s_rstd[threadIdx.x]);
    }
    __syncthreads();
    const int cpg = C / groups;
    for (int c = threadIdx.x; c < C; c += 256)
        gn_affine(s_mean[c / cpg], s_rstd[c / cpg], gamma[c], beta[c], L.out_scale[l][(long)n * C + c], L.out_shift[l][(long)n * C + c]);
}

// what gn_stats_kernel's thread mapping and the 64-entry mean/rstd tables can take
static bool gn_shape_ok(int C, int groups, int ws_chunks) {
    return !((C & 3) || C < 4 || C > 1024 || groups < 1 || groups > 64 || C % groups || ((C / groups) & 3) || 256 % (C >> 2) || ws_chunks < 1);
}

}  // namespace cmk

using namespace cmk;

static int groupnorm_inplace(float* x, const float* gamma, const float* beta, double* ws, int ws_chunks, int N, int HW, int C, int groups, float eps,
                             bool relu, void* stream) {
    if (!x || !gamma || !beta || !ws) return fail(CMK_EINVAL, "groupnorm: null pointer%s", "");
    if (!gn_shape_ok(C, groups, ws_chunks)) return fail(CMK_EINVAL, "groupnorm: unsupported C/groups%s", "");
    if (N < 1 || HW < 1) return fail(CMK_EINVAL, "groupnorm: N, H*W >= 1%s", "");
    hipLaunchKernelGGL(gn_stats_kernel, dim3(ws_chunks, N), dim3(256), 0, (hipStream_t)stream, x, ws, HW, C, groups, ws_chunks);
    int rc = check_launch("gn_stats");
    if (rc) return rc;
    long total = (long)HW * (C >> 2);
    int bpi = stream_grid(total);
    if (bpi > 1024) bpi = 1024;
    hipLaunchKernelGGL(relu ? gn_apply_kernel<true> : gn_apply_kernel<false>, dim3(bpi, N), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, ws,
                       HW, C, groups, ws_chunks, eps, bpi);
    return check_launch("gn_apply");
}

extern "C" int cmk_groupnorm_relu_nhwc(float* x, const float* gamma, const float* beta, double* ws, int ws_chunks, int N, int HW, int C,
                                       int groups, float eps, void* stream) {
    return groupnorm_inplace(x, gamma, beta, ws, ws_chunks, N, HW, C, groups, eps, true, stream);
}

extern "C" int cmk_groupnorm_nhwc(float* x, const float* gamma, const float* beta, double* ws, int ws_chunks, int N, int HW, int C,
                                  int groups, float eps, void* stream) {
    return groupnorm_inplace(x, gamma, beta, ws, ws_chunks, N, HW, C, groups, eps, false, stream);
}

extern "C" int cmk_groupnorm_affine(const float* x, const float* gamma, const float* beta, double* ws, int ws_chunks, int N, int HW, int C,
                                    int groups, float eps, float* out_scale, float* out_shift, void* stream) {
    if (!x || !gamma || !beta || !ws || !out_scale || !out_shift) return fail(CMK_EINVAL, "groupnorm_affine: null pointer%s", "");
    if (!gn_shape_ok(C, groups, ws_chunks)) return fail(CMK_EINVAL, "groupnorm_affine: unsupported C/groups%s", "");
    if (N < 1 || HW < 1) return fail(CMK_EINVAL, "groupnorm_affine: N, H*W >= 1%s", "");
    hipLaunchKernelGGL(gn_stats_kernel, dim3(ws_chunks, N), dim3(256), 0, (hipStream_t)stream, x, ws, HW, C, groups, ws_chunks);
    int rc = check_launch("gn_stats");
    if (rc) return rc;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, ws, gamma, beta, out_scale, out_shift, HW, C, groups,
                       ws_chunks, eps);
    return check_launch("gn_finalize");
}

extern "C" int cmk_groupnorm_affine_multi(const float* const* xs, const int* HWs, int nlev, const float* gamma, const float* beta, double* ws,
                                          int ws_chunks, int N, int C, int groups, float eps, float* const* out_scale, float* const* out_shift,
                                          void* stream) {
    if (!xs || !HWs || !gamma || !beta || !ws || !out_scale || !out_shift) return fail(CMK_EINVAL, "groupnorm_affine_multi: null pointer%s", "");
    if (nlev < 1 || nlev > GN_MAXL) return fail(CMK_EINVAL, "groupnorm_affine_multi: 1..5 levels%s", "");
    if (!gn_shape_ok(C, groups, ws_chunks)) return fail(CMK_EINVAL, "groupnorm_affine_multi: unsupported C/groups%s", "");
    if (N < 1) return fail(CMK_EINVAL, "groupnorm_affine_multi: N >= 1%s", "");
    GnLevels L;
    L.nlev = nlev;
    for (int l = 0; l < GN_MAXL; ++l) {
        bool ok = l < nlev;
        if (ok && (!xs[l] || !out_scale[l] || !out_shift[l] || HWs[l] < 1)) return fail(CMK_EINVAL, "groupnorm_affine_multi: bad level%s", "");
        L.x[l] = ok ? xs[l] : nullptr; L.out_scale[l] = ok ? out_scale[l] : nullptr; L.out_shift[l] = ok ? out_shift[l] : nullptr;
        L.HW[l] = ok ? HWs[l] : 1;
    }
    hipLaunchKernelGGL(gn_stats_multi_kernel, dim3(ws_chunks, N, nlev), dim3(256), 0, (hipStream_t)stream, L, ws, N, C, groups, ws_chunks);
    int rc = check_launch("gn_stats_multi");
    if (rc) return rc;
    hipLaunchKernelGGL(gn_finalize_multi_kernel, dim3(N, nlev), dim3(256), 0, (hipStream_t)stream, L, ws, gamma, beta, N, C, groups, ws_chunks, eps);
    return check_launch("gn_finalize_multi");
}

extern "C" int cmk_groupnorm_affine_tiles(const double* ws, const int* Hs, const int* Ws, const int* recs, int nlev, const float* gamma, const float* beta, int N,
                                          int C, int groups, float eps, float* const* out_scale, float* const* out_shift, void* stream) {
    if (!ws || !Hs || !Ws || !recs || !gamma || !beta || !out_scale || !out_shift) return fail(CMK_EINVAL, "groupnorm_affine_tiles: null pointer%s", "");
    if (nlev < 1 || nlev > GN_MAXL || N < 1) return fail(CMK_EINVAL, "groupnorm_affine_tiles: 1..5 levels%s", "");
    if (groups < 1 || groups > 64 || C % groups || C > 4096) return fail(CMK_EINVAL, "groupnorm_affine_tiles: unsupported C/groups%s", "");
    GnTileLevels L;
    int begin = 0;
    for (int l = 0; l < GN_MAXL; ++l) {
        const bool ok = l < nlev;
        if (ok && (!out_scale[l] || !out_shift[l] || Hs[l] < 1 || Ws[l] < 1 || recs[l] < 1)) return fail(CMK_EINVAL, "groupnorm_affine_tiles: bad level%s", "");
        L.out_scale[l] = ok ? out_scale[l] : nullptr; L.out_shift[l] = ok ? out_shift[l] : nullptr;
        L.HW[l] = ok ? Hs[l] * Ws[l] : 1;
        L.tiles[l] = ok ? recs[l] : 0;                                     // cmk_conv_gn_records of the producing conv
        L.tile_begin[l] = begin;
        begin += N * L.tiles[l];
    }
    hipLaunchKernelGGL(gn_finalize_tiles_kernel, dim3(N, nlev), dim3(256), 0, (hipStream_t)stream, L, ws, gamma, beta, N, C, groups, eps);
    return check_launch("gn_finalize_tiles");
}
