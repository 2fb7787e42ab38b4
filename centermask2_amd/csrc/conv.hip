// The conv front door of libcmk_hip.so: every extern "C" conv entry point, the validation of descriptors, the choice of a kernel for
// a launch (resolve), its launch or the plan of it (dispatch, run; conv_args.hpp LaunchPlan) and the split-K reduce kernel that finishes
// the launches of every kernel file that leaves raw partial sums (conv_igemm.hip, conv_wino6.hip, conv_pw.hip).  The kernels live in files
// of their own (conv_args.hpp).
#include <algorithm>

#include "conv_args.hpp"

namespace cmk {

// split-K second pass: y = epilogue(sum_z ws[z]); one thread = 4 couts of one pixel
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int ksplit, long total_pix, int cout_pad,
                                                           const float* __restrict__ scale, const float* __restrict__ shift, int Cout,
                                                           int relu_upto, const float* __restrict__ res, int res_cs, int res_co,
                                                           float* __restrict__ y, int y_cs, int y_co) {
    const int c4n = cout_pad >> 2;
    const long total = total_pix * c4n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long pix = i / c4n;
        const int co = (int)(i - pix * c4n) * 4;
        if (co >= Cout) continue;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < ksplit; ++z) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(ws + ((long)z * total_pix + pix) * cout_pad + co);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = co + j;
            if (c < Cout) {
                float v = s[j] * scale[c] + shift[c];
                if (res) v += res[pix * res_cs + res_co + c];
                if (c < relu_upto) v = fmaxf(v, 0.f);
                y[pix * y_cs + y_co + c] = v;
            }
        }
    }
}

static int validate(const cmk_conv_desc* d) {
    if (!d || !d->x || !d->w || !d->y || !d->scale || !d->shift) return fail(CMK_EINVAL, "conv: null pointer%s", "");
    if (d->ksize != 1 && d->ksize != 3) return fail(CMK_EINVAL, "conv: ksize must be 1 or 3%s", "");
    if (d->stride != 1 && d->stride != 2) return fail(CMK_EINVAL, "conv: stride must be 1 or 2%s", "");
    if (d->ksize == 1 && d->stride != 1) return fail(CMK_EINVAL, "conv: 1x1 stride 2 unsupported%s", "");
    if (d->Cin <= 0 || (d->Cin & 15)) return fail(CMK_EINVAL, "conv: Cin (%s%ld) must be a positive multiple of 16", "", d->Cin);
    if (d->Cout <= 0 || d->N <= 0 || d->H <= 0 || d->W <= 0) return fail(CMK_EINVAL, "conv: empty shape%s", "");
    if ((d->x_cs & 3) || (d->x_co & 3)) return fail(CMK_EINVAL, "conv: input view must be 16-byte aligned per pixel%s", "");
    if (((uintptr_t)d->x & 15) || ((uintptr_t)d->w & 15)) return fail(CMK_EINVAL, "conv: x/w must be 16-byte aligned%s", "");
    if (d->x_co + d->Cin > d->x_cs || d->y_co + d->Cout > d->y_cs) return fail(CMK_EINVAL, "conv: channel view out of range%s", "");
    if (d->res_mode < 0 || d->res_mode > 2 || (d->res_mode && !d->res)) return fail(CMK_EINVAL, "conv: bad residual%s", "");
    if ((d->in_scale == nullptr) != (d->in_shift == nullptr)) return fail(CMK_EINVAL, "conv: in_scale and in_shift come together%s", "");
    if (d->in_scale && d->ksize == 1 && ((long)d->H * d->W) % 256) return fail(CMK_EINVAL, "conv: input affine on a 1x1 conv needs H*W %% 256 == 0%s", "");
    if (d->pool_ws && d->ksize != 1) return fail(CMK_EINVAL, "conv: pooled sums are for 1x1 convs%s", "");
    return CMK_OK;
}

// the checks of cmk_conv2d_nhwc_multi, on the caller's own tune fields
static int validate_multi(const cmk_conv_desc* descs, int n) {
    if (!descs || n < 1 || n > MAXP) return fail(CMK_EINVAL, "conv_multi: need 1..%s%ld problems", "", MAXP);
    bool same_w = true;
    for (int i = 0; i < n; ++i) {
        int rc = validate(&descs[i]);
        if (rc) return rc;
        const cmk_conv_desc *a = &descs[0], *b = &descs[i];
        same_w = same_w && b->w == a->w && b->w_wino == a->w_wino && b->w_wino6 == a->w_wino6 && b->w_split == a->w_split && b->w_splith == a->w_splith;
        if (b->Cin != a->Cin || b->Cout != a->Cout || b->ksize != a->ksize || b->stride != a->stride ||
            b->relu_upto != a->relu_upto || b->in_relu != a->in_relu || b->x_cs != a->x_cs || b->x_co != a->x_co || b->y_cs != a->y_cs ||
            b->y_co != a->y_co || b->res_mode != 0 || b->tune_wm != a->tune_wm || b->tune_sc != a->tune_sc || b->tune_wn != a->tune_wn || (b->in_scale == nullptr) != (a->in_scale == nullptr) ||
            b->gn_ws != a->gn_ws || b->gn_groups != a->gn_groups || b->splitk > 1 || b->pool_ws)
            return fail(CMK_EINVAL, "conv_multi: problems must share channels/views/flags and carry no residual%s", "");
    }
    // problems with different weights (the cls and the bbox tower of the FCOS head, fcos.py:227-231, in one launch) and more than 5 problems:
    // the F(4x4) kernels only, which take the packed weights per problem
    if ((!same_w || n > 5) && (descs[0].tune_wm != 6 || descs[0].tune_wn != 1) && descs[0].tune_wm != 11)
        return fail(CMK_EINVAL, "conv_multi: different weights per problem / more than 5 problems need tune_wm 6, tune_wn 1 (the F(4x4) map kernels)%s", "");
    for (int i = 0; i < n; ++i)
        if (descs[0].tune_wm == 6 && !descs[i].w_wino6) return fail(CMK_EINVAL, "conv_multi: w_wino6 missing%s", "");
    return CMK_OK;
}

static void fill_problem(ConvProblem& p, const cmk_conv_desc* d) {
    p.x = d->x; p.y = d->y; p.scale = d->scale; p.shift = d->shift;
    p.in_scale = d->in_scale; p.in_shift = d->in_shift;
    p.w = d->w_wino6;
    p.N = d->N; p.H = d->H; p.W = d->W;
    p.Ho = out_size(d->H, d->stride);
    p.Wo = out_size(d->W, d->stride);
    p.tiles_h = p.tiles_w = p.tile_begin = 0;
    p.total_pix = (long)p.N * p.Ho * p.Wo;
}

static int setup_gn(ConvArgs& a, const cmk_conv_desc* d) {
    const int cpg = d->gn_groups > 0 ? d->Cout / d->gn_groups : 0;
    if (d->relu_upto != 0 || d->gn_groups < 1 || d->Cout % d->gn_groups || cpg > 32 || (cpg & (cpg - 1)))
        return fail(CMK_EINVAL, "conv: fused GroupNorm statistics need relu_upto == 0 and a power-of-two group width <= 32%s", "");
    a.gn_ws = d->gn_ws; a.gn_cpg = cpg; a.gn_groups = d->gn_groups;
    return CMK_OK;
}

// The tile height (4 | 2) with which descriptor d runs on the pointwise GEMM kernel (conv_pw.hip), 0 if it does not: tune_wm 8 as given, or
// the untuned default — 1x1 convs with enough pixels and output channels to fill the chip (measured 1.12-1.2x conv_igemm on every concat /
// lateral / deconv shape of the model, tools/conv_probe.py time --set pw -v 1/32/4 8/32/4 8/32/2), 256-pixel workgroups from 2 rounds on.
static int pointwise_mt(const cmk_conv_desc* d, int n) {
    const int cout32 = (d->Cout + 31) / 32;
    const long total_pix = (long)d->N * d->H * d->W;
    if (d->ksize != 1 || n != 1 || cout32 <= 7 || (d->Cin & 31) || d->in_scale || d->in_relu || d->gn_ws || total_pix * d->x_cs * 4 >= (1L << 31))
        return 0;
    if (d->splitk > 1 && (d->tune_wm != 8 || !d->splitk_ws || d->res_mode == 2 || d->pool_ws || (d->Cin >> 4) % (2 * d->splitk))) return 0;
    if (d->res_mode == 2 && ((d->W & 1) || d->pool_ws || (long)d->N * d->Hr * d->Wr * d->res_cs * 4 >= (1L << 31))) return 0;     // FPN top-down add: even widths
    if (d->tune_wm == 8) return (d->tune_wn == 4 || d->tune_wn == 2) ? d->tune_wn : 0;
    if (d->tune_wm == 10) return (d->w_split && d->tune_wn == 4 && d->res_mode != 1 && d->splitk <= 1) ? 4 : 0;      // the bf16-split form: the 256-pixel tile
    if (d->tune_wm == 12) return (d->w_splith && d->tune_wn == 4 && d->res_mode != 1 && d->splitk <= 1) ? 4 : 0;     // the fp16-split form
    if (d->tune_wm || d->tune_sc || d->tune_wn) return 0;
    const long ctiles = cdiv(cout32, 4);
    const long wg2 = ((total_pix + 127) / 128) * ctiles, wg4 = ((total_pix + 255) / 256) * ctiles;
    return wg2 >= 256 ? (wg4 >= 1024 ? 4 : 2) : 0;
}

// The same for the gather form of a 3x3 conv on that kernel (tune_wm 9, or the untuned default for stride-2 convs of at least 1024
// 256-pixel workgroups: stem_3).
static int gather_mt(const cmk_conv_desc* d, int n) {
    const int cout32 = (d->Cout + 31) / 32;
    const long in_pix = (long)d->N * d->H * d->W;
    const long out_pix = (long)d->N * (d->stride == 1 ? d->H : (d->H - 1) / 2 + 1) * (d->stride == 1 ? d->W : (d->W - 1) / 2 + 1);
    if (d->ksize != 3 || n != 1 || (cout32 != 4 && cout32 <= 7) || (d->Cin & 31) || d->in_scale || d->in_relu || d->res_mode == 2 ||
        d->gn_ws || d->pool_ws || in_pix * d->x_cs * 4 >= (1L << 31) || d->H >= 32768 || d->W >= 32768)
        return 0;
    if (d->splitk > 1 && (d->tune_wm != 9 || !d->splitk_ws || (9 * (d->Cin >> 4)) % (2 * d->splitk))) return 0;
    if (d->tune_wm == 9) return (d->tune_wn == 4 || d->tune_wn == 2) ? d->tune_wn : 0;
    if (d->tune_wm == 10) return (d->w_split && d->tune_wn == 4 && d->res_mode == 0 && d->splitk <= 1) ? 4 : 0;      // the bf16-split gather form
    if (d->tune_wm == 12) return (d->w_splith && d->tune_wn == 4 && d->res_mode == 0 && d->splitk <= 1) ? 4 : 0;     // the fp16-split gather form
    if (d->tune_wm || d->tune_sc || d->tune_wn || d->stride != 2) return 0;
    const long ctiles = cdiv(cout32, 4);
    const long wg4 = ((out_pix + 255) / 256) * ctiles;
    return wg4 >= 1024 ? 4 : 0;          // measured (tools/conv_probe.py time --set s2 -v tuned 9/32/4 9/32/2): stem_3 1.28x conv_igemm; the 14 -> 7 maskiou conv and P6/P7 stay on its split-K gather form
}

// The variant a launch of these (validated) descriptors runs: the caller's tune fields as given, or the untuned default when they are all
// zero.  gn: the launch produces fused GroupNorm statistics (gn_ws set, or cmk_conv_resolve's with_gn_stats) — the forms that do are
// preferred; when none applies, the choice among the others.
static Variant resolve(const cmk_conv_desc* descs, int n, bool gn) {
    const cmk_conv_desc* d = &descs[0];
    if (d->tune_wm || d->tune_sc || d->tune_wn) return Variant{d->tune_wm, d->tune_sc, d->tune_wn};     // the caller measured and picked one
    // the 2-WG/CU Winograd form wins on every 3x3 stride-1 shape measured (tools/conv_probe.py time --set v39 roi -v 1/16/4 5/16/2), so take it whenever the caller packed the
    // transformed weights; otherwise the direct-kernel cost model decides
    const bool wino = d->ksize == 3 && d->stride == 1 && d->res_mode == 0 && !d->in_relu && d->Cin >= 32 && d->splitk <= 1;
    // F(4x4,3x3) where its 12x40 tiles are reasonably full and there are enough of them (measured on the model's maps, tools/conv_probe.py time --set v39 roi -v 5/16/2 6/16/roi:
    // 1.1-1.5x the 2x2 form down to 25x40 maps, 0.4x on 14x14 RoI maps whose tiles are 20 % full)
    if (wino && d->w_wino6 && !(d->Cin & 7)) {
        double px = 0.0, covered = 0.0;
        long wgs = 0;
        for (int i = 0; i < n; ++i) {
            const long t = (long)descs[i].N * cdiv(descs[i].H, 12) * cdiv(descs[i].W, 40);
            px += (double)descs[i].N * descs[i].H * descs[i].W;
            covered += (double)t * 480.0;
            wgs += t * cdiv(d->Cout, 32);
        }
        // maps of at most 16 x 14 (the 14x14 RoI features): two whole maps per workgroup instead of 12x40 tiles that would be 20 % full
        if (n == 1 && d->H <= 16 && d->W <= 14 && !gn && (long)cdiv(d->N, 2) * cdiv(d->Cout, 32) >= 256) return Variant{6, 16, 2};
        if (px >= 0.55 * covered && wgs >= 256) return Variant{6, 16, 1};
    }
    if (wino && d->w_wino) return Variant{5, 16, 2};
    const int cout32 = (d->Cout + 31) / 32;
    const int ho = out_size(d->H, d->stride), wo = out_size(d->W, d->stride);
    // stride-2 3x3 on a map of at most 16x16 outputs (maskiou conv4 14->7, P6/P7): the spatial tiles would be mostly empty
    if (d->ksize == 3 && d->stride == 2 && n == 1 && d->res_mode != 2 && !d->in_scale && ho <= 16 && wo <= 16) {
        const int cout_pad32 = cout32 <= 7 ? cout32 : cdiv(cout32, 4) * 4;
        const long total_pix = (long)d->N * ho * wo;
        return Variant{7, 32, (cout_pad32 % 4 == 0 && total_pix >= 8192) ? 4 : (cout_pad32 % 2 == 0 && total_pix >= 2048) ? 2 : 1};
    }
    if (const int mt = pointwise_mt(d, n)) return Variant{8, 32, mt};
    if (const int mt = gather_mt(d, n)) return Variant{9, 32, mt};
    return choose_variant(descs, n, d->ksize * d->ksize, d->stride, cout32);
}

// Workgroup slots of the current device for the F(4x4) kernels: CUs x 2 (conv_wino6_kernel, two workgroups per CU) or x 1 (the paired
// form); read once per device.  0 when no device answers (the tail is then off).
static int wino6_slots(bool pair) {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = __atomic_load_n(&cus[dev], __ATOMIC_ACQUIRE);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
        __atomic_store_n(&cus[dev], n, __ATOMIC_RELEASE);
    }
    return pair ? n : 2 * n;
}

// The tail of a descriptor (cmk.h splitk_tail): spatial tiles and ways, 0 / 0 when it is off or the plan finds no ragged round to fill.
static void wino6_tail_of(const cmk_conv_desc* d, int& tiles, int& ways) {
    tiles = ways = 0;
    if (d->splitk_tail <= 1 || d->tune_wm != 6 || d->tune_wn != 2 || (d->tune_sc != 0 && d->tune_sc != 16 && d->tune_sc != 32)) return;
    const int st = cdiv(d->N, 2), pairs = d->Cin >> 4;
    if (d->splitk_tail_tiles > 0) {          // as given (tests; a caller with a plan of its own)
        tiles = std::min(d->splitk_tail_tiles, st);
        ways = d->splitk_tail;
        return;
    }
    const bool pair = d->tune_sc == 32;
    const int ct = cdiv(d->Cout, 32);
    int pt = 0, pw = 0;
    cmk_wino6_tail_plan(st, pair ? cdiv(ct, 2) : ct, pairs, wino6_slots(pair), &pt, &pw);
    if (pt > 0) { tiles = pt; ways = std::min(d->splitk_tail, pw); }
}

// The kernels that produce fused GroupNorm statistics: the Winograd forms and the direct fp16-split 3x3
static bool writes_gn_records(int tune_wm) { return tune_wm == 5 || tune_wm == 6 || tune_wm == 11; }

// The launch of the explicit variant d->tune_wm/sc/wn (d: the first descriptor, resolved).  Returns with a.ksplit > 1 when the kernel left
// split-K partial sums for run() to reduce.  plan: conv_args.hpp LaunchPlan.
static int dispatch(ConvArgs& a, const cmk_conv_desc* d, const cmk_conv_desc* descs, int n, hipStream_t st, LaunchPlan* plan) {
    const int cout32 = (d->Cout + 31) / 32;
    const int cout_pad128 = cdiv(cout32, 4) * 128;      // Cout padded to the 128 couts of a conv_pw / conv_sp3 workgroup column
    if (d->gn_ws) {
        if (!writes_gn_records(d->tune_wm))
            return fail(CMK_EINVAL, "conv: fused GroupNorm statistics are only produced by the Winograd form%s", "");
        int rc = setup_gn(a, d);
        if (rc) return rc;
    }
    if (d->splitk_tail > 1 && d->tune_wm != 6)      // (tune_wm 6 sorts out its own forms below)
        return fail(CMK_EINVAL, "conv: tail split-K is a feature of the RoI-pair F(4x4) forms (tune_wm 6, tune_wn 2, tune_sc 16 or 32)%s", "");
    if (d->tune_wm == 5) {          // Winograd F(2x2,3x3): 3x3 stride 1, no residual / input ReLU
        if (d->ksize != 3 || d->stride != 1 || d->res_mode != 0 || d->in_relu || !d->w_wino)
            return fail(CMK_EINVAL, "conv: Winograd variant not available for this conv%s", "");
        if (d->splitk > 1) return fail(CMK_EINVAL, "conv: split-K is a direct-kernel feature%s", "");
        a.w = d->w_wino;
        return launch_wino4r(a, st, plan);
    }
    if (d->tune_wm == 6) {          // Winograd F(4x4,3x3): same conditions, its own packed weights
        if (d->ksize != 3 || d->stride != 1 || d->res_mode != 0 || d->in_relu || !d->w_wino6 || (d->Cin & 7))
            return fail(CMK_EINVAL, "conv: Winograd F(4x4,3x3) variant not available for this conv%s", "");
        a.w = d->w_wino6;
        a.ws = d->splitk_ws;          // split-K slabs
        a.ksplit = d->splitk > 1 ? d->splitk : 1;
        a.cout_pad = cmk_conv_cout_pad(d->Cout);
        if (d->tune_sc != 0 && d->tune_sc != 16 && d->tune_sc != 32 && d->tune_sc != 64)
            return fail(CMK_EINVAL, "conv: tune_wm 6 takes tune_sc 16 (32 couts per workgroup), 32 (paired) or 64 (shared V)%s", "");
        const bool pair = d->tune_sc == 32;      // 64 couts per workgroup, halo and pass 1 shared by the two cout tiles
        if (d->splitk_tail > 1) {     // tail split-K (cmk.h splitk_tail): only the ragged last round of a RoI-pair launch is split
            if (d->tune_sc == 64 || d->tune_wn != 2 || n != 1 || d->gn_ws || a.ksplit > 1)
                return fail(CMK_EINVAL, "conv: Winograd tail split-K needs tune_sc 16 or 32, tune_wn 2, one problem, no GroupNorm statistics and no splitk beside it%s", "");
            wino6_tail_of(d, a.tail_tiles, a.tail_ksplit);
            if (a.tail_tiles > 0 && !d->splitk_ws) return fail(CMK_EINVAL, "conv: Winograd tail split-K needs a workspace (cmk_conv_tail_ws_floats)%s", "");
        }
        if (a.ksplit > 1) {           // F(4x4) with split-K (conv_wino6.hip forms): partial sums + the reduce kernel above
            if (d->tune_sc == 64 || (d->tune_wn != 1 && d->tune_wn != 2) || n != 1) return fail(CMK_EINVAL, "conv: Winograd split-K needs tune_sc 16 or 32, tune_wn 1 or 2, one problem%s", "");
            return launch_wino6(a, d->tune_wn == 2 ? 1 : 0, pair, st, plan);       // (tune_wn 2: run as the tail that takes every tile)
        }
        if (d->tune_wn != 1 && d->tune_wn != 2) return fail(CMK_EINVAL, "conv: tune_wm 6 takes tune_wn 1 (12x40 map tiles) or 2 (pairs of RoI maps up to 16x14)%s", "");
        if (d->tune_sc == 64) return launch_wino6s(a, d->tune_wn == 2 ? 1 : 0, st, plan);      // 64 couts per workgroup, shared frequency image
        return launch_wino6(a, d->tune_wn == 2 ? 1 : 0, pair, st, plan);
    }
    a.ksplit = d->splitk > 1 ? d->splitk : 1;
    a.ws = d->splitk_ws;
    if (d->pool_ws && !pointwise_mt(d, n)) return fail(CMK_EINVAL, "conv: pooled sums are produced by the pointwise GEMM kernel only (cmk_conv_pool_rows)%s", "");
    a.pool_ws = d->pool_ws;
    if (d->tune_wm == 8) {                             // pointwise GEMM kernel (conv_pw.hip); tune_wn = accumulator rows per wave
        if (d->ksize != 1 || cout32 <= 7) return fail(CMK_EINVAL, "conv: pointwise variant needs a 1x1 conv with Cout > 224%s", "");
        a.cout_pad = cout_pad128;
        if (a.ksplit > 1 && !pointwise_mt(d, n)) return fail(CMK_EINVAL, "conv: pointwise variant: split-K not available for this conv%s", "");
        return launch_pw(a, d->tune_wn, st, plan);
    }
    // opt-in: the pointwise GEMM from split products (fp32-accurate): 10 = three bf16 pieces per operand (cmk.h w_split), 12 = two fp16 pieces /
    // three products (cmk.h w_splith, w_splith_scale)
    if (d->tune_wm == 10 || d->tune_wm == 12) {
        const bool f16 = d->tune_wm == 12;
        if (!(d->ksize == 1 ? pointwise_mt(d, n) : gather_mt(d, n)) || (f16 && !(d->w_splith_scale > 0.f)))
            return fail(CMK_EINVAL, f16 ? "conv: the fp16-split variant needs w_splith, w_splith_scale and a conv the pointwise GEMM kernel takes (1x1, or 3x3 in its gather form)%s"
                                        : "conv: the bf16-split variant needs w_split and a conv the pointwise GEMM kernel takes (1x1, or 3x3 in its gather form)%s", "");
        a.cout_pad = cout_pad128;
        a.w = reinterpret_cast<const float*>(f16 ? d->w_splith : d->w_split);
        if (f16) a.p[0].acc_scale = d->w_splith_scale;
        a.ksplit = 1;
        a.ga_stride = d->ksize == 3 ? d->stride : 0;
        return launch_pw_split(a, f16 ? 2 : 1, st, plan);
    }
    if (d->tune_wm == 11) {                            // opt-in: direct 3x3 conv on bf16-split products (conv_sp3.hip); tune_sc = pieces, tune_wn = geometry
        if (d->ksize != 3 || d->stride != 1 || !d->w_splith || d->splitk > 1 || d->res_mode != 0 || d->in_relu || d->pool_ws)
            return fail(CMK_EINVAL, "conv: the direct fp16-split variant needs w_splith and a plain 3x3 stride-1 conv%s", "");
        for (int i = 0; i < n; ++i) {
            if (!descs[i].w_splith || !(descs[i].w_splith_scale > 0.f)) return fail(CMK_EINVAL, "conv: w_splith / w_splith_scale missing%s", "");
            a.p[i].w = reinterpret_cast<const float*>(descs[i].w_splith);
            a.p[i].acc_scale = descs[i].w_splith_scale;
        }
        a.cout_pad = cout_pad128;
        a.ksplit = 1;
        return launch_sp3(a, d->tune_wn, d->tune_sc, st, plan);
    }
    if (d->tune_wm == 9) {                             // gather form of a 3x3 conv on the pointwise GEMM kernel; tune_wn = accumulator rows per wave
        const int mt = gather_mt(d, n);
        if (!mt) return fail(CMK_EINVAL, "conv: pointwise gather variant not available for this conv%s", "");
        a.cout_pad = cout_pad128;
        a.ga_stride = d->stride;
        return launch_pw(a, mt, st, plan);
    }
    if (d->tune_wm == 7) {                             // gather form: 3x3 (stride 1|2) as a flattened-pixel GEMM over 9x the K chunks
        if (d->ksize != 3 || n != 1 || d->res_mode == 2 || d->in_scale || (d->tune_wn != 1 && d->tune_wn != 2 && d->tune_wn != 4))
            return fail(CMK_EINVAL, "conv: gather variant not available for this conv%s", "");
        const int cout_pad32 = cout32 <= 7 ? cout32 : cdiv(cout32, 4) * 4;
        if (cout_pad32 % d->tune_wn) return fail(CMK_EINVAL, "conv: gather variant: Cout tiles %% WN != 0%s", "");
        a.cout_pad = cout_pad32 * 32;
        a.ga_stride = d->stride;
        return launch_igemm_gather(a, d->tune_wn, cout_pad32 / d->tune_wn, st, plan);
    }
    const Variant v{d->tune_wm, d->tune_sc, d->tune_wn};
    if (!variant_ok(d->ksize * d->ksize, d->stride, cout32, v.wm, v.sc, v.wn)) return fail(CMK_EINVAL, "conv: variant not available for this shape%s", "");
    return launch_igemm(a, d->ksize, d->stride, cout32, v, st, plan);
}

// plan: fill it instead of launching (cmk_conv_plan).  There gn_groups > 0 without a gn_ws asks for the launch as with statistics where the
// resolved kernel writes them: the workspace is sized by the answer.
static int run(const cmk_conv_desc* descs, int n, void* stream, LaunchPlan* plan = nullptr) {
    const cmk_conv_desc* d = &descs[0];
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.nprob = n;
    for (int i = 0; i < n; ++i) fill_problem(a.p[i], &descs[i]);
    a.w = d->w; a.res = d->res;
    a.Cin = d->Cin; a.Cout = d->Cout;
    a.x_cs = d->x_cs; a.x_co = d->x_co; a.y_cs = d->y_cs; a.y_co = d->y_co;
    a.res_cs = d->res_cs; a.res_co = d->res_co; a.res_mode = d->res_mode; a.Hr = d->Hr; a.Wr = d->Wr;
    if (a.res_mode == 2 && (a.Hr * 2 < a.p[0].Ho || a.Wr * 2 < a.p[0].Wo)) return fail(CMK_EINVAL, "conv: upsampled residual too small%s", "");
    a.relu_upto = d->relu_upto; a.in_relu = d->in_relu;
    const bool ask_gn = plan && !d->gn_ws && d->gn_groups > 0;
    const Variant v = resolve(descs, n, d->gn_ws != nullptr || ask_gn);
    cmk_conv_desc dv = *d;          // zero tune fields launch exactly as the explicit variant they resolve to
    dv.tune_wm = v.wm; dv.tune_sc = v.sc; dv.tune_wn = v.wn;
    static double no_ws;            // stands for the workspace in a plan; nothing is launched, so nothing writes through it
    if (ask_gn && writes_gn_records(v.wm)) dv.gn_ws = &no_ws;
    hipStream_t st = (hipStream_t)stream;
    int rc = dispatch(a, &dv, descs, n, st, plan);
    if (rc || plan) return rc;
    if (a.ksplit <= 1 && a.tail_ksplit > 1 && a.tail_tiles > 0) {
        // tail split-K (conv_wino6, RoI pairs): the images of the tail's tiles are one contiguous range of pixels at the end of y; the
        // slabs hold those images only.  Same fixed-order sum and epilogue as below, over that range.
        const ConvProblem& p = a.p[0];
        const long pix0 = (long)2 * (a.total_tiles - a.tail_tiles) * p.Ho * p.Wo, tpix = p.total_pix - pix0;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)std::min<long>((tpix * (a.cout_pad >> 2) + 255) / 256, 256L * 32)), dim3(256), 0, st, a.ws, a.tail_ksplit,
                           tpix, a.cout_pad, p.scale, p.shift, a.Cout, a.relu_upto, (const float*)nullptr, 0, 0, p.y + pix0 * a.y_cs, a.y_cs, a.y_co);
        return check_launch("splitk_reduce (tail)");
    }
    if (a.ksplit <= 1) return rc;
    const ConvProblem& p = a.p[0];      // split-K (one problem): sum the partial sums and apply the epilogue
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)std::min<long>((p.total_pix * (a.cout_pad >> 2) + 255) / 256, 256L * 32)), dim3(256), 0, st, a.ws, a.ksplit, p.total_pix,
                       a.cout_pad, p.scale, p.shift, a.Cout, a.relu_upto, a.res_mode == 1 ? a.res : nullptr, a.res_cs, a.res_co, p.y, a.y_cs,
                       a.y_co);
    return check_launch("splitk_reduce");
}

}  // namespace cmk

extern "C" int cmk_conv_cout_pad(int Cout) {
    int c32 = (Cout + 31) / 32;
    return c32 <= 7 ? c32 * 32 : ((c32 + 3) / 4) * 128;
}

extern "C" int64_t cmk_conv_packed_floats(int Cout, int Cin, int ksize) {
    int64_t taps = (int64_t)ksize * ksize;
    int64_t nch = (Cin + 15) / 16;
    return taps * nch * cmk_conv_cout_pad(Cout) * 16;
}

extern "C" int cmk_conv_gn_tiles(int H, int W) { return ((H + 7) / 8) * ((W + 15) / 16); }

// {sum, sumsq} records per image that a Winograd conv with fused GroupNorm statistics writes (tune_wm 6: the F(4x4) map kernels, otherwise
// the F(2x2) kernel), from the kernels' own constants; cmk_conv_plan answers for any launch
extern "C" int cmk_conv_gn_records(int H, int W, int tune_wm) {
    return tune_wm == 6 ? cmk::wino6_gn_records(H, W) : cmk::wino4r_gn_records(H, W);
}

extern "C" int64_t cmk_splith_packed_halves(int Cout, int Cin) {     // per tap: two fp16 pieces per weight (cmk.h w_splith)
    return (int64_t)((Cin + 15) / 16) * (((Cout + 127) / 128) * 4) * 2 * 64 * 8;
}

extern "C" int64_t cmk_split_packed_halves(int Cout, int Cin) {      // per tap of the conv: a 3x3 conv in the gather form holds nine of these, tap-major
    return (int64_t)((Cin + 15) / 16) * (((Cout + 127) / 128) * 4) * 3 * 64 * 8;
}

extern "C" int64_t cmk_wino_packed_floats(int Cout, int Cin) {
    return (int64_t)((Cin + 15) / 16) * ((Cout + 63) / 64) * 16 * 64 * 16;
}

extern "C" int cmk_conv_pool_rows(const cmk_conv_desc* d) {
    if (!d) return 0;
    const int mt = cmk::pointwise_mt(d, 1);
    return (mt && (long)d->H * d->W >= 32 * mt) ? 32 * mt : 0;
}

// floats of splitk_ws a descriptor's tail needs: ways x the tail's images x H*W x cout_pad; 0 when the tail is off
extern "C" int64_t cmk_conv_tail_ws_floats(const cmk_conv_desc* d) {
    if (!d) return 0;
    int tiles = 0, ways = 0;
    cmk::wino6_tail_of(d, tiles, ways);
    if (tiles <= 0 || ways <= 1) return 0;
    const int st = (d->N + 1) / 2;
    const int64_t images = d->N - 2 * (int64_t)(st - tiles);
    return (int64_t)ways * images * d->H * d->W * cmk_conv_cout_pad(d->Cout);
}

extern "C" int cmk_conv2d_nhwc(const cmk_conv_desc* d, void* stream) {
    int rc = cmk::validate(d);
    if (rc) return rc;
    return cmk::run(d, 1, stream);
}

extern "C" int cmk_conv2d_nhwc_multi(const cmk_conv_desc* descs, int n, void* stream) {
    int rc = cmk::validate_multi(descs, n);
    if (rc) return rc;
    return cmk::run(descs, n, stream);
}

extern "C" int cmk_conv_plan(const cmk_conv_desc* descs, int n, char* kernel, int kernel_cap, double* executed_flops, int* gn_records) {
    int rc = n == 1 ? cmk::validate(descs) : cmk::validate_multi(descs, n);
    if (rc) return rc;
    cmk::LaunchPlan plan;
    memset(&plan, 0, sizeof(plan));
    rc = cmk::run(descs, n, nullptr, &plan);
    if (rc) return rc;
    if (kernel && kernel_cap > 0) snprintf(kernel, kernel_cap, "%s", plan.kernel);
    if (executed_flops) *executed_flops = (double)plan.executed_flops;
    for (int i = 0; gn_records && i < n; ++i) gn_records[i] = plan.gn_records[i];
    return CMK_OK;
}

extern "C" int cmk_conv_resolve(const cmk_conv_desc* descs, int n, int with_gn_stats, int variant[3]) {
    int rc = n == 1 ? cmk::validate(descs) : cmk::validate_multi(descs, n);
    if (rc) return rc;
    if (!variant) return cmk::fail(CMK_EINVAL, "conv_resolve: null variant%s", "");
    const cmk::Variant v = cmk::resolve(descs, n, with_gn_stats || descs[0].gn_ws);
    variant[0] = v.wm; variant[1] = v.sc; variant[2] = v.wn;
    return CMK_OK;
}
