/*
 * cmk.h — C ABI of libcmk_hip.so, the MI355X (gfx950) kernels under the CenterMask2 inference path.
 *
 * The reference (Zeng-Yan/centermask2) is pure Python; every arithmetic step of its path reaches native code
 * through PyTorch / detectron2 / torchvision operators.  Each entry point below replaces one such operator
 * call site (cited per function, paths relative to the reference root).  Conventions:
 *   - the caller owns every buffer, including workspaces; the library never allocates, frees or synchronises;
 *   - all pointers are device pointers; all launches go to the `stream` argument (a hipStream_t passed as void*);
 *   - activations are NHWC float32; a tensor "view" is (pointer, channel stride `cs`, channel offset `co`), so a
 *     conv can write straight into a slice of an OSA concat buffer (vovnet.py:324 never materialises);
 *   - returns 0, or a negative CMK_E* code; cmk_last_error() gives the message (thread-local); nothing throws;
 *   - no state beyond one-time, per-device kernel attributes (set on the first launch on each device, idempotent); one process
 *     per GPU each loads its own copy.  Launches go to the CURRENT device's stream the caller passes: the caller selects the
 *     device (hipSetDevice / torch.cuda.device) that owns the pointers before calling.
 */
#ifndef CMK_H
#define CMK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CMK_OK 0
#define CMK_EINVAL (-1)   /* bad argument / unsupported shape */
#define CMK_ELAUNCH (-2)  /* HIP launch error */

int cmk_version(void);                 /* ABI version, currently 5 (2: cmk_conv_desc.w_wino6, cmk_groupnorm_affine_tiles takes record counts;
                                          3: cmk_conv_desc.pool_ws, cmk_ese_gate_pooled, cmk_pack_records; 4: cmk_conv_desc.w_split;
                                          5: cmk_conv_desc.w_splith, w_splith_scale) */
const char* cmk_arch(void);            /* "gfx950" */
const char* cmk_last_error(void);

/* ---- convolution as implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------------------------------------
 * Replaces aten::conv2d (+ FrozenBN fold, bias, ReLU) at vovnet.py:205-236, fpn.py:27-35, d2 FPN lateral/output
 * convs, fcos.py:169-200, sam.py:58-83, maskiou_head.py:81-93 and the Linear layers maskiou_head.py:89-91.
 * Weights are pre-packed by cmk_pack_conv_weight_size/the host packer into [tap][Cin/16][cout_pad][16].
 * y = act( conv(x) * scale[c] + shift[c] (+ residual) ),  act = ReLU on channels [0, relu_upto).              */
typedef struct {
    const float* x; int x_cs; int x_co;         /* input view, (N,H,W,Cin) */
    const float* w;                             /* packed weights */
    const float* scale; const float* shift;     /* per output channel, length >= Cout */
    const float* res; int res_cs; int res_co;   /* optional residual view */
    int res_mode;                               /* 0 none, 1 same resolution, 2 nearest-upsample x2 of (N,Hr,Wr,*) */
    int Hr; int Wr;
    float* y; int y_cs; int y_co;               /* output view, (N,Ho,Wo,Cout) */
    int N; int H; int W; int Cin; int Cout;
    int ksize;                                  /* 1 or 3 (padding ksize/2) */
    int stride;                                 /* 1 or 2 */
    int relu_upto;                              /* ReLU applied to output channels < relu_upto */
    int in_relu;                                /* ReLU applied to the input while staging (fpn.py:34) */
    /* optional tile variant picked by the caller's autotuner (all 0 = let the library's cost model choose; cmk_conv_resolve tells which
     * explicit variant that is):
     * tune_wm in {1,2} (128 or 256 pixels per workgroup), tune_sc in {16,32} (sub-tile 2x16 or 1x32 pixels; 32 for 1x1),
     * tune_wn in 1..7 (32*tune_wn output channels per workgroup; must divide the padded Cout).  Results are bitwise
     * identical across variants (the K order per output does not depend on the tile).
     * tune_wm == 7 (with tune_wn in {1,2,4}) selects the gather form of a 3x3 conv (stride 1|2): a flattened-pixel GEMM whose K walks
     * 9 taps x Cin/16 chunks, each A row gathered per tap — for maps too small to fill the spatial tiles (the 14->7 maskiou conv
     * maskiou_head.py:84, P6/P7 fpn.py:32-35); same K order, so again bitwise identical to the tiled variants.
     * tune_wm == 8 (with tune_wn in {4,2}) selects the pointwise GEMM kernel (conv_pw.hip) for a 1x1 conv with Cout > 224, Cin % 32 == 0,
     * no fused input affine / input ReLU (the upsampled residual only with an even W; split-K with K chunks % (2*splitk) == 0): 64*tune_wn pixels x 128 output channels per workgroup, weights
     * fetched straight into registers (the packed layout is the same); again the same bits as the tiled variants.  It is also the
     * untuned default for such convs when they make at least 256 workgroups (vovnet.py:222-236 aggregation convs, the deconv).
     * tune_wm == 9 (tune_wn in {4,2}): the gather form of a 3x3 conv (stride 1|2) on that kernel — K walks 9 taps x Cin/16 chunks, rows
     * gathered per tap with bounds-checked loads; Cout in 97..128 or > 224, Cin % 32 == 0, one problem, no fused affine / upsampled
     * residual; bitwise identical to the tune_wm 7 form; the untuned default for stride-2 convs of at least 1024 workgroups
     * of 256 pixels (stem_3 vovnet.py:412). */
    int tune_wm; int tune_sc; int tune_wn;
    /* tune_wm == 5 selects the fused Winograd F(2x2,3x3) kernel (3x3 stride 1, no residual; the default for such convs when w_wino
     * is given): same fp32 arithmetic on the matrix pipe with 2.25x fewer multiplies; results differ from the direct kernel by fp32
     * rounding only.  It needs the weights pre-transformed to U = G g G^T (cmk_wino_packed_floats floats), packed
     * [Cin/16][ceil(Cout/64)][step 4][fh 2][ng 2][fl 2][piece 2][lane 64][4 floats]: frequency (row-major index of the 4x4 grid) =
     * 8*fh + 2*step + fl, output channel = ntile*64 + ng*32 + (lane & 31), input channel = chunk*16 + 8*(lane >> 5) + 4*piece + j —
     * every operand load of a wave is one contiguous KiB. */
    const float* w_wino;
    /* optional fused GroupNorm+ReLU of the PRODUCER (fcos.py:182-186): per (image, input channel) x' = relu(x*in_scale + in_shift)
     * is applied while the input tile is staged, so the normalised tensor is never written; arrays of N*Cin floats from
     * cmk_groupnorm_affine.  Supported by the direct kernels and the Winograd kernel. */
    const float* in_scale; const float* in_shift;
    /* split-K (direct kernels incl. the gather form, one problem, res_mode 0|1): splitk >= 2 workgroup rows each own 1/splitk of the
     * 16-channel K chunks (K chunks % (2*splitk) == 0) and write raw partial sums to splitk_ws (splitk * N*Ho*Wo * cmk_conv_cout_pad(Cout)
     * floats, caller-owned); a second launch sums them and applies the epilogue.  For skinny GEMMs (maskiou_fc1: 400 x 12544 x 1024,
     * maskiou_head.py:116) whose M x N tiles cannot fill 256 CUs.  0/1 = off. */
    int splitk; float* splitk_ws;
    /* optional fused GroupNorm STATISTICS of this conv's output (the GroupNorm that follows it, fcos.py:182-186): only with
     * tune_wm == 5, relu_upto == 0 and Cout/gn_groups a power of two <= 32.  The kernel writes {sum, sum of squares} per
     * (spatial tile of 8x16 outputs, row parity, group) to gn_ws as doubles: record index ((tile*2 + parity)*gn_groups + group),
     * tiles numbered image-major per problem (for _multi: problems back to back) with cmk_conv_gn_tiles(H, W) tiles per image;
     * cmk_groupnorm_affine_tiles turns them into the per-(image, channel) scale/shift.  NULL = off.
     * With tune_wm == 6 the records are per (spatial tile of 12x40 outputs, wave 0..3, group): index ((tile*4 + wave)*gn_groups + group);
     * cmk_conv_gn_records(H, W, tune_wm) gives the records per image of either form, cmk_conv_plan those of any launch. */
    double* gn_ws; int gn_groups;
    /* tune_wm == 6 selects the fused Winograd F(4x4,3x3) kernel (conv_wino6.hip; 3x3 stride 1, no residual, Cin % 8 == 0; tune_wn 1 = 12x40-pixel
     * tiles of one image, tune_wn 2 = two whole maps of at most 16 rows x 14 columns per workgroup, for the 14x14 RoI features): 36 multiplies
     * per 4x4 outputs, 1.78x fewer than F(2x2,3x3); fp32 throughout, error ~1.6x the 2x2 form's (tools/wino_numerics.py).  Needs
     * U = G g G^T (6x6 per filter, points 0, +-1, +-2, inf), cmk_wino6_packed_floats floats packed
     * [Cin/8][ceil(Cout/32)][wave 4][slot 9][lane 64][4 floats]: slot k < 6 is frequency (row = wave, column = k), slot k >= 6 is
     * (row = 4 + wave/2, column = 3*(wave%2) + k - 6); output channel = tile*32 + (lane & 31), input channel = chunk*8 + 4*(lane >> 5) + j.
     * tune_sc == 64 with tune_wm == 6 selects the "shared V" form of the same arithmetic (conv_wino6s.hip; tune_sc 16 or 0 = conv_wino6.hip): one
     * 8-wave workgroup per CU computes 64 output channels of a spatial tile from ONE frequency image of the input kept in LDS, so the halo is
     * fetched and transformed once per 64 channels instead of once per 32; same packed weights, same K order: bit-identical results.  It is
     * the faster form for launches of about one round of workgroups (the 50x80 maps of stage 4, vovnet.py:90-98); the start-up tuner decides.
     * tune_sc == 32 with tune_wm == 6 selects the paired form (conv_wino6.hip, conv_wino6p_kernel): one 8-wave workgroup per CU covers 64 couts
     * as two conv_wino6 cout tiles that share the halo loads, the column transform and the fused input affine; each wave's own work, the packed
     * weights, the GroupNorm records and split-K are those of tune_sc 16: bit-identical results.  Other tune_sc values than
     * 0, 16, 32 and 64 are refused. */
    const float* w_wino6;
    /* optional fused average-pool partial sums of the (scaled, shifted, ReLU'd) OUTPUT, for the eSE gate of the OSA aggregation conv
     * (vovnet.py:255-256 avg_pool over the conv the block just produced): only the pointwise GEMM kernel produces them — ask
     * cmk_conv_pool_rows(d) first; it returns R > 0 (rows of flattened pixels per record) when this descriptor, as tuned, runs on that
     * kernel and H*W >= R, else 0.  pool_ws then receives 2 * ceil(N*H*W / R) records of Cout floats: record 2g = the sum over the rows
     * of block g (pixels gR .. gR+R-1) that belong to the image of the block's first pixel, record 2g+1 = the sum over its rows that
     * belong to the next image (0 if none); every record is written.  cmk_ese_gate_pooled turns them into the gate.  NULL = off. */
    float* pool_ws;
    /* OPT-IN, tune_wm == 10 (tune_sc 32, tune_wn 4): a plain 1x1 conv (Cin % 16 == 0, Cout > 224 or 97..128, no residual / input affine / split-K;
     * pool_ws allowed) as the same GEMM with every fp32 product rebuilt from bf16 pieces on v_mfma_f32_32x32x16_bf16: x = hi + mid + lo with
     * hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (round to nearest even; exact to 2^-24), the six products of weight >= 2^-16
     * accumulated in fp32.  The result carries the error of an fp32 accumulation (measured: that of a sequential fp32 fma chain), NOT the bits
     * of the fp32-MFMA kernels.  The activations are fp32 and are split inside the kernel; the weights are split by the caller:
     * w_split = cmk_split_packed_halves(Cout, Cin) 16-bit values, [Cin/16][cout_pad/32][piece hi|mid|lo][lane 64][8], lane = 32*hh + li holding
     * input channels 16*chunk + 8*hh + 0..7 of output channel 32*tile + li (cout_pad = Cout rounded up to 128, zero filled).
     * No caller of this repository selects it by default (ops.ALLOW_SPLIT_BF16); NULL = not available. */
    const void* w_split;
    /* (tune_wm 11 also takes tune_sc 21: the same geometries with one cout tile per wave — workgroups of 64 / 128 couts: less cout padding for
     * layers of 160 / 192 couts, more and smaller workgroups for the small maps.)
     * OPT-IN, tune_wm 12 (tune_sc 32, tune_wn 4): the pointwise GEMM / gather form of tune_wm 10 on TWO fp16 pieces per operand, three products
     * (half the MFMAs of the bf16 form, the same fp32-class error); takes pool_ws and res_mode 2 like tune_wm 10; packing w_splith (1 tap for a
     * 1x1 conv, 9 tap-major for a 3x3 conv) and w_splith_scale as described next.
     * OPT-IN, tune_wm 11 (conv_sp3.hip; tune_sc = 2 pieces, tune_wn = tile geometry 0..3): a 3x3 stride-1 conv as a DIRECT implicit GEMM on
     * v_mfma_f32_32x32x16_f16 with every fp32 operand split into TWO fp16 pieces (22 bits of significand: h = fp16(x), m = fp16(x - h), the
     * residual is exact) and the products m*h, h*m, h*h accumulated in fp32.  The representation error is below an fp32 GEMM's own accumulation
     * error, so the result carries the error of an fp32 accumulation — NOT the bits of the fp32-MFMA kernels.  Activations are split inside the
     * kernel (scaled by 2^-4, residual by 2^11).  The window, as measured on an MI355X (tune_wm 11 and 12 alike; tests/conv_cases.py "f16_domain"
     * holds the promised part): finite and at fp32-class error up to max|x| = 1.04e6 (65504 * 2^4); from 1.05e6 on every output that reads an
     * element above that is NaN (h = Inf, the residual Inf - Inf), at 2e6 nearly all and at 1e7 all of them; never Inf.  Downwards the two pieces
     * carry 22 bits of x only while h is a normal fp16, |x| >= 2^-10; below that an activation keeps an ABSOLUTE error of about 2^-31, which is
     * nothing beside activations of order 1 but shows on a tensor that is small as a whole: max|x| = 2^-17 comes out 8e-5 of max|ref| off,
     * 2^-21 1e-3, 2^-25 2e-2, 2^-30 0.5 (always finite).  A weight channel at 2^-16 of the layer's largest keeps the full accuracy.
     * The caller packs the weights:
     * w' = w * S_w, S_w the power of two with max |w'| in [2^14, 2^15); w_splith = taps x cmk_splith_packed_halves(Cout, Cin) fp16 values,
     * [tap][Cin/16][cout_pad/32][piece h|m][lane 64][8] (lane = 32*hh + li: input channels 16*chunk + 8*hh + 0..7 of output channel 32*tile + li;
     * cout_pad = Cout rounded up to 128, zero filled); w_splith_scale = 1 / S_w.  Takes in_scale/in_shift, gn_ws (records per image:
     * cmk_conv_plan), and in cmk_conv2d_nhwc_multi up to 10 problems that may differ in their weights.  No residual, split-K or pooled sums.
     * No caller of this repository selects it by default (ops.ALLOW_SPLIT_F16); NULL = not available. */
    const void* w_splith;
    float w_splith_scale;
    /* OPT-IN, tune_wm 6 with tune_wn 2 and tune_sc 16 | 32: "tail split-K".  A RoI-pair launch whose workgroups do not fill a whole number
     * of rounds of the chip (400 RoIs x 256 couts: 1600 workgroups on 512 places = 3.125 rounds) spends its last round with most CUs idle
     * for a whole workgroup life.  splitk_tail >= 2 runs the last splitk_tail_tiles spatial tiles (pairs of images) as splitk_tail short
     * workgroups per (tile, cout tile), dispatched last in the same launch; each owns whole chunk pairs of Cin / 16, spread as evenly as
     * possible (splitk_tail <= Cin / 16), and stores raw partial sums to splitk_ws (cmk_conv_tail_ws_floats(d) floats: the tail's images
     * only); a reduce launch over those images sums them in a fixed order and applies scale / shift / ReLU.  The other images get the bits
     * of the launch without a tail; the tail's images differ from it by fp32 rounding.  splitk_tail_tiles > 0 is taken as given (capped at
     * the launch's tiles); 0 asks cmk_wino6_tail_plan with the current device's places (CUs x 2, paired form x 1) — the plan's tiles and at
     * most its ways, and no tail at all where it finds no ragged round.  One problem, no gn_ws, no splitk beside it; tune_sc 64, tune_wn 1 and every other tune_wm refuse it.
     * splitk_tail 0 | 1 = off: nothing is on unless the caller names it.
     * (splitk > 1 with tune_wn 2 is the case "every tile is tail": splitk <= Cin / 16 ways, the full-size split-K workspace.) */
    int splitk_tail; int splitk_tail_tiles;
} cmk_conv_desc;
/* What a conv reads, and where a non-finite input can show (every tune_wm; tests/conv_cases.py "nonfinite" and the guards of every row):
 * a launch depends on nothing but the channels [x_co, x_co + Cin) of its N images (and [res_co, res_co + Cout) of the residual) — the other
 * channels of the tensor, the memory before and behind it, and what the output view held may be any bit pattern, NaN included, and do not
 * change one output bit.  An Inf or NaN at one input pixel reaches only the outputs that read it: the k x k outputs around it for the
 * direct, gather, pointwise and split forms (at stride 2 those it lands on), the 2x2 (tune_wm 5) or 4x4 (tune_wm 6) output tiles,
 * anchored at the image's corner, whose 4x4 or 6x6 input window holds it for the Winograd forms (Inf - Inf in the transform: the whole
 * tile may be NaN).  Every other output of that image, every other image — the other map of a RoI pair, the other problems of a _multi
 * launch — and their pooled sums (pool_ws) and GroupNorm records (gn_ws) keep the bits of the launch without it; wherever the exact result
 * is non-finite the output is non-finite.  The fused ReLU is fmaxf: relu(NaN) = 0 on channels below relu_upto and behind in_relu /
 * in_scale, as in groupnorm.hip. */
int cmk_conv2d_nhwc(const cmk_conv_desc* d, void* stream);
int cmk_conv_pool_rows(const cmk_conv_desc* d);
/* Same conv applied to up to 5 inputs of different H x W in ONE launch (the FCOS towers/predictors share their weights
 * across the FPN levels, fcos.py:227-238).  All descriptors must share w, Cin, Cout, ksize, stride, views and flags and
 * carry no residual; x, y, N, H, W, scale, shift, in_scale/in_shift may differ.
 * With tune_wm == 6, tune_wn == 1 (the F(4x4) map kernels, which take the packed weights per problem) the problems may also differ in their
 * weights (w, w_wino6) and there may be up to 10 of them: conv k of the FCOS head's cls tower and of its bbox tower — same level shapes,
 * different weights, fcos.py:227-231 — run as one launch of 2 x 5 problems.  Fused GroupNorm records (gn_ws) are numbered over the spatial
 * tiles of all problems in order, so the records of problems 5..9 follow those of problems 0..4. */
int cmk_conv2d_nhwc_multi(const cmk_conv_desc* descs, int n, void* stream);
/* The explicit variant cmk_conv2d_nhwc (n == 1) / cmk_conv2d_nhwc_multi would run for these descriptors, as variant = {tune_wm, tune_sc,
 * tune_wn}: the caller's tune fields unchanged when set, else the untuned default (splitk, which the caller sets with its workspace, counts).
 * Validates the descriptors as the launch does; never touches a device.  with_gn_stats != 0: prefer the forms that produce fused GroupNorm
 * statistics exactly as a launch with gn_ws set does (gn_ws may still be NULL: its size depends on the answer); when none applies, return
 * the choice among the others rather than fail. */
int cmk_conv_resolve(const cmk_conv_desc* descs, int n, int with_gn_stats, int variant[3]);
/* What cmk_conv2d_nhwc (n == 1) / cmk_conv2d_nhwc_multi would launch for these descriptors, as tuned (zero tune fields resolve as in a
 * launch): validates and refuses exactly as the launch does, launches nothing and uses no stream.  The answer comes from the launcher that
 * picks the template instantiation.  kernel (kernel_cap bytes, or NULL): the instantiation as a profiler names it, without the "void cmk::"
 * prefix and the argument list, e.g. "conv_pw_kernel<4, true, false, false, false, 0>".  executed_flops (or NULL): what the matrix pipe
 * executes, tile padding included; the split-product forms in fp32-equivalent FLOPs.  gn_records (n ints, or NULL): per problem the {sum,
 * sumsq} records per image the launch writes through gn_ws, 0 where it writes none.
 * gn_groups > 0 with gn_ws == NULL asks how large that workspace has to be (as cmk_conv_resolve's with_gn_stats): where the resolved kernel
 * produces the statistics the launch is planned — and refused — as with a gn_ws; where it does not, as without (gn_records all 0).
 * Touches no device, except that a tail with splitk_tail_tiles == 0 reads the current device's CU count (cmk_conv_tail_ws_floats). */
int cmk_conv_plan(const cmk_conv_desc* descs, int n, char* kernel, int kernel_cap, double* executed_flops, int* gn_records /* n ints or NULL */);
/* number of floats of the packed layout for (Cout, Cin, k): taps * ceil(Cin/16) * cout_pad * 16 */
int64_t cmk_conv_packed_floats(int Cout, int Cin, int ksize);
int cmk_conv_cout_pad(int Cout);
int64_t cmk_wino_packed_floats(int Cout, int Cin);
int64_t cmk_wino6_packed_floats(int Cout, int Cin);
/* Tail split-K plan (cmk_conv_desc.splitk_tail), pure host arithmetic: spatial_tiles x cout_tiles workgroups on `slots` places at a time.
 * tail_units = (spatial_tiles * cout_tiles) mod slots, rounded down to whole spatial tiles -> *tail_tiles; *ways = the largest of 8, 4, 2
 * with tail_tiles * cout_tiles * ways <= slots and ways <= chunk_pairs (Cin / 16).  0 tiles / 0 ways when there is no ragged round, less
 * than one full round, or a tail of more than half a round.  (200, 8, 16, 512) -> 8 tiles, 8 ways. */
int cmk_wino6_tail_plan(int spatial_tiles, int cout_tiles, int chunk_pairs, int slots, int* tail_tiles, int* ways);
/* the 8-channel chunks [*c_lo, *c_hi) of piece `piece` of `ways` of a conv of `chunks` chunks, as the RoI-pair kernel splits them */
void cmk_wino6_piece_bounds(int chunks, int ways, int piece, int* c_lo, int* c_hi);
/* floats of splitk_ws that the tail of d needs (reads the current device's CU count when splitk_tail_tiles is 0); 0 = the tail is off */
int64_t cmk_conv_tail_ws_floats(const cmk_conv_desc* d);
int64_t cmk_split_packed_halves(int Cout, int Cin);          /* 16-bit elements of cmk_conv_desc.w_split */
int64_t cmk_splith_packed_halves(int Cout, int Cin);         /* 16-bit elements PER TAP of cmk_conv_desc.w_splith */
/* spatial tiles per image of the fused-statistics conv (8 x 16 outputs each) */
int cmk_conv_gn_tiles(int H, int W);
/* {sum, sumsq} records per image written through cmk_conv_desc.gn_ws by the Winograd kernel tune_wm (5 or 6) on an H x W map (any other
 * kernel: cmk_conv_plan) */
int cmk_conv_gn_records(int H, int W, int tune_wm);

/* ---- deformable 3x3 conv of the VoVNet DCN stages (DFConv3x3.forward vovnet.py:185-201: d2 DeformConv / ModulatedDeformConv,
 * stride 1, pad 1, dilation 1, groups 1, no bias; wired in at vovnet.py:292-298 when MODEL.VOVNET.STAGE_WITH_DCN is set),
 * folded FrozenBN and optional ReLU:  y = act( deform_conv(x, offsets[, mask]) * scale[c] + shift[c] ).
 * x, y are NHWC channel-slice views as above (x: 16-byte aligned, x_cs and x_co multiples of 4); w is packed exactly like
 * cmk_conv_desc.w for a 3x3 conv (cmk_conv_packed_floats(Cout, Cin, 3) floats).  offsets is the raw (N,H,W,off_cs) output of the
 * offset conv: for deformable group g and tap k = 3i+j channel g*18 + 2k holds dy and g*18 + 2k + 1 holds dx; with modulated != 0
 * channel 18*dg + g*9 + k holds the mask LOGIT (the sigmoid is applied here).  Input channel c belongs to group c / (Cin/dg).  The
 * sample (h-1+i+dy, w-1+j+dx) is bilinear with corners outside the map read as 0, and 0 outside (-1,H) x (-1,W).  "0" means not
 * read: an Inf or NaN of x reaches an output only through a corner that lies in the map and belongs to a sample inside
 * (-1,H) x (-1,W); such a corner counts even at weight 0 (0 * Inf = NaN), nothing else does.  The ReLU is fmaxf: relu(NaN) = 0, as in
 * the other conv epilogues.  Offsets and mask logits must be finite.
 * Supported: N, H, W, Cin, Cout >= 1, Cin % 16 == 0, dg in {1, 2, 4} with (Cin/dg) % 8 == 0, off_cs >= 18*dg (27*dg modulated).
 * Views: 0 <= x_co, x_co + Cin <= x_cs, x_cs and x_co multiples of 4; 0 <= y_co, y_co + Cout <= y_cs (any stride and offset: y is
 * written float by float); x == y is allowed when the two channel slices are disjoint and refused when they overlap.
 * Alignment: x and w are read as 16-byte vectors and must be 16-byte aligned; offsets, scale, shift and y are read and written as single
 * floats and need 4 bytes only.  N*H*W * max(x_cs, y_cs) and N*H*W * off_cs must stay below 2^31.
 * Every check is made before the launch and returns CMK_EINVAL. */
int cmk_deform_conv3x3_nhwc(const float* x, int x_cs, int x_co, const float* offsets, int off_cs, const float* w,
                            const float* scale, const float* shift, float* y, int y_cs, int y_co, int N, int H, int W,
                            int Cin, int Cout, int dg, int modulated, int relu, void* stream);

/* ---- depth-wise 3x3, pad 1, stride 1|2, no bias / norm / activation (vovnet.py:110-119 'dw_conv3x3', the dw half of the
 * depth-wise VoVNet bodies V-19-slim-dw-eSE / V-19-dw-eSE vovnet.py:30-48).  x, y are NHWC channel-slice views
 * (pixel stride *_cs, offset *_co floats); w is tap-major [9][C].  The same front door as cmk_dwconv3x3_bn_act_nhwc below
 * (without scale, shift and the clamps): N, H, W >= 1, C a multiple of 4, the view, overlap, alignment and size rules. */
int cmk_dwconv3x3_nhwc(const float* x, int x_cs, int x_co, const float* w, float* y, int y_cs, int y_co,
                       int N, int H, int W, int C, int stride, void* stream);

/* ---- depth-wise 3x3 of a MobileNetV2 inverted-residual block (mobilenet.py:38-76) with its surroundings fused:
 *   y = clamp(dw3x3(min(x, in_max)) * scale[c] + shift[c], out_min, out_max),  pad 1, stride 1|2, C % 4 == 0.
 * min(x, in_max) finishes the ReLU6 of the producer (the stem / expand 1x1 run with the plain ReLU epilogue); scale/shift is the
 * folded FrozenBN; the padding is zeros of the clamped input.  in_max = +inf, out_min = -inf, out_max = +inf switch the clamps
 * off; a NaN bound or out_min > out_max is refused.  A NaN propagates (torch.nn.ReLU6).  x, y: NHWC channel-slice views; w tap-major
 * [9][C]; all pointers 16-byte aligned.  N, H, W >= 1; *_cs and *_co multiples of 4 floats with 0 <= co and co + C <= cs; x == y is
 * allowed for disjoint channel slices (stride 1) and refused when the slices overlap (a thread would read what another wrote).
 * Output map ((H-1)/stride + 1, (W-1)/stride + 1); N*Ho*Wo*C/4 <= 2^31 - 2^21: the kernel walks a 32-bit index with a grid stride of
 * up to 2^21 threads.  Every check is made before the launch and returns CMK_EINVAL. */
int cmk_dwconv3x3_bn_act_nhwc(const float* x, int x_cs, int x_co, const float* w, const float* scale, const float* shift,
                              float in_max, float out_min, float out_max, float* y, int y_cs, int y_co,
                              int N, int H, int W, int C, int stride, void* stream);

/* ---- grouped 3x3 conv of a ResNeXt bottleneck (d2 BottleneckBlock.conv2, MODEL.RESNETS.NUM_GROUPS > 1) with its FrozenBN folded:
 *   y = [relu](gconv3x3(x) * scale[c] + shift[c]),  pad 1, stride 1|2, no bias, Cin = Cout = C, `groups` >= 2 groups of Cg = C/groups,
 * Cg in {4, 8, 16, 32, 64}.  Exact fp32; a group reads only its own Cg input channels (a NaN / Inf stays inside its group); a NaN passes
 * the ReLU.  Output map ((H-1)/stride + 1, (W-1)/stride + 1).  x, y: NHWC channel-slice views; w: 9*Cg*C floats in the packing written
 * down in csrc/conv_group3.hip (ops.pack_group_weight); all pointers 16-byte aligned, offsets and strides multiples of 4 floats with
 * 0 <= co and co + C <= cs; x == y is allowed for disjoint channel slices (stride 1) and refused when the slices overlap;
 * N*Ho*Wo*C/4 < 2^31.  Every check is made before the launch and returns CMK_EINVAL.
 * One launch, no workspace.  Additive entry: the ABI version stays 5. */
int cmk_group_conv3x3_nhwc(const float* x, int x_cs, int x_co, const float* w, const float* scale, const float* shift,
                           float* y, int y_cs, int y_co, int N, int H, int W, int C, int groups, int stride, int relu, void* stream);

/* ---- stem_1: 3x3 stride-2 conv on the NCHW 3-channel image (vovnet.py:409), BN-folded, ReLU, NHWC out -------- */
int cmk_stem_conv_nchw3(const float* x, const float* w /* [27][Cout] */, const float* scale, const float* shift,
                        float* y, int N, int H, int W, int Cout, void* stream);

/* d2 BasicStem: y = max_pool2d(relu(conv7x7_s2_p3(x) * scale[c] + shift[c]), kernel 3, stride 2, padding 1)
 * x (N,3,H,W) NCHW fp32; w [147][Cout], k = (kh*7 + kw)*3 + ci; y (N,Hp,Wp,Cout) NHWC channel-slice view.
 * Hc = (H-1)/2 + 1, Wc likewise (conv); Hp = (Hc-1)/2 + 1, Wp likewise (pool). Pool padding never wins (-inf).
 * One launch (csrc/stem7_pool.hip): the conv map stays in LDS.  Cout must be 64.  Conv taps outside the image are zeros; a NaN
 * behaves as in torch (relu keeps it, the max returns it for every window that holds it).  N, H, W >= 1; y_cs and y_co multiples of 4
 * floats with 0 <= y_co and y_co + 64 <= y_cs; y 16-byte aligned, x, w, scale, shift 4-byte; 3*H*W < 2^31.  Every check is made before
 * the launch and returns CMK_EINVAL. */
int cmk_stem7x7_bn_relu_maxpool_nchw3(const float* x, const float* w, const float* scale, const float* shift,
                                      float* y, int y_cs, int y_co, int N, int H, int W, int Cout, void* stream);

/* ---- max pool k3 s2 ceil_mode, no padding (vovnet.py:349-350); k2 s2 (maskiou_head.py:93,108) ----------------- */
/* gate: optional (N*C) non-negative channel gate applied after the max (the eSE scale of the producer block, folded in).
 * A window that holds a NaN comes out NaN (torch max_pool2d); H, W >= 3. */
int cmk_maxpool3x3s2_ceil_nhwc(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co,
                               int N, int H, int W, int C, const float* gate, void* stream);

/* MaxPool2d(kernel 1, stride 2): every second pixel — d2's LastLevelMaxPool, the top block build_vovnet_fpn_backbone (vovnet.py:504-524)
 * hands to the FPN; Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1. */
int cmk_maxpool1x1s2_nhwc(const float* x, int x_cs, int x_co, float* y, int y_cs, int y_co, int N, int H, int W, int C, void* stream);

/* ---- eSE (vovnet.py:247-260): gate = relu6(W * mean_HW(x) + b + 3) / 6 ; y = x * gate (+ identity) ------------
 * ws: N * ese_chunks * C floats of workspace for the two-stage mean.  A NaN in an image's map makes that image's gates NaN
 * (torch relu6 keeps it), so the image comes out NaN.  N, HW >= 1, C % 4 == 0, ws_chunks >= 1, else refused.     */
int cmk_ese_gate(const float* x, int x_cs, int x_co, const float* fc_w /* [C][C] row = out */, const float* fc_b,
                 float* gate /* N*C */, float* ws, int ws_chunks, int N, int HW, int C, void* stream);
int cmk_ese_scale(const float* x, int x_cs, int x_co, const float* gate, const float* identity, int id_cs, int id_co,
                  float* y, int y_cs, int y_co, int N, int HW, int C, void* stream);
/* the gate from the partial sums the producing conv left in pool_ws (cmk_conv_desc.pool_ws; rows = cmk_conv_pool_rows of that conv):
 * no pass over the map.  Fixed summation order. */
int cmk_ese_gate_pooled(const float* pool_ws, int rows, const float* fc_w, const float* fc_b, float* gate, int N, int HW, int C, void* stream);

/* ---- GroupNorm(32) + ReLU in place (fcos.py:182-186) ---------------------------------------------------------
 * ws: N * groups * gn_chunks * 2 doubles.                                                                    */
int cmk_groupnorm_relu_nhwc(float* x, const float* gamma, const float* beta, double* ws, int ws_chunks,
                            int N, int HW, int C, int groups, float eps, void* stream);

/* The same without the ReLU (d2 get_norm("GN") behind a conv with no activation: MODEL.FPN.NORM "GN", vovnet.py:550) */
int cmk_groupnorm_nhwc(float* x, const float* gamma, const float* beta, double* ws, int ws_chunks,
                       int N, int HW, int C, int groups, float eps, void* stream);
/* y (N,H,W,C dense) += nearest-neighbour 2x upsampling of coarse (N,Hc,Wc,C dense): d2 FPN's top-down sum when a norm sits between the
 * lateral conv and the sum (otherwise the sum rides in the lateral conv's epilogue, cmk_conv_desc.res_mode 2) */
int cmk_upsample2x_add_nhwc(float* y, const float* coarse, int N, int H, int W, int Hc, int Wc, int C, void* stream);

/* Statistics only: out_scale/out_shift (N*C each) such that GroupNorm(x)[n,:,c] = x*out_scale[n,c] + out_shift[n,c];
 * the consumer conv applies them (cmk_conv_desc.in_scale/in_shift).  ws as above. */
int cmk_groupnorm_affine(const float* x, const float* gamma, const float* beta, double* ws, int ws_chunks,
                         int N, int HW, int C, int groups, float eps, float* out_scale, float* out_shift, void* stream);

/* The same for up to 5 tensors (the FPN levels of one tower conv) in two launches; xs/out_scale/out_shift/HWs are HOST arrays
 * of nlev entries; ws: nlev * N * groups * ws_chunks * 2 doubles. */
int cmk_groupnorm_affine_multi(const float* const* xs, const int* HWs, int nlev, const float* gamma, const float* beta, double* ws,
                               int ws_chunks, int N, int C, int groups, float eps, float* const* out_scale, float* const* out_shift,
                               void* stream);
/* Second half of the fused form: the statistics were written by the conv itself (cmk_conv_desc.gn_ws, all levels of one
 * cmk_conv2d_nhwc[_multi] call, N images each); this turns them into the same per-(image, channel) scale/shift. */
/* recs[l] = cmk_conv_gn_records(Hs[l], Ws[l], tune_wm of the producing conv): records per image of level l */
int cmk_groupnorm_affine_tiles(const double* ws, const int* Hs, const int* Ws, const int* recs, int nlev, const float* gamma, const float* beta,
                               int N, int C, int groups, float eps, float* const* out_scale, float* const* out_shift, void* stream);

/* ---- FCOS candidate selection + box decode (fcos_outputs.py:396-466) ------------------------------------------ */
typedef struct {
    const float* logits;   /* (N, HW, C) */
    const float* regctr;   /* (N, HW, 5): relu(scale*bbox_pred) (4) , ctrness logit (1) */
    int H; int W; int stride;
} cmk_fcos_level;
/* Per image i the candidates of all levels are appended in level order, location-major / class-minor
 * (the order of torch.nonzero, fcos_outputs.py:429 and Instances.cat :391-392).
 * cand_* have capacity `cap` rows per image; counts[i] receives the TRUE number: counts[i] > cap means rows beyond cap were dropped —
 * the caller compares (it already reads the counts) and re-runs with a larger capacity; the reference is unbounded (:444-449).
 * thresh_with_ctr: MODEL.FCOS.THRESH_WITH_CTR (:410-420): the candidate test is sigmoid(cls)*sigmoid(ctr) > thr instead of sigmoid(cls) > thr. */
int cmk_fcos_select(const cmk_fcos_level* levels, int num_levels, int N, int C, float pre_nms_thresh, int thresh_with_ctr,
                    float* cand_box /* N*cap*4 */, float* cand_score, int32_t* cand_cls, float* cand_loc /* N*cap*2 */,
                    int32_t* counts /* N */, int32_t* block_counts /* workspace */, int64_t block_counts_len,
                    int cap, void* stream);
int64_t cmk_fcos_select_ws_len(const cmk_fcos_level* levels, int num_levels, int N, int C);

/* ---- batched NMS + top-k (layers/ml_nms.py:93 -> d2 batched_nms; fcos_outputs.py:472-482) --------------------
 * Stable descending sort by score (ties by candidate index), torchvision's coordinate trick
 * (boxes + cls * (max_coord + 1)) for < 40000 candidates, per-class suppression otherwise, greedy IoU > thr,
 * the first `topk` (1..1024) survivors are written.  sort_ws: 4 * N * cap uint32.                                       */
int cmk_nms_topk(const float* cand_box, const float* cand_score, const int32_t* cand_cls, const float* cand_loc,
                 const int32_t* counts, int N, int cap, float iou_thr, int topk,
                 float* out_box /* N*topk*4 */, float* out_score, int64_t* out_cls, float* out_loc, int32_t* out_idx,
                 int32_t* out_count /* N */, uint32_t* sort_ws, void* stream);
/* The same launch with the overlap measure as an argument; cmk_nms_topk forwards here with metric 0.
 *   metric 0   IoU: inter / (area_a + area_b - inter), the arithmetic and the bits of cmk_nms_topk.
 *   metric 1   IoS, intersection over the smaller box: inter / fminf(area_a, area_b).  A box nested in a larger one of its class scores
 *              1 however small it is.  A zero smaller area gives 0 / 0 = NaN, which is not > thr: such a box suppresses nothing and is
 *              not suppressed.
 * A candidate is suppressed when its measure with a kept box exceeds thr.  The sort, the class separation (coordinate trick below 40000
 * candidates, per class from there on), the top-k limit and out_idx are those of cmk_nms_topk.  Refused: what cmk_nms_topk refuses, and
 * a metric other than 0 or 1. */
int cmk_nms_topk_metric(const float* cand_box, const float* cand_score, const int32_t* cand_cls, const float* cand_loc,
                        const int32_t* counts, int N, int cap, float thr, int metric, int topk,
                        float* out_box /* N*topk*4 */, float* out_score, int64_t* out_cls, float* out_loc, int32_t* out_idx,
                        int32_t* out_count /* N */, uint32_t* sort_ws, void* stream);

/* ---- multi-level ROIAlignV2 with CenterMask's ratio level assignment (pooler.py:80-118,290-366) ---------------- */
int cmk_roi_align_ratio(const float* const* feats /* host array of device pointers */, const int* feat_h, const int* feat_w,
                        const float* scales, int num_levels, int min_level, int C,
                        const float* boxes /* N*topk*4 */, const int32_t* counts, const float* img_area /* N */,
                        int N, int topk, int out_size, int sampling_ratio,
                        float* y, int y_cs /* (N*topk, out, out, y_cs) */, int32_t* out_level, void* stream);

/* The general pooler (pooler.py:192-288): aligned = 1 ROIAlignV2 / 0 ROIAlign v1 (torchvision roi_align aligned flag, :243-255);
 * assign_by_area = 0 the "ratio" rule above / 1 FPN Eqn.(1): floor(canonical_level + log2(sqrt(area) / canonical_box_size + eps))
 * clamped to the levels (pooler.py:121-152; img_area may then be NULL).
 * CMK_EINVAL before any launch: num_levels outside [1, 4], a level with feat_h or feat_w < 1, C % 4, y_cs < C or y_cs % 4, N, topk or
 * out_size < 1, canonical_box_size <= 0 under the area rule, or ceil(out_size^2 / 4) * (N*topk rounded up to 8) workgroups above 2^31 - 1. */
int cmk_roi_align_pool(const float* const* feats, const int* feat_h, const int* feat_w, const float* scales, int num_levels, int min_level,
                       int C, const float* boxes, const int32_t* counts, const float* img_area, int N, int topk, int out_size,
                       int sampling_ratio, int aligned, int assign_by_area, float canonical_box_size, int canonical_level,
                       float* y, int y_cs, int32_t* out_level, void* stream);

/* ---- SAG-Mask spatial attention (sam.py:23-28) in place -------------------------------------------------------
 * C % 4 == 0, S, R, topk >= 1, R % topk == 0, and 3*S*S*4 bytes of dynamic LDS at most 65536 (S <= 73): CMK_EINVAL otherwise. */
int cmk_spatial_attention(float* x /* (R,S,S,C) */, const float* w /* [2][3][3] */, const int32_t* counts, int topk,
                          int R, int S, int C, void* stream);

/* ---- mask predictor for the predicted class only + sigmoid (sam.py:83,97; mask_head.py:202-208) ---------------
 * deconv_out: (R, S, S, 4, C) = relu(deconv) laid out (dh,dw)-major; masks: (R, 2S, 2S).
 * C % 4 == 0, S, topk >= 1, R in [1, 65535] (the grid's y dimension), R % topk == 0: CMK_EINVAL otherwise.   */
int cmk_mask_predict(const float* deconv_out, const float* pw /* [classes][C] */, const float* pb,
                     const int64_t* cls, const int32_t* counts, int topk, int R, int S, int C,
                     float* masks, float* mask_logits_opt, void* stream);

/* ---- maxpool 2x2 of the masks into channel `co` of the MaskIoU input (maskiou_head.py:108-112) ----------------
 * A NaN wins its window as in max_pool2d.  R, S >= 1 and 0 <= y_co < y_cs: CMK_EINVAL otherwise. */
int cmk_mask_pool_concat(const float* masks /* (R,2S,2S) */, float* y, int y_cs, int y_co, int R, int S, void* stream);

/* ---- mask_scores = scores * iou[cls] (maskiou_head.py:50-60) --------------------------------------------------
 * R >= 1 and iou_cs >= 1: CMK_EINVAL otherwise. */
int cmk_mask_iou_score(const float* iou /* (R, classes_stride) */, int iou_cs, const float* scores, const int64_t* cls,
                       float* mask_scores, int R, void* stream);

/* ---- keypoint R-CNN heatmap decode (the tail of KRCNNConvDeconvUpsampleHead.layers keypoint_head.py:219-224 — bilinear x2 — and
 * keypoint_rcnn_inference keypoint_head.py:89-116 -> detectron2 heatmaps_to_keypoints, source absent: restated from its published
 * behaviour; reached from CenterROIHeads._forward_keypoint center_heads.py:520-553).
 * dec: the score_lowres ConvTranspose2d(k4, s2, p1) output in packed form, an NHWC view (N*topk, S, S, dec_cs) whose channels
 * [dec_co, dec_co + 4K) hold phase (py, px) of keypoint k at (2py+px)*K + k, i.e. map28[2a+py][2b+px] = dec[a][b][(2py+px)K + k].
 * Per valid (RoI, keypoint), fp32: map56 = upsample_bilinear2d(map28, x2, align_corners=False) (in LDS); the map resized to
 * Hc x Wc = ceil(max(y1-y0, 1)) x ceil(max(x1-x0, 1)) by upsample_bicubic2d (align_corners=False, A = -0.75, scale 4S/Hc in fp32,
 * source not clamped, taps clamped), evaluated on the fly; its FIRST maximum in row-major order (a NaN counts as the largest value,
 * as in torch.argmax) at (yi, xi); out (N*topk, K, 3) = (x, y, score) with x = (xi + 0.5) * (w / Wc) + x0, y likewise, and
 * score = 1 / sum(exp(map56 - max)) — the reference's columns [0, 1, 3] of heatmaps_to_keypoints.  Rows past counts[n] are written as
 * zeros.  Static launch (at most 8 workgroups per (RoI, keypoint), one per 8192 output pixels, then one combine launch), fixed-order
 * reductions, ties to the lower index: deterministic.  boxes (N, topk, 4) xyxy.  S in [1, 16], K >= 1.
 * ws: cmk_keypoint_decode_ws_len(N * topk, K) 4-byte words of workspace (0 for bad arguments). */
int64_t cmk_keypoint_decode_ws_len(int R, int K);
int cmk_keypoint_decode(const float* dec, int dec_cs, int dec_co, int S, int K, const float* boxes, const int32_t* counts, int N, int topk,
                        float* ws, int64_t ws_len, float* out, void* stream);

/* ---- input side: (x - mean) / std of one CHW image (uint8 if src_is_u8 else float32) into its zero-padded slot
 * (3,H,W) of the batched NCHW tensor (deploy_utils.py:76-98; d2 preprocess_image + ImageList.from_tensors).  mean3 / std3
 * are HOST arrays of 3 floats. ------------------------------------------------------------------------------------- */
int cmk_preprocess_chw(const void* src, int src_is_u8, float* dst, int h, int w, int H, int W, const float* mean3,
                       const float* std3, void* stream);

/* ---- input side, resize: detectron2's ResizeShortestEdge on a uint8 HWC image with 3 channels, i.e. PIL.Image.resize(BILINEAR), byte
 * for byte (deploy_utils.py:60-73 does it on the CPU).  Separable: a horizontal pass (h,w,3) -> (h,new_w,3) rounded to uint8, then a
 * vertical pass; the caller skips the horizontal pass when new_w == w, and a vertical entry given no tables (new_h == h, ksize_y 0) copies.
 * Tables of one axis in -> out (DEVICE memory, computed on the host in double precision as Pillow's Resample.c does):
 *   ksize        = cmk_resize_ksize(in, out) = int(ceil(max(in / out, 1))) * 2 + 1   (0 for sizes < 1)
 *   bounds[2*i]  = first input index of output i,  bounds[2*i+1] = number of taps (<= ksize)
 *   kk[i*ksize+t] = int(0.5 + weight * 2^22);      out = clamp((2^21 + sum_t in[lo + t] * kk[i*ksize + t]) >> 22, 0, 255)
 * The kernels clamp the tap ranges to the source, so no table can make them read outside it.
 *   cmk_resize_h_u8          dst: caller-owned (h,new_w,3) uint8, 4-byte aligned
 *   cmk_resize_v_u8          src (h,new_w,3) -> dst (new_h,new_w,3) uint8: the pure resize
 *   cmk_resize_v_preprocess  src (h,new_w,3) -> ((float)v - mean) / std into the image's zero-padded slot (3,H,W) of the NCHW batch, the
 *                            same bits as cmk_preprocess_chw fed the resized image; reverse_channels swaps channels 0 and 2 first;
 *                            mean3 / std3 are HOST arrays of 3 floats.  H, new_h <= 65535. ----------------------------------------- */
int cmk_resize_ksize(int in_size, int out_size);
int cmk_resize_h_u8(const uint8_t* src, int h, int w, int new_w, const int32_t* bounds_x, const int32_t* kk_x, int ksize_x, uint8_t* dst,
                    void* stream);
int cmk_resize_v_u8(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y, uint8_t* dst,
                    void* stream);
int cmk_resize_v_preprocess(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                            float* dst, int H, int W, const float* mean3, const float* std3, int reverse_channels, void* stream);

/* ---- test-time augmentation (detectron2 GeneralizedRCNNWithTTA, modeling/test_time_augmentation.py): the geometry of the input
 * pipeline, mirrored, and its inverses.  An augmentation a is (new_w, new_h, flip): the image resized to new_h x new_w and, with flip,
 * the resized bytes mirrored along x (d2 applies [resize, flip]).
 *   cmk_resize_v_preprocess_hflip   cmk_resize_v_preprocess writing column new_w - 1 - x: the mirrored image in its zero-padded slot, the
 *                                   padding still on the right and bottom; every pixel has the bits the plain entry gives it.
 * The box maps take a per-augmentation table in DEVICE memory, 5 floats each: (new_w, new_h, rx, ry, flip != 0).  The ratios are
 * computed in double on the host and rounded once to fp32; every step is one fp32 operation, nothing is fused.
 *   cmk_tta_boxes_to_image   the detections of all augmentations -> one cmk_nms_topk candidate set of capacity A*K in the image frame
 *                            (rx = w / new_w, ry = h / new_h).  det_* are the padded (A,K,..) outputs of cmk_nms_topk, det_counts (A)
 *                            clamped to [0, K].  Per valid detection: with flip x0' = new_w - x1, x1' = new_w - x0; then x * rx, y * ry;
 *                            then clipped to [0,img_w] x [0,img_h] (d2 Boxes.clip).  loc is mapped as a point by the same rule, without
 *                            the clip; score is copied, cls narrowed to int32.  Candidates are written compacted in augmentation order
 *                            and in the detector's order within an augmentation; cand_count[0] = sum of the clamped counts.
 *   cmk_tta_boxes_to_aug     the inverse for the mask pass (rx = new_w / w, ry = new_h / h): box (K,4) in the image frame, count[0]
 *                            clamped to [0, K] -> out_box (A,K,4): x * rx, y * ry, then with flip x0' = new_w - x1, x1' = new_w - x0; rows
 *                            at and beyond the count are zeros; out_counts[a] = the clamped count for every a.
 *   cmk_tta_reduce_masks     masks (A,K,S,S) soft masks, flips (A) int32, mask_scores (A,K), count[0] clamped to [0, K] ->
 *                            out_masks[k] = (sum_a m_a[k]) / A with the masks of flipped augmentations mirrored along x, out_scores[k]
 *                            likewise: fp32, added in augmentation order starting from 0, one division by (float)A; rows at and beyond
 *                            the count are zeros.  mask_scores and out_scores may both be NULL (MASKIOU_ON off).
 * Refused: null pointers, A < 1 or A > 4096, K < 1 or K > 65535, S < 1 or S > 1024, img_w / img_h not in [1, 65535]. -------------- */
int cmk_resize_v_preprocess_hflip(const uint8_t* src, int h, int new_h, int new_w, const int32_t* bounds_y, const int32_t* kk_y, int ksize_y,
                                  float* dst, int H, int W, const float* mean3, const float* std3, int reverse_channels, void* stream);
int cmk_tta_boxes_to_image(const float* det_box, const float* det_score, const int64_t* det_cls, const float* det_loc,
                           const int32_t* det_counts, const float* table, int A, int K, int img_w, int img_h, float* cand_box,
                           float* cand_score, int32_t* cand_cls, float* cand_loc, int32_t* cand_count, void* stream);
int cmk_tta_boxes_to_aug(const float* box, const int32_t* count, const float* table, int A, int K, float* out_box, int32_t* out_counts,
                         void* stream);
int cmk_tta_reduce_masks(const float* masks, const int32_t* flips, const float* mask_scores, const int32_t* count, int A, int K, int S,
                         float* out_masks, float* out_scores, void* stream);

/* ---- sliced inference (TEST.SLICE, modeling/sliced_inference.py): a large image cut into T equal, overlapping tiles, every tile resized
 * by the ordinary test rule to new_h x new_w and run as a pass of its own, optionally the whole image as pass T; the detections of all
 * A = T (+ 1) passes mapped back and merged by cmk_nms_topk_metric.
 * The map takes a per-pass table in DEVICE memory, 6 floats each: (x0, y0, rx, ry, tw, th) with (x0, y0) the tile's corner in the image,
 * tw x th its size there, rx = tw / new_w and ry = th / new_h computed in double on the host and rounded once to fp32 (the whole image:
 * x0 = y0 = 0, tw x th the image).  Every step is one fp32 operation, nothing is fused.
 *   cmk_slice_boxes_to_image   det_* are the padded (A,K,..) outputs of the passes, det_counts (A) clamped to [0, K].  Per valid detection:
 *                              x' = x * rx, then x' + x0, the same for y; then clipped to the pass's own window [x0, x0 + tw] x
 *                              [y0, y0 + th] (the bounds are one fp32 addition each).  loc is mapped as a point by the same rule, without
 *                              the clip; score is copied, cls narrowed to int32.  Candidates are written compacted in pass order and in
 *                              the detector's order within a pass; cand_count[0] = the sum of the clamped counts; cand_src (A*K) int32
 *                              receives a*K + k, the padded slot the candidate came from (what a mask gather indexes with).  Rows at
 *                              and beyond each count are never read; outputs beyond cand_count[0] are not written.
 * Refused: null pointers, A < 1 or A > 4096, K < 1 or K > 65535, img_w / img_h not in [1, 65535], boxes not 16-byte aligned. ----------- */
int cmk_slice_boxes_to_image(const float* det_box, const float* det_score, const int64_t* det_cls, const float* det_loc,
                             const int32_t* det_counts, const float* table, int A, int K, int img_w, int img_h, float* cand_box,
                             float* cand_score, int32_t* cand_cls, float* cand_loc, int32_t* cand_src, int32_t* cand_count, void* stream);

/* ---- output side: paste (R,S,S) soft masks into (R,H,W) uint8 bitmasks at `threshold` (deploy_utils.py:151-156 ->
 * d2 ROIMasks.to_bitmasks: bilinear grid_sample, align_corners=False, zero padding); boxes (R,4) are the rescaled and
 * clipped output boxes. ------------------------------------------------------------------------------------------------ */
int cmk_paste_masks(const float* masks, const float* boxes, int R, int S, int H, int W, float threshold, uint8_t* out,
                    void* stream);

/* ---- COCO RLE of those bitmasks, the "segmentation" of a result (evaluation/coco_evaluation.py:362-427), in two phases around one
 * host read of the run totals.  masks (R,H,W) bytes 0/1 as cmk_paste_masks writes them.  Runs are taken over the column-major
 * flattening (position x*H + y) and start with a zeros run, 0 long for a mask whose first pixel is set; the string writes every count
 * as 5-bit groups, low group first, + 0x20 while more follow, + 48, counts from the fourth on as the signed difference to the count two
 * back (pycocotools' rleToString as restated by wire.rle_to_string; at most 7 characters per count).
 * ws: cmk_rle_ws_bytes(R, H, W) bytes, 8-byte aligned (0 for arguments the launches refuse): R+1 int64 run offsets, then one int32
 * per (mask, 64-row chunk, column).  Refused: H or W < 1, H*W >= 2^31 - 1 (positions and run totals are int32), R > 65535, null pointers,
 * a workspace too small.  R == 0 is CMK_OK with no launch. */
int64_t cmk_rle_ws_bytes(int R, int H, int W);
/* evaluation/coco_evaluation.py:362-427, count phase: n_runs[r] = runs of mask r; ws keeps the scanned offsets for the encode phase. */
int cmk_rle_count(const uint8_t* masks, int R, int H, int W, void* ws, int64_t ws_bytes, int32_t* n_runs, void* stream);
/* evaluation/coco_evaluation.py:362-427, encode phase, after cmk_rle_count on the same masks, ws and n_runs.  With T the sum of n_runs
 * and off[r] the sum of n_runs[0..r): counts (T int32) gets the run lengths of mask r at off[r]; bytes (7*T) its string at 7*off[r],
 * lens[r] characters long; starts (T int32) is scratch. */
int cmk_rle_encode(const uint8_t* masks, int R, int H, int W, const void* ws, int64_t ws_bytes, const int32_t* n_runs, int32_t* starts,
                   int32_t* counts, uint8_t* bytes, int64_t* lens, void* stream);

/* ---- mask IoU counts for COCO evaluation (evaluation/coco_evaluation.py:543-591 hands results and annotations to pycocotools, whose
 * hot loop is the IoU of every detection mask with every ground-truth mask of an image).  A packed mask is ceil(H*W / 64) 64-bit words:
 * bit p % 64 of word p / 64 is the row-major pixel p = y*W + x, the unused high bits of the last word are zero.  All results are
 * integers.  Refused: H or W < 1, H*W >= 2^31 - 1 (positions and areas are int32), a mask count above 65535, null pointers (the bitmask
 * output of the decoder excepted).  A mask count of 0 is CMK_OK with no launch.  Nothing is allocated or synchronised.
 * evaluation/coco_evaluation.py:543-591, detections: masks (R,H,W) bytes 0/1 as cmk_paste_masks writes them -> words (R, ceil(H*W/64))
 * and areas[r], the set pixels of mask r. */
int cmk_mask_pack_bits(const uint8_t* masks, int R, int H, int W, uint64_t* words, int32_t* areas, void* stream);
/* evaluation/coco_evaluation.py:543-591, ground truth: the inverse of the RLE encoder.  Mask m is given by the inclusive prefix sums
 * cum[off[m]] .. cum[off[m+1] - 1] of its COCO run lengths (column-major positions x*H + y, zeros run first, possibly 0 long); the last
 * prefix sum of every mask must be H*W, which the caller checks: the kernel does not.  Writes the packed row-major words, areas, and the
 * (M,H,W) byte bitmasks unless `bitmasks` is null. */
int cmk_rle_decode_pack(const int32_t* cum, const int64_t* off, int M, int H, int W, uint64_t* words, int32_t* areas, uint8_t* bitmasks,
                        void* stream);
/* evaluation/coco_evaluation.py:543-591, the table: inter[n*M + m] = popcount(det[n] AND gt[m]) over packed det (N, words) and
 * gt (M, words).  Zeroes inter on the stream, then accumulates with integer atomics.  N == 0 or M == 0: CMK_OK, nothing written. */
int cmk_mask_intersections(const uint64_t* det, int N, const uint64_t* gt, int M, int H, int W, int32_t* inter, void* stream);
/* Boundary IoU (Cheng et al., CVPR 2021; iouType "boundary" of the published boundary evaluation API, restated in DESIGN §3 "COCO
 * evaluation" and never run beside it): the boundary of a mask m is m AND NOT eroded, where eroded(y,x) = 1 iff every pixel of the
 * (2d+1)x(2d+1) square centred on (y,x) lies inside the image and is set (the mask zero-padded by one pixel, eroded d times with a 3x3
 * all-ones element).  words: R packed masks as the two producers above write them; bwords (R, ceil(H*W/64)) gets the packed boundary of
 * each in the same layout, unused high bits zero, bareas[r] its set pixels.  Out of place: bwords must not overlap words.  No byte
 * bitmap is read or written.  bwords and bareas are zeroed on the stream and filled with integer OR / add atomics (a 64-pixel word of the
 * linear layout belongs to several rows or tiles).  With 2d+1 > min(H, W) no square fits, the erosion is empty and bwords is a copy of words, for any
 * d >= 1.  Otherwise d is at most CMK_BOUNDARY_MAX_D at any W: the halo of 2d rows lies in 64 KiB of LDS.  Refused before any launch:
 * the conditions above, d < 1, d > CMK_BOUNDARY_MAX_D where a square fits.  R == 0 is CMK_OK with no launch. */
#define CMK_BOUNDARY_MAX_D 128
int cmk_mask_boundary_bits(const uint64_t* words, int R, int H, int W, int d, uint64_t* bwords, int32_t* bareas, void* stream);
/* The inverse of cmk_mask_pack_bits: packed words (R, ceil(H*W/64)) -> masks (R,H,W) bytes 0/1. */
int cmk_mask_unpack_bits(const uint64_t* words, int R, int H, int W, uint8_t* masks, void* stream);
/* Overlap counts for Cityscapes instance evaluation (evaluation/cityscapes_evaluation.py:47-130 writes every predicted mask as a PNG for
 * cityscapesscripts, whose hot loop compares it with the ground-truth image once per ground-truth instance; the rule is restated in
 * DESIGN §3 "Cityscapes evaluation").  words: N packed masks as cmk_mask_pack_bits writes them.  cols: H*W row-major uint16, the column
 * of each pixel.  table[n*C + c] = the pixels p with bit p of mask n set and cols[p] == c; a pixel whose column is >= C is counted
 * nowhere.  Zeroes table on the stream, then accumulates with integer atomics (a C-entry histogram in LDS per workgroup, hence the cap
 * on C).  Refused before any launch: null pointers, H or W < 1, H*W >= 2^31 - 1, N outside [0, 65535], C outside
 * [1, CMK_LABEL_MAX_COLS].  N == 0 is CMK_OK with no launch.  Nothing is allocated or synchronised. */
#define CMK_LABEL_MAX_COLS 4096
int cmk_mask_label_counts(const uint64_t* words, int N, const uint16_t* cols, int H, int W, int C, int32_t* table, void* stream);

/* ---- visualizer (visualizer.py:21-38 hands the post-processed Instances to detectron2's Visualizer.draw_instance_predictions, which
 * draws on the host with matplotlib; this picture is the package's own, in integer arithmetic: DESIGN §3 "Visualizer").  Images are
 * (H,W,3) uint8, colours are bytes in the image's channel order.  Refused by all three: H or W < 1, H*W >= 2^31 - 1, n < 0 or n > 65535,
 * a line width or font scale outside 1..16, null pointers.  Nothing is allocated or synchronised.
 * visualizer.py:21-38, the record of one instance: cmk_vis_record_ints() int32, a multiple of 4 (the layout is the library's own);
 * cmk_vis_compose reads records through 16-byte loads and refuses a records pointer that is not 16-byte aligned. */
int cmk_vis_record_ints(void);
/* visualizer.py:21-38, per instance, on the device: records[j] describes instance order[j] (the draw order, largest box first): the
 * integer box rect floor(clamp(c, +-2^20)) or "no box, no label" for a NaN coordinate, the label NAME + " " + P + "%" as glyph indices of
 * the 41-glyph font (P = clamp(floor(score * 100 + 0.5), 0, 100) in float64, NaN -> 0; at most 32 glyphs), its plate rect clamped into the
 * image, and col = palette[k mod 64] (k the original index, or the class with color_by_class), edge = col*154 >> 8,
 * text = col + ((255 - col)*179 >> 8).  names: num_names rows of 32 glyph indices with name_lens; a class outside [0, num_names) is
 * named "C<id>".  palette: 64 x 3 bytes.  boxes (n,4), scores (n), classes (n) int64, order (n) int64.  n == 0: CMK_OK, no launch.
 * Nothing outside the inputs is read whatever they hold: an order[j] outside [0, n) stands for j, a name length is clamped into [0, 32],
 * a glyph byte above 40 is glyph 40. */
int cmk_vis_prepare(const float* boxes, const float* scores, const int64_t* classes, const int64_t* order, const uint8_t* names,
                    const int32_t* name_lens, int num_names, const uint8_t* palette, int n, int H, int W, int font_scale, int color_by_class,
                    int32_t* records, void* stream);
/* visualizer.py:21-38, the picture: image_out = image_in with, per record in order, the box frame (line_width thick, opaque col), the
 * mask fill c = (c*(256 - alpha256) + col*alpha256 + 128) >> 8, the mask outline (set pixels with an unset or outside 4-neighbour,
 * opaque edge), the label plate c = (c*51 + 128) >> 8 and its glyphs (font: 41 x 7 row bytes, bit 4 the left column; font_scale^2 pixels
 * per font pixel; opaque text).  words: the packed masks of cmk_mask_pack_bits, (n, ceil(H*W/64)), indexed by ORIGINAL instance; null
 * draws no masks.  alpha256 in [0, 256].  Out of place: overlapping images are refused.  n == 0 copies the image (records, font unused). */
int cmk_vis_compose(const uint8_t* image_in, uint8_t* image_out, int H, int W, const uint64_t* words, const int32_t* records, int n,
                    const uint8_t* font, int line_width, int font_scale, int alpha256, void* stream);
/* visualizer.py:21-38, keypoints, IN PLACE on the composed image.  keypoints (n, num_keypoints, 3) as (x, y, score), indexed by original
 * instance; a point is visible iff score > threshold and neither coordinate is NaN; centres floor(clamp(c, +-2^15)).  Per record in
 * order: the skeleton's segments (num_segments pairs of keypoint indices; both ends visible; pixels within line_width / 2 of the segment,
 * exact in int64; colour col), then the visible points as discs of radius max(2, line_width + 1) in keypoint_color (bytes 0..2).  The
 * latest primitive wins a pixel: winner, (H,W) int32 scratch, takes the atomic maximum of the sequence numbers, a second pass colours.
 * A segment with an index outside [0, num_keypoints) is not drawn.  num_keypoints in [1, 1024], num_segments in [0, 4096].
 * n == 0: CMK_OK, no launch. */
int cmk_vis_keypoints(uint8_t* image, int H, int W, const float* keypoints, const int32_t* records, int n, int num_keypoints,
                      const int32_t* skeleton, int num_segments, float threshold, int line_width, int keypoint_color, int32_t* winner,
                      void* stream);
/* cmk_vis_prepare with the colour of an instance chosen by the caller: col = palette[color_ids[k] mod 64] (k the original index, the
 * remainder taken non-negative; color_by_class is not consulted).  color_ids (n) int32 by ORIGINAL instance, e.g. the track ids of
 * cmk_vis_track_assign.  A null color_ids is cmk_vis_prepare, bit for bit. */
int cmk_vis_prepare_ids(const float* boxes, const float* scores, const int64_t* classes, const int64_t* order, const uint8_t* names,
                        const int32_t* name_lens, int num_names, const uint8_t* palette, int n, int H, int W, int font_scale, int color_by_class,
                        const int32_t* color_ids, int32_t* records, void* stream);

/* ---- video: instance ids that follow objects from frame to frame (the reference's demo.py --video-input draws with detectron2's
 * VideoVisualizer, whose _assign_colors matches a frame's instances to the previous frame's by IoU on the host; restated in DESIGN §3
 * "Video").  The track table lives on the device: max_tracks rows of box (4 float), class (int64), id (int32), ttl (int32) and, in mask
 * mode, packed mask words and area, plus counters (4 int32: n_tracks, next_id, dropped, spare).  A frame's update reads one table and
 * writes another (the two halves of a ping-pong pair, never in place); counters are updated in place.  Nothing is read back, allocated or
 * synchronised.  Refused by all: null pointers, max_tracks outside [1, 1024], n outside [0, max_tracks], rows outside [0, max_tracks].
 * The float64 table iou[i*n + j] of old row i < rows against new instance j < n, boxes as (x1, y1, x2, y2): iw = min(x2) - max(x1),
 * ih = min(y2) - max(y1), inter = iw*ih if both are positive, else 0, iou = inter / (a_old + a_new - inter) with a = (x2-x1)*(y2-y1),
 * all in float64 without contraction; a zero union or a NaN gives 0.  rows == 0 or n == 0: CMK_OK, no launch. */
int cmk_vis_track_iou_boxes(const float* old_boxes, int rows, const float* new_boxes, int n, double* iou, void* stream);
/* One frame of the association rule.  With T = min(n_tracks, rows): value[i][j] of old row i < T and new instance j is 0 where the
 * classes differ, else iou[i*n + j] (box mode, `iou` given) or inter[i*n + j] / (old_areas[i] + new_areas[j] - inter[i*n + j]) in float64
 * (mask mode, `inter` given, the table of cmk_mask_intersections(old words, rows, new words, n); a zero union gives 0); exactly one of iou
 * and inter is non-null unless n == 0.  best[i] is the first j that attains the row maximum; i is a candidate iff the maximum is
 * > threshold.  New j takes the id of the smallest candidate i with best[i] == j, every other new instance next_id, next_id + 1, .. in
 * order of j.  Every other old row misses: ttl - 1, and survives iff that is > 0.  The new table: the n new instances in order with
 * ttl = `ttl`, then the survivors in old order while they fit in max_tracks; the rest add to `dropped`.  src[slot] = j for a new row,
 * n + i for a survivor (the map cmk_vis_track_gather follows); track_ids[j] is the id of new instance j.  Always launches (n == 0 ages the
 * table).  A NaN value counts as 0; counters[0] is clamped into [0, rows].  ttl in [1, 255], threshold in [0, 1].  Out of place: an out
 * array overlapping its old array (max_tracks rows of each) is refused. */
int cmk_vis_track_assign(const double* iou, const int32_t* inter, const int32_t* old_areas, const int32_t* new_areas, int rows,
                         const float* old_boxes, const int64_t* old_classes, const int32_t* old_ids, const int32_t* old_ttl,
                         const float* new_boxes, const int64_t* new_classes, int n, int max_tracks, int ttl, double threshold,
                         float* out_boxes, int64_t* out_classes, int32_t* out_ids, int32_t* out_ttl, int32_t* src, int32_t* track_ids,
                         int32_t* counters, void* stream);
/* Mask mode, after cmk_vis_track_assign on the same src and counters: out row s < n_tracks gets the ceil(H*W/64) words and the area of
 * new instance src[s], or of old row src[s] - n.  rows: how many out rows can be live (n_tracks <= rows is the caller's bound; the grid).
 * Out of place: out_words overlapping old_words or new_words is refused, as is H*W >= 2^31 - 1.  rows == 0: CMK_OK, no launch.
 * A src[s] that names neither (negative, or n + max_tracks and above) leaves out row s unwritten; rows at and beyond
 * min(n_tracks, max_tracks, rows) are never written. */
int cmk_vis_track_gather(const int32_t* src, const int32_t* counters, const uint64_t* old_words, const int32_t* old_areas,
                         const uint64_t* new_words, const int32_t* new_areas, int n, int rows, int max_tracks, int H, int W,
                         uint64_t* out_words, int32_t* out_areas, void* stream);

/* ---- mask contours: the exact outlines of packed masks as closed loops of int32 lattice vertices (x, y), 0 <= x <= W, 0 <= y <= H
 * (the reference's visualizer.py:35-37 reaches polygons through detectron2's GenericMask.mask_to_polygons; the rule here is this
 * package's own, DESIGN §3 "Contours").  Pixel (row r, column c) is the square [c, c+1] x [r, r+1], outside the image is background,
 * foreground is 4-connected.  Every unit edge between a set and an unset pixel is walked once with the foreground on the right (a set
 * pixel's top edge runs +x, its right edge +y, with y down); at a saddle vertex (the two set pixels of the 2x2 diagonal) the walk turns
 * right.  Only corners are emitted.  A loop starts at its smallest vertex in (y, x) order, the loops of a mask are sorted by that start.
 * Outer boundaries have a positive doubled area sum(x_i*y_{i+1} - x_{i+1}*y_i), holes a negative one.
 * Two phases around one host read of the corner totals, as the RLE entries.  words: R packed masks as cmk_mask_pack_bits writes them.
 * ws: cmk_vis_contour_ws_bytes(R, H, W) bytes, 8-byte aligned (0 for arguments the launches refuse): R+1 int64 corner offsets, one int64
 * per (mask, 1024 words of its vertex lattice), then one int32 per (mask, lattice row, 64 vertices of it).  Refused by both phases before any launch: null pointers, H or W < 1,
 * H*W >= 2^31 - 1, R outside [0, 65535], a workspace too small, outputs that overlap the inputs.  R == 0 is CMK_OK with no launch.
 * Nothing is allocated or synchronised. */
int64_t cmk_vis_contour_ws_bytes(int R, int H, int W);
/* visualizer.py:35-37, count phase: n_corners[r] (device, R int32) = vertices of all loops of mask r, always even (-1 where they do not
 * fit int32); ws keeps the scanned offsets for the trace phase. */
int cmk_vis_contour_count(const uint64_t* words, int R, int H, int W, void* ws, int64_t ws_bytes, int32_t* n_corners, void* stream);
/* Scratch bytes of the trace phase for `total` corners (0 for a negative total): corner records, successor links and the ping-pong
 * buffers of the loop ranking. */
int64_t cmk_vis_contour_trace_ws_bytes(int total);
/* visualizer.py:35-37, trace phase, after cmk_vis_contour_count on the same words and ws.  n_corners: the R totals the count phase
 * wrote, read back by the caller and passed here in HOST memory; with T their sum and off[r] the sum of n_corners[0..r), xy (device,
 * 2*T int32) gets the vertices of mask r at off[r] as x, y pairs, loop after loop in canonical order, and head (device, T int32) is 1 at
 * the first vertex of every loop, else 0.  scratch: cmk_vis_contour_trace_ws_bytes(T) bytes on the device, 16-byte aligned.  Also
 * refused: an n_corners that is negative or odd, a T that does not fit int32, a scratch too small.  T == 0 launches nothing.  No kernel
 * writes outside [0, T) whatever the device totals are. */
int cmk_vis_contour_trace(const uint64_t* words, int R, int H, int W, const void* ws, int64_t ws_bytes, const int32_t* n_corners,
                          void* scratch, int64_t scratch_bytes, int32_t* xy, int32_t* head, void* stream);

/* ---- multi-GPU result exchange (the reference's analogue: comm.gather in evaluation/coco_evaluation.py:155-156) ----------
 * One fixed-stride float record per image, written straight into the all-gather send buffer:
 * [box 4K | score K | mask_score K | loc 2K | class K (as float) | mask K*hw*hw | count], K*(9 + hw*hw) + 1 floats.
 * N in [1, 65535] (the grid's y dimension), K, hw >= 1 and a record width that fits an int: CMK_EINVAL otherwise. */
int cmk_pack_records(const float* box, const float* score, const float* mask_scores, const float* loc, const int64_t* cls,
                     const float* masks, const int32_t* counts, int N, int K, int mask_hw, float* rec /* N * width */, void* stream);

/* The same record for a KEYPOINT_ON model, the keypoints in front of the count (cmk_pack_records is unchanged; no new ABI version):
 * [box 4K | score K | mask_score K | loc 2K | class K | mask K*hw*hw | keypoints K*Kp*3 (x, y, score) | count],
 * K*(9 + hw*hw + 3*Kp) + 1 floats.  keypoints (N, K, Kp, 3).  N in [1, 65535], K, hw, Kp >= 1. */
int cmk_pack_records_kp(const float* box, const float* score, const float* mask_scores, const float* loc, const int64_t* cls,
                        const float* masks, const float* keypoints, const int32_t* counts, int N, int K, int mask_hw, int num_keypoints,
                        float* rec /* N * width */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
