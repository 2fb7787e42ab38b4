// Shared by the conv kernels of libcmk_hip.so and their front door (conv.hip): launch arguments (one struct passed by value), vector types
// and the prototypes through which conv.hip reaches each kernel file.
#pragma once
#include "cmk_common.hpp"

namespace cmk {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// bounds-checked 16- | 8-byte loads: lanes whose byte offset lies outside [0, num_records) of the resource get 0
__device__ f32x4 buffer_load_f32x4(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ f32x2 buffer_load_f32x2(i32x4 rsrc, int voffset, int soffset, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");

// buffer resource {base, num_records = bytes, raw dword format} over `bytes` bytes from a wave-uniform base
__device__ __forceinline__ i32x4 buffer_rsrc(const void* base, int bytes) {
    const unsigned long long b = (unsigned long long)base;
    i32x4 rsrc;
    rsrc.x = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffull));
    rsrc.y = __builtin_amdgcn_readfirstlane((int)((b >> 32) & 0xffffull));
    rsrc.z = __builtin_amdgcn_readfirstlane(bytes);
    rsrc.w = 0x00020000;
    return rsrc;
}

// a pointer every lane holds the same value of, moved to the scalar unit (the saddr of the epilogues' global_store walks)
__device__ __forceinline__ unsigned long long wave_uniform_u64(const void* p) {
    const unsigned long long b = (unsigned long long)p;
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)b);
}

constexpr int PST = 20;      // LDS row pitch in floats: 16 channels + 4 pad
constexpr int MAXP = 10;     // problems per launch: the 5 FPN levels, twice where two convs with different weights share a launch (F(4x4) kernels)
constexpr int LDS_CU = 160 * 1024;

// workgroups per CU the register budget allows (accumulators: 16 VGPRs per 32x32 tile)
__host__ __device__ constexpr int occ_of(int wm, int wn, int stride) { return (stride == 1 && (wm == 1 ? wn <= 5 : wn <= 2)) ? 3 : 2; }

struct ConvProblem {
    const float* x; float* y; const float* scale; const float* shift;
    const float* in_scale; const float* in_shift;   // optional (N, Cin): x' = relu(x * in_scale + in_shift) while staging (fused GroupNorm+ReLU)
    const float* w;                                 // F(4x4) kernels: this problem's packed U (problems of one launch may differ in weights); conv_sp3: its fp16 split packing
    float acc_scale;                                // conv_sp3: 1 / S_w of this problem's weights (cmk.h w_splith_scale)
    int N, H, W, Ho, Wo;
    int tiles_h, tiles_w, tile_begin;
    long total_pix;  // N*Ho*Wo
};

struct ConvArgs {
    ConvProblem p[MAXP];
    int nprob;
    const float* w; const float* res;
    int Cin, Cout;
    int x_cs, x_co, y_cs, y_co, res_cs, res_co, res_mode, Hr, Wr;
    int relu_upto, in_relu;
    int cout_pad;
    int total_tiles;   // spatial tiles of all problems (XCD-aware kernels pad the grid to a multiple of 8 tiles)
    int ksplit;        // split-K: blockIdx.y owns an (even) range of the 16-channel chunks and writes raw partial sums to ws
    float* ws;         // [ksplit][total_pix][cout_pad]; with a tail (below): [tail_ksplit][tail images][H*W][cout_pad]
    // conv_wino6, RoI-pair geometry: "tail split-K".  The last tail_tiles spatial tiles (pairs of images) are not run as one workgroup per
    // (tile, cout tile) but as tail_ksplit short ones that share its chunk loop and leave raw partial sums in ws; their blocks follow the
    // main_blocks blocks of the other tiles in the grid, so they are dispatched last and fill the ragged last round.  0 = off.
    int tail_tiles, tail_ksplit, main_blocks;
    double* gn_ws;     // Winograd 2-WG form: per (spatial tile, row parity, group) partial {sum, sum of squares} of the outputs (fused GroupNorm statistics)
    int gn_cpg, gn_groups;
    int ga_stride;     // gather form (GA): stride of the 3x3 conv whose taps are walked as 9x more K chunks
    float* pool_ws;    // conv_pw only: per 32*MT-row block two records of Cout floats (cmk.h: cmk_conv_desc.pool_ws)
    int grid_y;   // N tiles; the N-tile index is the FASTEST block coordinate so the workgroups sharing an input tile run together (L2 reuse)
};

// per-device one-time kernel attribute set-up (hipFuncSetAttribute is per device; a process may drive several)
struct DeviceOnce {
    unsigned char done[64] = {0};
    template <typename F>
    int run(F&& f) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail(CMK_ELAUNCH, "hipGetDevice failed%s", "");
        if (__atomic_load_n(&done[dev], __ATOMIC_ACQUIRE)) return CMK_OK;
        int rc = f();
        if (rc == CMK_OK) __atomic_store_n(&done[dev], 1, __ATOMIC_RELEASE);   // idempotent: a race only repeats the call
        return rc;
    }
};

struct Variant { int wm, sc, wn; };

// What a launch would run, said by the code that picks it (cmk_conv_plan).  Every launch_* below takes a LaunchPlan*: null launches; otherwise
// all checks and the geometry set-up run as for a launch, and the leaf launcher — the template function that names the kernel — fills the plan
// next to its hipLaunchKernelGGL and returns before it touches a device.
struct LaunchPlan {
    char kernel[96];            // the instantiation as a profiler prints it, minus "void cmk::" and the argument list
    int64_t executed_flops;     // FLOPs the matrix pipe executes, tile padding included (blocks that only pad the grid to 8 tiles are not); the
                                // split-product forms in fp32-equivalent FLOPs
    int gn_records[MAXP];       // per problem: {sum, sumsq} records per image written through gn_ws; 0 = none
};

inline const char* tf(bool b) { return b ? "true" : "false"; }      // a bool template argument as a demangled name spells it
constexpr int64_t MFMA_FLOPS = 2 * 32 * 32 * 2;      // one v_mfma_f32_32x32x2_f32

inline int out_size(int h, int stride) { return stride == 1 ? h : (h - 1) / 2 + 1; }     // k3 p1 s2: floor((H+2-3)/2)+1

// conv_igemm.hip: the direct implicit-GEMM kernel, variant v (= WM, SC, WN) of a 1x1 or a 3x3 stride 1 | 2 conv; sets a.cout_pad
int launch_igemm(ConvArgs& a, int ksize, int stride, int cout32, Variant v, hipStream_t st, LaunchPlan* plan);
// conv_igemm.hip: its gather form (cmk.h tune_wm 7), wn = 4 | 2 | 1 cout tiles per wave
int launch_igemm_gather(ConvArgs& a, int wn, int grid_y, hipStream_t st, LaunchPlan* plan);
// conv_igemm.hip: whether the direct kernel has variant (wm, sc, wn) for this conv, and the cost model's choice among those it has
bool variant_ok(int taps, int stride, int cout32, int wm, int sc, int wn);
Variant choose_variant(const cmk_conv_desc* descs, int n, int taps, int stride, int cout32);
// conv_wino4r.hip: fused Winograd F(2x2,3x3); its {sum, sumsq} records per H x W image (cmk.h gn_ws)
int launch_wino4r(ConvArgs& a, hipStream_t st, LaunchPlan* plan);
int wino4r_gn_records(int H, int W);
// conv_wino6.hip: fused Winograd F(4x4,3x3); pair: the paired form, 64 couts per workgroup from one shared W image (one 8-wave workgroup per CU)
int launch_wino6(ConvArgs& a, int geo, bool pair, hipStream_t st, LaunchPlan* plan);
int wino6_gn_records(int H, int W);      // records per H x W image of the three F(4x4) kernels (map tiles; the RoI-pair geometry writes none)
// conv_wino6s.hip: the same, 64 couts per workgroup from one frequency image shared through LDS (one 8-wave workgroup per CU)
int launch_wino6s(ConvArgs& a, int geo, hipStream_t st, LaunchPlan* plan);
// conv_pw.hip: 1x1 conv as a GEMM with the weights fetched straight into registers; mt = 4 | 2 accumulator rows per wave
int launch_pw(ConvArgs& a, int mt, hipStream_t st, LaunchPlan* plan);
// conv_pw.hip, opt-in: the same GEMM from split products (fp32-accurate; mode 1: three bf16 pieces, a.w = cmk.h w_split; 2: two fp16 pieces, w_splith)
int launch_pw_split(ConvArgs& a, int mode, hipStream_t st, LaunchPlan* plan);
// conv_sp3.hip, opt-in: 3x3 stride-1 conv as a direct implicit GEMM on fp16-split products (halo tile in LDS, 2 pieces per operand, geo 0..3)
int launch_sp3(ConvArgs& a, int geo, int pieces, hipStream_t st, LaunchPlan* plan);

}  // namespace cmk
