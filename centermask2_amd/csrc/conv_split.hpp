// Split products, shared by the opt-in kernels that build fp32-accurate products on the 16-bit matrix instructions (conv_pw.hip SPLIT 1 | 2,
// conv_sp3.hip): the split of a staged float4 into 16-bit pieces and the groups of MFMAs that multiply the pieces, small terms first.
#pragma once
#include "conv_args.hpp"

namespace cmk {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- two fp16 pieces: x = h + m, h = fp16(x), m = fp16(x - h): 11 + 11 = 22 bits of significand, the residual x - h is exact in fp32 ----------
// fp16's narrow exponent is handled by scaling, all powers of two (exact):
//   activations  x' = x * 2^-4 (|x| up to 1e6 stays finite; measured: up to 65504 * 2^4 = 1.04e6, NaN beyond — h = Inf, the residual Inf - Inf);
//                the residual is stored as fp16((x' - h) * 2^11), a normal fp16 down to |x| = 2^-21 (unscaled it would be subnormal below
//                |x| = 0.06); h itself is subnormal below |x| = 2^-10, so from there on x keeps an absolute error of about 2^-31 and not 22 bits
//                (measured on whole tensors that small: cmk.h tune_wm 11), and the weight piece the residual meets is multiplied by 2^-11 in
//                registers (4 packed multiplies per tap and cout tile);
//   weights      w' = w * S_w with S_w the power of two that puts max |w'| in [2^14, 2^15) (host, per conv): both pieces of every weight
//                larger than 2^-17 of the largest are normal fp16;
//   the accumulator is multiplied by 2^4 / S_w in the epilogue (folded into the per-channel scale).
constexpr float SPLIT_SX = 0.0625f, SPLIT_RS = 2048.f;      // activation scale 2^-4, residual scale 2^11

// x: four activations already times SPLIT_SX; h, m: their pieces as two packed pairs each (m = the residual times SPLIT_RS)
__device__ __forceinline__ void split_f16(f32x4 x, u32x2& h, u32x2& m) {
    auto pk = [](float x0, float x1) { return __builtin_bit_cast(unsigned, f16x2{(_Float16)x0, (_Float16)x1}); };       // round to nearest even
    auto unpk = [](unsigned p) { const f16x2 h_ = __builtin_bit_cast(f16x2, p); return f32x2{(float)h_.x, (float)h_.y}; };
    h.x = pk(x.x, x.y); h.y = pk(x.z, x.w);
    const f32x2 h01 = unpk(h.x), h23 = unpk(h.y);
    const f32x4 r1 = f32x4{x.x - h01.x, x.y - h01.y, x.z - h23.x, x.w - h23.y} * SPLIT_RS;      // exact: h holds the leading bits of x
    m.x = pk(r1.x, r1.y); m.y = pk(r1.z, r1.w);
}

// the weight piece that meets the activations' scaled residual
__device__ __forceinline__ f16x8 split_f16_bhs(f16x8 Bh) { return Bh * (_Float16)(1.f / SPLIT_RS); }

// m*h, h*m, h*h (what is dropped, m*m, is 2^-22 of the product); Bhs = split_f16_bhs(Bh)
__device__ __forceinline__ f32x16 mfma3_f16(f16x8 Ah, f16x8 Am, f16x8 Bh, f16x8 Bm, f16x8 Bhs, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Am, Bhs, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
    return acc;
}

// ---- three bf16 pieces: x = h + m + l exactly to 2^-24, h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even; no scaling ----
// one piece: returns bf16(r), two packed pairs, and leaves what it does not hold in r — three calls give h, m, l (a caller stores each as it appears)
__device__ __forceinline__ u32x2 split_bf16_piece(f32x4& r) {
    auto pk = [](float x0, float x1) { unsigned p; asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(x0), "v"(x1)); return p; };
    auto f_lo = [](unsigned p) { return __builtin_bit_cast(float, p << 16); };
    auto f_hi = [](unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); };
    u32x2 h;
    h.x = pk(r.x, r.y); h.y = pk(r.z, r.w);
    r = f32x4{r.x - f_lo(h.x), r.y - f_hi(h.x), r.z - f_lo(h.y), r.w - f_hi(h.y)};
    return h;
}

// the six products of weight >= 2^-16: l*h, h*l, m*m, m*h, h*m, h*h
__device__ __forceinline__ f32x16 mfma6_bf16(bf16x8 Ah, bf16x8 Am, bf16x8 Al, bf16x8 Bh, bf16x8 Bm, bf16x8 Bl, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Am, Bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc, 0, 0, 0);
    return acc;
}

}  // namespace cmk
