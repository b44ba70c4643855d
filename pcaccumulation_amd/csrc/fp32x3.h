// The "fp32x3" compute mode: fp32 accuracy on the 16-bit matrix cores.  The one definition of its arithmetic, shared by conv_split.hip (3x3 convolutions),
// mlp_split.hip (per-point linear layers) and pfn_block_split.hip (the pillar encoder's residual block).  fp32 tensors in and out, every product formed
// from fp16 hi / lo halves of SCALED operands,
//
//     s x = x_hi + x_lo (+ 2^-22 s|x|),  t w = w_hi + w_lo:   (t w)(s x)  ~=  w_hi x_lo + w_lo x_hi + w_hi x_hi      (w_lo x_lo <= 2^-22 dropped)
//
// three v_mfma_f32_32x32x16_f16 per fragment pair, fp32 accumulation, result divided by s t.  Every kernel issues the terms in the order
// hi*lo, lo*hi, hi*hi (small terms first) and writes the three MFMA calls out where they stand: a helper around them changed the register
// allocation of one mlp_split.hip kernel.  fp16 carries 11 significant bits, so hi + lo keep 22 (fp32 has 24): relative error ~3e-7 per product -- the first version of conv_split.hip split into bf16 halves (8 + 8 bits, 4e-6
// per product, 2e-5 after the U-Net) and left the c4 scene-flow EPE 1.04e-3 from the reference and the gradient norms of the
// ill-conditioned loss terms up to 6 % off (profiles/r03_gradnorm_sensitivity.txt).  fp16's narrow exponent range is handled by
// power-of-two scales: s per input TENSOR (from its absolute maximum, pcacc_absmax256: the scaled maximum lands in [2^13, 2^14)), t for
// the weights, fixed where they are prepared or staged (per output-channel row in conv_split.hip and mlp_split.hip, per matrix in
// pfn_block_split.hip: three policies, each in its file).  Elements far below the tensor's maximum lose relative, not
// absolute precision (their lo half becomes subnormal): errors stay below 2^-22 of the LARGEST operand, which is what a sum needs.
// Rate: a third of the fp16 / bf16 matrix rate = 5x the fp32 MFMA rate (v_mfma_f32_32x32x2_f32 runs at 1/16).  This is the mode in
// which the dense stacks (models/unet.py:11-20,45-113, models/stpn.py:13-43 -- fp32 convolutions in the reference) meet north_star's
// 1e-3 on hand-written kernels; the fp32 mode used the library's fp32 convolutions for that (98.8 ms per step, 43 ms of it MIOpen).
#pragma once
#include "common.h"

typedef _Float16 x3_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 x3_f16x2 __attribute__((ext_vector_type(2)));
typedef pcacc_f32x16 x3_f32x16;

#define X3_AMAX_PARTS 256                      // partial maxima pcacc_absmax256 leaves for its consumers

// power-of-two scale that puts a tensor's absolute maximum into [2^13, 2^14) (fp16 overflows at 65504); 1 for an all-zero tensor.
// A non-finite maximum gives scale 1: the non-finite element then reaches the output as inf / NaN, as it would in fp32 arithmetic.
__device__ __forceinline__ float x3_scale_of(float amax)
{
    if (!(amax > 0.f) || !(amax < __builtin_inff())) return 1.f;
    int k;
    frexpf(amax, &k);                                         // amax = m 2^k, m in [0.5, 1)
    return ldexpf(1.f, 14 - k);
}
__device__ __forceinline__ float x3_wave_max(float m)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    return m;
}
// largest of the 256 partial maxima of one tensor (and of a second one when given): every lane reduces them (wave-uniform result, no LDS,
// no barrier)
__device__ __forceinline__ float x3_amax(const float *__restrict__ parts, const float *__restrict__ parts2)
{
    const int lane = threadIdx.x & 63;
    float m = fmaxf(fmaxf(parts[lane], parts[lane + 64]), fmaxf(parts[lane + 128], parts[lane + 192]));
    if (parts2) m = fmaxf(m, fmaxf(fmaxf(parts2[lane], parts2[lane + 64]), fmaxf(parts2[lane + 128], parts2[lane + 192])));
    return x3_wave_max(m);
}

__device__ __forceinline__ uint32_t x3_pack(float a, float b)
{
    const pcacc_f32x2 f = {a, b};
    const x3_f16x2 r = __builtin_convertvector(f, x3_f16x2);  // round to nearest even
    return *reinterpret_cast<const uint32_t *>(&r);
}
__device__ __forceinline__ pcacc_f32x2 x3_unpack(uint32_t v)
{
    return __builtin_convertvector(*reinterpret_cast<const x3_f16x2 *>(&v), pcacc_f32x2);
}

#ifdef PCACC_X3_EXPERIMENT
// common.h: precision-map experiment build.  One word per translation unit, set through that file's pcacc_x3_experiment_* entry point.
static __device__ int x3_xword;
static inline int x3_set_word(int word, void *stream)
{
    if (hipStreamSynchronize(pcacc_stream(stream)) != hipSuccess) return PCACC_E_LAUNCH;     // kernels already queued keep the word they were launched under
    return hipMemcpyToSymbol(HIP_SYMBOL(x3_xword), &word, sizeof(int)) == hipSuccess ? PCACC_OK : PCACC_E_LAUNCH;
}
#endif
// WEIGHT: the operand is a weight (the experiment build treats activations and weights separately; no difference in the shipped library)
template <bool WEIGHT = false>
__device__ __forceinline__ void x3_split2(float a, float b, uint32_t &hi, uint32_t &lo)
{
#ifdef PCACC_X3_EXPERIMENT
    const bool drop = pcacc_x_apply(WEIGHT ? PCACC_X_W(x3_xword) : PCACC_X_ACT(x3_xword), a, b);
#endif
    hi = x3_pack(a, b);
    const pcacc_f32x2 back = x3_unpack(hi);
    lo = x3_pack(a - back[0], b - back[1]);                   // exact differences (Sterbenz); an inf hi gives NaN here, as it should
#ifdef PCACC_X3_EXPERIMENT
    if (drop) lo = 0u;
#endif
}
// eight fp32, scaled by s -> eight fp16 hi + eight fp16 lo (round to nearest even both times)
template <bool WEIGHT = false>
__device__ __forceinline__ void x3_split8(const float4 &a, const float4 &b, float s, uint4 &hi, uint4 &lo)
{
    x3_split2<WEIGHT>(a.x * s, a.y * s, hi.x, lo.x);
    x3_split2<WEIGHT>(a.z * s, a.w * s, hi.y, lo.y);
    x3_split2<WEIGHT>(b.x * s, b.y * s, hi.z, lo.z);
    x3_split2<WEIGHT>(b.z * s, b.w * s, hi.w, lo.w);
}

__device__ __forceinline__ float4 x3_relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }
// Two fp32 masks that differ only where the mask is NaN -- keep them two.  x3_mask4 keeps v where m > 0: a NaN mask drops (the ReLU backward fused
// into staging, the output masks of the row layers).  x3_outmask4 zeroes v where m <= 0: a NaN mask keeps (aten::threshold_backward).
__device__ __forceinline__ float4 x3_mask4(float4 v, float4 m)
{
    return make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
}
__device__ __forceinline__ float4 x3_outmask4(float4 v, float4 m)
{
    return make_float4(m.x <= 0.f ? 0.f : v.x, m.y <= 0.f ? 0.f : v.y, m.z <= 0.f ? 0.f : v.z, m.w <= 0.f ? 0.f : v.w);
}
