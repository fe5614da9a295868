// Classification of the samples a staging lane of the wide ring takes (disc_ring_wide_impl.hpp, stage_batch): which
// batches hold a sample the integer chain cannot take.  Nothing of the kernel is in here, so that a lab program can
// include it beside a copy of the expressions it replaced (tools/ubench/classify_lab.hip walks every float32 pattern).
//
// A batch asks two questions of its samples: is any of them not a whole number, and is any non-finite or of a magnitude
// the int32 sums cannot hold (|trunc(x)| > lim, that is |x| >= lim + 1).  Per row of two samples a lane spends
//   * v_fract_f32 of each and ONE v_or3_b32 into facc: fract(x) = x - floor(x) is +0 for a whole number (-0 at most: bit
//     31 is masked), a non-zero pattern below 1.0 for any other finite x, denormals included, and a NaN for a NaN; a finite
//     result is below 1.0 and has bit 30 clear, a NaN has it set, so the OR of the bits keeps both answers apart;
//   * ONE v_max3_f32 with |.| source modifiers into amax.  A float maximum drops a NaN operand, which is why the NaN
//     question goes through facc; an infinity stays one.
// No convert back, no mask of the sign, no compare per row: the compares are three a batch, on the accumulators.
#pragma once

#include <stdint.h>

namespace topo {

struct WideClassAcc {
    uint32_t facc = 0;  // OR of the bits of fract(x) over the lane's samples of the batch
    float amax = 0.0f;  // largest |x| among them (NaNs dropped)
};

// One row's two samples into the lane's accumulators.  (Inline assembly for the maximum: written as fmaxf the operands
// are first made canonical, an instruction each, which only matters for the NaNs that facc catches anyway.)
__device__ __forceinline__ void wide_classify_row(WideClassAcc& a, float x0, float x1) {
    const uint32_t f0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_fractf(x0));
    const uint32_t f1 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_fractf(x1));
    a.facc = a.facc | f0 | f1;
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(a.amax) : "v"(x0), "v"(x1));
}

// The lane's answers for its samples of a batch.
// wild: a NaN (bit 30 of a fractional part) or |x| >= lim + 1, infinities among them; the compare is ordered, so an amax
// that a signalling NaN turned into a NaN is false here and true by facc.
__device__ __forceinline__ bool wide_lane_wild(const WideClassAcc& a, float lim_plus_1) {
    return (a.facc & 0x40000000u) != 0 || a.amax >= lim_plus_1;
}
// frac: some sample has a fractional part (to be read only where no lane is wild)
__device__ __forceinline__ bool wide_lane_frac(const WideClassAcc& a) { return (a.facc & 0x7fffffffu) != 0; }

// The two flags of a batch from the lanes' answers: bad - the chain cannot take the batch - and frac_only - it holds
// fractional samples and no non-finite or absurd one.
__device__ __forceinline__ int wide_class_flags(bool wild, bool any_frac, int bad_bit, int frac_only_bit) {
    const bool bad = wild || any_frac;
    const bool fr = !wild && any_frac;
    return (bad ? bad_bit : 0) | (fr ? frac_only_bit : 0);
}

// ... of a wave's batch
__device__ __forceinline__ int wide_classify_batch(const WideClassAcc& a, float lim_plus_1, int bad_bit, int frac_only_bit) {
    const bool wild = __builtin_amdgcn_ballot_w64(wide_lane_wild(a, lim_plus_1)) != 0;
    const bool any_frac = __builtin_amdgcn_ballot_w64(wide_lane_frac(a)) != 0;
    return wide_class_flags(wild, any_frac, bad_bit, frac_only_bit);
}

}  // namespace topo
