// svx_unit.h -- the arithmetic of one unit-norm database row (populate_index, svecalign/postprocess/prep_index.py:153-185),
// shared by k_unit_rows (svx_margin.hip) and the alignment-row gather (svx_alignrows.hip) so that both write the same bits.
//
// Lane map of a row of d elements (d a multiple of 32, at most 1024): lane l owns the 8 elements
// [512 t + 8 l, 512 t + 8 l + 8), t = 0, 1, ... while they are inside the row.  A lane adds the squares of its elements
// to `ss` in element order, t ascending; the 64 partial sums are combined by wave_sum; every element is scaled by
// unit_scale(sum) -- one multiplication -- and rounded to fp16 / bf16 by pack_pair.
#pragma once
#include "svx_knn.h"

// ss + the squares of 8 consecutive elements, in order.  The fused multiply-add is spelled out: left to the compiler,
// `ss += a * a` came out as a mix of v_fma and v_pk_mul + v_add that differs from one kernel to the next, and two
// kernels that must agree bit for bit on any input cannot leave a rounding to instruction selection.
__device__ __forceinline__ float unit_sumsq8(float ss, const float* a) {
#pragma unroll
    for (int j = 0; j < 8; j++) ss = __builtin_fmaf(a[j], a[j], ss);
    return ss;
}

// 1 / |row| from the wave's sum of squares; a zero row stays zero
__device__ __forceinline__ float unit_scale(float ss) { return ss > 0.f ? 1.0f / sqrtf(ss) : 0.f; }

// 8 consecutive elements scaled and rounded to storage: one 16-byte piece of the unit row
__device__ __forceinline__ uint4 unit_pack8(const float* a, float inv, bool bf) {
    uint4 v;
    v.x = pack_pair(a[0] * inv, a[1] * inv, bf);
    v.y = pack_pair(a[2] * inv, a[3] * inv, bf);
    v.z = pack_pair(a[4] * inv, a[5] * inv, bf);
    v.w = pack_pair(a[6] * inv, a[7] * inv, bf);
    return v;
}
