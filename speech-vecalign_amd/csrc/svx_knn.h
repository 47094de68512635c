// svx_knn.h -- device helpers shared by the fused GEMM + top-k kernels (svx_margin.hip: k_knn_mean, svx_search.hip:
// k_knn_search): database tile fetch by LDS-DMA, the MFMA step, query element loads, 16-lane DPP reductions.
#pragma once
#include "svx_common.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

#define KNN_DT 32       // database rows per LDS tile
#define KNN_KSTEPS 32   // 32-element k-steps held in registers (d <= 1024)
#define KNN_KMAX 64
#define KNN_SPAD 33
// LDS row stride of a database tile: always the full 1024 elements + 16 B (conflict-free b128 reads); for
// d < 1024 the columns past d are cleared once and stay zero, so the MFMA loop needs no bounds test.
#define KNN_RS (KNN_KSTEPS * 64 + 16)

__device__ __forceinline__ uint32_t pack_pair(float a, float b, bool bf) {
    if (bf) {
        uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
        ua = (ua + 0x7fffu + ((ua >> 16) & 1u)) >> 16;
        ub = (ub + 0x7fffu + ((ub >> 16) & 1u)) >> 16;
        return ua | (ub << 16);
    }
    const uint16_t ha = __builtin_bit_cast(uint16_t, (_Float16)a), hb = __builtin_bit_cast(uint16_t, (_Float16)b);
    return (uint32_t)ha | ((uint32_t)hb << 16);
}

// 8 consecutive elements of a query row, widened to fp32.
template <typename QE>
__device__ __forceinline__ void load8(const typename QE::storage* p, float* f) {
    if (QE::VEC == 4) {
        load_piece<QE>(p, f);
        load_piece<QE>(p + 4, f + 4);
    } else {
        load_piece<QE>(p, f);
    }
}

template <bool BF>
__device__ __forceinline__ void mma16(f32x4_t& acc, const uint4& a, const uint4& b) {
    if (BF)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    else
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ const uint4 knn_zero16 = {0u, 0u, 0u, 0u};

// One 1-KiB piece of a database tile, global -> LDS with no register stop-over (global_load_lds_dwordx4:
// every lane names its own 16 source bytes, the wave's 64 pieces land back to back at a wave-uniform LDS
// address).  Piece i of wave w is half (i & 1) of tile row w * KNN_DT / NW + (i >> 1).  Rows past the end of
// the database are read from its last row and masked out at the top-k update; lanes past the row's d elements
// copy zeros, so the LDS columns past d are always zero and the MFMA loop needs no bounds test.
template <int NW>
__device__ __forceinline__ void knn_fetch_piece(const uint16_t* __restrict__ db, long t, long N, int d, char* buf, int w, int lane, int i) {
    const int r = w * (KNN_DT / NW) + (i >> 1), h = i & 1;
    long gr = t * KNN_DT + r;
    gr = gr < N ? gr : N - 1;
    const char* src = reinterpret_cast<const char*>(db + gr * (long)d) + h * 1024 + lane * 16;
    if (h * 1024 + lane * 16 >= 2 * d) src = reinterpret_cast<const char*>(&knn_zero16);
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(buf + r * KNN_RS + h * 1024), 16, 0, 0);
}

// min over the 16 lanes that share lane >> 4, result in all of them (DPP row rotations)
__device__ __forceinline__ float row16_min(float v) {
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false)));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
    return v;
}
