// svx_slab.h -- the LDS-DMA slab ring of the band-cost kernel (svx_band.hip: band2_block) and of the tile sweep's cost
// phase (svx_tiles.hip: k_band_tiles, k_band_tiles_gen; svx_tiles_bwd.hip: k_band_tiles_bwd), and the small device helpers
// the cost kernels share (those also serve svx_costs.hip, svx_given.hip and band3_block).  DESIGN.md 5, 6 and 6f.  Device
// code only, gfx950 only.
//
// The ring: rows travel global -> LDS by LDS-DMA (global_load_lds_dwordx4, no VGPR stop-over, no ds_write) in 64-byte
// k-slabs = one MFMA k-step, into S stages: slab k is multiplied out of stage k % S while slabs k + 1 .. k + S - 2 are
// in flight, one workgroup barrier per slab, and the barrier does not drain the DMA queue (a counted s_waitcnt vmcnt
// waits for exactly this wave's pieces of slab k).  A stage holds NSLOT overlap layers ("slots") x ROWS rows.
//
// LDS image of a stage: row r (slot * ROWS + loc) holds its 64-byte slab as four 16-byte pieces; piece kg sits at
// 64 r + 16 (kg ^ h[(r >> 2) & 3]), h = {0, 2, 3, 1}: the 16 lanes of every ds_read_b128 service group (rows
// {0-3, 12-15} of one k-group with rows {4-11} of the next) then cover all 16 bank quads.  Every DMA lane names its own
// 16 source bytes, so the swizzle costs nothing.
//
// CONTRACT.  The stages are SEPARATE __shared__ objects, declared in the kernel (each aligned to 1024 bytes, STAGE bytes
// long) and handed to run() as individual pointers.  The compiler orders ds_reads against pending LDS-DMA writes by
// object: with the stages carved out of one array, or reached by indexing an array of stage pointers at run time, it
// puts s_waitcnt vmcnt(0) in front of every ring read -- a DMA round trip per slab, the counted wait void.  Nothing
// here indexes anything by stage number, everything inlines into the kernel, and `wave` is the caller's readfirstlane
// SGPR (everything indexed by it stays scalar).  The only barriers are the one s_barrier per slab in step(), inside the
// block-uniform k < NK test; callers order their own LDS traffic around run().
#pragma once
#include "svx_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int SLAB_BYTES = 64;     // bytes of a row per k-slab

// what a DMA lane reads when its row does not exist or its piece lies past the row's end
static __device__ const uint4 slab_zero16[4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};

__device__ __forceinline__ float cost_formula(float sumx, int p, int q, float n0, float n1) {
#pragma clang fp contract(off)
    // dp_core.pyx:259-260, evaluated in double like the generated C, stored to float
    return (float)((((2.0 * (double)p) * (double)q) * (1.0 - (double)sumx)) / ((1e-6 + (double)n0) + (double)n1));
}

// one k-slab (16 bytes per lane of A and of B) into a 16 x 16 accumulator tile
template <typename E>
__device__ __forceinline__ void mma_slab16(f32x4_t& acc, const uint4& a, const uint4& b);
template <>
__device__ __forceinline__ void mma_slab16<ElemBF16>(f32x4_t& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_slab16<ElemF16>(f32x4_t& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_slab16<ElemF32>(f32x4_t& acc, const uint4& a, const uint4& b) {
    // lane (row r, group g) holds floats 4g .. 4g+3 of the 16-float slab; MFMA j multiplies element j of every
    // lane: the four lanes of a row supply k = j, 4 + j, 8 + j, 12 + j -- A and B use the same map
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ int slab_swz(int row_in_tile) { return (0x1320 >> (4 * ((row_in_tile >> 2) & 3))) & 3; }
// a lane's MFMA fragment inside a 16-row tile of a stage: row lane & 15, k-group lane >> 4
__device__ __forceinline__ int slab_lane_off(int lane) { return (lane & 15) * SLAB_BYTES + 16 * ((lane >> 4) ^ slab_swz(lane & 15)); }

// One side of the staged block (x: source rows, y: target rows): rows org .. org + rows - 1 of every layer are wanted,
// rows outside [0, lim) do not exist.  v = [layer][lim][d] rows, nrm / inv = [layer][lim] per-row scalars (inv may be null).
struct SlabSide {
    const void* v;
    const float* nrm;
    const float* inv;
    int org, rows, lim;
};
struct SlabSlot {   // what a stage slot holds; side < 0: nothing.  shift: the slot stages rows org + shift ... of its side
    int side, layer;   // (the backward tile sweep prices the edges LEAVING its nodes: layer k, k rows further on)
    int shift = 0;
};
struct SlabPair {   // the slots an alignment type multiplies
    int x, y;
};

template <typename E, int ROWS, int NSLOT, int WAVES, int S>
struct SlabRing {
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int STAGE = NSLOT * ROWS * SLAB_BYTES;   // bytes
    static constexpr int NQ = NSLOT * ROWS / 16;              // 1-KiB DMA pieces per slab
    static constexpr int PW = NQ / WAVES;                     // ... per wave
    static constexpr int KEL = SLAB_BYTES / (int)sizeof(typename E::storage);  // elements per slab
    static constexpr int SPT = (NSLOT * ROWS + THREADS - 1) / THREADS;         // staged rows per thread
    static_assert(NQ % WAVES == 0, "DMA pieces must divide over the waves");
    static_assert(S >= 2 && S <= 5, "ring depth");
    static_assert(PW * (S - 2) <= 63, "vmcnt is a 6-bit counter");

    // a lane's DMA sources: piece q = wave + WAVES i covers rows 16 q .. 16 q + 15, lane -> (row, 16-byte piece)
    struct Src {
        const char* p[PW];
        unsigned live;
        int piece_byte, rowbytes, wave;
    };
    // a wave's units: (alignment type, 16-row x tile); every unit multiplies its x tile with the y tiles of `umask`
    template <int UPW>
    struct Units {
        int aoff[UPW], boffb[UPW], umask[UPW];
    };

    // per-row scalars of the staged rows tid, tid + THREADS, ... (needed in the caller's epilogue only: kept in
    // registers, the loads ride out the k loop; store_scalars puts them where the epilogue reads them)
    template <class SlotOf>
    static __device__ __forceinline__ void row_scalars(SlotOf slot_of, const SlabSide& sx, const SlabSide& sy, int tid, float (&nrm)[SPT],
                                                       float (&inv)[SPT]) {
#pragma unroll
        for (int i = 0; i < SPT; i++) {
            const int r = tid + i * THREADS;
            nrm[i] = 0.f;
            inv[i] = 1.f;
            const int slot = r / ROWS, loc = r % ROWS;
            const SlabSlot sl = slot_of(slot);
            if (sl.side >= 0) {
                const int side = sl.side;
                const int gi = (side ? sy.org : sx.org) + loc + sl.shift, nn = side ? sy.lim : sx.lim;
                if (loc < (side ? sy.rows : sx.rows) && gi >= 0 && gi < nn) {
                    const size_t o = (size_t)sl.layer * nn + gi;
                    nrm[i] = (side ? sy.nrm : sx.nrm)[o];
                    const float* iv = side ? sy.inv : sx.inv;
                    if (iv) inv[i] = iv[o];
                }
            }
        }
    }
    static __device__ __forceinline__ void store_scalars(float* snrm, float* sinv, int tid, const float (&nrm)[SPT], const float (&inv)[SPT]) {
#pragma unroll
        for (int i = 0; i < SPT; i++) {
            const int r = tid + i * THREADS;
            if (r < NSLOT * ROWS) {
                snrm[r] = nrm[i];
                sinv[r] = inv[i];
            }
        }
    }

    template <class SlotOf>
    static __device__ __forceinline__ void sources(SlotOf slot_of, const SlabSide& sx, const SlabSide& sy, int rowbytes, int wave, int lane,
                                                   Src& s) {
        const int piece = (lane & 3) ^ slab_swz(lane >> 2);
        s.live = 0;
        s.piece_byte = piece * 16;
        s.rowbytes = rowbytes;
        s.wave = wave;
#pragma unroll
        for (int i = 0; i < PW; i++) {
            const int q = wave + WAVES * i;
            const int r = 16 * q + (lane >> 2);
            const int slot = r / ROWS, loc = r % ROWS;
            s.p[i] = reinterpret_cast<const char*>(slab_zero16);
            const SlabSlot sl = slot_of(slot);
            if (sl.side >= 0) {
                const int side = sl.side;
                const int gi = (side ? sy.org : sx.org) + loc + sl.shift, nn = side ? sy.lim : sx.lim;
                if (loc < (side ? sy.rows : sx.rows) && gi >= 0 && gi < nn) {
                    s.p[i] = reinterpret_cast<const char*>(side ? sy.v : sx.v) + ((size_t)sl.layer * nn + gi) * rowbytes + piece * 16;
                    s.live |= 1u << i;
                }
            }
        }
    }

    // slab k of every staged row -> stage
    static __device__ __forceinline__ void issue(const Src& s, int k, char* stage) {
#pragma unroll
        for (int i = 0; i < PW; i++) {
            const char* g = s.p[i] + (size_t)k * SLAB_BYTES;
            if (!((s.live >> i) & 1u) || k * SLAB_BYTES + s.piece_byte >= s.rowbytes) g = reinterpret_cast<const char*>(slab_zero16);
            __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(stage + (s.wave + WAVES * i) * 1024), 16, 0, 0);
        }
    }

    // unit u = wave + WAVES s of `nunits` = types x XT: type u / XT, x tile u % XT.  With XT <= 2 tiles per side the
    // band touches all of a unit's tile pairs (the mask is all or nothing); the unused corner of a larger staging area
    // is masked by tmask[x tile] = bits of the y tiles that hold band cells (LDS, block-uniform).
    template <int UPW, int XT, class TypeSlots>
    static __device__ __forceinline__ void units(TypeSlots type_slots, int nunits, const int* tmask, int wave, int lane, Units<UPW>& un,
                                                 f32x4_t (&acc)[UPW][XT]) {
        const int loff = slab_lane_off(lane);
#pragma unroll
        for (int s = 0; s < UPW; s++) {
#pragma unroll
            for (int j = 0; j < XT; j++) acc[s][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            const int u = wave + WAVES * s;
            const int tl = u < nunits ? u / XT : 0, xt = u % XT;
            const SlabPair ts = type_slots(tl);
            un.aoff[s] = (ts.x * ROWS + xt * 16) * SLAB_BYTES + loff;
            un.boffb[s] = (ts.y * ROWS) * SLAB_BYTES + loff;
            un.umask[s] = u < nunits ? (XT <= 2 ? (1 << XT) - 1 : __builtin_amdgcn_readfirstlane(tmask[xt])) : 0;
        }
    }

    template <int UPW, int XT>
    static __device__ __forceinline__ void mma(const Units<UPW>& un, f32x4_t (&acc)[UPW][XT], const char* stage) {
        uint4 fa[UPW], fb[UPW][XT];
#pragma unroll
        for (int s = 0; s < UPW; s++) {
            if (un.umask[s]) {  // scalar
                fa[s] = *reinterpret_cast<const uint4*>(stage + un.aoff[s]);
#pragma unroll
                for (int j = 0; j < XT; j++)
                    if (XT <= 2 || ((un.umask[s] >> j) & 1)) fb[s][j] = *reinterpret_cast<const uint4*>(stage + un.boffb[s] + j * 16 * SLAB_BYTES);
            }
        }
#pragma unroll
        for (int s = 0; s < UPW; s++) {
            if (un.umask[s]) {
#pragma unroll
                for (int j = 0; j < XT; j++)
                    if (XT <= 2 || ((un.umask[s] >> j) & 1)) mma_slab16<E>(acc[s][j], fa[s], fb[s][j]);
            }
        }
    }

    // wait until at most `younger` (<= N) slabs' pieces of this wave are pending: only rungs a depth can reach are emitted
    template <int N>
    static __device__ __forceinline__ void wait_younger(int younger) {
        if constexpr (N == 0) {
            wait_vm<0>();
        } else {
            if (younger >= N) wait_vm<N * PW>();
            else wait_younger<N - 1>(younger);
        }
    }

    template <int UPW, int XT>
    static __device__ __forceinline__ void step(int k, int NK, const Src& src, const Units<UPW>& un, f32x4_t (&acc)[UPW][XT], const char* rd,
                                                char* wr) {
        if (k < NK) {
            const int younger = (NK - 1 - k) < (S - 2) ? (NK - 1 - k) : (S - 2);  // slabs issued after slab k
            wait_younger<S - 2>(younger);
            __builtin_amdgcn_s_barrier();   // every wave's pieces of slab k have landed; stage (k-1) % S is free
            asm volatile("" ::: "memory");
            if (k + S - 1 < NK) issue(src, k + S - 1, wr);
            mma<UPW, XT>(un, acc, rd);
        }
    }

    // the k loop over NK slabs; st0 .. st(S-1) are the caller's stage objects (the rest are not touched)
    template <int UPW, int XT>
    static __device__ __forceinline__ void run(int NK, const Src& src, const Units<UPW>& un, f32x4_t (&acc)[UPW][XT], char* st0, char* st1,
                                               char* st2, char* st3, char* st4) {
        if (0 < NK) issue(src, 0, st0);
        if (S >= 3 && 1 < NK) issue(src, 1, st1);
        if (S >= 4 && 2 < NK) issue(src, 2, st2);
        if (S >= 5 && 3 < NK) issue(src, 3, st3);
        for (int k0 = 0; k0 < NK; k0 += S) {
            if constexpr (S == 2) {
                step<UPW, XT>(k0, NK, src, un, acc, st0, st1);
                step<UPW, XT>(k0 + 1, NK, src, un, acc, st1, st0);
            } else if constexpr (S == 3) {
                step<UPW, XT>(k0, NK, src, un, acc, st0, st2);
                step<UPW, XT>(k0 + 1, NK, src, un, acc, st1, st0);
                step<UPW, XT>(k0 + 2, NK, src, un, acc, st2, st1);
            } else if constexpr (S == 4) {
                step<UPW, XT>(k0, NK, src, un, acc, st0, st3);
                step<UPW, XT>(k0 + 1, NK, src, un, acc, st1, st0);
                step<UPW, XT>(k0 + 2, NK, src, un, acc, st2, st1);
                step<UPW, XT>(k0 + 3, NK, src, un, acc, st3, st2);
            } else {
                step<UPW, XT>(k0, NK, src, un, acc, st0, st4);
                step<UPW, XT>(k0 + 1, NK, src, un, acc, st1, st0);
                step<UPW, XT>(k0 + 2, NK, src, un, acc, st2, st1);
                step<UPW, XT>(k0 + 3, NK, src, un, acc, st3, st2);
                step<UPW, XT>(k0 + 4, NK, src, un, acc, st4, st3);
            }
        }
    }
};
