// fqss_mfma.h -- the split-bf16 MFMA idiom of the hot GEMMs (qgemm.hip, teacher.hip, gemm_x3.hip, attn_long.hip), written once.
//
// An fp32-grade product on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the fp32-MFMA rate): an fp32 value is cut EXACTLY into
// three bf16 pieces by truncation (24-bit mantissa = 8 + 8 + 8), pairs of pieces are packed with v_perm, the pieces are staged in LDS
// as bf16 planes, A fragments are read k-contiguous as bf16x8, B fragments of an n-contiguous plane through the transposing read
// ds_read_tr16_b64, and the partial products are issued smallest pieces first into fp32 accumulators.  Values on an 8-bit grid
// (quantizer codes) are one exact bf16 piece.  Everything here is stateless and inlined; pre-operations on the values (GroupNorm /
// PReLU prologues, scales, validity masks) stay with the callers.
// The ORDER in which independent operations are written decides the schedule the compiler emits, and these kernels are tuned
// instruction by instruction: the packers below come in the orders their callers were measured with (pair by pair / element by
// element), and a caller whose pre-operation sits between an element's load and its remainders keeps that loop and uses bf_rem /
// pack_bf4 (k_tgemm, k_tgemm2, the q-GEMM stages).  Compare the assembly before and after when touching any of it.
#pragma once
#include "fqss_dev.h"

namespace fqss {
#if defined(__HIPCC__)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- the exact three-way split
__device__ __forceinline__ float bf_trunc(float f) { return __uint_as_float(__float_as_uint(f) & 0xFFFF0000u); }
__device__ __forceinline__ unsigned short bf_bits(float f) { return (unsigned short)(__float_as_uint(f) >> 16); }

// exact 3-way split g = b1 + b2 + b3: every piece is bf16-representable (<= 8 significant bits), the remainders are exact
__device__ __forceinline__ void split3(float g, unsigned short& b1, unsigned short& b2, unsigned short& b3) {
    const float h1 = bf_trunc(g), r1 = g - h1, h2 = bf_trunc(r1), r2 = r1 - h2;
    b1 = bf_bits(h1);
    b2 = bf_bits(h2);
    b3 = bf_bits(r2);
}

// what truncation to bf16 leaves of f (exact): the next piece is its truncation
__device__ __forceinline__ float bf_rem(float f) { return f - bf_trunc(f); }

// a bf16 pair out of two fp32 words: v_perm picks their high halves (= truncation), lo into bits 0-15
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
__device__ __forceinline__ uint2 pack_bf4(const float (&x)[4]) { return make_uint2(pack_bf2(x[0], x[1]), pack_bf2(x[2], x[3])); }

// two fp32 values -> one packed bf16 pair of their heads, middles and tails (pair by pair)
__device__ __forceinline__ void split3_pack2(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
    const float ar = bf_rem(a), br = bf_rem(b);
    const float al = bf_rem(ar), bl = bf_rem(br);
    h = pack_bf2(a, b);
    m = pack_bf2(ar, br);
    l = pack_bf2(al, bl);
}
// four fp32 values -> head, middle and tail as four packed bf16 each (one 8-B LDS write per plane), element by element
struct Split3x4 { uint2 h, m, l; };
__device__ __forceinline__ Split3x4 split3_pack4(const float (&x)[4]) {
    float r1[4], r2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r1[e] = bf_rem(x[e]);
        r2[e] = bf_rem(r1[e]);
    }
    return {pack_bf4(x), pack_bf4(r1), pack_bf4(r2)};
}
// eight fp32 values -> three MFMA fragments
__device__ __forceinline__ void split3_pack8(const float (&x)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    union { bf16x8 v; uint32_t w[4]; } uh, um, ul;
#pragma unroll
    for (int q = 0; q < 4; ++q) split3_pack2(x[2 * q], x[2 * q + 1], uh.w[q], um.w[q], ul.w[q]);
    h = uh.v; m = um.v; l = ul.v;
}

// four u8 codes of one word -> four packed bf16 (exact: integers <= 255): v_cvt_f32_ubyte0..3 + two v_perm
__device__ __forceinline__ uint2 codes4_to_bf(uint32_t w) {
    const float f0 = (float)(w & 0xFFu), f1 = (float)((w >> 8) & 0xFFu), f2 = (float)((w >> 16) & 0xFFu), f3 = (float)(w >> 24);
    return make_uint2(pack_bf2(f0, f1), pack_bf2(f2, f3));
}

// ---------------------------------------------------------------- fragments
// B fragment B[k = 8 h + 0..7][n] out of an n-contiguous [k][n] plane in LDS: two transposed 4 (k) x 16 (n) block reads, rows
// kr .. kr + 3 and kr + 4 .. kr + 7.  (kr, nc): this lane's row and column of the plane (TrLane).
template <int LD>
__device__ __forceinline__ bf16x8 lds_read_tr_bf16x8(const unsigned short (*plane)[LD], int kr, int nc) {
    union { bf16x8 v; s16x4 h[2]; } u;
    u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(&plane[kr][nc]));
    u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(&plane[kr + 4][nc]));
    return u.v;
}
// lane geometry of the transposed read of a 32-column fragment: the 16-lane group gq reads a 4 (k) x 16 (n) block -- row kr() (and
// kr() + 4) of a 16-deep k-step, columns nc(n0) .. nc(n0) + 3.  (tr_lane() once per kernel, kr() / nc() where the address is formed:
// the split the kernels were scheduled with.)
struct TrLane {
    int gq, tq, tp;
    __device__ __forceinline__ int kr() const { return 8 * (gq >> 1) + tq; }
    __device__ __forceinline__ int nc(int n0) const { return n0 + 16 * (gq & 1) + 4 * tp; }      // n0: the fragment's first column
};
__device__ __forceinline__ TrLane tr_lane(int lane) {
    const int gq = lane >> 4, li = lane & 15;
    return {gq, li >> 2, li & 3};
}

// The six partial products (A piece, B piece) of weight >= 2^-16, smallest pieces first so that the large products are added last:
// l.h, h.l, m.m, m.h, h.m, h.h.  The three dropped ones (m.l, l.m, l.l) lie below 2^-24 of the product, under the fp32 rounding of the sum.
constexpr int kX3A[6] = {2, 0, 1, 1, 0, 0}, kX3B[6] = {0, 2, 1, 0, 1, 0};
__device__ __forceinline__ void x3_products(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
#pragma unroll
    for (int sp = 0; sp < 6; ++sp) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kX3A[sp]], b[kX3B[sp]], acc, 0, 0, 0);
}

// ---------------------------------------------------------------- global loads of hand-scheduled load rings
// Load rings are hand-scheduled: the compiler sinks plain loads next to their first use (draining the ring to
// vmcnt(0) every chunk), so the loads are issued through asm and retired with an explicit s_waitcnt that
// carries the stage's registers as in/out operands (every use of the data is ordered after the wait).  The waits stay beside the
// stage structs of their kernels: their operand lists are those structs.
__device__ __forceinline__ void gload16(f32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void gload16(u32x4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void gload8(u32x2& d, const void* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }

#endif  // __HIPCC__
}  // namespace fqss
