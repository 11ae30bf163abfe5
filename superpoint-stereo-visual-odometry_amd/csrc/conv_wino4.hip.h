// conv_wino4.hip.h -- K2x: 3x3 convolution by the Winograd minimal-filtering algorithm F(4x4, 3x3) on the gfx950 fp32 matrix
// cores, bias + ReLU (+ 2x2 max-pool) fused.  fp32 throughout: operands, products and accumulation.
//
// Replaces, like the other conv_*.hip.h, the TensorRT engine the reference enqueues at
// feature_detection_neural_network.cpp:169 for the 3x3 Conv/Relu/MaxPool nodes of the SuperPoint graphs.
//
// Y(4x4) = A^T [ (G g G^T) .* (B^T d B) ] A per 6x6 input patch d (patches overlap by 2) and 3x3 filter g, interpolation
// points {0, +-1, +-2, inf}:
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// 36 multiplies per 4x4 outputs and channel pair instead of 144: 1/4 of the direct method's matrix work, 9/16 of
// F(2x2, 3x3)'s (conv_wino2.hip.h).  The price is numerical: the transforms amplify rounding (coefficients up to 8 instead
// of 1); on this network's tensors the error against a float64 evaluation is 0.4 - 2.7 x the direct kernel's (measured per
// tensor at 360x1176, 376x1240 and 192x640 by tests/test_gpu_network.py::test_winograd_layers_stay_at_fp32_rounding_level, bar
// 4 x + 2e-7: worst tensor 2.5e-6 of its maximum against 0.9e-6 direct and 0.5e-6 for F(2x2)), 40 x inside the 1e-4 bar
// against the oracle.
//
// Structure = conv_wino2.hip.h's (8 waves, two per SIMD, LDS-DMA staging, input transform of the next item between the matrix
// instructions of the current one, one barrier per item) with these differences:
//   * workgroup tile = 64 output channels x 32 Winograd tiles (4 x 8 tiles = 16 rows x 32 columns of output); wave (cq, tb) owns
//     16 channels x 16 tiles x all 36 positions on v_mfma_f32_16x16x4_f32: 144 accumulator registers;
//   * item = (tile, chunk of FOUR input channels): one matrix instruction per position and item; filters U [pos/4 9][cq 4]
//     [lane 64][4] and transformed input V [h 2][q/4 5][tb 2][lane 64][4] in LDS, both read by ds_read_b128 (nine + ten reads per item).
//     The matrix instructions run in the order p' = 18 h + 3 i + c of the positions (i, j = 3 h + c): the half h of the columns
//     that one transforming thread produces is contiguous, so its eighteen stores carry compile-time offsets.  (The 4-byte
//     stores hit every fourth bank -- SQ_LDS_BANK_CONFLICT: 40 % of the LDS cycles -- but pieces of 3 positions + 1 pad written
//     by conflict-free 16-byte stores and read by twelve instead of ten instructions measured 1-2 % SLOWER: stores are the one
//     thing that is nearly free beside an fp32 matrix instruction, reads are not);
//   * the input transform of an item is 128 patches of 6 x 6: TWO threads per patch, rows {0,1,2} / {3,4,5} for the row pass,
//     nine v_permlane32_swap exchanges, columns {0,1,2} / {3,4,5} for the column pass (the partner sits 32 lanes away, so the
//     swap leaves "rows 0-2" and "rows 3-5" in the same registers of both halves: no selects); waves 0-3 transform the even
//     items, waves 4-7 the odd ones, each transform in two halves in two consecutive items (rows + row pass two items ahead,
//     exchange + column pass + stores one item ahead; 18 registers carry it across the barrier), so that in every item BOTH
//     waves of a SIMD do half a transform;
//   * a wave's issue priority falls as it advances through an item (WINO4_PRIO below), so that the two waves of a SIMD reach the
//     item's barrier together;
//   * the matrix stream of an item waits only for the operand piece it is about to use: the operand reads (and the transform's three row
//     reads) are issued by inline assembly and waited for by s_waitcnt lgkmcnt(N) with N counted at compile time (ITEM = 1, see
//     WINO4_ITEM_LEAD below); the compiler's own placement drained the LDS queue six times per item.  Measured on one MI355X, same
//     box, old item against new: conv1b 403 -> 390 us inside the benchmark, matrix stream 3425 -> 3317 cycles per item
//     (profiles/wino4_item_*); ITEM = 2 also issues the item's LDS-DMA from a scalar base and a lane offset, and ITEM = 3, the default, cuts
//     the item's scalar and no-result instructions (both below);
//   * the inverse transform (36 -> 16 per output channel and tile) runs in registers, as before.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include <vector>
#include "conv_mfma.hip.h"

#ifndef WINO4_LEAD      // tuning (tools/wino_bench.hip): operand reads LEAD slots ahead; transform step s in slot XF_START + s * XF_STRIDE
#define WINO4_LEAD 6
#endif
// The input transform of an item is done in two halves, in two consecutive items, by the same waves: H1 (steps 0..5: the patch rows
// from the raw tile, row pass) two items ahead, H2 (steps 6..9: exchange, column pass, stores into V) one item ahead.  In every item one
// group of waves does H1 of item k + 2 and the other H2 of item k + 1: the same extra work for both waves of a SIMD.  (With a whole
// transform per item by alternating groups, the transforming wave's matrix stream took 3900 cycles and the other's 2630, which then
// waited 1300 cycles at the barrier while the transforming wave ran alone: tools/wino_bench -DWINO_STAMPS -DWINO_STAMPS_ROLES.)
// A wave's issue priority falls as it advances through an item (s_setprio 3, 2, 1, 0 at slots 0, 9, 18, 27): of the two waves of a SIMD
// the one that is BEHIND wins the matrix pipe.  Without it the older wave of each SIMD (waves 0-3) wins every arbitration, finishes
// its item ~1000 cycles ahead and stands at the barrier while the younger one runs on alone with every stall of its own exposed
// (stamps by wave, tools/wino_bench -DWINO_STAMPS: barrier wait 1180 / 180 cycles per item -> 560 / 200).  0: off; 2..4: other
// schedules that measured no better.
#ifndef WINO4_PRIO
#define WINO4_PRIO 1
#endif
#ifndef WINO4_H1_STEPS
#define WINO4_H1_STEPS 6   // steps of the first half (6: up to the row pass; 7: + the exchange -- no better)
#endif
#ifndef WINO4_H1_START
#define WINO4_H1_START 3
#endif
#ifndef WINO4_H1_STRIDE
#define WINO4_H1_STRIDE 5
#endif
#ifndef WINO4_H2_START
#define WINO4_H2_START 4
#endif
#ifndef WINO4_H2_STRIDE
#define WINO4_H2_STRIDE 8
#endif
// The item with counted operand waits (template parameter ITEM = 1; 0 = the item as it was, for A/B runs and the bit-for-bit test:
// spvo_set_tuning "wino4_item").  Same matrix instructions, same order, same operands.  What differs is how a wave waits for its operand
// reads.  In the ITEM = 0 form the compiler places the waits, and because the transform steps (with LDS operations of their own) sit in
// wave-uniform branches it falls back to s_waitcnt lgkmcnt(0) at the joins: six full drains per item, each of which also waits for the
// reads issued one or two matrix instructions earlier, the very latency LEAD was meant to cover.  In the ITEM = 1 form the operand reads
// are ds_read_b128 / ds_read_b64 in inline assembly, which the compiler's wait insertion does not see, and before the matrix instruction
// that first uses a piece stands s_waitcnt lgkmcnt(N) with N = the number of operand reads issued, in program order, behind the later of the
// two pieces it needs (wino4_wait_count below).  LDS operations return in order, so every LDS operation the transform adds in between
// only makes the true number outstanding larger than N: the wait errs on the safe side.  The compiler's own waits (for the transform's
// reads) count only what it tracks and are for the same reason never too loose.  The half-used B pieces (4 and 9: positions 16 and
// 17) are read as 8 bytes, so that no read's destination overlaps an older read's; the role predicate is scalar arithmetic.
//
// ITEM = 2 is ITEM = 1 with its LDS-DMA issued as global_load_lds_dwordx4 vOff, s[base:base+1]: the scalar 64-bit base of the
// chunk / tile, advanced by scalar adds (also from one of the five filter pieces to the next: 8192 bytes do not fit the immediate), and the
// thread's 32-bit lane offset, which never changes (glds16_sv, conv_mfma.hip.h).  fp32 matrix and vector instructions share the issue, and
// ITEM = 1 has a 64-bit vector add (v_lshl_add_u64) in front of each of the item's seven loads, which computes an address and no result.
// Nothing else differs.  The loads remain the compiler's builtin: it still counts vmcnt for them and still writes M0 in front of each.
// WAIT RULE, unchanged: the kernel waits for its LDS-DMA only by the explicit s_waitcnt vmcnt(0) at every item's start and in front of the
// epilogue; nothing else may rely on staged data.  Measured, same box, items alternating in one process: conv1b 379 -> 367 us, matrix
// stream 3313 -> 3225 cycles per item.  (The other address arithmetic of the item -- LDS addresses of the buffers k & 1, the copies that
// assemble packed operands in the transform -- was taken out too, measured step by step, and put back: NOTES.md, "F(4x4) item: LDS-DMA
// from a scalar base".)
#ifndef WINO4_ITEM_LEAD
#define WINO4_ITEM_LEAD 6
#endif
//
// ITEM = 3 is ITEM = 2 with the instructions of the item that compute no value of the result cut down, in steps that can be switched one by one
// (WINO4_ITEM3_STEPS, a mask; measurement builds of tools/wino_bench.hip instantiate ITEM = 16 + mask to time each step on top of the ones before):
//    1  the two 64-bit DMA bases (filter slab of the filter cursor, raw tile of the raw cursor) are RUNNING pointers: one scalar add when the
//       cursor steps to the next chunk, a fresh base when it steps to the next tile, instead of base + chunk * stride (64-bit multiplies) in
//       every item; the five filter pieces chain their base (+ 8192 each) through one register pair; the LDS side (M0) is a scalar that
//       swaps between the two buffers by one subtraction per item.  glds16_sv's form of the load is kept (wino4_glds16_run): the builtin,
//       so the compiler owns M0 and counts vmcnt, and the WAIT RULE above holds word for word;
//    2  the role test launders ONE scalar in place (no copy in front of every s_cmp), and that scalar flips by one s_xor per item;
//    4  the counted operand wait has its pieces as INPUTS only: read -> wait is ordered by data dependence, wait -> matrix instruction by the
//       order of volatile statements and the scheduling barrier around every matrix instruction.  (As in / out operands the wait counted as a
//       writer of the matrix instruction's sources and the hazard recogniser put an s_nop behind each of the 14.)  tools/wino4_wait_check.py
//       checks on the listing that no instruction touches a pending read's destination;
//    8  LDS addresses are kept, not rebuilt: wave group g = (wave >> TB) & 1 does H1 exactly in the items with k & 1 == g and H2 in the others, so
//       the raw tile it reads and the V buffer it writes are ALWAYS buffer g -- two addresses computed once; the two operand bases swap
//       between their buffers by one vector subtraction each per item (base = sum of the two - base);
//   16  the row pass of H1 is written out, one v_fma_f32 / v_fmamk_f32 / v_add_f32 / v_sub_f32 per operation of wino4_in6, so that the compiler
//       cannot pair them into v_pk_fma_f32 (dearer beside matrix instructions than the two it replaces) and assemble the pairs with moves.
// Same matrix instructions, same order, same operands, same transform arithmetic: the same bits as items 0 - 2.  One body, as before.
// A wave executes 200 / 211 instructions per item (first-half / second-half role) instead of 258 / 268 (tools/wino4_wait_check.py counts them).
// Measured, same box, items alternating in one process: conv1b 366 -> 356 us, the other layers -4.9 .. -6.6 %, matrix stream 3225 -> 3097 cycles
// per item, barrier 396 -> 335 (profiles/wino4_item3_*; NOTES.md, "F(4x4) item: scalar and no-result instructions cut", has every step by itself:
// the scalar steps are worth 0 - 1 %, steps 8 and 16 the rest).
#ifndef WINO4_ITEM3_STEPS
#define WINO4_ITEM3_STEPS 31
#endif
#ifndef WINO4_ABL
#define WINO4_ABL 0  // measurement builds only (tools/wino_bench.hip): 1 no input transform, 2 no filter staging, 4 no raw staging, 8 operands read once, 16 no stores
#endif

#ifndef SPVO_STATIC_BANDS
#define SPVO_STATIC_BANDS 1   // measurement builds: 0 = tile = blockIdx.x in launches without a.sched
#endif

namespace spvo {

// TB = tile blocks of 16 Winograd tiles (2 x 8 tiles = 8 rows x 32 columns of output) a workgroup covers: 2 = the 8-wave form (16 x 32
// outputs), 1 = the 4-wave form (8 x 32 outputs, one wave per SIMD) for layers whose 16 x 32 tiles would leave half the CUs without a
// workgroup (conv4a / conv4b: 45 x 147 = 15 tiles per image and 64 output channels).  Same filter slabs, same per-wave work.
template <int TB>
struct Wino4TileT {
  static constexpr int CK = 4, TH = 8 * TB, TW = 32, LW = TW + 8, LH = TH + 2, NT = 16 * TB, NTH = 256 * TB;
  static constexpr int IN_FLOATS = CK * LH * LW;        // 2880 (1600): raw halo tile of one chunk, row = x0-4 .. x0+35
  static constexpr int U_FLOATS = 36 * CK * CO_TILE;    // 9216: one filter slab
  static constexpr int V_FLOATS = 10 * TB * 64 * 4;     // 5120 (2560): transformed input of one chunk, per column half 18 positions in 5 pieces of four
  static constexpr int RAW_OFF = 0, U_OFF = 2 * IN_FLOATS, V_OFF = U_OFF + 2 * U_FLOATS;
  static constexpr int LDS_BYTES = (V_OFF + 2 * V_FLOATS) * 4 + 16;   // 137 744 (107 024) (+ the slot through which a tile's successor is published)
};
using Wino4Tile = Wino4TileT<2>;

// OIHW weights + bias -> slabs [co_tile][chunk][p'/4 9][cq 4][lane 64][4] of U = G g G^T (double), then [co_tiles * 64] biases.
// p' = 18 (j / 3) + 3 i + j % 3 (the kernel's instruction order); lane = 16 (ci & 3) + (co & 15): the A operand of
// v_mfma_f32_16x16x4_f32 (row co & 15, k = ci).
inline std::vector<float> pack_conv_weights_wino4(const float *w, const float *bias, int cout, int cin) {
  constexpr int CK = Wino4Tile::CK;
  const int co_tiles = (cout + CO_TILE - 1) / CO_TILE, nch = cin / CK;
  std::vector<float> out((size_t)co_tiles * nch * Wino4Tile::U_FLOATS + (size_t)co_tiles * CO_TILE, 0.f);
  static const double G[6][3] = {{0.25, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
  for (int ct = 0; ct < co_tiles; ++ct)
    for (int o = 0; o < CO_TILE; ++o) {
      const int co = ct * CO_TILE + o;
      if (co >= cout) continue;
      out[(size_t)co_tiles * nch * Wino4Tile::U_FLOATS + co] = bias[co];
      for (int ci = 0; ci < cin; ++ci) {
        const float *g = w + ((size_t)co * cin + ci) * 9;
        double t[6][3];
        for (int a = 0; a < 6; ++a)
          for (int k = 0; k < 3; ++k) t[a][k] = G[a][0] * g[0 * 3 + k] + G[a][1] * g[1 * 3 + k] + G[a][2] * g[2 * 3 + k];
        float *slab = out.data() + ((size_t)ct * nch + ci / CK) * Wino4Tile::U_FLOATS;
        const int lane = 16 * (ci % CK) + (o & 15), cq = o >> 4;
        for (int a = 0; a < 6; ++a)
          for (int b = 0; b < 6; ++b) {
            const int pos = 18 * (b / 3) + 3 * a + b % 3;
            slab[(((pos >> 2) * 4 + cq) * 64 + lane) * 4 + (pos & 3)] = (float)(t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2]);
          }
      }
    }
  return out;
}

// 1-D transforms.  in6: B^T x (12 operations), out4: A^T m (10 operations).
__device__ __forceinline__ void wino4_in6(const float x0, const float x1, const float x2, const float x3, const float x4, const float x5, float (&o)[6]) {
  const float e = fmaf(-4.f, x2, x4), od = fmaf(-4.f, x1, x3), e2 = x4 - x2, o2 = x3 - x1;
  o[0] = fmaf(4.f, x0, fmaf(-5.f, x2, x4));
  o[1] = e + od;
  o[2] = e - od;
  o[3] = fmaf(2.f, o2, e2);
  o[4] = fmaf(-2.f, o2, e2);
  o[5] = fmaf(4.f, x1, fmaf(-5.f, x3, x5));
}
__device__ __forceinline__ void wino4_out4(const float m0, const float m1, const float m2, const float m3, const float m4, const float m5, float (&y)[4]) {
  const float a = m1 + m2, b = m1 - m2, c = m3 + m4, d = m3 - m4;
  y[0] = (m0 + a) + c;
  y[1] = fmaf(2.f, d, b);
  y[2] = fmaf(4.f, c, a);
  y[3] = fmaf(8.f, d, b) + m5;
}

// in6 with one instruction per operation (ITEM = 3, step 16): the same twelve operations in the same association, so the same bits.  ONE
// statement: between two asm statements of which the second reads what the first wrote, the hazard recogniser puts an s_nop.
__device__ __forceinline__ void wino4_in6_written_out(const float x0, const float x1, const float x2, const float x3, const float x4, const float x5, float (&o)[6]) {
  float t, u;
  asm("v_fma_f32 %6, -4.0, %10, %12\n\t"          // e  = -4 x2 + x4
      "v_fma_f32 %7, -4.0, %9, %11\n\t"           // od = -4 x1 + x3
      "v_fmamk_f32 %0, %10, 0xc0a00000, %12\n\t"  // -5 x2 + x4
      "v_fmamk_f32 %5, %11, 0xc0a00000, %13\n\t"  // -5 x3 + x5
      "v_add_f32 %1, %6, %7\n\t"
      "v_sub_f32 %2, %6, %7\n\t"
      "v_sub_f32 %6, %12, %10\n\t"                // e2 = x4 - x2
      "v_sub_f32 %7, %11, %9\n\t"                 // o2 = x3 - x1
      "v_fma_f32 %0, 4.0, %8, %0\n\t"
      "v_fma_f32 %5, 4.0, %9, %5\n\t"
      "v_fma_f32 %3, 2.0, %7, %6\n\t"
      "v_fma_f32 %4, -2.0, %7, %6"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(t), "=&v"(u)
      : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "v"(x4), "v"(x5));
}

// glds16_sv (conv_mfma.hip.h) on a RUNNING base (ITEM = 3, step 1).  The caller launders the base IN PLACE (wino4_opaque_base: the next `base += step`
// then works on the same register pair; laundering a copy costs a 64-bit move per piece) and outside any lane-dependent branch (a scalar changed
// under one would have to become a vector value); the lane offset is laundered here, in the block of the load.
__device__ __forceinline__ void wino4_opaque_base(const char *&uniform_base) { asm volatile("" : "+s"(uniform_base)); }
__device__ __forceinline__ void wino4_glds16_run(const char *opaque_uniform_base, unsigned &lane_off, float *lds_wave_base) {
  asm volatile("" : "+v"(lane_off));
  glds16(reinterpret_cast<const float *>(opaque_uniform_base + lane_off), lds_wave_base);
}

// the same on two output channels at once (v_pk_add_f32 / v_pk_fma_f32: the epilogue has no matrix instructions to hide behind)
typedef float wino4_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wino4_out4(const wino4_f32x2 m0, const wino4_f32x2 m1, const wino4_f32x2 m2, const wino4_f32x2 m3, const wino4_f32x2 m4,
                                           const wino4_f32x2 m5, wino4_f32x2 (&y)[4]) {
  const wino4_f32x2 a = m1 + m2, b = m1 - m2, c = m3 + m4, d = m3 - m4;
  y[0] = (m0 + a) + c;
  y[1] = __builtin_elementwise_fma(wino4_f32x2{2.f, 2.f}, d, b);
  y[2] = __builtin_elementwise_fma(wino4_f32x2{4.f, 4.f}, c, a);
  y[3] = __builtin_elementwise_fma(wino4_f32x2{8.f, 8.f}, d, b) + m5;
}

// ---- operand reads of an item in program order (ITEM = 1): the matrix instructions run p = 0 .. 35; slot q holds the read of A piece q / 4
// when q % 4 == 0, then the read of B piece wino4_b_piece(q) when q is that piece's first position.  Slots 0 .. LEAD - 1 are issued in
// front of the item, slot p + LEAD behind matrix instruction p.
constexpr int wino4_b_piece(int p) { return 5 * (p / 18) + ((p % 18) >> 2); }
constexpr bool wino4_slot_reads_a(int q) { return (q & 3) == 0; }
constexpr bool wino4_slot_reads_b(int q) { return q == 0 || wino4_b_piece(q) != wino4_b_piece(q - 1); }
constexpr int wino4_reads_before(int q_end) {   // reads in slots 0 .. q_end - 1
  int n = 0;
  for (int q = 0; q < q_end && q < 36; ++q) n += (wino4_slot_reads_a(q) ? 1 : 0) + (wino4_slot_reads_b(q) ? 1 : 0);
  return n;
}
constexpr int wino4_first_slot_b(int piece) { return 18 * (piece / 5) + 4 * (piece % 5); }
// operand reads that may still be in flight when matrix instruction p starts: those issued behind the later of its two pieces
constexpr int wino4_wait_count(int p, int lead) {
  const int issued = wino4_reads_before(p + lead);
  const int qa = p & ~3, qb = wino4_first_slot_b(wino4_b_piece(p));
  const int ia = wino4_reads_before(qa);                                          // index of the A piece's read
  const int ib = wino4_reads_before(qb) + (wino4_slot_reads_a(qb) ? 1 : 0);       // index of the B piece's read (behind the slot's A read)
  const int n = issued - 1 - (ia > ib ? ia : ib);
  return n < 0 ? 0 : (n > 15 ? 15 : n);                                           // lgkmcnt is a 4-bit field
}
template <class F, int... P>
__device__ __forceinline__ void wino4_for_each(F &&f, std::integer_sequence<int, P...>) { (f(std::integral_constant<int, P>{}), ...); }

template <bool POOL, bool RELU, int TAG = 0, int TB = 2, int ITEM = 3>
__global__ __launch_bounds__(256 * TB, TB) void conv_wino4_kernel(const ConvArgs a) {
  using T = Wino4TileT<TB>;
  constexpr int CK = T::CK, LW = T::LW, LH = T::LH, LW4 = LW / 4, NTH = T::NTH;
  constexpr int IN_V4 = T::IN_FLOATS / 4;        // 720 (400) 16-byte pieces per raw tile
  constexpr int U_V4 = T::U_FLOATS / 4;          // 2304 per filter slab
  constexpr bool NEW_ITEM = ITEM != 0 && !(WINO4_ABL & 8);   // (the read-once ablation exists in the earlier item only)
  constexpr int STEPS = !NEW_ITEM ? 0 : ITEM == 3 ? (WINO4_ITEM3_STEPS) : ITEM >= 16 ? ITEM - 16 : 0;   // ITEM = 3's steps (mask: see WINO4_ITEM3_STEPS)
  constexpr bool S_PTR = (STEPS & 1) != 0, S_ROLE = (STEPS & 2) != 0, S_WAIT = (STEPS & 4) != 0, S_LDS = (STEPS & 8) != 0, S_ROW = (STEPS & 16) != 0;
  constexpr bool DMA_SV = ITEM >= 2;             // LDS-DMA from a scalar base
  constexpr int NIT_U = (U_V4 + NTH - 1) / NTH;  // 5, the last one by threads 0..255 (9, all full)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef float f32x4v __attribute__((ext_vector_type(4)));

  extern __shared__ __attribute__((aligned(16))) float smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int c16 = lane & 15, g4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cq = wave & 3, tb = wave >> 2;
  const size_t in_plane = (size_t)a.in_hp * a.in_wp;
  const size_t out_plane = (size_t)a.out_hp * a.out_wp;
  const int n_tiles = a.tiles_x * a.tiles_y * a.co_tiles * a.batch;

  struct TileRef { const float *in_base, *w_base; int x0, y0, ct, img; };
  auto decode = [&](int id) {
    TileRef t;
    const int tx = id % a.tiles_x;
    id /= a.tiles_x;
    const int ty = id % a.tiles_y;
    id /= a.tiles_y;
    t.ct = id % a.co_tiles;
    t.img = id / a.co_tiles;
    t.x0 = tx * T::TW;
    t.y0 = ty * T::TH;
    t.in_base = a.in + ((size_t)t.img * a.in_ctot + a.in_coff) * in_plane + (size_t)(t.y0 + PADY - 1) * a.in_wp + (t.x0 + PADX - 4);
    t.w_base = a.wpack + (size_t)t.ct * a.n_chunks * T::U_FLOATS;
    return t;
  };

  // ---- staging plans (wave-uniform 64-bit base + 32-bit lane offset).  Raw tile: pieces 0..511 by every thread, pieces
  // 512..719 by threads 256.. (waves 4-7, which carry one filter piece less: six LDS-DMA instructions per wave and item everywhere);
  // 4-wave form: pieces 0..255 by every thread, 256..399 by threads 0..143
  auto raw_piece_off = [&](int idx) {
    idx = min(idx, IN_V4 - 1);
    const int ci = idx / (LH * LW4);
    const int rem = idx - ci * (LH * LW4);
    const int r = rem / LW4;
    const int q = rem - r * LW4;
    return 4u * (unsigned)(ci * (int)in_plane + r * a.in_wp + q * 4);
  };
  constexpr int R0 = NTH - 256;   // first thread that carries a second raw piece
  unsigned roff0 = raw_piece_off(tid), roff1 = raw_piece_off(NTH + (tid - R0));   // (not const: ITEM = 2 passes them through glds16_sv)
  const bool raw2 = tid >= R0 && NTH + (tid - R0) < IN_V4;
  auto issue_raw = [&](const TileRef &t, int chunk, float *buf) {
    const char *inb = reinterpret_cast<const char *>(t.in_base + (size_t)chunk * CK * in_plane);
    glds16(reinterpret_cast<const float *>(inb + roff0), buf + (wave * 64) * 4);
    if (raw2) glds16(reinterpret_cast<const float *>(inb + roff1), buf + (NTH + (wave - R0 / 64) * 64) * 4);
  };
  unsigned uoff = 16u * (unsigned)tid;
  auto issue_u = [&](const TileRef &t, int chunk, float *buf) {
    const char *wb = reinterpret_cast<const char *>(t.w_base + (size_t)chunk * T::U_FLOATS);
#pragma unroll
    for (int it = 0; it < NIT_U; ++it)
      if (it < NIT_U - 1 || tid < U_V4 - (NIT_U - 1) * NTH) glds16(reinterpret_cast<const float *>(wb + (uoff + 16u * NTH * it)), buf + (it * NTH + wave * 64) * 4);
  };
  // ITEM = 2: the same pieces as "scalar base + lane offset" (glds16_sv), no vector instruction for an address.  A filter piece advances
  // the scalar base: its 8192-byte step fits neither the instruction's immediate nor, without a vector add, the lane offset.
  auto issue_raw2 = [&](const TileRef &t, int chunk, float *buf) {
    const char *inb = reinterpret_cast<const char *>(t.in_base + (size_t)chunk * CK * in_plane);
    glds16_sv(inb, roff0, buf + (wave * 64) * 4);
    if (raw2) glds16_sv(inb, roff1, buf + (NTH + (wave - R0 / 64) * 64) * 4);
  };
  auto issue_u2 = [&](const TileRef &t, int chunk, float *buf) {
    const char *wb = reinterpret_cast<const char *>(t.w_base + (size_t)chunk * T::U_FLOATS);
#pragma unroll
    for (int it = 0; it < NIT_U; ++it)
      if (it < NIT_U - 1 || tid < U_V4 - (NIT_U - 1) * NTH) glds16_sv(wb + (size_t)16 * NTH * it, uoff, buf + (it * NTH + wave * 64) * 4);
  };
  // ITEM = 3, step 1: the same pieces from running bases (wp3: the filter cursor's slab, rp3: the raw cursor's tile and chunk; advance3 below) into
  // `lds` = LDS address of (buffer, this wave's 1 KiB), which swaps between the two buffers once per item
  // (The filter base walks through the slab's pieces and is left at the LAST piece; advance3 adds what is missing to the next slab, U_TAIL3.  The
  // last piece is carried by whole waves, so its test is scalar.)
  const char *wp3 = nullptr, *rp3 = nullptr;
  constexpr int U_TAIL3 = T::U_FLOATS * 4 - (NIT_U - 1) * 16 * NTH, U_LAST_WAVES3 = (U_V4 - (NIT_U - 1) * NTH) / 64;
  static_assert((U_V4 - (NIT_U - 1) * NTH) % 64 == 0, "the last filter piece by whole waves");
  auto lds_ptr3 = [](unsigned lds) { return (float *)(__attribute__((address_space(3))) float *)(uintptr_t)lds; };
  auto issue_raw3 = [&](unsigned lds) {
    wino4_opaque_base(rp3);
    wino4_glds16_run(rp3, roff0, lds_ptr3(lds));
    if (raw2) wino4_glds16_run(rp3, roff1, lds_ptr3(lds + (NTH - R0) * 16));
  };
  auto issue_u3 = [&](unsigned lds) {
#pragma unroll
    for (int it = 0; it < NIT_U; ++it) {
      if (it) wp3 += 16 * NTH;
      wino4_opaque_base(wp3);
      if (it < NIT_U - 1 || wave < U_LAST_WAVES3) wino4_glds16_run(wp3, uoff, lds_ptr3(lds + it * NTH * 16));
    }
  };

  // ---- input transform: two threads per patch.  u = tid & 255: input channel = u >> 6 (= wave & 3), tile = lane & 31 (tile row
  // tile >> 3, tile column tile & 7), half h = lane >> 5 (patch rows 3 h .. 3 h + 2 in the row pass, columns 3 h .. in the column pass)
  // (4-wave form: 64 patches = two waves; input channel = 2 (wave & 1) + bit 4 of the lane, tile = lane & 15)
  const int x_ci = TB == 2 ? (wave & 3) : 2 * (wave & 1) + ((lane >> 4) & 1), x_tile = TB == 2 ? (lane & 31) : (lane & 15), x_h = lane >> 5;
  const int x_trow = x_tile >> 3, x_tcol = x_tile & 7;
  const int raw_off = x_ci * (LH * LW) + (4 * x_trow + 3 * x_h) * LW + 4 * x_tcol + 3;   // LDS row 0 = output row y0 - 1, LDS column 4 = output column x0
  // V[h][q / 4][tb][lane = 16 ci + (tile & 15)][q & 3], q = 3 i + c: this thread writes (h, i = 0..5, c = 0..2)
  const int v_off = x_h * (1280 * TB) + (x_tile >> 4) * 256 + (16 * x_ci + (x_tile & 15)) * 4;   // + (q >> 2) * 256 TB + (q & 3) floats
  // Steps of one patch half: 0..2 read row r (b32, b128, b32 = columns 3, 4 .. 7, 8 of the halo row), 3..5 row pass of row r,
  // 6 the exchange, 7..9 column pass of column c + stores
  float xr[3][6];        // rows after the row pass; xr[r][0..2] stay, xr[r][3..5] are swapped with the partner's
  f32x4v xa[3];
  float xs0[3], xs1[3];
  f32x2 xs2[3];          // (ITEM = 1, inside an item: xs0 and xs1 of a row as they come from one ds_read2_b32)
  auto xf_step = [&](const float *raw, float *vb, int st) {
    if (st < 3) {
      const float *d = raw + raw_off + st * LW;
      xs0[st] = d[0];
      xa[st] = *reinterpret_cast<const f32x4v *>(d + 1);
      xs1[st] = d[5];
    } else if (st < 6) {
      const int r = st - 3;
      wino4_in6(xs0[r], xa[r][0], xa[r][1], xa[r][2], xa[r][3], xs1[r], xr[r]);
    } else if (st == 6) {
      // h = 0 keeps columns 0-2 and needs the partner's rows 3-5 of them; h = 1 keeps columns 3-5 and needs rows 0-2.  One swap per
      // value: v0 = the value in column c, v1 = the value in column c + 3; lanes 32-63 of v0 <-> lanes 0-31 of v1.  Afterwards, in
      // BOTH halves, v0 holds rows 0-2 and v1 rows 3-5 of the thread's own three columns.
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
          const u32x2s sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(xr[r][c]), __float_as_uint(xr[r][c + 3]), false, false);
          xr[r][c] = __uint_as_float(sw[0]);
          xr[r][c + 3] = __uint_as_float(sw[1]);
        }
    } else {
      const int c = st - 7;
      float o[6];
      wino4_in6(xr[0][c], xr[1][c], xr[2][c], xr[0][c + 3], xr[1][c + 3], xr[2][c + 3], o);
#pragma unroll
      for (int i = 0; i < 6; ++i) vb[v_off + ((3 * i + c) >> 2) * (256 * TB) + ((3 * i + c) & 3)] = o[i];
    }
  };

  const int a_lane = cq * 64 + lane;   // 16-byte pieces in a filter slab: + (pos / 4) * 256
  const int b_lane = tb * 64 + lane;   // 16-byte pieces in a V buffer:     + (5 h + q / 4) * 64 TB

  // ---- tile assignment: conv_wino2.hip.h's XCD-banded counters (a.sched), or blockIdx.x + k gridDim.x
  const int band = blockIdx.x & 7;
  auto wgs_before = [&](int b) { return min(b, (int)gridDim.x & 7) + b * ((int)gridDim.x >> 3); };
  auto band_lo = [&](int b) { return (int)((long)n_tiles * wgs_before(b) / (int)gridDim.x); };
  auto band_hi = [&](int b) { return band_lo(b + 1); };
  auto band_wgs = [&](int b) { return wgs_before(b + 1) - wgs_before(b); };
  auto steal = [&]() {
    for (int k = 1; k < 8; ++k) {
      const int b = (band + k) & 7;
      if (band_lo(b) + band_wgs(b) >= band_hi(b)) continue;
      const int v = band_lo(b) + band_wgs(b) + atomicAdd(a.sched + b, 1);
      if (v < band_hi(b)) return v;
    }
    return n_tiles;
  };
  auto all_done = [&]() {
    if (a.sched && tid == 0 && atomicAdd(a.sched + 8, 1) == (int)gridDim.x - 1)
      for (int k = 0; k < 9; ++k) a.sched[k] = 0;
  };
  int *const sched_slot = reinterpret_cast<int *>(smem + (T::LDS_BYTES - 16) / 4);
  // static assignment (a.sched == nullptr: single-round launches, short K loops): the same XCD bands without the counters -- workgroup
  // blockIdx.x takes tile (workgroups of lower bands) + (its rank in its band), a permutation of 0 .. gridDim.x - 1, then + k gridDim.x.
  // With tile = blockIdx.x neighbouring tiles sat on different XCDs and every L2 fetched its own copy of the halos and of the lines
  // tiles share: conv3a / conv3b / conv4a / conv4b / convPa+Da moved 2.8 - 6 x their algorithmic bytes (profiles/r04_pmc_layers.json)
  int tile_id = SPVO_STATIC_BANDS ? wgs_before(band) + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
  if (a.sched) {
    tile_id = band_lo(band) + (blockIdx.x >> 3);
    if (tile_id >= band_hi(band)) {
      if (tid == 0) *sched_slot = steal();
      __syncthreads();
      tile_id = *sched_slot;
      __syncthreads();
    }
  }
  if (tile_id >= n_tiles) {
    all_done();
    return;
  }
  TileRef cur = decode(tile_id);

  // prefetch cursors over the item sequence: filters one item ahead, raw tiles two items ahead
  int nxt_id = tile_id + gridDim.x;
  int dyn_fetch = 0;
  struct Cursor { TileRef t; int chunk, id; };
  auto advance = [&](Cursor &q) {
    if (++q.chunk == a.n_chunks) {
      asm volatile("" ::: "memory");   // a real branch, taken once per tile
      q.chunk = 0;
      q.id = a.sched ? nxt_id : q.id + (int)gridDim.x;
      if (q.id < n_tiles) q.t = decode(q.id);
    }
  };
  // ITEM = 3, step 1: advance() that also moves the cursor's DMA base `p`: by `step` bytes to the next chunk, or to the new tile's base
  // (the add comes first and unconditionally, the rare tile step overwrites it: advance()'s control flow, no second join)
  auto advance3 = [&](Cursor &q, const char *&p, long step, bool filters) {
    p += step;
    if (++q.chunk == a.n_chunks) {
      asm volatile("" ::: "memory");   // a real branch, taken once per tile
      q.chunk = 0;
      q.id = a.sched ? nxt_id : q.id + (int)gridDim.x;
      if (q.id < n_tiles) {
        q.t = decode(q.id);
        p = filters ? reinterpret_cast<const char *>(q.t.w_base) : reinterpret_cast<const char *>(q.t.in_base);
      }
    }
  };
  Cursor cu{cur, 0, tile_id};
  issue_raw(cu.t, 0, smem + T::RAW_OFF);
  issue_u(cu.t, 0, smem + T::U_OFF);
  advance(cu);                                   // item 1
  if (cu.id < n_tiles) issue_raw(cu.t, cu.chunk, smem + T::RAW_OFF + T::IN_FLOATS);
  Cursor cr = cu;
  advance(cr);                                   // item 2
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  if (wave < 2 * TB) {                           // item 0's transform has nothing to hide behind ...
#pragma unroll
    for (int st = 0; st < 10; ++st) xf_step(smem + T::RAW_OFF, smem + T::V_OFF, st);
  } else {                                       // ... nor has the first half of item 1's (the other group: its second half follows in item 0)
#pragma unroll
    for (int st = 0; st < WINO4_H1_STEPS; ++st) xf_step(smem + T::RAW_OFF + T::IN_FLOATS, smem + T::V_OFF + T::V_FLOATS, st);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // raw tile 0 is read: item 2's goes there (first half of its transform: in item 0)
  if (cr.id < n_tiles) issue_raw(cr.t, cr.chunk, smem + T::RAW_OFF);
  advance(cr);                                   // item 3

#ifdef WINO_STAMPS   // diagnostic build (tools/wino_bench.hip): shader-clock cycles per wave waiting for LDS-DMA / stores at an item's start (o[7]: of
                     // which in a tile's SECOND item, the first wait behind an epilogue's stores), at the barrier, in the matrix stream, in epilogues
  unsigned long long st_dma = 0, st_bar = 0, st_mfma = 0, st_epi = 0, st_items = 0, st_post = 0, st_bar_xf = 0, st_mfma_xf = 0;   // _xf: in the items in which this wave does the transform's first half
  const unsigned long long st_t0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
  int st_c = 0;
#endif
  int k = 0;                    // items done: selects the buffers and the transforming half
  bool drained = false;         // the LDS-DMA this item needs has been waited for already
  constexpr unsigned OOB = 0xFFFFFFFFu;

  // ITEM = 3: what an item takes from k, kept as running values instead (each moves by one instruction per item; values here: item 0)
  auto lds_addr = [](const void *p) { return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)p; };
  const int grp3 = (wave >> TB) & 1;
  int xf3 = grp3 ^ 1;                                                        // step 2: the role scalar (H1 of item k + 2 when != 0)
  unsigned lds_u3 = lds_addr(smem + T::U_OFF + T::U_FLOATS + wave * 256);    // step 1: where the DMA of filters (k + 1) ...
  unsigned lds_raw3 = lds_addr(smem + T::RAW_OFF + T::IN_FLOATS + wave * 256);   //     ... and of raw tile (k + 3) go: buffer (k + 1) & 1, this wave's first KiB (LDS address)
  const unsigned lds_u_swap3 = 2 * lds_u3 - T::U_FLOATS * 4, lds_raw_swap3 = 2 * lds_raw3 - T::IN_FLOATS * 4;   // (sum of the two buffers' addresses)
  unsigned ua3 = lds_addr(reinterpret_cast<const f32x4v *>(smem + T::U_OFF) + a_lane);   // step 8: operand bases in buffer k & 1 ...
  unsigned va3 = lds_addr(reinterpret_cast<const f32x4v *>(smem + T::V_OFF) + b_lane);
  unsigned ua_swap3 = 2 * ua3 + T::U_FLOATS * 4, va_swap3 = 2 * va3 + T::V_FLOATS * 4;   //         ... swapped by base = (sum of the two) - base
  unsigned ra3 = lds_addr(smem + T::RAW_OFF + grp3 * T::IN_FLOATS + raw_off);            //         H1's rows: always raw buffer grp3
  unsigned vst3 = lds_addr(smem + T::V_OFF + grp3 * T::V_FLOATS + v_off);                //         H2's stores: always V buffer grp3
  if constexpr (S_LDS) asm volatile("" : "+v"(ua3), "+v"(va3), "+v"(ra3), "+v"(vst3), "+v"(ua_swap3), "+v"(va_swap3));   // (kept in registers: never rebuilt inside the loop)
  auto xf_store3 = [&](int c) {   // xf_step's steps 7 + c (column pass of column c, stores) through the kept address
    float o[6];
    wino4_in6(xr[0][c], xr[1][c], xr[2][c], xr[0][c + 3], xr[1][c + 3], xr[2][c + 3], o);
    float __attribute__((address_space(3))) *vp = (float __attribute__((address_space(3))) *)(uintptr_t)vst3;
#pragma unroll
    for (int i = 0; i < 6; ++i) vp[((3 * i + c) >> 2) * (256 * TB) + ((3 * i + c) & 3)] = o[i];
  };
  if constexpr (S_PTR) {
    wp3 = reinterpret_cast<const char *>(cu.t.w_base + (size_t)cu.chunk * T::U_FLOATS);
    rp3 = reinterpret_cast<const char *>(cr.t.in_base + (size_t)cr.chunk * CK * in_plane);
  }
  const long raw_step3 = (long)(CK * in_plane * 4);

  while (tile_id < n_tiles) {
    if (a.sched) {
      if (tid == 0) dyn_fetch = band_lo(band) + band_wgs(band) + atomicAdd(a.sched + band, 1);
    } else {
      nxt_id = tile_id + gridDim.x;
    }

    // acc[pos]: position pos = 6 i + j of this wave's 16 tiles; register r = output channel 16 cq + 4 g4 + r, lane c16 = tile
    f32x4v acc[36];
    auto item = [&](auto first_tag, bool publish) {
      constexpr bool FIRST = decltype(first_tag)::value;   // the tile's first chunk: C = 0 in every accumulator's (only) instruction
      // group k & 1 (waves 0-3 / 4-7) does the first half of item k + 2's transform, the other group the second half of item k + 1's
      // (wave-uniform: a scalar branch per step)
      // (ITEM = 1: from the two scalars, so that the per-step branches are s_cmp / s_cbranch_scc without vector instructions)
      const bool XF = NEW_ITEM ? (((wave >> TB) ^ k) & 1) == 0 : __builtin_amdgcn_readfirstlane((wave >> TB) == (k & 1) ? 1 : 0) != 0;
#ifdef WINO_STAMPS
      const unsigned long long ts0 = __builtin_amdgcn_s_memtime();
#endif
      if (!drained) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      drained = false;
#ifdef WINO_STAMPS
      const unsigned long long ts1 = __builtin_amdgcn_s_memtime();
#endif
      if (publish && tid == 0) *sched_slot = dyn_fetch < band_hi(band) ? dyn_fetch : n_tiles;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (publish) nxt_id = __builtin_amdgcn_readfirstlane(*sched_slot);
#ifdef WINO_STAMPS
      const unsigned long long ts2 = __builtin_amdgcn_s_memtime();
      st_dma += ts1 - ts0; st_bar += ts2 - ts1;
      if (st_c == 1) st_post += ts1 - ts0;
      if (XF) st_bar_xf += ts2 - ts1;
#endif
      const float *ub = smem + T::U_OFF + (k & 1) * T::U_FLOATS;
      const float *vb = smem + T::V_OFF + (k & 1) * T::V_FLOATS;
      float *u_next = smem + T::U_OFF + ((k + 1) & 1) * T::U_FLOATS;
      const float *raw_next2 = smem + T::RAW_OFF + (k & 1) * T::IN_FLOATS;    // raw(k+2): landed before this item, read by H1 now
      float *raw_next3 = smem + T::RAW_OFF + ((k + 1) & 1) * T::IN_FLOATS;    // raw(k+3) replaces raw(k+1), whose H1 ran during item k-1
      float *v_next = smem + T::V_OFF + ((k + 1) & 1) * T::V_FLOATS;
      const f32x4v *ub4 = reinterpret_cast<const f32x4v *>(ub) + a_lane;
      const f32x4v *vb4 = reinterpret_cast<const f32x4v *>(vb) + b_lane;
      // 36 matrix instructions in the order p' = 18 h + q (q = 3 i + c; position 6 i + 3 h + c); operands: A piece p' / 4 (9 reads),
      // B piece 5 h + q / 4 (10 reads), each read LEAD instructions before its first use
      if constexpr (NEW_ITEM) {
        // operand reads the compiler does not track + counted waits (see WINO4_ITEM_LEAD above); B pieces 4 and 9 as 8 bytes in bh[h]
        constexpr int LEAD = WINO4_ITEM_LEAD;
        static_assert(LEAD >= 1 && LEAD <= 36, "WINO4_ITEM_LEAD");
        static_assert(WINO4_PRIO <= 1, "the other priority schedules exist in the ITEM = 0 form only");
        f32x4v av[9], bv[10];
        f32x2 bh[2];
        static_assert(WINO4_H1_STEPS >= 6, "the row reads and the row pass that waits for them run in one item");
        // the role as a scalar, compared afresh at every step: s_cmp + s_cbranch_scc, no lane mask kept in a register pair and no vector
        // instructions (the empty asm keeps the compiler from merging the comparisons into such a mask)
        const int xf_s = ((wave >> TB) ^ k ^ 1) & 1;
        // (ITEM = 3, step 2: the running scalar itself is laundered, in place -- a copy of xf_s costs an s_mov_b32 in front of every comparison)
        auto is_xf = [xf_s, &xf3]() __attribute__((always_inline)) {
          if constexpr (S_ROLE) { asm volatile("" : "+s"(xf3)); return xf3 != 0; }
          else { int t = xf_s; asm volatile("" : "+s"(t)); return t != 0; }
        };
        const unsigned ra = S_LDS ? ra3 : (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)(raw_next2 + raw_off);
        const unsigned ua = S_LDS ? ua3 : (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)ub4;
        const unsigned va = S_LDS ? va3 : (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)vb4;
        auto read_slot = [&av, &bv, &bh, ua, va](auto qc) __attribute__((always_inline)) {
          constexpr int q = decltype(qc)::value;
          if constexpr (q < 36 && wino4_slot_reads_a(q)) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(av[q >> 2]) : "v"(ua), "n"((q >> 2) * 256 * 16));
          constexpr int j = wino4_b_piece(q < 36 ? q : 35);
          if constexpr (q < 36 && wino4_slot_reads_b(q) && j % 5 == 4) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(bh[j / 5]) : "v"(va), "n"(j * 64 * TB * 16));
          if constexpr (q < 36 && wino4_slot_reads_b(q) && j % 5 != 4) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bv[j]) : "v"(va), "n"(j * 64 * TB * 16));
        };
        auto step = [&](auto pc) __attribute__((always_inline)) {
          constexpr int p = decltype(pc)::value;
          constexpr int ph = p / 18, pq = p % 18, pos = 6 * (pq / 3) + 3 * ph + pq % 3, bj = wino4_b_piece(p);
          constexpr bool half = bj % 5 == 4;
          // the first use of a piece: wait for it (the asm's operands tie the wait between the reads and the matrix instruction)
          // (ITEM = 3, step 4: the pieces as inputs only and a scheduling barrier behind the wait -- see WINO4_ITEM3_STEPS)
          constexpr bool waits_here = wino4_slot_reads_a(p) || wino4_slot_reads_b(p);
          auto set_prio = []() __attribute__((always_inline)) {
#if WINO4_PRIO
            if constexpr (p == 0) asm volatile("s_setprio 3");
            if constexpr (p == 9) asm volatile("s_setprio 2");
            if constexpr (p == 18) asm volatile("s_setprio 1");
            if constexpr (p == 27) asm volatile("s_setprio 0");
#endif
          };
          if constexpr (S_WAIT && waits_here) {
            set_prio();   // (in front of the wait: behind it, the scheduling barrier would leave it behind the matrix instruction)
            if constexpr (half) asm volatile("s_waitcnt lgkmcnt(%2)" : : "v"(av[p >> 2]), "v"(bh[bj / 5]), "n"(wino4_wait_count(p, LEAD)));
            else asm volatile("s_waitcnt lgkmcnt(%2)" : : "v"(av[p >> 2]), "v"(bv[bj]), "n"(wino4_wait_count(p, LEAD)));
            __builtin_amdgcn_sched_barrier(0);
          } else if constexpr (waits_here) {
            if constexpr (half) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(av[p >> 2]), "+v"(bh[bj / 5]) : "n"(wino4_wait_count(p, LEAD)));
            else asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(av[p >> 2]), "+v"(bv[bj]) : "n"(wino4_wait_count(p, LEAD)));
          }
          const float a_op = av[p >> 2][p & 3];
          float b_op;
          if constexpr (half) b_op = bh[bj / 5][pq & 3];
          else b_op = bv[bj][pq & 3];
          if constexpr (!(S_WAIT && waits_here)) set_prio();
          if (FIRST) acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_op, b_op, f32x4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          else acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_op, b_op, acc[pos], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (!(WINO4_ABL & 2) && p == 1 && cu.id < n_tiles) {
            if constexpr (S_PTR) issue_u3(lds_u3);
            else if constexpr (DMA_SV) issue_u2(cu.t, cu.chunk, u_next);
            else issue_u(cu.t, cu.chunk, u_next);
          }
          if (!(WINO4_ABL & 4) && p == 4 && cr.id < n_tiles) {
            if constexpr (S_PTR) issue_raw3(lds_raw3);
            else if constexpr (DMA_SV) issue_raw2(cr.t, cr.chunk, raw_next3);
            else issue_raw(cr.t, cr.chunk, raw_next3);
          }
          read_slot(std::integral_constant<int, p + LEAD>{});
          // the transform: H1 of item k + 2 (its three row reads the same way: issued untracked in steps 0..2, waited for by count in front
          // of the row pass of steps 3..5) or H2 of item k + 1
          constexpr bool h1_slot = !(WINO4_ABL & 1) && p >= WINO4_H1_START && p < WINO4_H1_START + WINO4_H1_STEPS * WINO4_H1_STRIDE && (p - WINO4_H1_START) % WINO4_H1_STRIDE == 0;
          constexpr bool h2_slot = !(WINO4_ABL & 1) && p >= WINO4_H2_START && p < WINO4_H2_START + (10 - WINO4_H1_STEPS) * WINO4_H2_STRIDE && (p - WINO4_H2_START) % WINO4_H2_STRIDE == 0;
          auto h1 = [&](auto stc) __attribute__((always_inline)) {
            constexpr int st = decltype(stc)::value;
            if constexpr (st < 3) {
              asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(xs2[st]) : "v"(ra), "n"(st * LW), "n"(st * LW + 5));
              asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xa[st]) : "v"(ra), "n"((st * LW + 1) * 4));
            } else {
              if constexpr (st < 6) {
                // behind row st - 3's reads: the operand reads of the slots up to this one's, and two reads per later row
                constexpr int p_rd = p - 3 * WINO4_H1_STRIDE;
                constexpr int n = wino4_reads_before(p + LEAD + 1) - wino4_reads_before(p_rd + LEAD + 1) + 2 * (5 - st);
                asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(xs2[st - 3]), "+v"(xa[st - 3]) : "n"(n > 15 ? 15 : n));
                xs0[st - 3] = xs2[st - 3][0];
                xs1[st - 3] = xs2[st - 3][1];
              }
              if constexpr (S_ROW && st < 6) wino4_in6_written_out(xs0[st - 3], xa[st - 3][0], xa[st - 3][1], xa[st - 3][2], xa[st - 3][3], xs1[st - 3], xr[st - 3]);
              else xf_step(raw_next2, v_next, st);
            }
          };
          auto h2 = [&](auto stc) __attribute__((always_inline)) {
            constexpr int st = decltype(stc)::value;
            if constexpr (S_LDS && st >= 7) xf_store3(st - 7);
            else xf_step(raw_next2, v_next, st);
          };
          constexpr int st1 = (p - WINO4_H1_START) / WINO4_H1_STRIDE, st2 = WINO4_H1_STEPS + (p - WINO4_H2_START) / WINO4_H2_STRIDE;
          // (one test per step, also in the slot that holds a step of either half, p = 28: as if / else the join gets the values of both
          // halves as phis, and the compiler pays for them with twelve 64-bit moves per item -- built for ITEM = 3, read in the listing, taken out)
          if constexpr (h1_slot) { if (is_xf()) h1(std::integral_constant<int, st1>{}); }
          if constexpr (h2_slot) { if (!is_xf()) h2(std::integral_constant<int, st2>{}); }
          __builtin_amdgcn_sched_barrier(0);
        };
        wino4_for_each(read_slot, std::make_integer_sequence<int, LEAD>{});
        wino4_for_each(step, std::make_integer_sequence<int, 36>{});
      } else {
        constexpr int LEAD = WINO4_LEAD;
        f32x4v av[9], bv[10];
        auto b_piece = [](int p) { return 5 * (p / 18) + ((p % 18) >> 2); };
#pragma unroll
        for (int p = 0; p < ((WINO4_ABL & 8) ? 36 : LEAD); ++p) {
          if ((WINO4_ABL & 8) && k > 0) break;
          if ((p & 3) == 0) av[p >> 2] = ub4[(p >> 2) * 256];
          if (p == 0 || b_piece(p) != b_piece(p - 1)) bv[b_piece(p)] = vb4[b_piece(p) * (64 * TB)];
        }
#pragma unroll
        for (int p = 0; p < 36; ++p) {
          const int ph = p / 18, pq = p % 18, pos = 6 * (pq / 3) + 3 * ph + pq % 3;
          const float a_op = av[p >> 2][p & 3], b_op = bv[b_piece(p)][pq & 3];
#if WINO4_PRIO
#if WINO4_PRIO == 1
          if (p == 0) asm volatile("s_setprio 3");
          if (p == 9) asm volatile("s_setprio 2");
          if (p == 18) asm volatile("s_setprio 1");
          if (p == 27) asm volatile("s_setprio 0");
#elif WINO4_PRIO == 2   // the younger wave of a SIMD (tb = 1) keeps each level longer
          if (p == 0) asm volatile("s_setprio 3");
          if (tb == 0) { if (p == 6) asm volatile("s_setprio 2"); if (p == 15) asm volatile("s_setprio 1"); if (p == 24) asm volatile("s_setprio 0"); }
          else { if (p == 12) asm volatile("s_setprio 2"); if (p == 24) asm volatile("s_setprio 1"); }
#elif WINO4_PRIO == 3   // two levels only: high in the first half of the item
          if (p == 0) asm volatile("s_setprio 1");
          if (p == 18) asm volatile("s_setprio 0");
#elif WINO4_PRIO == 4   // older wave one level below the younger one throughout, both falling
          if (tb == 0) { if (p == 0) asm volatile("s_setprio 2"); if (p == 12) asm volatile("s_setprio 1"); if (p == 24) asm volatile("s_setprio 0"); }
          else { if (p == 0) asm volatile("s_setprio 3"); if (p == 12) asm volatile("s_setprio 2"); if (p == 24) asm volatile("s_setprio 1"); }
#endif
#endif
          if (FIRST) acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_op, b_op, f32x4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          else acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_op, b_op, acc[pos], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (!(WINO4_ABL & 2) && p == 1 && cu.id < n_tiles) issue_u(cu.t, cu.chunk, u_next);
          if (!(WINO4_ABL & 4) && p == 4 && cr.id < n_tiles) issue_raw(cr.t, cr.chunk, raw_next3);
          const int q = p + LEAD;
          if (!(WINO4_ABL & 8) && q < 36) {
            if ((q & 3) == 0) av[q >> 2] = ub4[(q >> 2) * 256];
            if (b_piece(q) != b_piece(q - 1)) bv[b_piece(q)] = vb4[b_piece(q) * (64 * TB)];
          }
          if (!(WINO4_ABL & 1) && XF && p >= WINO4_H1_START && p < WINO4_H1_START + WINO4_H1_STEPS * WINO4_H1_STRIDE && (p - WINO4_H1_START) % WINO4_H1_STRIDE == 0)
            xf_step(raw_next2, v_next, (p - WINO4_H1_START) / WINO4_H1_STRIDE);                          // H1 of item k + 2
          if (!(WINO4_ABL & 1) && !XF && p >= WINO4_H2_START && p < WINO4_H2_START + (10 - WINO4_H1_STEPS) * WINO4_H2_STRIDE && (p - WINO4_H2_START) % WINO4_H2_STRIDE == 0)
            xf_step(raw_next2, v_next, WINO4_H1_STEPS + (p - WINO4_H2_START) / WINO4_H2_STRIDE);        // H2 of item k + 1 (registers of this wave's H1 in the item before)
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if constexpr (S_PTR) {
        advance3(cu, wp3, U_TAIL3, true);
        advance3(cr, rp3, raw_step3, false);
        lds_u3 = lds_u_swap3 - lds_u3;
        lds_raw3 = lds_raw_swap3 - lds_raw3;
      } else {
        advance(cu);
        advance(cr);
      }
      if constexpr (S_ROLE) xf3 ^= 1;
      if constexpr (S_LDS) {
        ua3 = ua_swap3 - ua3;
        va3 = va_swap3 - va3;
      }
      ++k;
#ifdef WINO_STAMPS
      { const unsigned long long dt = __builtin_amdgcn_s_memtime() - ts2; st_mfma += dt; if (XF) st_mfma_xf += dt; }
      ++st_items; ++st_c;
#endif
    };
#ifdef WINO_STAMPS
    st_c = 0;
#endif
    item(std::true_type{}, false);
    for (int c = 1; c < a.n_chunks; ++c) item(std::false_type{}, a.sched != nullptr && c == 1);

    // everything in flight for the next item has landed before this tile's stores queue up behind it
#ifdef WINO_STAMPS
    const unsigned long long te0 = __builtin_amdgcn_s_memtime();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    drained = true;

    // ---------------------------------------------------------------- epilogue: Y = A^T M A, bias, ReLU, (pool), store
    const int co0 = cur.ct * CO_TILE + cq * 16 + 4 * g4;   // this lane's four output channels co0 .. co0 + 3
    float *co_base = a.out + (((size_t)cur.img * a.out_ctot + a.out_coff) + (size_t)cur.ct * CO_TILE + cq * 16) * out_plane;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(co_base, 0, 0x7FFFFFFF, 0x00020000);
    const int oplane = (int)out_plane;
    const int kmax = a.cout - co0;                                             // channels r < kmax of this lane's 4 exist
    const float *bias_p = a.wpack + (size_t)a.co_tiles * a.n_chunks * T::U_FLOATS + min(co0, a.cout - 1);
    const int trow = 2 * tb + (c16 >> 3), tcol = c16 & 7;
    auto relu = [](float v) { return RELU ? __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff()) : v; };
    const int oy = cur.y0 + 4 * trow, ox = cur.x0 + 4 * tcol;                  // first output pixel of this lane's tile
#pragma unroll
    for (int rp = 0; rp < 2; ++rp) {   // channels 2 rp, 2 rp + 1 of this lane's four: two per vector instruction
      typedef wino4_f32x2 f32x2;
      const f32x2 bias_v = {bias_p[2 * rp < kmax ? 2 * rp : 0], bias_p[2 * rp + 1 < kmax ? 2 * rp + 1 : 0]};
      auto pr = [&](int p) { return f32x2{acc[p][2 * rp], acc[p][2 * rp + 1]}; };
      f32x2 z[6][4];   // column pass: z[j][.] = A^T M[., j]
#pragma unroll
      for (int j = 0; j < 6; ++j) wino4_out4(pr(0 + j), pr(6 + j), pr(12 + j), pr(18 + j), pr(24 + j), pr(30 + j), z[j]);
      f32x2 y2[4][4];   // row pass: y[i][.] = A^T z[., i]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wino4_out4(z[0][i], z[1][i], z[2][i], z[3][i], z[4][i], z[5][i], y2[i]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) y2[i][jj] += bias_v;
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
      const int r = 2 * rp + e;
      float y[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) y[i][jj] = relu(y2[i][jj][e]);
      const bool ch_ok = r < kmax;
      // Stores: one 16-byte piece per tile row (8 bytes per pooled row).  A tile that straddles the right edge writes ZEROS into
      // the plane's right padding (at least PADX = 4 columns, zero by construction and read as such by the next layer's halo),
      // so that odd widths and widths that are not multiples of 4 take the same wide stores.
      if constexpr (POOL) {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const int ow = a.W >> 1;
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
          float pv[2];
#pragma unroll
          for (int pj = 0; pj < 2; ++pj)
            pv[pj] = fmaxf(fmaxf(y[2 * pi][2 * pj], y[2 * pi][2 * pj + 1]), fmaxf(y[2 * pi + 1][2 * pj], y[2 * pi + 1][2 * pj + 1]));
          const int py = (oy >> 1) + pi, px = ox >> 1;
          const unsigned vo = (ch_ok && py < (a.H >> 1) && px < ow) ? 4u * (unsigned)(4 * g4 * oplane + (py + PADY) * a.out_wp + (px + PADX)) : OOB;
          const u32x2 v = {__float_as_uint(pv[0]), __float_as_uint(px + 1 < ow ? pv[1] : 0.f)};
          __builtin_amdgcn_raw_buffer_store_b64(v, rsrc, (WINO4_ABL & 16) ? OOB : vo, r * oplane * 4, 0);
        }
      } else {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int yy = oy + i;
          const unsigned vo = (ch_ok && yy < a.H && ox < a.W) ? 4u * (unsigned)(4 * g4 * oplane + (yy + PADY) * a.out_wp + (ox + PADX)) : OOB;
          const u32x4 v = {__float_as_uint(y[i][0]), __float_as_uint(ox + 1 < a.W ? y[i][1] : 0.f), __float_as_uint(ox + 2 < a.W ? y[i][2] : 0.f),
                           __float_as_uint(ox + 3 < a.W ? y[i][3] : 0.f)};
          __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (WINO4_ABL & 16) ? OOB : vo, r * oplane * 4, 0);
        }
      }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#ifdef WINO_STAMPS
    st_epi += __builtin_amdgcn_s_memtime() - te0;
#endif
    tile_id = nxt_id;
    if (tile_id < n_tiles) cur = decode(tile_id);
  }
  all_done();   // the last workgroup out resets the counters for the next launch
#ifdef WINO_STAMPS
  if (lane == 0 && a.stamps) {
    unsigned long long *o = a.stamps + 8 * (blockIdx.x * (4 * TB) + wave);
    o[0] = st_dma; o[1] = st_bar; o[2] = st_mfma; o[3] = st_epi; o[4] = st_items;
    o[5] = __builtin_amdgcn_s_memtime() - st_t0; o[6] = __builtin_amdgcn_s_memrealtime() - st_r0; o[7] = st_post;
#ifdef WINO_STAMPS_ROLES   // o[0], o[7]: matrix stream and barrier wait (in front) of the items in which this wave did the transform's FIRST half: half of its items
    o[0] = st_mfma_xf; o[7] = st_bar_xf;
#endif
  }
#endif
}

}  // namespace spvo
