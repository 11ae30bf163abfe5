// conv_packed.hip.h -- what the packed-channel convolution kernels share: conv_f16_kernel (conv_f16.hip.h, layout C8),
// conv_i8_kernel (conv_i8.hip.h, C16) and conv_s3_kernel (conv_bf16x3.hip.h, C8x3).
//
// All three store an activation as 16-byte PIECES -- one pixel x one channel group (x one of the three bf16 planes in
// C8x3) -- which is one lane's operand of the matrix instruction, and in pieces they are one design: a workgroup of 4
// waves = 64 output channels x (4*WR rows) x (32*WC columns); the reduction runs over chunks of CKG channel groups whose
// halo tile and weight slab arrive by global_load_lds_dwordx4 in an LDS ring; the kernel is persistent and prefetches
// across tiles.  Here, once: the tile geometry, the tile reference and its decode, the host-side slab packer, and the
// table of tile variants the launchers instantiate.
//
// What is NOT here, on purpose: the staging plan and its issue loop, the accumulator start from the bias row, the
// multiply loops and the fp32-planes epilogue still stand in each kernel.  Each was moved into a function of this header
// and changed the machine code of some instance; the two that changed least (issue loop, bias start: one instruction a
// slot or two away in 29 f16 / i8 instances) were timed layer by layer against the parent and did not stay inside its
// spread (NOTES.md, "The packed-channel conv kernels' ...").  A function is simplified on its own before it is inlined,
// and the result is not what the same text gives inside the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <vector>
#include "conv_mfma.hip.h"

namespace spvo {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- geometry, in 16-byte pieces
// PLANES: planes per channel group (1; 3 in C8x3).  BIAS_P_: pieces of the fp32 bias row behind a weight slab (0: none).
template <int KS, int CKG_, int WR, int WC, int PLANES_, int BIAS_P_>
struct PackedTile {
  static constexpr int CKG = CKG_, PLANES = PLANES_;
  static constexpr int TH = 4 * WR, TW = 32 * WC, HALO = KS / 2;
  static constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
  static constexpr int IN_P = CKG * PLANES * LH * LW;            // one pixel of one plane
  static constexpr int W_P = KS * KS * CKG * PLANES * CO_TILE;   // one (tap, group, plane, co) row
  static constexpr int BIAS_P = BIAS_P_;
  static constexpr int SLAB_P = W_P + BIAS_P;                    // a chunk's weights in global memory
  static constexpr int BUF_P = IN_P + SLAB_P;                    // a chunk in LDS
  static constexpr int NIT = (BUF_P + 255) / 256;                // staging instructions per thread and chunk
};

// ---------------------------------------------------------------- tile reference
// E: the element type of the tensor and the slabs, EPP = 16 / sizeof(E) elements per piece.  The bases are typed and the
// offsets count elements, as the kernels wrote them before they shared this text: the compiler's address code is theirs.
template <class E>
struct TileRef { const E *in_base, *w_base; int x0, y0, ct, img; };

template <class T, class Args>
__device__ __forceinline__ auto decode_tile(const Args &a, int id, size_t in_plane) {
  using E = std::remove_cv_t<std::remove_pointer_t<decltype(a.in)>>;
  constexpr int EPP = 16 / sizeof(E);
  TileRef<E> t;
  const int tx = id % a.tiles_x;
  id /= a.tiles_x;
  const int ty = id % a.tiles_y;
  id /= a.tiles_y;
  t.ct = id % a.co_tiles;
  t.img = id / a.co_tiles;
  t.x0 = tx * T::TW;
  t.y0 = ty * T::TH;
  t.in_base = a.in + (((size_t)t.img * a.in_gtot + a.in_goff) * T::PLANES * in_plane + (size_t)(t.y0 + PADY - T::HALO) * a.in_wp + (t.x0 + PADX - T::HALO)) * EPP;
  t.w_base = a.wpack + (size_t)t.ct * a.n_chunks * T::SLAB_P * EPP;
  return t;
}

// ---------------------------------------------------------------- host side: the weight slabs
// OIHW weights of type S -> slabs [co_tile][chunk][tap][group][plane][co 64][EPP] of E, `split(value, E[PLANES])` giving a
// value's planes; with BIAS, 64 fp32 biases follow the rows (chunk 0; zeros elsewhere).  EPP: elements per 16-byte piece.
template <class E, int PLANES, bool BIAS, class S, class Split>
inline std::vector<E> pack_conv_slabs(const S *w, const float *bias, int cout, int cin, int ks, int ckg, Split split) {
  constexpr int EPP = 16 / sizeof(E);
  const int co_tiles = (cout + CO_TILE - 1) / CO_TILE, ck = EPP * ckg, nch = (cin + ck - 1) / ck, taps = ks * ks;   // (a last chunk that cin does not fill keeps zeros in the groups it lacks: INT8 engines, conv_i8.hip.h ODD)
  const size_t rows = (size_t)taps * ckg * PLANES * CO_TILE * EPP, slab = rows + (BIAS ? CO_TILE / 4 * EPP : 0);   // in elements
  std::vector<E> out((size_t)co_tiles * nch * slab, (E)0);
  for (int ct = 0; ct < co_tiles; ++ct)
    for (int ch = 0; ch < nch; ++ch) {
      E *s = out.data() + ((size_t)ct * nch + ch) * slab;
      for (int o = 0; o < CO_TILE; ++o) {
        const int co = ct * CO_TILE + o;
        if (co >= cout) continue;
        for (int t = 0; t < taps; ++t)
          for (int g = 0; g < ckg; ++g)
            for (int e = 0; e < EPP; ++e) {
              if (ch * ck + g * EPP + e >= cin) continue;
              E pc[PLANES];
              split(w[((size_t)co * cin + ch * ck + g * EPP + e) * taps + t], pc);
              for (int q = 0; q < PLANES; ++q) s[((((size_t)t * ckg + g) * PLANES + q) * CO_TILE + o) * EPP + e] = pc[q];
            }
        if (BIAS && ch == 0) reinterpret_cast<float *>(s + rows)[o] = bias[co];
      }
    }
  return out;
}

// ---------------------------------------------------------------- host side: the tile variants
// The tiles the launchers have kernels for (choose_variant offers these): KS x (WR, WC) x fused 2x2 pooling, each with the
// channel groups per chunk of its precision -- G3 for the 3x3 layers, G1 for the 1x1 layers, and G1N (0: none) for the 1x1
// layers whose cin G1 does not divide.
template <int KS_, int CKG_, int WR_, int WC_, bool POOL_>
struct TileVariant { static constexpr int KS = KS_, CKG = CKG_, WR = WR_, WC = WC_; static constexpr bool POOL = POOL_; };

template <int KS, int WR, int WC, bool POOL, int G3, int G1, int G1N, class F, class N>
inline int with_tile_groups(int ckg, F &f, N &none) {
  constexpr int G = KS == 3 ? G3 : G1;
  if (ckg == G) return f(TileVariant<KS, G, WR, WC, POOL>{});
  if constexpr (KS == 1 && G1N != 0) {
    if (ckg == G1N) return f(TileVariant<1, G1N, WR, WC, POOL>{});
  }
  return none();
}

// f(TileVariant<...>{}) for the variant (ks, groups per chunk, wr, wc, pool); none() where there is no such kernel
template <int G3, int G1, int G1N, class F, class N>
inline int with_tile_variant(int ks, int ckg, int wr, int wc, bool pool, F f, N none) {
  switch (ks * 1000 + wr * 100 + wc * 10 + (pool ? 1 : 0)) {
    case 3220: return with_tile_groups<3, 2, 2, false, G3, G1, G1N>(ckg, f, none);
    case 3210: return with_tile_groups<3, 2, 1, false, G3, G1, G1N>(ckg, f, none);
    case 3120: return with_tile_groups<3, 1, 2, false, G3, G1, G1N>(ckg, f, none);
    case 3110: return with_tile_groups<3, 1, 1, false, G3, G1, G1N>(ckg, f, none);
    case 3221: return with_tile_groups<3, 2, 2, true, G3, G1, G1N>(ckg, f, none);
    case 3211: return with_tile_groups<3, 2, 1, true, G3, G1, G1N>(ckg, f, none);
    case 1220: return with_tile_groups<1, 2, 2, false, G3, G1, G1N>(ckg, f, none);
    case 1120: return with_tile_groups<1, 1, 2, false, G3, G1, G1N>(ckg, f, none);
    case 1110: return with_tile_groups<1, 1, 1, false, G3, G1, G1N>(ckg, f, none);
    case 1221: return with_tile_groups<1, 2, 2, true, G3, G1, G1N>(ckg, f, none);
    case 1211: return with_tile_groups<1, 2, 1, true, G3, G1, G1N>(ckg, f, none);
    default: return none();
  }
}

}  // namespace spvo
