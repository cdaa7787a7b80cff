// The GEMM tile table: one row per tile shape (DFU_TILES), the only source of tile facts, and
// the dispatch entries of each tile's kernels (gemm_t*.hip, gemm_p8.hip, gemm_ps.hip).
#pragma once
#ifdef __HIP__  // the kernels, for the entry macros below (plain C++ reads the table alone)
#include "gemm_kernel.h"
#endif

// X(name, TM, TN, workgroups per CU, phased, tail-split, step_us, round_us) in tile-id order:
// id = row + 1 is ABI (dfu_gemm_desc.tile, gemm_tuned.inc; Python: ops.TILES).
// phased: the phase-scheduled kernels (gemm_p8.hip, gemm_ps.hip): no split-pair A, no fp32
// atomics, no in-kernel split-K reduction.  tail-split: Tail in gemm.hip.
// step_us / round_us, the wave-quantisation cost model: a launch takes ceil(tiles * splits /
// (256 CUs * workgroups per CU)) rounds, each costing round_us (prologue fill + epilogue) +
// k-steps * step_us.  Fitted on MI355X to tools/gemm_bench.py --sweep (ViT qkv K=768 vs fc2
// K=3072 forward rows, r01).  At 2 per CU two co-resident workgroups share the MFMA pipe (step
// cost ~doubles) but hide each other's fill and epilogue.  The phased and the 64-column tiles
// are priced high: only the offline-tuned table or a tile hint selects them.
#define DFU_TILES(X)                                                                   \
  X(128x128, 128, 128, 1, false, true, 0.57, 4.8)                                      \
  X(256x128, 256, 128, 1, false, false, 0.89, 8.3)                                     \
  X(128x256, 128, 256, 1, false, false, 0.90, 7.4)                                     \
  X(256x256, 256, 256, 1, false, false, 1.41, 13.9)                                    \
  X(128x128o2, 128, 128, 2, false, true, 0.70, 6.1)                                    \
  X(128x128w4, 128, 128, 2, false, false, 0.65, 6.1) /* 4 waves */                     \
  X(256x256p8, 256, 256, 1, true, false, 3.0, 20.0)  /* K-contiguous A and B only */   \
  X(256x256ps, 256, 256, 1, true, false, 3.0, 20.0)  /* persistent */                  \
  X(192x256ps, 192, 256, 1, true, false, 3.0, 20.0)  /* persistent, K-contiguous A */  \
  X(256x64, 256, 64, 1, false, false, 3.0, 20.0)     /* 4 waves, K-contiguous B */     \
  X(128x64o2, 128, 64, 2, false, false, 3.0, 20.0)   /* 4 waves, K-contiguous B */

namespace dfu {
struct GemmArgs;
typedef void (*gemm_fn)(const GemmArgs);
// Entry.e of an fp16-operand kernel (dfu_gemm_desc.operand_type 1): the epilogue | kF16Key
constexpr int kF16Key = 64;
// Entry.e of an interleaved-pair bf16x3 kernel (dfu_gemm_desc.x3_pairs): the epilogue | kX3Key
constexpr int kX3Key = 128;
struct Entry {
  int a, b, e, tile;
  gemm_fn fn;
  int lds_bytes;
  int threads;
};
#define X(name, ...) T##name,
enum TileId { DFU_TILES(X) NTILES };
#undef X
// a tile's kernels, kTable<name>[kTable<name>N]: defined next to their instantiations
#define X(name, ...)                   \
  extern const Entry kTable##name[]; \
  extern const int kTable##name##N;
DFU_TILES(X)
#undef X
}  // namespace dfu

#define DFU_ENTRY(A, B, E, TMv, TNv, TID)                                             \
  {                                                                                   \
    A, B, E, TID, &dfu::gemm_kernel<A, B, E, TMv, TNv>, dfu::Tile<TMv, TNv>::LDS_BYTES, \
        dfu::Tile<TMv, TNv>::NT                                                       \
  }
#define DFU_ENTRY_OCC(A, B, E, TMv, TNv, OCCv, TID)                       \
  {                                                                       \
    A, B, E, TID, &dfu::gemm_kernel<A, B, E, TMv, TNv, OCCv>,             \
        dfu::Tile<TMv, TNv, OCCv>::LDS_BYTES, dfu::Tile<TMv, TNv, OCCv>::NT   \
  }
#define DFU_ENTRY_NST(A, B, E, TMv, TNv, NSTv, TID)                       \
  {                                                                       \
    A, B, E, TID, &dfu::gemm_kernel<A, B, E, TMv, TNv, 1, NSTv>,          \
        dfu::Tile<TMv, TNv, 1, NSTv>::LDS_BYTES, dfu::Tile<TMv, TNv, 1, NSTv>::NT \
  }
// 4-wave workgroups (2x2 waves of 64x64), OCCv per CU
#define DFU_ENTRY_W4(A, B, E, TMv, TNv, OCCv, TID)                              \
  {                                                                             \
    A, B, E, TID, &dfu::gemm_kernel<A, B, E, TMv, TNv, OCCv, 0, 4>,             \
        dfu::Tile<TMv, TNv, OCCv, 0, 4>::LDS_BYTES, dfu::Tile<TMv, TNv, OCCv, 0, 4>::NT \
  }
// interleaved-pair bf16x3 kernels (gemm_kernel<..., X3 = true>), keyed epilogue | kX3Key
#define DFU_ENTRY_X3(A, B, E, TMv, TNv, OCCv, NWv, TID)                                      \
  {                                                                                          \
    A, B, (E) | dfu::kX3Key, TID, &dfu::gemm_kernel<A, B, E, TMv, TNv, OCCv, 0, NWv, true>,   \
        dfu::Tile<TMv, TNv, OCCv, 0, NWv>::LDS_BYTES, dfu::Tile<TMv, TNv, OCCv, 0, NWv>::NT  \
  }
