// General fp32-in / fp32-out GEMM on fp16 MFMA with the 3-product hi/lo split (see
// mlp_f16x3.hip for the numerics), for the layer-by-layer training path: the forward layers
// with their activations kept (model.py:95-120), the input-gradient products dX = dY . W and
// the weight gradients dW = dY^T . X of the reference's autograd backward (model.py:256-282).
//
//   C (M x N) = epilogue( A (M x K) . B (K x N) )
//
// Workgroup: 256 threads = 4 waves in 2 x 2, C tile 128 x 128, each wave 64 x 64 = 4 x 4
// MFMA 16x16 tiles with two fp32 accumulators (hi*hi and the 2^11-scaled cross terms: the lo
// parts stay normal in fp16 down to |x * scale| = 2^-14, so a fixed operand scale covers
// gradients over many orders of magnitude).  Per 32-deep k-step the A and B tiles are loaded
// into registers PF steps ahead (the loads fly under the MFMAs; the bias-gradient row sums read
// them only when they are published), split into fp16 hi / lo planes and stored to a
// double-buffered LDS image laid out [row][k] (k contiguous, 80-B rows), from which each lane
// reads its 8-element MFMA fragments with one ds_read_b128; one barrier per k-step.  Operands
// stored reduction-major (A as [K][M], B as [K][N]) are transposed in registers while staging
// (4 x 4 blocks), so every GEMM of the backward pass reads its operands in place.
//
// This file is the one translation unit of the GEMM: the C API, the kernel selection
// (route_of), the split policy and the batch planner.  The kernels are in the headers below,
// one per family.
#include "gemm_params.hpp"       // Params, tile / K-chunk order, split-K reduce kernels
#include "gemm_tile_f16x3.hpp"   // k_gemm_f16x3 (the kernel described above) and its batch
#include "gemm_bf16_km.hpp"      // k_gemm_bf16_km
#include "gemm_bf16_dma.hpp"     // k_gemm_bf16_dma, k_gemm_bf16_dma256 and their batches
#include "gemm_f1.hpp"           // k_gemm_f1, k_gemm_f1h_batch
#include "gemm_stream.hpp"       // k_gemm_skinny_bf16, k_gemm_segsum_bf16
#include "gemm_small.hpp"        // k_gemm_small_f32, k_gemm_small_f32_wave, k_gemm_small_batch

using namespace aon;
using namespace aon::gemm;

// ---- kernel selection: one decision per product, taken here and nowhere else ------------------
enum class Route {
  Small,    // k_gemm_small_f32(_wave): tiny exact-fp32 products
  SegSum,   // k_gemm_segsum_bf16: weight gradient against a per-ray B (b_rdiv > 1)
  Skinny,   // k_gemm_skinny_bf16: weight gradient of at most 4 rows
  F1,       // k_gemm_f1: single-accumulator 256 x 256 / 128 x 256 / 256 x 64
  Dma256,   // k_gemm_bf16_dma256: bf16 LDS-DMA, 256 x 256 tiles
  Dma128,   // k_gemm_bf16_dma: bf16 LDS-DMA, 128 x 128 tiles
  BfKm,     // k_gemm_bf16_km: bf16 MFMA, register-staged (any other mma_bf16 product)
  Generic,  // k_gemm_f16x3
};

// The first route whose conditions hold, in this order.  The split policy once tested Dma256
// and F1 ahead of SegSum and Skinny; the order does not matter for those pairs, which exclude
// each other:
//   Dma256 / SegSum: Dma256 needs b_rdiv == 1, SegSum b_rdiv > 1.
//   Dma256 / Skinny: Dma256 needs M % 256 == 0, Skinny 1 <= M <= 4.
//   F1 / SegSum:     F1 needs b_rdiv == 1 and a tiled B, SegSum b_rdiv > 1 and a row-major B.
//   F1 / Skinny:     F1 needs M of 128 or 256 and a tiled A, Skinny M <= 4 and a row-major A.
static Route route_of(const aon_gemm_args* a) {
  const int64_t b_rdiv = a->b_kc ? 1 : a->b_rdiv;
  const bool whole_store = a->n_store == 0 || a->n_store == a->N;
  // tiny fp32 products
  if (a->exact_fp32 && !a->mma_bf16 && a->M * a->N <= 65536 && a->K <= 1024 && !a->A2 &&
      !a->mask && !a->relu && !a->rowsum && !a->a_amax && !a->a_tiled && !a->b_tiled &&
      b_rdiv == 1 && !a->k_splits && whole_store)
    return Route::Small;
  // a plain fp32 weight gradient (reduction-major fp32 operands, no epilogue): the parity mode's
  // heads / per-ray columns stream in exact fp32, its 256-wide products may take k_gemm_f1
  const bool plain32 = !a->mma_bf16 && !a->a_bf16 && !a->b_bf16 && !a->a_kc && !a->b_kc && !a->A2 &&
                       !a->bias && !a->mask && !a->relu && !a->exact_fp32;
  // weight gradient against a per-ray B: the bf16 mode's, or the parity mode's in exact fp32
  if ((a->mma_bf16 || plain32) && !a->a_kc && !a->b_kc && b_rdiv > 1 && !a->b_tiled &&
      a->M % 8 == 0 && a->M >= 8 && a->M <= 256 && aligned16(a->A) && a->lda % 8 == 0 &&
      !a->k_splits && whole_store)
    return Route::SegSum;
  // weight gradient of at most 4 rows on a B of up to 256 columns: the bf16 mode's (B bf16), or
  // the parity mode's in exact fp32
  if (((a->mma_bf16 && a->b_bf16) || plain32) && a->M >= 1 && a->M <= 4 && !a->a_tiled &&
      b_rdiv == 1 && a->N % 8 == 0 && a->N <= 256 && aligned16(a->B) && a->ldb % 8 == 0 &&
      !a->k_splits && whole_store)
    return Route::Skinny;
  // the fused kernels' tiled fp32 tensors in one of k_gemm_f1's shapes, with the caller's
  // single-accumulator licence (f16_single)
  const bool f1_shape = (a->M == 256 && (a->N == 256 || a->N == 64)) || (a->M == 128 && a->N == 256);
  if (a->f16_single && plain32 && !a->c_trans && a->a_tiled && a->b_tiled && f1_shape &&
      a->lda == a->M && a->ldb == a->N && b_rdiv == 1 && aligned16(a->A) && aligned16(a->B) &&
      a->K >= 8 * 1024)
    return Route::F1;
  // both operands bf16 and reduction-major in whole 128 x 128 tiles with 16-B runs: the LDS-DMA
  // kernels, on 256 x 256 tiles when the product is whole ones
  if (a->mma_bf16 && a->a_bf16 && a->b_bf16 && a->M % BM == 0 && a->N % BN == 0 && b_rdiv == 1 &&
      aligned16(a->A) && aligned16(a->B) && a->lda % 8 == 0 && a->ldb % 8 == 0)
    return a->M % BM2 == 0 && a->N % BM2 == 0 ? Route::Dma256 : Route::Dma128;
  return a->mma_bf16 ? Route::BfKm : Route::Generic;
}

// ---- split policy: K chunks of a lone product -------------------------------------------------
static int64_t gemm_splits(const aon_gemm_args* a, Route r) {
  const auto chunk_groups = [](int64_t s) { return s >= 8 ? s / 8 * 8 : (s < 1 ? 1 : s); };
  switch (r) {
    case Route::Small:
      return 1;
    case Route::SegSum: {  // one chunk of 2048 / M rays (whole segments) per workgroup
      const int64_t rays = (a->K + a->b_rdiv - 1) / a->b_rdiv, rb = 2048 / a->M;
      return rays > 0 ? (rays + rb - 1) / rb : 1;
    }
    case Route::Skinny: {  // ~512 chunks of whole 16-row blocks (two workgroups per CU)
      const int64_t kc = ((a->K + 511) / 512 + kSkinnyRows - 1) / kSkinnyRows * kSkinnyRows;
      return a->K > 0 ? (a->K + kc - 1) / kc : 1;
    }
    case Route::F1:
    case Route::Dma256: {
      if (a->k_splits > 0) return a->k_splits;
      // one workgroup per CU: 256 K chunks of a single 256 x 256 tile (chunks of >= 1024 rows;
      // the coarse level's 266k rows still fill the chip -- 2048-row chunks left half of it idle)
      const int64_t t2 = r == Route::F1 ? 1 : (a->M / BM2) * (a->N / BM2);
      if (t2 >= 256 || a->K < 8 * 1024) return 1;
      const int64_t cap = a->K / 1024 < 256 ? a->K / 1024 : 256;
      return chunk_groups(256 / t2 < cap ? 256 / t2 : cap);
    }
    case Route::Dma128:
    case Route::BfKm:
    case Route::Generic:
      break;
  }
  // the 128 x 128-tile kernels: split the reduction only when the tile grid alone cannot fill
  // the chip and K is long
  const int64_t tiles = ((a->M + BM - 1) / BM) * ((a->N + BN - 1) / BN);
  if (a->k_splits > 0) return a->k_splits;
  if (tiles >= 512 || a->K < 8 * 1024 || a->A2) return 1;
  int64_t cap = a->K / 2048;
  if (cap > 256) cap = 256;
  // Dma128: one round of 512 workgroups: 128 splits of a 2 x 2 tile grid measured 0.196 ms
  // against 0.216 / 0.233 ms for 192 / 256 (profiles/r02/ab_gemm)
  if (r == Route::Dma128) return chunk_groups(512 / tiles < cap ? 512 / tiles : cap);
  // whole rounds of 512 workgroups (2 per CU): two rounds when K is long enough, else one --
  // a grid a few workgroups past a round runs its tail as a second, nearly empty round (a
  // 266k-row weight gradient on 544 workgroups took as long as one on 1024)
  // (split_of places chunks in groups of 8, one per XCD)
  return chunk_groups(cap * tiles >= 1024 ? 1024 / tiles : (cap < 512 / tiles ? cap : 512 / tiles));
}

// K rows per chunk (Params::kchunk) for `splits` chunks
static int64_t gemm_kchunk(const aon_gemm_args* a, Route r, int64_t splits) {
  if (r == Route::SegSum) return 2048 / a->M * a->b_rdiv;  // whole segments per workgroup
  if (splits <= 1) return a->K > 0 ? a->K : 1;
  const int64_t kround = r == Route::Skinny ? kSkinnyRows : BK;
  return ((a->K + splits - 1) / splits + kround - 1) / kround * kround;
}

// floats of one K chunk's partials: the C tile and the rowsum entries that ride along
static size_t partial_floats(const aon_gemm_args* a) {
  return (size_t)(a->M * a->N + (a->c_trans ? a->N : a->M));
}

extern "C" size_t aon_gemm_workspace_bytes(const aon_gemm_args* a) {
  if (!a) return 0;
  const int64_t s = gemm_splits(a, route_of(a));
  return s > 1 ? (size_t)s * partial_floats(a) * sizeof(float) : 0;
}

// ---- what aon_gemm and the batch launcher share: argument checks and the Params filler --------
// (`fn`: the entry point's name, as AON_REQUIRE would prefix it)
static int check_product(const char* fn, const aon_gemm_args* a) {
#define AON_GEMM_CHECK(cond, msg)                            \
  do {                                                       \
    if (!(cond)) {                                           \
      ::aon::set_error(std::string(fn) + ": " + (msg));      \
      return -1;                                             \
    }                                                        \
  } while (0)
  AON_GEMM_CHECK(a->A && a->B && a->C, "null operand");
  AON_GEMM_CHECK(a->lda >= 1 && a->ldb >= 1 &&
                     a->ldc >= (a->c_trans ? a->M : (a->n_store > 0 ? a->n_store : a->N)),
                 "bad leading dimension (c_trans: ldc >= M, C holds N rows)");
  AON_GEMM_CHECK(a->K < (int64_t(1) << 32) && (a->b_kc || a->b_rdiv < (int64_t(1) << 32)),
                 "K and b_rdiv must be below 2^32");
  AON_GEMM_CHECK(a->a_scale > 0.f && a->b_scale > 0.f, "operand scales must be positive");
  AON_GEMM_CHECK(!a->a_tiled || (!a->a_kc && a->lda == a->M && a->M % 16 == 0),
                 "a_tiled: reduction-major A of width lda = M (a multiple of 16)");
  AON_GEMM_CHECK(!a->b_tiled || (!a->b_kc && a->b_rdiv == 1 && a->ldb == a->N && a->N % 16 == 0),
                 "b_tiled: reduction-major B of width ldb = N (a multiple of 16), b_rdiv = 1");
  AON_GEMM_CHECK(a->n_store >= 0 && a->n_store <= a->N, "n_store must be in [0, N]");
#undef AON_GEMM_CHECK
  return 0;
}

// everything of Params that the arguments alone decide; the chunking, the tile grid and the
// split-K workspace are the caller's
static void fill_params(const aon_gemm_args& a, Params& p) {
  p = Params{};
  p.c_trans = a.c_trans;
  p.a_tiled = a.a_tiled;
  p.b_tiled = a.b_tiled;
  p.nstore = a.n_store > 0 ? a.n_store : a.N;
  p.M = a.M; p.N = a.N; p.K = a.K;
  p.A = a.A; p.lda = a.lda;
  p.A2 = a.A2; p.lda2 = a.A2 ? a.lda2 : 0; p.K1 = a.A2 ? a.K1 : INT64_MAX;
  p.a2_rdiv = a.A2 ? a.a2_rdiv : 1;
  p.B = a.B; p.ldb = a.ldb; p.b_rdiv = a.b_kc ? 1 : a.b_rdiv;
  p.C = a.C; p.ldc = a.ldc;
  p.bias = a.bias; p.mask = a.mask; p.ldm = a.ldm;
  p.relu = a.relu; p.accumulate = a.accumulate;
  p.sa = a.a_scale; p.sb = a.b_scale; p.inv_s = 1.0f / (a.a_scale * a.b_scale);
  p.sa_bits = a.a_amax;
  p.rowsum = a.rowsum;
}

// ---- launch helpers: the template instance for the operands' layout, type and alignment -------
template <bool AKC, bool BKC>
static void launch_generic(const Params& p, bool va, bool vb, dim3 grid, hipStream_t st) {
#define AON_F16_L(VA_, VB_) \
  hipLaunchKernelGGL((k_gemm_f16x3<AKC, BKC, VA_, VB_>), grid, dim3(THREADS), 0, st, p)
  if (va && vb) AON_F16_L(true, true);
  else if (va) AON_F16_L(true, false);
  else if (vb) AON_F16_L(false, true);
  else AON_F16_L(false, false);
#undef AON_F16_L
}

template <typename TA, typename TB>
static void launch_bf(const Params& p, bool va, bool vb, dim3 grid, hipStream_t st) {
#define AON_BF_L(VA_, VB_) \
  hipLaunchKernelGGL((k_gemm_bf16_km<TA, TB, VA_, VB_>), grid, dim3(THREADS), 0, st, p)
  if (va && vb) AON_BF_L(true, true);
  else if (va) AON_BF_L(true, false);
  else if (vb) AON_BF_L(false, true);
  else AON_BF_L(false, false);
#undef AON_BF_L
}

template <typename TA, bool BT, typename TB = __bf16>
static void launch_skinny(const Params& p, dim3 grid, hipStream_t st) {
  const dim3 block((unsigned)(2 * p.N));  // 16 row phases x N / 8 column groups
  constexpr int SK = AON_GEMM_SKINNY_SK, SK2 = AON_GEMM_SKINNY_SK2;
  const bool narrow = p.N <= 128;
  switch (p.M) {
#define AON_SKINNY_L(M_)                                                                            \
  if (narrow) hipLaunchKernelGGL((k_gemm_skinny_bf16<M_, TA, BT, SK2, TB>), grid, block, 0, st, p); \
  else hipLaunchKernelGGL((k_gemm_skinny_bf16<M_, TA, BT, SK, TB>), grid, block, 0, st, p)
    case 1: AON_SKINNY_L(1); break;
    case 2: AON_SKINNY_L(2); break;
    case 3: AON_SKINNY_L(3); break;
    default: AON_SKINNY_L(4); break;
#undef AON_SKINNY_L
  }
}

// RND: the bf16 mode (operands staged as bf16); false: the parity mode's, exact fp32
template <typename TA, typename TB, bool RND>
static void launch_segsum(const Params& p, dim3 grid, hipStream_t st) {
  if (p.a_tiled) hipLaunchKernelGGL((k_gemm_segsum_bf16<TA, TB, true, RND>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((k_gemm_segsum_bf16<TA, TB, false, RND>), grid, dim3(256), 0, st, p);
}

extern "C" int aon_gemm(const aon_gemm_args* a, void* work, size_t work_bytes,
                        aon_stream_t stream) {
  AON_REQUIRE(a, "null args");
  if (const int rc = check_product(__func__, a)) return rc;
  AON_REQUIRE(a->M >= 0 && a->N >= 0 && a->K >= 0, "bad shape");
  AON_REQUIRE(!a->A2 || (a->a_kc && a->K1 >= 0 && a->K1 <= a->K && a->lda2 >= 1 && a->a2_rdiv >= 1),
              "A2 needs a_kc, 0 <= K1 <= K, lda2 >= 1, a2_rdiv >= 1");
  AON_REQUIRE(!a->mask || a->ldm >= a->N, "bad mask leading dimension");
  AON_REQUIRE(a->b_kc || a->b_rdiv >= 1, "b_rdiv must be >= 1");
  const bool bf = a->mma_bf16 != 0;
  AON_REQUIRE(bf || (!a->a_bf16 && !a->b_bf16), "bf16 operands need mma_bf16");
  AON_REQUIRE(!bf || (!a->a_kc && !a->b_kc && !a->A2 && !a->bias && !a->mask && !a->relu &&
                      !a->a_amax),
              "mma_bf16 computes reduction-major weight gradients only (a_kc = b_kc = 0, no A2 / "
              "bias / mask / relu / a_amax)");
  const Route r = route_of(a);
  AON_REQUIRE(!a->exact_fp32 || r == Route::Small,
              "exact_fp32: tiny fp32 products only (M N <= 65536, K <= 1024, no A2 / mask / relu / "
              "rowsum / a_amax / tiled operands / k_splits / n_store)");
  AON_REQUIRE(a->n_store == 0 || a->n_store == a->N || r == Route::Dma256 || r == Route::Dma128 ||
                  (!a->mma_bf16 && !a->exact_fp32),
              "n_store < N: the bf16 LDS-DMA weight-gradient path (both operands bf16, M and N "
              "multiples of 128) or an fp32 product");
  if (a->M == 0 || a->N == 0) return 0;
  AON_REQUIRE(!a->c_trans || r == Route::Skinny, "c_trans: the skinny path only (M <= 4)");
  AON_REQUIRE(!a->rowsum || !a->a_kc, "rowsum needs a reduction-major A (a_kc = 0)");
  Params p;
  fill_params(*a, p);
  p.kchunk = gemm_kchunk(a, r, gemm_splits(a, r));
  const int64_t zs = a->K > 0 ? (a->K + p.kchunk - 1) / p.kchunk : 1;
  if (zs > 1) {
    AON_REQUIRE(work && work_bytes >= (size_t)zs * partial_floats(a) * sizeof(float),
                "split-K needs aon_gemm_workspace_bytes() of workspace");
    p.part = static_cast<float*>(work);
    p.rowsum_part = p.part + zs * a->M * a->N;
  }
  // C tile edge of the kernel that runs (k_gemm_f1: the whole product is one tile)
  const int64_t bmt = r == Route::Dma256 ? BM2 : BM;
  const int64_t tiles_m = r == Route::F1 ? 1 : (a->M + bmt - 1) / bmt;
  const int64_t tiles_n = r == Route::F1 ? 1 : (a->N + bmt - 1) / bmt;
  const int64_t gm = tiles_m < 8 ? tiles_m : 8;
  const int64_t blocks = (tiles_m + gm - 1) / gm * gm * tiles_n;
  AON_REQUIRE(blocks < (1ll << 31), "too large");
  p.tiles_m = (int)tiles_m;
  p.tiles_n = (int)tiles_n;
  p.gm = (int)gm;
  p.tblocks = (int)blocks;
  p.zsplit = (int)zs;
  // split-K: one 1-D grid, the tiles of a K chunk on one XCD (split_of)
  const int64_t gx = zs > 1 ? 8 * blocks * ((zs + 7) / 8) : blocks;
  AON_REQUIRE(gx < (1ll << 31), "too large");
  const dim3 grid((unsigned)gx, 1, 1);       // the tiled kernels
  const dim3 chunks((unsigned)zs, 1, 1);     // the streaming kernels: one workgroup per K chunk
  // float4 staging when the 4-element runs are 16-B aligned
  const bool va = aligned16(a->A) && a->lda % 4 == 0 && (!a->A2 || a->K1 % 4 == 0);
  const bool vb = aligned16(a->B) && a->ldb % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  switch (r) {
    case Route::Small:
      if (a->K <= 16)
        hipLaunchKernelGGL(k_gemm_small_f32, grid_for(a->M * a->N, 256, 1 << 20), 256, 0, st, p,
                           a->a_kc, a->b_kc);
      else
        hipLaunchKernelGGL(k_gemm_small_f32_wave, grid_for(a->M * a->N, 4, 1 << 20), 256, 0, st, p,
                           a->a_kc, a->b_kc);
      break;
    case Route::SegSum:
      if (!bf) launch_segsum<float, float, false>(p, chunks, st);
      else if (a->a_bf16 && a->b_bf16) launch_segsum<__bf16, __bf16, true>(p, chunks, st);
      else if (a->a_bf16) launch_segsum<__bf16, float, true>(p, chunks, st);
      else if (a->b_bf16) launch_segsum<float, __bf16, true>(p, chunks, st);
      else launch_segsum<float, float, true>(p, chunks, st);
      break;
    case Route::Skinny:
      if (!bf) {
        if (a->b_tiled) launch_skinny<float, true, float>(p, chunks, st);
        else launch_skinny<float, false, float>(p, chunks, st);
      } else if (a->a_bf16 && a->b_tiled) launch_skinny<__bf16, true>(p, chunks, st);
      else if (a->a_bf16) launch_skinny<__bf16, false>(p, chunks, st);
      else if (a->b_tiled) launch_skinny<float, true>(p, chunks, st);
      else launch_skinny<float, false>(p, chunks, st);
      break;
    case Route::F1:
      if (a->M == 128) hipLaunchKernelGGL((k_gemm_f1<128, 256>), grid, dim3(THREADS2), 0, st, p);
      else if (a->N == 64) hipLaunchKernelGGL((k_gemm_f1<256, 64>), grid, dim3(THREADS2), 0, st, p);
      else hipLaunchKernelGGL((k_gemm_f1<256, 256>), grid, dim3(THREADS2), 0, st, p);
      break;
    case Route::Dma256:
      hipLaunchKernelGGL(k_gemm_bf16_dma256, grid, dim3(THREADS2), 0, st, p);
      break;
    case Route::Dma128:
      hipLaunchKernelGGL(k_gemm_bf16_dma, grid, dim3(THREADS), 0, st, p);
      break;
    case Route::BfKm: {
      // element size of each operand: 8-B (bf16) or 16-B (fp32) runs of 4 rows
      const bool va16 = a->a_bf16 ? (reinterpret_cast<uintptr_t>(a->A) & 7) == 0 && a->lda % 4 == 0 : va;
      const bool vb16 = a->b_bf16 ? (reinterpret_cast<uintptr_t>(a->B) & 7) == 0 && a->ldb % 4 == 0 : vb;
      if (a->a_bf16 && a->b_bf16) launch_bf<__bf16, __bf16>(p, va16, vb16, grid, st);
      else if (a->a_bf16) launch_bf<__bf16, float>(p, va16, vb16, grid, st);
      else if (a->b_bf16) launch_bf<float, __bf16>(p, va16, vb16, grid, st);
      else launch_bf<float, float>(p, va16, vb16, grid, st);
      break;
    }
    case Route::Generic:
      if (a->a_kc && a->b_kc) launch_generic<true, true>(p, va, vb, grid, st);
      else if (a->a_kc) launch_generic<true, false>(p, va, vb, grid, st);
      else if (a->b_kc) launch_generic<false, true>(p, va, vb, grid, st);
      else launch_generic<false, false>(p, va, vb, grid, st);
      break;
  }
  if (zs > 1) {
    const int rc = launch_status(__func__);
    if (rc) return rc;
    const int64_t outs = (int64_t)partial_floats(a);
    if (outs <= 4096)  // a few hundred outputs: 16 lanes each (sum_z16)
      hipLaunchKernelGGL(k_gemm_reduce<16>, grid_for(16 * outs, 256, 16384), 256, 0, st, p, (int)zs);
    else
      hipLaunchKernelGGL(k_gemm_reduce<4>, grid_for(4 * outs, 256, 16384), 256, 0, st, p, (int)zs);
  }
  return launch_status(__func__);
}

// ---- aon_gemm_batch: one level's weight gradients in one launch (+ one reduce) per class: the
// one-tile 256 x 256 bf16 products on k_gemm_bf16_dma256_batch, the other whole-128 x 128-tile
// bf16 products on k_gemm_bf16_dma_batch, the parity mode's 256 x 256 single-accumulator
// products on k_gemm_f1h_batch and its other whole-tile fp16x3 weight gradients on
// k_gemm_f16x3_batch; any other product runs as aon_gemm.
enum { kBatchNone = 0, kBatch256 = 1, kBatch128 = 2, kBatchF16 = 3, kBatchF1 = 4 };
constexpr int kBatchClasses[] = {kBatchF1, kBatchF16, kBatch256, kBatch128};

static int batch_class(const aon_gemm_args* a) {
  if (a->k_splits > 0 || a->K < 8 * 1024) return kBatchNone;
  const int64_t tiles = (a->M / BM) * (a->N / BN);
  switch (route_of(a)) {
    case Route::F1:  // (k_gemm_f1's other shapes: their own launch)
      return a->M == 256 && a->N == 256 ? kBatchF1 : kBatchNone;
    case Route::Dma256:
      return a->M == BM2 && a->N == BM2 ? kBatch256 : kBatchNone;
    case Route::Dma128:
      return tiles < 512 ? kBatch128 : kBatchNone;
    case Route::Generic: {
      // fp16x3 weight gradients dW = dY^T X: fp32 reduction-major operands in 16-B runs, whole
      // 128 x 128 tiles, no epilogue beyond accumulate (k_gemm_f16x3<false, false, true, true>)
      const bool ok = !a->a_bf16 && !a->b_bf16 && !a->a_kc && !a->b_kc && !a->A2 && !a->bias &&
                      !a->mask && !a->relu && !a->exact_fp32 && a->b_rdiv == 1 &&
                      a->M % BM == 0 && a->N % BN == 0 && (a->n_store == 0 || a->n_store == a->N) &&
                      aligned16(a->A) && a->lda % 4 == 0 && aligned16(a->B) && a->ldb % 4 == 0 &&
                      tiles < 512;
      return ok ? kBatchF16 : kBatchNone;
    }
    default:
      return kBatchNone;
  }
}

// workgroup tiles of one product of a class (k_gemm_f1h_batch: two half tiles)
static int64_t class_tiles(const aon_gemm_args* g, int cls) {
  return cls == kBatch256 ? 1 : cls == kBatchF1 ? 2 : (g->M / BM) * (g->N / BN);
}

struct BatchPlan {
  int idx[AON_GEMM_BATCH_MAX];  // products of the class, in argument order
  int n;
  int64_t K, kchunk, zs, tiles;
};

static BatchPlan plan_class(const aon_gemm_args* a, int count, int cls) {
  BatchPlan pl{};
  for (int i = 0; i < count; ++i)
    if (batch_class(&a[i]) == cls) {
      if (pl.n == 0) pl.K = a[i].K;
      if (a[i].K == pl.K) pl.idx[pl.n++] = i;  // other K: run alone (aon_gemm)
    }
  if (pl.n < 2) { pl.n = 0; return pl; }
  for (int j = 0; j < pl.n; ++j) pl.tiles += class_tiles(&a[pl.idx[j]], cls);
  // 256 x 256 tiles: one workgroup per CU (256 in all), chunks >= 1024 rows; 128 x 128 tiles:
  // two per CU (512), chunks >= 2048 rows -- each product's chunks longer by the batch size;
  // fp16x3: whole rounds of 512 as aon_gemm's split (two when K is long enough)
  const bool one = cls == kBatch256 || cls == kBatchF1;  // one 256 x 256 tile, one WG per CU
  const int64_t wgs = one ? 256 : 512, minrows = one ? 1024 : 2048;
  const int64_t cap = pl.K / minrows < 256 ? pl.K / minrows : 256;
  int64_t s = wgs / pl.tiles < cap ? wgs / pl.tiles : cap;
  if (cls == kBatchF16 && cap * pl.tiles >= 1024) s = 1024 / pl.tiles;
  s = s >= 8 ? s / 8 * 8 : (s < 1 ? 1 : s);
  pl.kchunk = s > 1 ? ((pl.K + s - 1) / s + BK - 1) / BK * BK : pl.K;
  pl.zs = (pl.K + pl.kchunk - 1) / pl.kchunk;
  return pl;
}

static size_t plan_bytes(const aon_gemm_args* a, const BatchPlan& pl) {
  if (pl.n == 0 || pl.zs <= 1) return 0;
  size_t f = 0;
  for (int j = 0; j < pl.n; ++j) f += (size_t)pl.zs * (a[pl.idx[j]].M * a[pl.idx[j]].N + a[pl.idx[j]].M);
  return f * sizeof(float);
}

static bool in_plan(const BatchPlan& pl, int i) {
  for (int j = 0; j < pl.n; ++j)
    if (pl.idx[j] == i) return true;
  return false;
}

// the batch's plans, one per class (kBatchClasses order)
struct BatchPlans {
  BatchPlan pl[4];
  bool planned(int i) const {
    for (const BatchPlan& p : pl)
      if (in_plan(p, i)) return true;
    return false;
  }
};
static BatchPlans plan_all(const aon_gemm_args* a, int count) {
  BatchPlans b;
  for (int c = 0; c < 4; ++c) b.pl[c] = plan_class(a, count, kBatchClasses[c]);
  return b;
}

extern "C" size_t aon_gemm_batch_workspace_bytes(const aon_gemm_args* a, int count) {
  if (!a || count < 1 || count > AON_GEMM_BATCH_MAX) return 0;
  const BatchPlans bp = plan_all(a, count);
  // the launches are stream-ordered: one workspace serves each in turn
  size_t m = 0;
  for (const BatchPlan& p : bp.pl) m = plan_bytes(a, p) > m ? plan_bytes(a, p) : m;
  for (int i = 0; i < count; ++i)
    if (!bp.planned(i)) {
      const size_t b = aon_gemm_workspace_bytes(&a[i]);
      m = b > m ? b : m;
    }
  return m;
}

static int run_plan(const aon_gemm_args* a, const BatchPlan& pl, int cls, void* work,
                    size_t work_bytes, hipStream_t st) {
  ParamsBatch pb;
  pb.count = pl.n;
  pb.zsplit = (int)pl.zs;
  pb.tile0[0] = 0;
  AON_REQUIRE(pl.zs == 1 || (work && work_bytes >= plan_bytes(a, pl)),
              "aon_gemm_batch needs aon_gemm_batch_workspace_bytes() of workspace");
  float* part = static_cast<float*>(work);
  const bool bf = cls == kBatch256 || cls == kBatch128;
  for (int j = 0; j < pl.n; ++j) {
    const aon_gemm_args* g = &a[pl.idx[j]];
    if (const int rc = check_product("aon_gemm_batch", g)) return rc;
    Params& p = pb.p[j];
    fill_params(*g, p);
    // a batch kernel is a plain weight gradient: what the classes do not take stays neutral
    p.A2 = nullptr; p.lda2 = 0; p.K1 = INT64_MAX; p.a2_rdiv = 1;
    p.b_rdiv = 1;
    p.bias = p.mask = nullptr;
    p.ldm = 0;
    p.relu = p.c_trans = 0;
    if (bf) {  // the bf16 kernels take no operand scales
      p.sa = p.sb = p.inv_s = 1.0f;
      p.sa_bits = nullptr;
    }
    p.kchunk = pl.kchunk;
    p.zsplit = (int)pl.zs;
    const int bmt = cls == kBatch256 || cls == kBatchF1 ? BM2 : BM;
    p.tiles_m = (int)(g->M / bmt);
    p.tiles_n = (int)(g->N / bmt);
    p.gm = p.tiles_m;
    p.tblocks = p.tiles_m * p.tiles_n;
    pb.tile0[j + 1] = pb.tile0[j] + p.tblocks;
    if (pl.zs > 1) {
      p.part = part;
      p.rowsum_part = p.part + pl.zs * g->M * g->N;
      part += pl.zs * (g->M * g->N + g->M);
    }
  }
  const dim3 grid((unsigned)(8 * pl.tiles * ((pl.zs + 7) / 8)), 1, 1);
  if (cls == kBatch256) hipLaunchKernelGGL(k_gemm_bf16_dma256_batch, grid, dim3(THREADS2), 0, st, pb);
  else if (cls == kBatchF1) hipLaunchKernelGGL(k_gemm_f1h_batch, grid, dim3(THREADS2), 0, st, pb);
  else if (cls == kBatch128) hipLaunchKernelGGL(k_gemm_bf16_dma_batch, grid, dim3(THREADS), 0, st, pb);
  else hipLaunchKernelGGL(k_gemm_f16x3_batch, grid, dim3(THREADS), 0, st, pb);
  if (pl.zs > 1) {
    const int rc = launch_status("aon_gemm_batch");
    if (rc) return rc;
    int64_t mx = 0;
    for (int j = 0; j < pl.n; ++j) {
      const int64_t w = 4 * (pb.p[j].M * pb.p[j].N + pb.p[j].M);
      mx = w > mx ? w : mx;
    }
    const dim3 rg((unsigned)grid_for(mx, 256, 16384), (unsigned)pl.n, 1);
    hipLaunchKernelGGL(k_gemm_reduce_batch, rg, dim3(256), 0, st, pb);
  }
  return launch_status("aon_gemm_batch");
}

extern "C" int aon_gemm_batch(const aon_gemm_args* a, int count, void* work, size_t work_bytes,
                              aon_stream_t stream) {
  AON_REQUIRE(a && count >= 0 && count <= AON_GEMM_BATCH_MAX, "bad batch");
  hipStream_t st = (hipStream_t)stream;
  const BatchPlans bp = plan_all(a, count);
  for (int c = 0; c < 4; ++c)
    if (bp.pl[c].n) {
      const int rc = run_plan(a, bp.pl[c], kBatchClasses[c], work, work_bytes, st);
      if (rc) return rc;
    }
  for (int i = 0; i < count; ++i)
    if (!bp.planned(i)) {
      const int rc = aon_gemm(&a[i], work, work_bytes, stream);
      if (rc) return rc;
    }
  return 0;
}

// whether two row-major views (rows x cols at row stride ld, cols <= ld) share an element:
// views of one matrix with the same ld compare as row / column rectangles (column slices of one
// dW -- the latent segments -- do not overlap), others by their byte extents
static bool views_overlap(const float* p, int64_t rp, int64_t cp, int64_t lp, const float* q,
                          int64_t rq, int64_t cq, int64_t lq) {
  const intptr_t a = reinterpret_cast<intptr_t>(p), b = reinterpret_cast<intptr_t>(q);
  const intptr_t ae = a + (intptr_t)(((rp - 1) * lp + cp) * 4), be = b + (intptr_t)(((rq - 1) * lq + cq) * 4);
  if (ae <= b || be <= a) return false;
  if (lp != lq || (b - a) % 4 != 0 || cp > lp || cq > lq) return true;
  int64_t d = (b - a) / 4;  // q's first element relative to p's, in elements
  int64_t row = d / lp, col = d % lp;
  if (col < 0) {
    col += lp;
    row -= 1;
  }
  // q covers columns [col, col + cq) of rows row.., wrapping into the next row past ld
  for (int w = 0; w < 2; ++w) {
    const int64_t c0 = w == 0 ? col : 0, c1 = w == 0 ? (col + cq < lp ? col + cq : lp) : col + cq - lp;
    const int64_t r0 = row + w;
    if (c1 <= c0) continue;
    if (r0 < rp && r0 + rq > 0 && c0 < cp && c1 > 0) return true;
  }
  return false;
}

extern "C" int aon_gemm_small_batch(const aon_gemm_args* a, int count, aon_stream_t stream) {
  AON_REQUIRE(a && count >= 0 && count <= AON_GEMM_SMALL_BATCH_MAX, "bad batch");
  if (count == 0) return 0;
  SmallBatch sb{};
  int group_of[AON_GEMM_SMALL_BATCH_MAX];
  int ng = 0;
  const aon_gemm_args* head[AON_GEMM_SMALL_BATCH_MAX];
  for (int i = 0; i < count; ++i) {
    const aon_gemm_args* g = &a[i];
    AON_REQUIRE(route_of(g) == Route::Small && g->A && g->B && g->C && g->M > 0 && g->N > 0 && g->K > 0 &&
                    g->ldc >= g->N,
                "aon_gemm_small_batch: exact_fp32 tiny products only (as aon_gemm's exact_fp32)");
    int gi = -1;
    for (int j = 0; j < ng; ++j)
      if (head[j]->C == g->C) gi = j;
    if (gi < 0) {
      head[ng] = g;
      gi = ng++;
    } else {
      const aon_gemm_args* h = head[gi];
      AON_REQUIRE(h->M == g->M && h->N == g->N && h->ldc == g->ldc && (h->K > 16) == (g->K > 16) &&
                      g->accumulate,
                  "aon_gemm_small_batch: products on one C must match in shape and accumulate");
    }
    group_of[i] = gi;
  }
  // no product may read or write what ANOTHER group writes (groups run concurrently), and no
  // product may read its own group's C other than through `accumulate`
  for (int x = 0; x < ng; ++x) {
    const aon_gemm_args* h = head[x];
    for (int i = 0; i < count; ++i) {
      const aon_gemm_args* g = &a[i];
      const int64_t ar = g->a_kc ? g->M : g->K, ac = g->a_kc ? g->K : g->M;
      const int64_t br = g->b_kc ? g->N : g->K, bc = g->b_kc ? g->K : g->N;
      AON_REQUIRE(group_of[i] == x || !views_overlap(h->C, h->M, h->N, h->ldc, g->C, g->M, g->N, g->ldc),
                  "aon_gemm_small_batch: outputs overlap");
      AON_REQUIRE(!views_overlap(h->C, h->M, h->N, h->ldc, g->A, ar, ac, g->lda) &&
                      !views_overlap(h->C, h->M, h->N, h->ldc, g->B, br, bc, g->ldb) &&
                      (!g->bias || !views_overlap(h->C, h->M, h->N, h->ldc, g->bias, 1, g->N, g->N)),
                  "aon_gemm_small_batch: a product reads a batch output");
    }
  }
  int k = 0;
  sb.unit0[0] = 0;
  for (int x = 0; x < ng; ++x) {
    sb.gfirst[x] = k;
    for (int i = 0; i < count; ++i) {
      if (group_of[i] != x) continue;
      const aon_gemm_args* g = &a[i];
      SmallItem& f = sb.it[k++];
      f.A = g->A; f.B = g->B; f.C = g->C; f.bias = g->bias;
      f.lda = g->lda; f.ldb = g->ldb; f.ldc = g->ldc;
      f.M = g->M; f.N = g->N; f.K = g->K;
      f.a_kc = g->a_kc; f.b_kc = g->b_kc; f.accumulate = g->accumulate;
    }
    const int64_t outs = head[x]->M * head[x]->N;
    sb.unit0[x + 1] = sb.unit0[x] + (head[x]->K > 16 ? outs : (outs + 63) / 64);
  }
  sb.gfirst[ng] = k;
  sb.ngroups = ng;
  const int64_t blocks = (sb.unit0[ng] + 3) / 4;
  AON_REQUIRE(blocks < (1ll << 31), "too large");
  hipLaunchKernelGGL(k_gemm_small_batch, (unsigned)blocks, 256, 0, (hipStream_t)stream, sb);
  return launch_status(__func__);
}
