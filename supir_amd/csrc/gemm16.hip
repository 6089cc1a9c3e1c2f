// bf16 MFMA GEMM on v_mfma_f32_16x16x32_bf16 for the shapes whose tile grid can be made EXACTLY a multiple of the 256 CUs
// (tiles 32..35 of the tile table).
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T )      same contract as gemm.hip, for M % BM == 0, N % BN == 0, K % (64 KS) == 0
//
// Why a second kernel family.  70 % of the GEMM launches of a 1024^2 step have M = 2048 and N = 1280 (to_q / to_out / ff.net.2 /
// proj_in / proj_out of the 1280-wide SpatialTransformers, sgm/modules/attention.py:100-106,213-219,587,611).  On the
// 32x32x16 tiles of gemm.hip that is 160 tiles of 128x128 (96 of 256 CUs idle) or 640 tiles of 64x64 (2.5 waves of workgroups,
// twice the L1 traffic per FLOP); measured hot: 17.4 / 14.6 us = 385-460 TFLOP/s whatever the tile.  What bounds a CU is its
// global->LDS fill rate (64 B/clk) and the bytes it can keep in flight (its LDS): a tile needs (BM + BN) * 128 B per K step, so
// the right tile is the squarest one that gives exactly one workgroup per CU: 2048 x 1280 / 256 = 128 x 80.  80 = 5 x 16, hence
// the 16x16x32 MFMA (same FLOP rate as 32x32x16).  N = 2560 (fused to_q|to_k) -> 128 x 160; the GEGLU projection
// (2048 x 10240, attention.py:87) -> 256 x 160 = 512 workgroups = two full rounds.
//
//  tile  BM x BN    waves          K groups  ring   LDS      used for
//   32   128 x  80  4x1 per group     2       2   104 KB   M = 2048, N = 1280 (also N = 640 at M = 8192)
//   33   128 x 160  2x2 per group     2       2   144 KB   N = 2560, M = 8192 x N = 640
//   34   256 x 160  8x1               1       3   156 KB   N = 10240 (GEGLU epilogue: value / gate interleaved per 16 rows of W)
//   35   128 x  80  4x1 per group     2       3   156 KB   tile 32 with a 3-deep ring (two K steps of loads in flight per group)
//   39   256 x 128  4x2               1       3   144 KB   128-channel outputs at M >= 64 K rows (VAE convolutions, sgm/modules/
//                                                          diffusionmodules/model.py:55-148: Cout = 128 at 512^2 / 1024^2)
//   40   256 x 256  4x2               1       2   128 KB   256 / 512-channel outputs of the VAE (32 B/clk of fill per CU: the one tile
//                                                          of the family under the 38 B/clk the loops sustain); one 32-wide K slice of
//                                                          fragments in registers at a time (128 accumulator registers)
//   45   512 x 128  4x2  8-phase      1       2   160 KB   the 128-channel outputs on the same schedule: the 256 x 128 tile needs 48 B/clk of fill per
//                                                          CU for its MFMAs (fill-bound: its K step ran 3222 cycles for 1024 of MFMA on 128 -> 128
//                                                          at 1024^2), 512 x 128 needs 40
//   42   256 x 256  2x4  8-phase      1       2   128 KB   the same outputs on the eight-phase ping-pong schedule (round 5, below): half-tile
//                                                          staging with three half-tiles in flight across the barriers, the two waves of
//                                                          every SIMD alternating between a fragment-read / load-issue segment and a
//                                                          16-MFMA segment
//
//  * 512 threads.  KS = 2: two K groups of four waves, group g takes K steps g, g+2, ... from its own LDS ring, so every SIMD
//    holds two waves (one per group) whose load issue / LDS reads / MFMAs interleave; the partial accumulators are
//    reduce-scattered through LDS after the loop (group g finishes token-fragment rows [g*MI/2, (g+1)*MI/2)) and both groups
//    run the epilogue on their half.  KS = 1: eight waves on one ring;
//  * global -> LDS by global_load_lds_dwordx4, 8 rows (1 KB) per wave instruction, source-side XOR swizzle
//    (chunk ^= (row >> 1) & 7), undone by the ds_read_b128 fragment reads: conflict-free for the 16-row x 4-chunk
//    fragment of the 16x16x32 MFMA (checked per ds_read_b128 lane group); S-deep ring, ONE raw s_barrier per K step, counted
//    vmcnt for S = 3 (every wave issues the same number of loads per stage);
//  * operands swapped (a = W rows, b = A rows): a lane ends with 4 consecutive channels of one token; the fused epilogue
//    is the one of gemm.hip (bias, LayerNorm fold / row statistics, row bias, residual, SiLU, GEGLU, alpha; bf16 output staged
//    through LDS for 16-byte row-contiguous stores); the transposed (V^T) variant swaps the operands back so that a lane
//    holds 4 consecutive tokens of one channel;
//  * exact shapes only (the dispatcher refuses anything else): no bounds checks anywhere in the kernel.
#include "kernels.h"
#include <type_traits>

typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <int N>
__device__ __forceinline__ void g16_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

#ifdef SUPIR_G16_TIMELINE
// tools/probes/g16_timeline.py only (never defined in the product build): per-wave s_memtime stamps of the kernel's phases
__device__ unsigned long long* g16_tl_buf;
extern "C" void supir_g16_tl_set(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g16_tl_buf), &p, sizeof(p)); }
#define G16_TL(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
// in-loop stamps (round 6): only at points where lgkmcnt is 0 anyway (s_memtime returns through lgkmcnt): loop top, after the counted
// wait, after the barrier, after the step's last MFMA + lgkmcnt(0).  ~4 scalar-cache round trips per K step: the split is what counts
#define G16_TLS(var) var = __builtin_amdgcn_s_memtime()
#define G16_TLACC(acc, a, b) acc += (b) - (a)
#else
#define G16_TL(var)
#define G16_TLS(var)
#define G16_TLACC(acc, a, b)
#endif

// zero page for the halo / padding rows of the implicit-GEMM (3x3 convolution) loader
__device__ __attribute__((aligned(256))) uint32_t g16_zero_page[64];

// MIXED (fused q|k|v projection, supir_gemm_bf16_qkv): tile columns [0, n_split) take the normal epilogue into C, tile columns
// [n_split, N) the transposed one into C2 (V^T, channel index n - n_split); decided per workgroup (tile_n), both main loops
// (they differ in the MFMA operand order) are in the kernel.
//
// NP = 2 (supir_gemm_grouped): two independent problems of identical shape in one grid.  Block b runs on XCD b % 8; problem q owns XCDs
// [4 q, 4 q + 4) -- its operands stay in those four L2s -- and maps its tiles over them exactly as a single problem does over eight.
// Used for the layer pairs GLVControl and the UNet encoder execute with identical shapes on independent data
// (SUPIR/modules/SUPIR_v0.py:499-540 next to :600-625): M = 2048 tokens per problem fill only half the machine with tiles big
// enough to be fed from L2 (128 x 80 at 49 FLOP per staged byte); two problems of 128 x 160 tiles are 256 workgroups at 65.
//
// Four-wave form (tile 38 = 128 x 80, 4x1 waves, ONE K group, 3-deep ring = 78 KB, round 4): half the threads and half the LDS of
// tile 35, so that TWO workgroups fit a CU -- in the two-stream step one of GLVControl's and one of the UNet encoder's (VERDICT r03
// item 2: every other tile of this family takes 104-156 KB and a CU then runs one workgroup of one chain at a time).  Same loader,
// same fragment layout, same epilogue; the K-group exchange disappears.
//
// LDS-staged HALO form of the 3x3 convolutions (HW_ > 0 = the map width; round 6, tiles 48-50).  The implicit-GEMM loader above stages every
// input pixel of a tile nine times (once per tap: (BM + BN) x 128 B per 64-wide K step); the counter passes show the price (fetch + write
// 2.2-6.1 x the operands, profiles/pmc_traffic.json) and the L2 -> LDS fill is what bounds these tiles.  Here a tile is BM / W whole rows of
// the map; per 64-channel chunk its (rows + 2) x (W + 2) input pixels -- the halo tile, zero page for what lies outside the image -- are
// staged ONCE, and the nine taps read their token fragments out of it at shifted addresses: the K loop runs (chunk, tap), the ring stages
// carry the W tiles only.  Per chunk a 128 x 80 tile on a 32 x 32 map stages 26 + 90 KB instead of 144 + 90 KB.
//   * halo pixel P = hy (W + 2) + hx lives at P * 128 B, its 16-byte chunk c at physical slot c ^ (P & 7): the 16 lanes of a ds_read_b128
//     group read 16 CONSECUTIVE pixels starting anywhere (the tap shift) and two adjacent chunks -- slot = (P & 1) * 8 + (c ^ (P & 7)) is a
//     bijection on any such window (enumerated: tools/probes/halo_swizzle_check.py), so every tap's fragment reads are conflict-free;
//   * two halo buffers (chunk parity).  The eight waves load chunk c + 2 into the buffer chunk c leaves, 8-pixel pieces (1 KB per wave
//     instruction, wave w takes pieces w, w + 8, ...), HQ pieces per wave and iteration in the NLI iterations after the last step of chunk
//     c -- early enough that the counted wait of the W ring (S = 3: everything but the previous iteration's loads has landed) covers them
//     S - 1 iterations later, before the first step of chunk c + 2;
//   * two K groups: group g takes steps g, g + 2, ... of the (chunk, tap) sequence -- taps of one chunk alternate between the groups, both
//     read the same halo buffers; the schedule above is in ITERATIONS (one step of each group), which both groups share;
//   * a wave's number of loads now varies by iteration (0..HQ halo pieces on top of the W chunks): the counted wait is selected, wave
//     uniformly, by the count of the previous iteration.
// Everything after the main loop (K-group exchange, epilogue, GroupNorm partials, prefetch) is the code of the other forms: a tile is still
// BM consecutive rows of the [M][N] output.
// Measured (profiles/r06): fetch + write per launch falls to 1.1-1.4 x the operands; texture-addresser busy 60 % -> 37 %; TIME is equal to
// the implicit-GEMM tiles within the box noise (0.94-1.09 x) -- the in-loop stamps show the loop is not bound by the fill (counted wait: 8
// cycles per step), nor by LDS (index pipe 28 % busy, no bank conflicts in either form), nor by the matrix pipe (39 %): a step is wait 8 /
// barrier 250 / reads + loads + MFMAs 1070 cycles against 640 of MFMA.  Three re-orderings of that step were built and measured on top of this
// form and of the implicit one -- the two K groups ping-ponging across two barriers, fragments software-pipelined inside each wave, the
// groups' load / MFMA order staggered -- all bitwise equal, all 5-15 % SLOWER (docs/roundlog.md section 6); they are not in the tree.
template <int BM, int BN, int WM, int WN, int KS, int S, bool TRANS, bool CONV = false, bool MIXED = false, int NP = 1, int HW_ = 0>
__global__ __launch_bounds__(64 * WM * WN * KS, (WM * WN * KS == 8 ? 2 : 1)) void gemm16_kernel(const GemmArgsN<NP> pp) {
#include "gemm16_body.inc"
}

// The plain single-problem tile with alpha loaded from a 4-byte device cell when the kernel runs (the ZeroCrossAttn output projection
// under a dynamic control scale, SUPIR_v0.py:138-152 with the per-step scale of sampling.py:557-559).  Same body, same arithmetic.
template <int BM, int BN, int WM, int WN, int KS, int S>
__global__ __launch_bounds__(64 * WM * WN * KS, (WM * WN * KS == 8 ? 2 : 1)) void gemm16_alpha_kernel(const GemmArgsN<1> pp_in,
                                                                                                  const float* __restrict__ alpha_cell) {
    constexpr bool TRANS = false, CONV = false, MIXED = false;
    constexpr int NP = 1, HW_ = 0;
    GemmArgsN<1> pp = pp_in;
    pp.p[0].alpha = *alpha_cell;
#include "gemm16_body.inc"
}

// The stride-1 3 x 3 convolution tile with the ZeroSFT epilogue (SUPIR/modules/SUPIR_v0.py:62-113): the convolution is zero_mul | zero_add
// (W rows interleaved [16 gamma | 16 beta]) and the epilogue applies GroupNorm(cat[x1, x2]) * (gamma + 1) + beta with the control-scale
// lerp instead of storing the two maps -- what conv3x3 + gn_apply_kernel<1, true, false> compute in two launches and a round trip of
// a [tokens][2 C] map through memory.  Same loader, ring and main loop as gemm16_kernel's convolution form; its own instantiations
// (one wave column: the (gamma, beta) fragment pairs lie in one lane), so no other launch changes.
template <int BM, int BN, int WM, int WN, int KS, int S, int HW_ = 0>
__global__ __launch_bounds__(64 * WM * WN * KS, 2) void gemm16_zsft_kernel(const GemmArgsN<1> pp, const ZsftArgs zs) {
    constexpr bool TRANS = false, CONV = true, MIXED = false;
    constexpr int NP = 1;
#define SUPIR_G16_ZSFT
#include "gemm16_body.inc"
#undef SUPIR_G16_ZSFT
}

template <int BM, int BN, int WM, int WN, int KS, int S>
static int launch_gemm16_zsft(const GemmArgs& a_in, const ZsftArgs& zs, hipStream_t st) {
    GemmArgsN<1> pp;
    pp.p[0] = a_in;
    GemmArgs& a = pp.p[0];
    a.korder = 0;
    const int tiles = (a.M / BM) * (a.N / BN);
    supir_choose_xcd_grid(a, a.M / BM, a.N / BN, 2.0 * (double)a.M * a.Cin, 2.0 * (double)a.N * a.K, 9, 1, 8);
    constexpr int smem = KS * S * (BM + BN) * 128 + 256 + 1024;   // the rings, the prefetch scratch row, sa | sb of the tile's 80 channels
    static_assert(smem <= 163840, "LDS");
    auto kern = gemm16_zsft_kernel<BM, BN, WM, WN, KS, S>;
    static bool attr_set = false;
    if (!attr_set) {
        if (supir_note_hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)) != SUPIR_OK) return SUPIR_ERR_HIP;
        attr_set = true;
    }
    SUPIR_LAUNCH(kern, dim3(tiles), dim3(64 * WM * WN * KS), smem, st, pp, zs);
    return SUPIR_LAUNCH_STATUS();
}

// tiles 33 (128 x 160, two K groups of 4 x 1 waves) and 34 (256 x 160, 8 x 1 waves).  a: the convolution 128 -> 2 C with the
// interleaved weights (a.N = 2 C; a.C / a.ldc = the [tokens][C] output); z: the GroupNorm / modulation operands
bool supir_gemm16_zsft_supported(const GemmArgs& a, const ZsftArgs& z, int tile) {
    if (tile != 33 && tile != 34) return false;
    const int bm = tile == 34 ? 256 : 128, ks = tile == 34 ? 1 : 2, s = tile == 34 ? 3 : 2;
    // the convolution: exact tiles, stride 1, pad 1, no upsampling, no other epilogue term
    if (a.M % bm || a.N % 160 || a.K % (64 * ks) || a.lda % 8 || (a.K >> 6) / ks < s - 1 || a.Cin % (64 * ks) || a.K != 9 * a.Cin) return false;
    if (a.stride != 1 || a.up || a.pad_t != 1 || a.pad_l != 1 || a.OH != a.H || a.OW != a.W) return false;
    if (a.out_mode != 0 || a.act != 0 || a.res || a.rowbias || a.ln_stats || a.rowstats_out || a.alpha != 1.0f || !a.bias) return false;
    if (a.ldc % 8 || (((size_t)a.C) & 15)) return false;
    // tile rows never straddle a batch element; a tile's 80 channels never straddle the two concat sources; the GroupNorm groups and both
    // sources are whole 10-channel partial units
    if (a.rows_per_batch != a.OH * a.OW || a.rows_per_batch % bm) return false;
    if (z.C <= 0 || a.N != 2 * z.C || z.C % 320 || z.C1 <= 0 || z.C1 > z.C || z.C1 % 80 || (z.C1 < z.C && !z.x2)) return false;
    if (!z.x1 || !z.gamma || !z.beta || !z.part_u1 || z.nch1 <= 0 || (z.C1 < z.C && (!z.part_u2 || z.nch2 <= 0))) return false;
    if (z.ld1 % 4 || (z.C1 < z.C && z.ld2 % 4) || z.ld1 < z.C1 || (z.C1 < z.C && z.ld2 < z.C - z.C1)) return false;
    if ((((size_t)z.x1) | ((size_t)z.x2) | ((size_t)z.x1raw) | ((size_t)z.x2raw)) & 7) return false;
    return true;
}

int supir_gemm16_zsft_launch(const GemmArgs& a, const ZsftArgs& z, hipStream_t st, int tile) {
    if (!supir_gemm16_zsft_supported(a, z, tile)) return SUPIR_ERR_SHAPE;
    if (tile == 34) return launch_gemm16_zsft<256, 160, 8, 1, 1, 3>(a, z, st);
    return launch_gemm16_zsft<128, 160, 4, 1, 2, 2>(a, z, st);
}

template <int BM, int BN, int WM, int WN, int KS, int S, bool TRANS, bool CONV = false, bool MIXED = false, int NP = 1, int HW_ = 0>
static int launch_gemm16(const GemmArgs* a_in, hipStream_t st, const float* alpha_cell = nullptr) {
    GemmArgsN<NP> pp;
    for (int q = 0; q < NP; ++q) {
        pp.p[q] = a_in[q];
        pp.p[q].korder = (CONV && S == 8 && supir_debug_knob_value(6) != 1) ? 1 : 0;   // tile 42 / 45 convolutions: chunk-major K order (knob 6 = 1: tap-major)
    }
    GemmArgs& a = pp.p[0];
    const int tiles = (a.M / BM) * (a.N / BN);
    if (NP > 1 && tiles % (8 / NP)) return SUPIR_ERR_SHAPE;
    const double a_bytes = CONV ? 2.0 * (double)a.M * (a.up ? 0.25 : (double)(a.stride * a.stride)) * a.Cin : 2.0 * (double)a.M * a.K;
    supir_choose_xcd_grid(a, a.M / BM, a.N / BN, a_bytes, 2.0 * (double)a.N * a.K, CONV ? (HW_ > 0 ? 2 : 9) : 1, 1, 8 / NP);
    for (int q = 1; q < NP; ++q) {   // identical shapes: identical tile maps
        pp.p[q].gm = a.gm;
        pp.p[q].gn = a.gn;
        pp.p[q].order = a.order;
    }
    // the ring(s) + the prefetch scratch row (the eight-phase tiles dump the prefetch into the last 256 bytes of their ring, which the
    // epilogue scratch never reaches: the 512 x 128 tile uses all 160 KB)
    // halo form: the rings hold W tiles only, two halo tiles of ((BM / W + 2) (W + 2) pixels, rounded up to 8) x 128 B behind them
    constexpr int halo_bytes = HW_ > 0 ? 2 * ((((BM / (HW_ > 0 ? HW_ : 1) + 2) * (HW_ + 2) + 7) / 8) * 1024) : 0;
    constexpr int smem = HW_ > 0 ? KS * S * BN * 128 + halo_bytes + 256 : KS * (S == 8 ? 2 : S) * (BM + BN) * 128 + (S == 8 ? 0 : 256);
    static_assert(smem <= 163840, "LDS");
    if (alpha_cell) {   // dynamic alpha: the plain single-problem tiles 32 / 33 / 34 / 35 only
        if constexpr (!TRANS && !CONV && !MIXED && NP == 1 && HW_ == 0 && S != 8 && ((BN == 80 && KS == 2) || BN == 160)) {
            auto kern = gemm16_alpha_kernel<BM, BN, WM, WN, KS, S>;
            static bool attr_set = false;
            if (!attr_set) {
                if (supir_note_hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)) != SUPIR_OK) return SUPIR_ERR_HIP;
                attr_set = true;
            }
            SUPIR_LAUNCH(kern, dim3(tiles), dim3(64 * WM * WN * KS), smem, st, pp, alpha_cell);
            return SUPIR_LAUNCH_STATUS();
        } else {
            return SUPIR_ERR_SHAPE;
        }
    }
    auto kern = gemm16_kernel<BM, BN, WM, WN, KS, S, TRANS, CONV, MIXED, NP, HW_>;
    static bool attr_set = false;
    if (!attr_set) {
        if (supir_note_hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)) != SUPIR_OK) return SUPIR_ERR_HIP;
        attr_set = true;
    }
    SUPIR_LAUNCH(kern, dim3(NP * tiles), dim3(64 * WM * WN * KS), smem, st, pp);
    return SUPIR_LAUNCH_STATUS();
}

// tiles 32 (128 x 80), 33 (128 x 160), 34 (256 x 160, GEGLU-capable), 35 (128 x 80, 3-deep rings): exact fits only
bool supir_gemm16_supported(const GemmArgs& a, int tile, bool conv) {
    if ((tile < 32 || tile > 35) && (tile < 38 || tile > 40) && tile != 42 && tile != 45 && (tile < 48 || tile > 51)) return false;
    const bool halo = tile >= 48;       // LDS-staged halo convolutions: 48 = 128 x 80 @ W 32, 49 = 128 x 160 @ W 64, 50 = 256 x 160 @ W 32, 51 = 256 x 160 @ W 64
    const bool wide = tile == 34 || tile == 39 || tile == 40 || tile == 42 || tile == 45 || tile == 50 || tile == 51;
    const int bm = tile == 45 ? 512 : wide ? 256 : 128;
    const int bn = (tile == 39 || tile == 45) ? 128 : (tile == 40 || tile == 42) ? 256 : (tile == 32 || tile == 35 || tile == 38 || tile == 48) ? 80 : 160;
    const int ks = (wide || tile == 38) ? 1 : 2, s = (tile == 32 || tile == 33 || tile == 40 || tile == 49 || tile == 51) ? 2 : 3;   // tiles 42 / 45: at least two K-tiles
    if (halo) {
        const int hw = (tile == 49 || tile == 51) ? 64 : 32;
        // whole map rows per tile, stride 1, pad 1, no upsampling; 32-bit element offsets inside one image
        if (!conv || a.W != hw || a.OW != hw || a.OH != a.H || a.stride != 1 || a.up || a.pad_t != 1 || a.pad_l != 1) return false;
        if (a.rows_per_batch != a.OH * a.OW || a.rows_per_batch % bm || (long)a.H * a.W * a.lda >= (1L << 31)) return false;
    }
    if (a.M % bm || a.N % bn || a.K % (64 * ks) || a.lda % 8 || (a.K >> 6) / ks < s - 1) return false;
    if (a.out_mode == 1 || a.ln_slots > 32) return false;
    // tiles 39 / 40: plain and convolution forms with the ordinary epilogue only (no transposed output, no GEGLU); their GroupNorm
    // partials come in 4-channel units (channel counts 128 / 256 / 512: 4 / 8 / 16 channels per group)
    if ((tile == 39 || tile == 40 || tile == 42 || tile == 45) && (a.out_mode != 0 || a.act == 2)) return false;
    if (a.gn_part_out && (a.out_mode != 0 || a.act == 2 || a.rows_per_batch <= 0 || a.rows_per_batch % bm || a.N % (bn % 10 == 0 ? 10 : 4))) return false;
    if (conv) {
        // tile 42 keeps 32-bit tap offsets against ONE image base per tile: rows of a tile in one batch element, the image below 2^31 elements
        if ((tile == 42 || tile == 45) && (a.rows_per_batch % bm || (long)a.H * a.W * a.lda >= (1L << 31) || (long)a.W * a.lda >= (1L << 24) || a.H >= (1 << 23))) return false;
        if (a.Cin % (64 * ks) || a.K != 9 * a.Cin || a.out_mode != 0 || a.act == 2 || a.ln_stats || a.rowstats_out) return false;
    }
    if (a.act == 2)
        return tile == 34 && a.out_mode == 0 && !a.res && !a.rowbias && !a.rowstats_out && a.ldc % 8 == 0 && (((size_t)a.C) & 15) == 0;
    if (a.out_mode == 2) return a.rows_per_batch % 4 == 0 && a.ldc % 4 == 0 && !a.res && !a.rowbias && a.act == 0;
    if (a.ldc % 8 || (((size_t)a.C) & 15)) return false;
    if ((a.res && a.ldr % 4) || (a.rowbias && a.ld_rb % 4)) return false;
    return true;
}

int supir_gemm16_launch(const GemmArgs& a, hipStream_t st, int tile, bool conv, const float* alpha_cell) {
    if (!supir_gemm16_supported(a, tile, conv)) return SUPIR_ERR_SHAPE;
    if (alpha_cell) {   // dynamic alpha (supir_gemm_bf16_ex_dyn): plain bf16-output GEMM on tiles 32..35, the tile the float call would run
        if (conv || a.out_mode != 0 || tile < 32 || tile > 35) return SUPIR_ERR_SHAPE;
        switch (tile) {
            case 32: return launch_gemm16<128, 80, 4, 1, 2, 2, false>(&a, st, alpha_cell);
            case 33: return launch_gemm16<128, 160, 2, 2, 2, 2, false>(&a, st, alpha_cell);
            case 34:
                if (a.act != 2 && (supir_debug_knob_value(1) == 1 || (supir_debug_knob_value(1) == 0 && a.M >= 8192)))
                    return launch_gemm16<256, 160, 4, 2, 1, 3, false>(&a, st, alpha_cell);
                return launch_gemm16<256, 160, 8, 1, 1, 3, false>(&a, st, alpha_cell);
            default: return launch_gemm16<128, 80, 4, 1, 2, 3, false>(&a, st, alpha_cell);
        }
    }
    if (conv) {
        switch (tile) {
            case 32: return launch_gemm16<128, 80, 4, 1, 2, 2, false, true>(&a, st);
            case 33: return launch_gemm16<128, 160, 2, 2, 2, 2, false, true>(&a, st);
            // 256 x 160: the eight waves as 4 x 2 (64 x 80 per wave: 18 fragment reads per K step instead of 24 for 8 x 1).  Same tile,
            // same K order: outputs bitwise equal; +3..5 % on the large convolutions (profiles/r04/micro_256x160_waves_*.log).
            // knob 1 = 2 forces 8 x 1 (A/B runs)
            case 34: return supir_debug_knob_value(1) != 2 ? launch_gemm16<256, 160, 4, 2, 1, 3, false, true>(&a, st)
                                                           : launch_gemm16<256, 160, 8, 1, 1, 3, false, true>(&a, st);
            case 38: return launch_gemm16<128, 80, 4, 1, 1, 3, false, true>(&a, st);
            case 39: return launch_gemm16<256, 128, 4, 2, 1, 3, false, true>(&a, st);
            case 40: return launch_gemm16<256, 256, 4, 2, 1, 2, false, true>(&a, st);
            case 42: return launch_gemm16<256, 256, 2, 4, 1, 8, false, true>(&a, st);
            case 45: return launch_gemm16<512, 128, 4, 2, 1, 8, false, true>(&a, st);
            case 48: return launch_gemm16<128, 80, 4, 1, 2, 3, false, true, false, 1, 32>(&a, st);
            case 49: return launch_gemm16<128, 160, 2, 2, 2, 2, false, true, false, 1, 64>(&a, st);
            case 50: return launch_gemm16<256, 160, 4, 2, 1, 3, false, true, false, 1, 32>(&a, st);
            case 51: return launch_gemm16<256, 160, 4, 2, 1, 2, false, true, false, 1, 64>(&a, st);
            default: return launch_gemm16<128, 80, 4, 1, 2, 3, false, true>(&a, st);
        }
    }
    const bool t = a.out_mode == 2;
    switch (tile) {
        case 39: return launch_gemm16<256, 128, 4, 2, 1, 3, false>(&a, st);
        case 40: return launch_gemm16<256, 256, 4, 2, 1, 2, false>(&a, st);
        case 42: return launch_gemm16<256, 256, 2, 4, 1, 8, false>(&a, st);
        case 45: return launch_gemm16<512, 128, 4, 2, 1, 8, false>(&a, st);
        case 38: return t ? launch_gemm16<128, 80, 4, 1, 1, 3, true>(&a, st) : launch_gemm16<128, 80, 4, 1, 1, 3, false>(&a, st);
        case 32: return t ? launch_gemm16<128, 80, 4, 1, 2, 2, true>(&a, st) : launch_gemm16<128, 80, 4, 1, 2, 2, false>(&a, st);
        case 33: return t ? launch_gemm16<128, 160, 2, 2, 2, 2, true>(&a, st) : launch_gemm16<128, 160, 2, 2, 2, 2, false>(&a, st);
        case 34:
            // knob 1 (tools only): the 256 x 160 tile with its eight waves as 4 x 2 (64 x 80 per wave: 18 fragment reads per K step
            // instead of 24) -- not for GEGLU (value / gate pairs need an even number of column fragments per wave)
            // default (knob 1 = 0): 4 x 2 for M >= 8192 (measured +2..4 % there, equal below); 1 forces 4 x 2, 2 forces 8 x 1
            if (a.act != 2 && (supir_debug_knob_value(1) == 1 || (supir_debug_knob_value(1) == 0 && a.M >= 8192)))
                return t ? launch_gemm16<256, 160, 4, 2, 1, 3, true>(&a, st) : launch_gemm16<256, 160, 4, 2, 1, 3, false>(&a, st);
            return t ? launch_gemm16<256, 160, 8, 1, 1, 3, true>(&a, st) : launch_gemm16<256, 160, 8, 1, 1, 3, false>(&a, st);
        default: return t ? launch_gemm16<128, 80, 4, 1, 2, 3, true>(&a, st) : launch_gemm16<128, 80, 4, 1, 2, 3, false>(&a, st);
    }
}

// Two problems in one launch (tiles 33 / 34 / 35; tile 32 is tile 35 with a shallower ring and has no grouped form).  What fixes the
// grid and the kernel instantiation must agree (M, N, K, output mode); every other argument -- pointers, strides, which optional
// operands are present, the convolution geometry -- is read per problem.
static bool g16_same_shape(const GemmArgs& x, const GemmArgs& y) {
    return x.M == y.M && x.N == y.N && x.K == y.K && x.out_mode == y.out_mode;
}

int supir_gemm16_launch_n(const GemmArgs* a, int n, hipStream_t st, int tile, bool conv) {
    if (n == 1) return supir_gemm16_launch(a[0], st, tile, conv);
    if (n != 2 || tile == 32 || tile >= 38) return SUPIR_ERR_SHAPE;      // (the halo tiles 48-51 have no grouped form)
    if (!supir_gemm16_supported(a[0], tile, conv) || !supir_gemm16_supported(a[1], tile, conv) || !g16_same_shape(a[0], a[1])) return SUPIR_ERR_SHAPE;
    // the wave arrangement of the 256 x 160 tile follows the single-launch policy (4 x 2 for convolutions and M >= 8192): a grouped launch
    // must stay bitwise the two single launches, GroupNorm partials and row statistics included (their cross-wave sums are ordered by it)
    const int knob = supir_debug_knob_value(1);
    if (conv) {
        switch (tile) {
            case 33: return launch_gemm16<128, 160, 2, 2, 2, 2, false, true, false, 2>(a, st);
            case 34: return knob != 2 ? launch_gemm16<256, 160, 4, 2, 1, 3, false, true, false, 2>(a, st)
                                      : launch_gemm16<256, 160, 8, 1, 1, 3, false, true, false, 2>(a, st);
            default: return launch_gemm16<128, 80, 4, 1, 2, 3, false, true, false, 2>(a, st);
        }
    }
    const bool t = a[0].out_mode == 2;
    const bool w42 = a[0].act != 2 && (knob == 1 || (knob == 0 && a[0].M >= 8192));
    switch (tile) {
        case 33: return t ? launch_gemm16<128, 160, 2, 2, 2, 2, true, false, false, 2>(a, st) : launch_gemm16<128, 160, 2, 2, 2, 2, false, false, false, 2>(a, st);
        case 34:
            if (w42) return t ? launch_gemm16<256, 160, 4, 2, 1, 3, true, false, false, 2>(a, st) : launch_gemm16<256, 160, 4, 2, 1, 3, false, false, false, 2>(a, st);
            return t ? launch_gemm16<256, 160, 8, 1, 1, 3, true, false, false, 2>(a, st) : launch_gemm16<256, 160, 8, 1, 1, 3, false, false, false, 2>(a, st);
        default: return t ? launch_gemm16<128, 80, 4, 1, 2, 3, true, false, false, 2>(a, st) : launch_gemm16<128, 80, 4, 1, 2, 3, false, false, false, 2>(a, st);
    }
}

// fused q|k|v projection: columns [0, n_split) -> C (normal epilogue), [n_split, N) -> C2 transposed.  Two tile widths, 256 x 160 (tile 34's
// loop, eight waves as 8 x 1) and 256 x 128 (tile 39's, 4 x 2): the launch takes the one with fewer rounds-of-256-workgroups x columns.
// (2048, 3840, 1280) -- the 1280-wide SpatialTransformers at 32^2 -- is 192 tiles of 256 x 160 (64 CUs idle) or 240 of 256 x 128, each
// 0.8 x the work: one round either way.  Same K order per output element: bitwise-equal results.
static int g16_qkv_check(const GemmArgs& a, int bn) {
    if (a.M % 256 || a.N % bn || a.n_split % bn || a.n_split <= 0 || a.n_split >= a.N || a.K % 64 || (a.K >> 6) < 2) return SUPIR_ERR_SHAPE;
    if (a.lda % 8 || a.ldc % 8 || (((size_t)a.C) & 15) || a.ldc2 % 4 || a.rows_per_batch % 4 || a.ln_slots > 32) return SUPIR_ERR_SHAPE;
    if (a.act != 0 || a.out_mode != 0 || a.res || a.rowbias || a.rowstats_out || !a.C2) return SUPIR_ERR_ARG;
    return SUPIR_OK;
}

// knob 4 (tools only): 1 forces 160 columns, 2 forces 128 where both fit
static int g16_qkv_bn(const GemmArgs& a) {
    const bool ok160 = a.N % 160 == 0 && a.n_split % 160 == 0, ok128 = a.N % 128 == 0 && a.n_split % 128 == 0;
    if (!ok128 || !ok160) return ok128 ? 128 : 160;
    const int knob = supir_debug_knob_value(4);
    if (knob == 1 || knob == 2) return knob == 1 ? 160 : 128;
    const long tm = a.M / 256;
    const long c160 = ((tm * (a.N / 160) + 255) / 256) * 160, c128 = ((tm * (a.N / 128) + 255) / 256) * 128;
    return c128 < c160 ? 128 : 160;
}

int supir_gemm16_qkv_launch(const GemmArgs& a, hipStream_t st) {
    const int bn = g16_qkv_bn(a);
    const int rc = g16_qkv_check(a, bn);
    if (rc != SUPIR_OK) return rc;
    if (bn == 128) return launch_gemm16<256, 128, 4, 2, 1, 3, false, false, true>(&a, st);
    if (supir_debug_knob_value(1)) return launch_gemm16<256, 160, 4, 2, 1, 3, false, false, true>(&a, st);
    return launch_gemm16<256, 160, 8, 1, 1, 3, false, false, true>(&a, st);
}

int supir_gemm16_qkv_launch_n(const GemmArgs* a, int n, hipStream_t st) {
    if (n == 1) return supir_gemm16_qkv_launch(a[0], st);
    if (n != 2) return SUPIR_ERR_SHAPE;
    for (int q = 0; q < 2; ++q) {
        const int rc = g16_qkv_check(a[q], 160);
        if (rc != SUPIR_OK) return rc;
    }
    if (!g16_same_shape(a[0], a[1])) return SUPIR_ERR_SHAPE;
    return launch_gemm16<256, 160, 8, 1, 1, 3, false, false, true, 2>(a, st);
}
