// bf16 MFMA GEMM / implicit-GEMM conv3x3 for gfx950 (MI355X).
//
//   C[M,N] = epilogue( A[M,K] . W[N,K]^T )        (every nn.Linear / 1x1 conv / 3x3 conv of the path)
//
// Replaces the cuBLAS / cuDNN calls issued by the reference's nn.Linear / nn.Conv2d modules
// (reference: sgm/modules/attention.py:87,100,106,213-219,587,611; sgm/modules/diffusionmodules/
// openaimodel.py:127,196,263,300; SUPIR/modules/SUPIR_v0.py:48,79-87; sgm/modules/diffusionmodules/model.py:60-124).
//
// Design (CDNA4):
//  * activations are NHWC bf16 ("tokens x channels"), weights are [N][K] bf16 with K contiguous, so both MFMA
//    operands are K-contiguous rows and are staged with the same code;
//  * global -> LDS by `global_load_lds_dwordx4` (no VGPR round trip). The LDS image is lane-linear, so the
//    bank-conflict swizzle is applied to the per-lane SOURCE address and undone on the ds_read_b128 side:
//    16-B chunk c of row r lives at chunk c ^ ((r>>1)&7)  (conflict-free for the 32x32x16 fragment read);
//  * 3x3 convolution is the same kernel with an im2col gather in the A loader: K runs (ky,kx,cin) and a
//    64-wide K step never straddles a tap because Cin % 64 == 0; the gather address of each row is computed once
//    per tap; halo / padding lanes read a zero page; stride 2, asymmetric padding (VAE Downsample) and
//    nearest-2x upsampling are folded into the gather;
//  * v_mfma_f32_32x32x16_bf16, 4 (or 8) waves, operands swapped (a = W rows, b = A rows) so that every lane
//    ends up with 4 consecutive output channels of one token; fused epilogue (bias, per-batch time-embedding add,
//    residual add, SiLU, GEGLU, scale, LayerNorm fold / row statistics), bf16 output staged through LDS so the
//    global stores are 16 B per lane and row-contiguous;
//  * S-deep LDS ring (2 by default), ONE raw s_barrier per K step, counted vmcnt for S > 2; the next tile's
//    global->LDS instructions are interleaved with the MFMA groups of the current one;
//  * XCD-aware workgroup -> tile mapping (8 private L2s); one-shot prefetch of a later launch's weights on the way out.
// tools/probes/gemm_timeline.hip builds this file with -DSUPIR_GEMM_TIMELINE for a per-phase s_memtime breakdown.
#include "kernels.h"
#include <stdlib.h>
#include <type_traits>

#ifndef SUPIR_DEFAULT_STAGES_CODE
#define SUPIR_DEFAULT_STAGES_CODE 1  /* 2-deep ring: measured best (deeper rings cost a resident workgroup per CU) */
#endif


__device__ __attribute__((aligned(256))) uint32_t g_zero_page[64];

#ifdef SUPIR_GEMM_TIMELINE
// tools/probes/gemm_timeline.hip only: per-wave s_memtime breakdown of the main loop (never defined in the product build)
__device__ unsigned long long* g_tl_buf;
extern "C" void supir_tl_set(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tl_buf), &p, sizeof(p)); }
#define TL_NOW() __builtin_amdgcn_s_memtime()
#endif

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// waves per SIMD the register allocator must leave room for: as many workgroups as the LDS ring lets a CU hold
constexpr int gemm_min_waves(int BM, int BN, int WM, int WN, int S, int KS) {
    int blocks = 163840 / (KS * S * (BM + BN) * 128 + 256);
    if (blocks < 1) blocks = 1;
    int w = blocks * WM * WN * KS / 4;
    return w < 1 ? 1 : (w > 6 ? 6 : w);
}

// KS > 1 (experimental, tile 7 only; NOT selected by any heuristic or autotune list until it has been validated and measured on
// hardware): KS groups of WM x WN waves share one output tile and take alternate K steps from their own LDS rings; the partial
// accumulators are exchanged through LDS after the loop (group g keeps row block i == g) and each group runs the epilogue of its
// row block.  Meant for the M = 2048 shapes: 160 tiles of 128x128 on 256 CUs leave one 4-wave workgroup per CU, i.e. one wave per
// SIMD with nothing to overlap LDS / load-issue latency with; two groups double that and halve the serial K loop.
template <int BM, int BN, int WM, int WN, int S, bool CONV, bool TRANS, int KS = 1>
__global__ __launch_bounds__(64 * WM * WN * KS, gemm_min_waves(BM, BN, WM, WN, S, KS)) void gemm_bf16_kernel(const GemmArgs p) {
#include "gemm_bf16_body.inc"
}

// The same tile with alpha loaded from a 4-byte device cell when the kernel runs (the ZeroCrossAttn output projection under a dynamic
// control scale, SUPIR_v0.py:138-152 with the per-step scale of sampling.py:557-559): one captured graph serves every step.  Same body,
// same arithmetic (t *= alpha before the residual).
template <int BM, int BN, int WM, int WN, int S>
__global__ __launch_bounds__(64 * WM * WN, gemm_min_waves(BM, BN, WM, WN, S, 1)) void gemm_bf16_alpha_kernel(const GemmArgs p_in,
                                                                                                         const float* __restrict__ alpha_cell) {
    constexpr bool CONV = false, TRANS = false;
    constexpr int KS = 1;
    GemmArgs p = p_in;
    p.alpha = *alpha_cell;
#include "gemm_bf16_body.inc"
}

static bool xcd_grid_enabled() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("SUPIR_XCD_GRID");
        v = (e && e[0] == '0') ? 0 : 1;
    }
    return v == 1;
}

// Choose the XCD partition for a tiles_m x tiles_n grid (see the kernel comment): a gm x gn grid of XCD regions and the tile
// order inside a region, minimising the bytes the eight private L2s have to pull in over the fabric.  Model (checked against
// rocprofv3 FETCH_SIZE, profiles/r02/pmc_summary.json): an XCD runs `slots` = 32 CUs x wgs_per_cu workgroups at a time; within one
// round the co-resident workgroups stream their operand panels through the L2 together, so each panel is fetched once.  What is
// re-fetched: (a) an operand that is swept more than once -- the implicit-GEMM input is read once per tap (resweep = 9) -- unless
// the XCD's share of it stays resident (<= ~3 MB of the 4 MB L2); (b) with several rounds per XCD, the operand that every round
// needs again, unless it fits beside the other round's band.  The first version of this model charged gn*A + gm*W only: it put the
// 1280-channel 32x32 convolutions on a (1, 8) grid whose 5.2 MB activation map does not stay resident -- 389 MB fetched for 35 MB
// of operands (11x), 4.5 TB/s of fabric traffic in an "MFMA-bound" kernel.
void supir_choose_xcd_grid(GemmArgs& a, int tiles_m, int tiles_n, double a_bytes, double w_bytes, int resweep, int wgs_per_cu, int nx) {
    a.gm = a.gn = 0;
    if (!xcd_grid_enabled() || ((tiles_m * tiles_n) % nx)) return;
    static int model = -1;
    if (model < 0) {
        const char* e = getenv("SUPIR_XCD_MODEL");   // 0: the round-1 cost model (kept for A/B runs)
        model = (e && e[0] == '0') ? 0 : 1;
    }
    const double c_bytes = 2.0 * (double)a.M * a.N / (double)nx;   // each XCD also write-allocates its share of the output
    const double RES = 3.0e6, BOTH = 3.5e6;
    const int slots = 32 * (wgs_per_cu < 1 ? 1 : wgs_per_cu);
    double best = 0.0;
    for (int gm = nx; gm >= 1; gm >>= 1) {
        const int gn = nx / gm;
        if (tiles_m % gm || tiles_n % gn) continue;
        if (model == 0) {
            double cost = gn * a_bytes + gm * w_bytes;
            if (a_bytes / gm + w_bytes / gn + c_bytes > 3.3e6) cost *= 1.5;
            if (a.gm == 0 || cost < best) {
                best = cost;
                a.gm = gm;
                a.gn = gn;
                a.order = (a_bytes / gm > w_bytes / gn) ? 1 : 0;
            }
            continue;
        }
        const double ax = a_bytes / gm, wx = w_bytes / gn;
        const int n_wg = (tiles_m / gm) * (tiles_n / gn);
        const int rounds = (n_wg + slots - 1) / slots;
        for (int order = 0; order < 2; ++order) {
            double at, wt;
            if (rounds == 1) {
                at = ax <= RES ? ax : resweep * ax;
                wt = wx;
            } else if (order == 1) {   // tile_n fastest: a round = a band of tile rows x all tile columns of the region
                const double band_a = ax / rounds;
                at = band_a <= RES ? ax : resweep * ax;
                wt = (wx + band_a <= BOTH) ? wx : rounds * wx;
            } else {                   // tile_m fastest: a round = all tile rows x a band of tile columns
                const double band_w = wx / rounds;
                wt = wx;
                at = (ax + band_w <= BOTH) ? ax : rounds * (ax <= RES ? ax : resweep * ax);
            }
            const double cost = at + wt;
            if (a.gm == 0 || cost < best) {
                best = cost;
                a.gm = gm;
                a.gn = gn;
                a.order = order;
            }
            if (rounds == 1) break;   // order is irrelevant inside a single round: keep 0
        }
    }
}

template <int BM, int BN, int WM, int WN, int S, bool CONV, bool TRANS, int KS = 1>
static int launch_gemm(const GemmArgs& a_in, hipStream_t st, const float* alpha_cell = nullptr) {
    GemmArgs a = a_in;
    {
        const double a_bytes = CONV ? 2.0 * (double)a.M * (a.up ? 0.25 : (double)(a.stride * a.stride)) * a.Cin
                                    : 2.0 * (double)a.M * a.K;
        constexpr int lds = KS * S * (BM + BN) * 128 + 256;
        supir_choose_xcd_grid(a, (a.M + BM - 1) / BM, (a.N + BN - 1) / BN, a_bytes, 2.0 * (double)a.N * a.K, CONV ? 9 : 1, 163840 / lds);
    }
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * (a.ksplit > 1 ? a.ksplit : 1);
    constexpr int smem = KS * S * (BM + BN) * 128 + 256;   // ring(s) + the prefetch scratch row
    if (alpha_cell) {   // dynamic alpha: plain GEMM forms only
        if constexpr (!CONV && !TRANS && KS == 1) {
            auto kern = gemm_bf16_alpha_kernel<BM, BN, WM, WN, S>;
            static bool attr_set = false;
            if (!attr_set) {
                if (supir_note_hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)) != SUPIR_OK) return SUPIR_ERR_HIP;
                attr_set = true;
            }
            SUPIR_LAUNCH(kern, dim3(tiles), dim3(64 * WM * WN), smem, st, a, alpha_cell);
            return SUPIR_LAUNCH_STATUS();
        } else {
            return SUPIR_ERR_SHAPE;
        }
    }
    auto kern = gemm_bf16_kernel<BM, BN, WM, WN, S, CONV, TRANS, KS>;
    static bool attr_set = false;
    if (!attr_set) {
        if (supir_note_hip_status(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem)) != SUPIR_OK) return SUPIR_ERR_HIP;
        attr_set = true;
    }
    SUPIR_LAUNCH(kern, dim3(tiles), dim3(64 * WM * WN * KS), smem, st, a);
    return SUPIR_LAUNCH_STATUS();
}

// Tile table (index -> block tile, wave grid, per-wave tile):
//   0: 128x128 2x2 (64x64)   1: 128x64 2x2 (64x32)   2: 64x128 2x2 (32x64)   3: 64x64 2x2 (32x32)
//   4: 256x128 4x2 (64x64, 512 threads)   5: 256x256 2x4 (128x64, 512 threads)   6: 256x128 2x2 (128x64)
//   7: 128x128 2x2 x 2 K groups (512 threads; experimental -- see the kernel comment; never chosen automatically)
// Heuristic default: biggest of tiles 0-3 that still yields >= ~1 wave of workgroups over 256 CUs; the Python layer
// autotunes over the whole table per problem shape.
int supir_gemm_select_tile(int M, int N, int act, int force_tile) {
    auto tiles = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    int sel = force_tile;
    if (act == 2 && (sel == 1 || sel == 3)) sel = -1;  // GEGLU needs 64 columns per wave (value + gate fragment pair)
    if (sel < 0 && act == 2) sel = (tiles(128, 128) >= 200) ? 0 : 2;
    if (sel < 0) {
        if (tiles(128, 128) >= 240) sel = 0;
        else if (N % 128 != 0 && tiles(128, 64) >= 200) sel = 1;
        else if (tiles(128, 64) >= 240) sel = 1;
        else if (tiles(64, 128) >= 240) sel = 2;
        else sel = 3;
    }
    return sel;
}

// `force_tile`: -1 auto; otherwise bits 0-2 = tile index (table above), bits 3-4 = LDS ring depth override
// (0 default, 1 -> 2 stages, 2 -> 3, 3 -> 4) -- the override exists for tools/bench_kernels.py's sweeps.
template <bool CONV, bool TRANS>
static int dispatch_gemm(const GemmArgs& a, hipStream_t st, int force_tile, const float* alpha_cell = nullptr) {
    const int sel = supir_gemm_select_tile(a.M, a.N, a.act, force_tile < 0 ? -1 : (force_tile & 7));
    int stages = force_tile < 0 ? 0 : ((force_tile >> 3) & 3);
    if (stages == 0) stages = SUPIR_DEFAULT_STAGES_CODE;
    stages += 1;
    if ((a.K >> 6) < 3 && stages > 2) stages = 2;
#define SUPIR_GEMM_CASE(BM_, BN_, WM_, WN_)                                        \
    switch (stages) {                                                              \
        case 2: return launch_gemm<BM_, BN_, WM_, WN_, 2, CONV, TRANS>(a, st, alpha_cell);     \
        default: return launch_gemm<BM_, BN_, WM_, WN_, 3, CONV, TRANS>(a, st, alpha_cell);    \
    }
    switch (sel) {
        case 0: SUPIR_GEMM_CASE(128, 128, 2, 2)
        case 1: SUPIR_GEMM_CASE(128, 64, 2, 2)
        case 2: SUPIR_GEMM_CASE(64, 128, 2, 2)
        case 3: SUPIR_GEMM_CASE(64, 64, 2, 2)
        case 4: return launch_gemm<256, 128, 4, 2, 2, CONV, TRANS>(a, st, alpha_cell);
        case 5: return launch_gemm<256, 256, 2, 4, 2, CONV, TRANS>(a, st, alpha_cell);
        case 6: return launch_gemm<256, 128, 2, 2, 2, CONV, TRANS>(a, st, alpha_cell);
        default:
            if (alpha_cell) return SUPIR_ERR_SHAPE;   // (tile 7 has no dynamic-alpha form)
            // tile 7 (experimental, explicit request only): 128x128 with two K groups; plain / transposed GEMM with K % 128 == 0,
            // else tile 0
            if constexpr (!CONV) {
                if (a.K % 128 == 0 && a.act != 2) return launch_gemm<128, 128, 2, 2, 2, false, TRANS, 2>(a, st);
            }
            SUPIR_GEMM_CASE(128, 128, 2, 2)
    }
#undef SUPIR_GEMM_CASE
}

// split-K finalize: out[m][n] = act(sum_s part[s][m][n] + bias[n]) in bf16; the partials are summed in split order (deterministic)
__global__ __launch_bounds__(256) void splitk_finalize_kernel(const float* __restrict__ part, int ksplit, int M, int N, int ld_part,
                                                              const float* __restrict__ bias, int act, bf16_t* __restrict__ out, int ldo) {
    const int nv = N >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * nv) return;
    const int m = (int)(idx / nv), n = (int)(idx - (long)m * nv) * 4;
    f32x4 acc = *(const f32x4*)(part + (size_t)m * ld_part + n);
    for (int s = 1; s < ksplit; ++s) {
        const f32x4 v = *(const f32x4*)(part + ((size_t)s * M + m) * ld_part + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
    }
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = acc[e] + (bias ? bias[n + e] : 0.f);
        if (act == 1) t = silu_f(t);
        y[e] = t;
    }
    const u32x2 o = {f2bf_pk(y[0], y[1]), f2bf_pk(y[2], y[3])};
    supir_store8(out + (size_t)m * ldo + n, o);
}

int supir_splitk_finalize_launch(const float* part, int ksplit, int M, int N, int ld_part, const float* bias, int act, bf16_t* out, int ldo,
                                 hipStream_t st) {
    if (ksplit < 1 || M <= 0 || N <= 0 || N % 4 || ld_part % 4 || ldo % 4 || act < 0 || act > 1) return SUPIR_ERR_SHAPE;
    const long total = (long)M * (N / 4);
    SUPIR_LAUNCH(splitk_finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, ksplit, M, N, ld_part, bias, act, out, ldo);
    return SUPIR_LAUNCH_STATUS();
}

// (sum, sum of squares) partials [M][ld][2] -> (mean, rstd) [M][2]; one thread per row, fixed summation order
__global__ __launch_bounds__(256) void rowstats_finalize_kernel(const float* __restrict__ part, float* __restrict__ out, int M,
                                                                int ld, int slots, int dim, float eps) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float* st = part + (size_t)m * ld * 2;
    float sm = 0.f, sq = 0.f;
    int sl = 0;
    for (; sl + 4 <= slots; sl += 4) {
        const f32x4 u = *(const f32x4*)(st + 2 * sl), v = *(const f32x4*)(st + 2 * sl + 4);
        sm += (u[0] + u[2]) + (v[0] + v[2]);
        sq += (u[1] + u[3]) + (v[1] + v[3]);
    }
    for (; sl < slots; ++sl) {
        sm += st[2 * sl];
        sq += st[2 * sl + 1];
    }
    const float inv = 1.0f / (float)dim;
    const float mean = sm * inv;
    float var = sq * inv - mean * mean;
    var = var > 0.f ? var : 0.f;
    out[(size_t)m * 2] = mean;
    out[(size_t)m * 2 + 1] = rsqrtf(var + eps);
}

int supir_rowstats_finalize_launch(const float* part, float* out, int M, int ld, int slots, int dim, float eps, hipStream_t st) {
    if (M <= 0 || slots <= 0 || ld < slots || (ld & 1) || dim <= 0) return SUPIR_ERR_SHAPE;
    SUPIR_LAUNCH(rowstats_finalize_kernel, dim3((M + 255) / 256), dim3(256), 0, st, part, out, M, ld, slots, dim, eps);
    return SUPIR_LAUNCH_STATUS();
}

int supir_gemm_launch(const GemmArgs& a_in, bool conv, hipStream_t st, int force_tile, const float* alpha_cell) {
    GemmArgs a = a_in;
    {
        // bytes each operand costs in L2 fills under the two orders (8 XCDs, each with a private L2)
        const double a_bytes = conv ? 2.0 * (double)a.M * (a.up ? 0.25 : (double)(a.stride * a.stride)) * a.Cin : 2.0 * (double)a.M * a.K;
        const double w_bytes = 2.0 * (double)a.N * a.K;
        const int tm = (a.M + 127) / 128, tn = (a.N + 127) / 128;
        const double cost_m_fast = a_bytes * (tn < 8 ? tn : 8) + w_bytes;
        const double cost_n_fast = w_bytes * (tm < 8 ? tm : 8) + a_bytes;
        a.order = cost_n_fast < cost_m_fast ? 1 : 0;
    }
    if (a.M <= 0 || a.N <= 0 || a.K <= 0) return SUPIR_ERR_ARG;
    if (a.ksplit > 1) {   // split-K: fp32 partials from the gemm.hip tiles 0..3 only, no epilogue terms, whole K steps per split
        if (force_tile < 0 || force_tile > 3 || a.out_mode != 1 || a.bias || a.res || a.rowbias || a.act != 0 || a.alpha != 1.0f ||
            a.rowstats_out || a.ln_stats || a.gn_part_out || a.K % (64 * a.ksplit) != 0)
            return SUPIR_ERR_SHAPE;
    }
    if (a.gn_part_out && ((force_tile < 32 || force_tile > 35) && (force_tile < 38 || force_tile > 40) && force_tile != 42 && force_tile != 45 && (force_tile < 48 || force_tile > 51))) return SUPIR_ERR_SHAPE;   // GroupNorm partials: gemm16 epilogues only
    if (alpha_cell && (conv || a.out_mode != 0 || a.ksplit > 1 || force_tile == 37 || force_tile > 35 || (force_tile >= 0 && force_tile < 32 && (force_tile & 7) == 7))) return SUPIR_ERR_SHAPE;
    if (force_tile == 37) return conv ? SUPIR_ERR_SHAPE : supir_gemm_big_launch(a, st);   // 256 x 320 GEGLU tile (gemm_big.hip)
    if (force_tile >= 32) {   // the 16x16x32-MFMA, 256-workgroup tiles (gemm16.hip): exact shapes only
        return supir_gemm16_launch(a, st, force_tile, conv, alpha_cell);
    }
    if (a.K % 64 != 0 || a.N % 4 != 0 || a.lda % 8 != 0) return SUPIR_ERR_SHAPE;
    if (conv && (a.Cin % 64 != 0 || a.K != 9 * a.Cin)) return SUPIR_ERR_SHAPE;
    if (a.act == 2 && (a.N % 128 != 0 || a.out_mode != 0 || a.res || a.rowbias)) return SUPIR_ERR_SHAPE;
    if (a.out_mode == 2) {
        if (a.act != 0 || a.res || a.rowbias) return SUPIR_ERR_SHAPE;
        return conv ? SUPIR_ERR_SHAPE : dispatch_gemm<false, true>(a, st, force_tile);
    }
    return conv ? dispatch_gemm<true, false>(a, st, force_tile) : dispatch_gemm<false, false>(a, st, force_tile, alpha_cell);
}
