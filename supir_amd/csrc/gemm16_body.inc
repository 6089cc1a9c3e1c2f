// Body of the gemm16.hip tile kernel (gemm16_kernel and its dynamic-alpha form gemm16_alpha_kernel).
// In scope: BM, BN, WM, WN, KS, S, TRANS, CONV, MIXED, NP, HW_ and pp (GemmArgsN<NP>).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NX = 8 / NP;                                               // XCDs per problem
    const int prob = NP == 1 ? 0 : (int)(blockIdx.x & 7) / NX;               // wave-uniform: a scalar offset into the kernarg segment
    const GemmArgs& p = pp.p[prob];
    const int vxcd = (int)blockIdx.x & (NX - 1), vidx = (int)blockIdx.x >> 3;   // XCD inside the problem's share, index on that XCD
    G16_TL(tl_start);
    constexpr int NW = WM * WN;                          // waves per K group
    constexpr bool PH8 = S == 8;                         // the eight-phase schedule (tile 42): S names the schedule, the ring is 2 deep
    constexpr int SD = PH8 ? 2 : S;
    constexpr bool HALO = HW_ > 0;
    static_assert(!HALO || (CONV && S != 8 && !MIXED && !TRANS && NP == 1 && BM % HW_ == 0 && HW_ % 16 == 0 && WM * WN * KS == 8), "halo form");
    constexpr int H_ROWS = HALO ? BM / HW_ : 1;          // output rows of the map per tile
    constexpr int H_RS = HW_ + 2;                        // halo row stride in pixels
    constexpr int H_PIX = (H_ROWS + 2) * H_RS;
    constexpr int H_PIECES = (H_PIX + 7) / 8;            // 8-pixel (1 KB) pieces of one halo tile
    constexpr int H_BYTES = H_PIECES * 1024;
    constexpr int H_PQ = (H_PIECES + 7) / 8;             // pieces per wave (piece id = wave + 8 q, all eight waves of the workgroup)
    constexpr int H_NLI_MAX = KS == 2 ? (S == 3 ? 3 : 4) : (S == 3 ? 7 : 8);   // iterations between "chunk c's buffer is free" and "chunk c + 2's data must be covered by the wait"
    constexpr int H_HQ = (H_PQ + H_NLI_MAX - 1) / H_NLI_MAX;                   // pieces per wave and load iteration
    constexpr int H_NLI = (H_PQ + H_HQ - 1) / H_HQ;                            // load iterations per halo tile
    static_assert(!HALO || H_HQ <= 2, "halo pieces per iteration: the counted wait has three variants");
    constexpr int A_BYTES = HALO ? 0 : BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES, RING = SD * STAGE_BYTES;
    constexpr int H_OFF = KS * RING;                     // LDS: [ring of group 0 | ring of group 1 | halo 0 | halo 1]
    constexpr int A_Q = HALO ? 0 : BM / 8 / NW;          // 8-row chunks of A per wave and K step (chunk id = wave + NW q)
    constexpr int B_CH = BN / 8, B_Q = (B_CH + NW - 1) / NW;   // chunks of W per tile / per wave (the last q may be partial)
    constexpr int LOADS = A_Q + B_Q;                     // global->LDS instructions per wave and stage
    constexpr int WTM = BM / WM, WTN = BN / WN, MI = WTM / 16, NI = WTN / 16, MIH = MI / KS;
    constexpr int NWT = NW * KS, NTHREADS = 64 * NWT;   // waves / threads per workgroup (8 / 512; tile 38: 4 / 256)
    static_assert((NWT == 8 || (NWT == 4 && KS == 1 && !MIXED && NP == 1)) && (BM / 8) % NW == 0 && (NW & 1) == 0,
                  "512 threads (or the four-wave single-group form); A chunks divide over the waves");
    static_assert(MI >= KS && MI % KS == 0 && WTN % 16 == 0 && (KS == 1 || KS == 2) && (S == 2 || S == 3 || S == 8), "tile / wave grid");
    // eight-phase schedule: 256 token rows, 8 waves; the wave tile's MI token fragments split into two halves, its NI channel fragments
    // into NA + NB parts.  Shipped: 256 x 256 as 2 x 4 waves (128 x 64 per wave, 2 + 2 fragments: tile 42).  The same code was measured
    // as 256 x 160 (4 x 2 waves, 3 + 2) and as 256 x 320 for the GEGLU projections (4 x 2, 5 + 5): bitwise the one-barrier tiles' results,
    // 5-10 % slower than tile 34 resp. equal to tile 37 -- phases of 8-12 MFMAs are too short for two barriers each, and 216 live registers
    // spill (profiles/r05/experiment_*); those instantiations are not built
    static_assert(!PH8 || ((BM == 256 || BM == 512) && KS == 1 && !TRANS && NP == 1 && NWT == 8 && (MI & 1) == 0 && NI >= 2 && (!MIXED || !CONV)), "eight-phase schedule");
    constexpr int PH_HR = WTM / 2;                       // token rows of one wave in an A half-tile
    constexpr int PH_AI = MI / 2;                        // token fragments per A half
    constexpr int PH_NA = (NI + 1) / 2, PH_NB = NI - PH_NA;   // channel fragments per wave in W part 0 / part 1
    constexpr int PH_WA_ROWS = WN * PH_NA * 16, PH_WB_ROWS = WN * PH_NB * 16;
    constexpr int PH_WA_CH = PH_WA_ROWS / 8, PH_WB_CH = PH_WB_ROWS / 8;          // 8-row chunks per W part
    constexpr int PH_WA_Q = (PH_WA_CH + 7) / 8, PH_WB_Q = (PH_WB_CH + 7) / 8;    // global -> LDS instructions per wave (the last may repeat chunk `wave`)
    constexpr int PH_A_HALF = BM * 64;                   // bytes of one A half-tile (BM / 2 rows of 128 B): 16 KB, 32 KB for the 512-row tile
    constexpr int PH_A_Q = BM / 128;                     // global -> LDS instructions per wave and A half-tile (8-row chunks wave + 8 q)
    constexpr int PH_OFF_W = 2 * PH_A_HALF, PH_OFF_WB = PH_OFF_W + PH_WA_ROWS * 128;   // LDS map of a K-tile buffer: [A0 | A1 | WA | WB]
    constexpr int PH_INFLIGHT = PH_A_Q + PH_WB_Q + PH_A_Q;   // loads per wave behind W part 0 of the next K-tile: A0, WB, A1 of the one after
    static_assert(!PH8 || (PH_WA_CH <= 24 && PH_WB_CH <= 24 && (PH_HR == 64 || (PH_HR == 32 && BM == 256)) && PH_OFF_WB + PH_WB_ROWS * 128 == STAGE_BYTES), "half-tile map");
    static_assert(!(CONV && TRANS) && !(MIXED && (TRANS || CONV || KS != 1)), "the implicit-GEMM loader has no transposed epilogue");
    // epilogue LDS map (the rings are idle by then): [0, XCH) K-group exchange, then per-wave C staging, bias / column sums,
    // row-statistics scratch
    constexpr int XCH_HALF = KS == 2 ? NW * MIH * NI * 4 * 64 * 4 : 0;   // bytes one group sends
    constexpr int XCH = 2 * XCH_HALF;
    constexpr int C_RS = WTN * 2 + 16;                         // staged row stride (bytes): 16-byte pad against bank conflicts
    constexpr int C_STAGE = 16 * C_RS;                         // one 16-token block per wave
    constexpr int OFF_CST = XCH, OFF_BIAS = OFF_CST + NWT * C_STAGE, OFF_RED = OFF_BIAS + 2 * BN * 4;
    constexpr int OFF_GN = OFF_RED + WN * BM * 8;               // GroupNorm column partials: [wave 0..NWT-1][WTN][2] fp32
    static_assert(OFF_GN + NWT * WTN * 8 <= KS * RING + (HALO ? 2 * H_BYTES : 0) - (PH8 ? 256 : 0), "epilogue scratch must fit the LDS rings");

    // wave-uniform ids as scalars (readfirstlane): LDS destinations / branches on them stay on the scalar unit
    const int bwave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // wave inside the workgroup, 0..7
    const int kg = KS == 2 ? bwave >> 2 : 0;           // K group
    const int wave = KS == 2 ? bwave & 3 : bwave;      // wave inside the group
    const int lane = (int)threadIdx.x & 63;
    const int tid = wave * 64 + lane;                  // thread inside the group
    const int wm = wave / WN, wn = wave % WN;
    const int quad = lane >> 4, l15 = lane & 15;
    char* ring = smem + kg * RING;

    const int tiles_m = p.M / BM, tiles_n = p.N / BN;
    int tile_m, tile_n;
    if (p.gm > 0) {   // 2-D XCD grid, see gemm.hip
        const int xcd = vxcd, idx = vidx;
        const int rm = tiles_m / p.gm, rn = tiles_n / p.gn;
        const int xm = xcd / p.gn, xn = xcd - xm * p.gn;
        int lm, ln;
        if (p.order == 0) { ln = idx / rm; lm = idx - ln * rm; }
        else { lm = idx / rn; ln = idx - lm * rn; }
        tile_m = xm * rm + lm;
        tile_n = xn * rn + ln;
    } else {
        // 1-D ranges: every XCD of the problem's share gets a contiguous run of tile ids (grouped launches: tiles % NX == 0)
        const int id = NP == 1 ? xcd_remap(blockIdx.x, tiles_m * tiles_n) : vxcd * (tiles_m * tiles_n / NX) + vidx;
        if (p.order == 0) { tile_n = id / tiles_m; tile_m = id - tile_n * tiles_m; }
        else { tile_m = id / tiles_n; tile_n = id - tile_m * tiles_n; }
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const bool tr = MIXED ? (n0 >= p.n_split) : TRANS;   // this workgroup's epilogue (wave-uniform)

    // ---- loader: wave w stages the 8-row chunks w, w+NW, w+2NW, ... of A and of W; lane -> row lane>>3, physical 16-B chunk lane&7.
    // NW is even, so the chunk ids of one wave all have the parity of w and the swizzle ((row >> 1) & 7 with row = 8*chunk + lane>>3)
    // is fixed per lane
    const int lrow = lane >> 3;
    const int lchunk = (lane & 7) ^ (((wave & 1) << 2) | (lane >> 4));
    const bf16_t* a_src = p.A + (size_t)(m0 + wave * 8 + lrow) * p.lda + lchunk * 8 + kg * 64;
    const bf16_t* b_src = p.Wt + (size_t)(n0 + wave * 8 + lrow) * p.K + lchunk * 8 + (HALO ? 0 : kg * 64);
    const size_t a_qstride = (size_t)(8 * NW) * p.lda, b_qstride = (size_t)(8 * NW) * p.K;
    // 3x3 convolution as implicit GEMM (same scheme as gemm.hip): K runs (ky, kx, cin) and a 64-wide K step never straddles a tap
    // (Cin % 64 == 0; Cin % 128 == 0 with two K groups); the gather address of each of this lane's A rows is computed once per
    // tap; halo / padding rows read the zero page; stride 2, asymmetric padding and nearest-2x upsampling fold into the gather
    int c_iy0[CONV && !HALO ? A_Q : 1], c_ix0[CONV && !HALO ? A_Q : 1];
    const bf16_t* c_base[CONV && !HALO ? A_Q : 1];
    const bf16_t* c_tap[CONV && !HALO ? A_Q : 1];
    int c_cin0 = kg * 64, c_ky = 0, c_kx = 0;
    const int VH = p.up ? 2 * p.H : p.H, VW = p.up ? 2 * p.W : p.W;
    // eight-phase schedule: a tile's 256 rows lie in ONE batch element (dispatcher), so the image base is wave-uniform and a lane keeps a
    // 32-bit element offset per row (< 0: halo / padding) instead of two pointers -- 10 VGPRs less in a kernel that sits at the 256 limit
    int ph8_toff[CONV && PH8 ? A_Q : 1];
    const bf16_t* ph8_cbase = nullptr;
    auto conv_set_tap = [&]() {
        if constexpr (CONV && !HALO) {
#pragma unroll
            for (int q = 0; q < A_Q; ++q) {
                int iy = c_iy0[q] + c_ky, ix = c_ix0[q] + c_kx;
                const bool ok = (unsigned)iy < (unsigned)VH && (unsigned)ix < (unsigned)VW;
                if (p.up) { iy >>= 1; ix >>= 1; }
                if constexpr (PH8) ph8_toff[q] = ok ? (iy * p.W + ix) * p.lda : -1;
                else c_tap[q] = ok ? c_base[q] + ((size_t)iy * p.W + ix) * p.lda : nullptr;
            }
        }
    };
    if constexpr (CONV && !HALO) {
#pragma unroll
        for (int q = 0; q < A_Q; ++q) {
            // eight-phase schedule: q = 2 h + qq is this lane's row of A-half h (token fragments [4h, 4h + 4) of both wave rows), wave row qq
            const int m = PH8 ? m0 + (q % PH_A_Q) * 128 + (q / PH_A_Q) * PH_HR + (PH_HR == 64 ? wave * 8 : (wave >> 2) * WTM + (wave & 3) * 8) + lrow
                              : m0 + (wave + NW * q) * 8 + lrow;
            const int b = m / p.rows_per_batch, r = m - b * p.rows_per_batch;
            const int oy = r / p.OW, ox = r - oy * p.OW;
            c_iy0[q] = oy * p.stride - p.pad_t;
            c_ix0[q] = ox * p.stride - p.pad_l;
            if constexpr (!PH8) c_base[q] = p.A + (size_t)b * p.H * p.W * p.lda + lchunk * 8;
        }
        if constexpr (PH8) ph8_cbase = p.A + (size_t)(m0 / p.rows_per_batch) * p.H * p.W * p.lda + lchunk * 8;
        conv_set_tap();
    }
    // ---- halo form: scalar (wave-uniform) state.  Step t of the (chunk, tap) sequence has chunk t / 9, tap t % 9, weight K offset
    // tap * Cin + chunk * 64; group g walks t = g, g + KS, ...  h_s*: the step whose W tile is staged next; h_r*: the step being read
    int h_stap = kg, h_schunk = 0, h_rtap = kg, h_rchunk = 0;
    int h_it = 0;                   // iteration (one step of each group) about to run
    int h_next = 2;                 // next chunk whose halo tile is loaded in the loop (0 and 1: prologue)
    int h_it0 = 8 / KS + 1;         // first load iteration of chunk h_next: the iteration after the last step of chunk h_next - 2, (9 c + 8) / KS + 1
    int h_cnt_prev = 0;             // halo pieces this wave issued in the previous iteration (the counted wait depends on it)
    const int h_nchunks = HALO ? p.Cin >> 6 : 0;
    int h_poff[HALO ? H_PQ : 1];    // per lane: element offset of its 16 bytes of piece (bwave + 8 q) inside the image, < 0: zero page
    int h_p0[HALO ? MI : 1];        // per lane: halo pixel index of token l15 of fragment i at tap (0, 0)
    const bf16_t* h_img = nullptr;
    if constexpr (HALO) {
        const int b = m0 / p.rows_per_batch, y0 = (m0 - b * p.rows_per_batch) / HW_;
        h_img = p.A + (size_t)b * p.H * p.W * p.lda;
        const int lg = (lane & 7) ^ (lane >> 3);     // logical chunk of this lane's slot: pixel P = 8 piece + (lane >> 3), so P & 7 = lane >> 3
#pragma unroll
        for (int q = 0; q < H_PQ; ++q) {
            const int P = (bwave + 8 * q) * 8 + (lane >> 3);
            const int hy = P / H_RS, hx = P - hy * H_RS;
            const int y = y0 - 1 + hy, x = hx - 1;
            const bool ok = P < H_PIX && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)HW_;
            h_poff[q] = ok ? (y * HW_ + x) * p.lda + lg * 8 : -1;
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int r = wm * WTM + i * 16;         // first token of the fragment inside the tile: 16 | W, so a fragment stays in one map row
            h_p0[i] = (r / HW_) * H_RS + (r % HW_) + l15;
        }
    }
    // pieces [q0, q1) of this wave's H_PQ (piece id bwave + 8 q), channel chunk `chunk`, into halo buffer chunk & 1; returns how many were
    // issued (wave-uniform).  Called with compile-time q0 / q1 only (fully unrolled), so h_poff stays in registers
    auto halo_issue = [&](int chunk, int q0, int q1) {
        int n = 0;
        if constexpr (HALO) {
            char* dst = smem + H_OFF + (chunk & 1) * H_BYTES + bwave * 1024;
            const bf16_t* base = h_img + chunk * 64;
#pragma unroll
            for (int q = 0; q < H_PQ; ++q) {
                if (q >= q0 && q < q1 && bwave + 8 * q < H_PIECES) {
                    const bf16_t* src = h_poff[q] >= 0 ? base + h_poff[q] : (const bf16_t*)g16_zero_page;
                    glds16(src, dst + q * 8192);
                    ++n;
                }
            }
        }
        return n;
    };
    // one global->LDS instruction: q < A_Q -> A chunk wave + NW q, else W chunk wave + NW (q - A_Q).  A wave whose last W chunk
    // would fall beyond the tile skips it when the ring is drained with vmcnt(0) (S == 2); with counted waits (S == 3) it re-loads
    // its first W chunk instead (same bytes to the same place), so that every wave has the same number of loads in flight
    auto stage_one = [&](int buf, int q) {
        char* sA = ring + buf * STAGE_BYTES;
        if (q < A_Q) {
            if constexpr (CONV) {
                const bf16_t* src = c_tap[q] ? c_tap[q] + c_cin0 : (const bf16_t*)g16_zero_page;
                glds16(src, sA + (wave + NW * q) * 1024);
            } else {
                glds16(a_src + q * a_qstride, sA + (wave + NW * q) * 1024);
            }
        } else {
            const int qb = q - A_Q;
            const bf16_t* bs = HALO ? b_src + (h_stap * p.Cin + h_schunk * 64) : b_src;
            if ((B_CH % NW == 0) || qb < B_Q - 1 || wave < (B_CH % NW))
                glds16(bs + qb * b_qstride, sA + A_BYTES + (wave + NW * qb) * 1024);
            else if (S > 2)
                glds16(bs, sA + A_BYTES + wave * 1024);
        }
    };
    auto stage_advance = [&]() {
        if constexpr (HALO) {
            h_stap += KS;
            if (h_stap >= 9) { h_stap -= 9; ++h_schunk; }
            return;
        }
        a_src += 64 * KS;
        b_src += 64 * KS;
        if constexpr (CONV) {
            c_cin0 += 64 * KS;
            if (c_cin0 >= p.Cin) {   // next tap (Cin % (64 KS) == 0: the K groups stay tap-aligned)
                c_cin0 -= p.Cin;
                if (++c_kx == 3) { c_kx = 0; ++c_ky; }
                conv_set_tap();
            }
        }
    };

    // epilogue vectors of this tile's BN columns, fetched now (one element per thread of group 0), parked in LDS after the loop
    float pre_bias = 0.f, pre_cs = 0.f;
    if constexpr (!TRANS) {
        if (kg == 0 && tid < BN && !tr) {
            if (p.bias) pre_bias = p.bias[n0 + tid];
            if (p.ln_stats) pre_cs = p.ln_colsum[n0 + tid];
        }
    }

    f32x4_t acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // fragment reads: row = base16 + l15, logical chunk 4*kk + quad, physical chunk ^ ((row >> 1) & 7) (bases are multiples of 16)
    const int sw = (l15 >> 1) & 7;
    const int a_row_off = (wm * WTM + l15) * 128;
    const int b_row_off = A_BYTES + (wn * WTN + l15) * 128;

    const int nk = (p.K >> 6) / KS;   // K steps of this group (>= S - 1: dispatcher; eight-phase schedule: >= 2)

    // ---- eight-phase schedule (tile 42): LDS = two K-tile buffers of four HALF-TILES [A0 | A1 | WA | WB].  A-half h holds token
    // fragments [h MI/2, (h + 1) MI/2) of EVERY wave row (local row wm * PH_HR + i * 16 + l15; 128 rows = 16 KB), W part 0 / 1 the first NA /
    // last NB channel fragments of every wave column (local row wn * N? * 16 + j * 16 + l15): a half-tile is what ONE phase's MFMAs newly
    // need, so it is free again a phase after it was read and its successor (K-tile + 2, same buffer) can be on its way seven phases
    // before it is needed.  A K-tile is four phases (256 x 256: AI = 4, NA = NB = 2; 256 x 160: AI = 2, NA = 3, NB = 2):
    //     phase  fragment reads (ds_read_b128)      MFMAs                               half-tile staged
    //       0    A0 (2 AI) + WA (2 NA)               A0 x WA   (2 AI NA)                 WA of K-tile u + 1
    //       1    WB (2 NB)                           A0 x WB   (2 AI NB)                 A0 of K-tile u + 2
    //       2    A1 (2 AI)                           A1 x WB                             WB of K-tile u + 2
    //       3    WA (2 NA, again)                    A1 x WA                             A1 of K-tile u + 2   + the K-tile's ONE counted wait
    // Each phase is [reads + loads + lgkmcnt(0)] s_barrier [MFMAs] s_barrier; waves 4-7 run ONE barrier behind waves 0-3, so on every
    // SIMD (one wave of each half) one wave is in its MFMA segment while the other reads fragments and issues loads.  Hazards (interval =
    // the time between two consecutive barriers; half g's phase p reads in interval 2p + g):
    //   WAR  a half-tile's last reads are complete (lgkmcnt(0)) before the barrier that ends their interval, for both wave halves by the
    //        end of interval 2p + 1; its successor is issued in phase p + 1 or later (interval >= 2p + 2);
    //   RAW  every wave waits vmcnt(PH_INFLIGHT) in the read segment of phase 3 (after issuing that phase's loads): everything up to WA of
    //        the NEXT K-tile -- the youngest half-tile it needs -- has landed, three half-tiles stay in flight; waves 4-7 execute that wait
    //        one interval later, i.e. before the barrier that ends interval 8u + 7, and the first read of K-tile u + 1 is in interval 8u + 8.
    // Every wave issues the same number of loads per half-tile (a W part with fewer than 16 chunks: the second instruction of the waves
    // beyond it re-loads their first chunk), so one count is right for all of them.
    int ph8_wt0 = 1, ph8_wt1 = 0, ph8_ka = 0;    // K-tile indices of the next WA / WB half-tiles to stage; K offset (elements) of the next A half-tiles
    // K-tile index -> K offset of the weight rows.  Convolutions, korder = 1 (round 5): the K loop runs (64-channel chunk, tap) instead
    // of (tap, chunk) -- the nine taps of one channel chunk back to back.  A tile's nine taps read three input rows shifted by a pixel:
    // tap-major, 32 workgroups of an XCD stream 32 x 262 KB through a 4 MB L2 between two taps of the same row and every tap re-fetches
    // it (512 -> 512 @ 256^2: 607 MB fetched for 139 MB of operands, profiles/pmc_traffic.json); chunk-major, a workgroup's nine taps
    // touch 3 rows x 258 px x 128 B = 99 KB, 3.2 MB per XCD
    auto ph8_koff = [&](int t) {
        if constexpr (CONV) {
            if (p.korder) {
                const int ch = t / 9, tap = t - ch * 9;
                return tap * p.Cin + ch * 64;
            }
        }
        return t * 64;
    };
    // addresses as (wave-uniform 64-bit base) + (per-lane 32-bit byte offset, constant over the loop): the loads take the scalar-base form
    // and the loop keeps ONE offset register per operand instead of a strength-reduced 64-bit pointer per load (10 loads = 20 VGPRs on
    // the 256 x 320 tile, which spilled)
    const char* ph8_a = nullptr;
    const char* ph8_w = nullptr;
    unsigned ph8_a_lane = 0, ph8_w_lane = 0;
    if constexpr (PH8) {
        ph8_a = (const char*)(p.A + (size_t)(m0 + (PH_HR == 64 ? wave * 8 : (wave >> 2) * WTM + (wave & 3) * 8)) * p.lda);
        ph8_w = (const char*)(p.Wt + (size_t)n0 * p.K);
        ph8_a_lane = (unsigned)(lrow * p.lda + lchunk * 8) * 2u;
        ph8_w_lane = (unsigned)(lrow * p.K + lchunk * 8) * 2u;
    }
    auto ph8_stage_a = [&](int buf, int h) {
        char* dst = smem + buf * STAGE_BYTES + h * PH_A_HALF + wave * 1024;
#pragma unroll
        for (int qq = 0; qq < PH_A_Q; ++qq) {
            if constexpr (CONV) {
                const int off = ph8_toff[PH_A_Q * h + qq];
                const bf16_t* src = off >= 0 ? ph8_cbase + (off + c_cin0) : (const bf16_t*)g16_zero_page;
                glds16(src, dst + qq * 8192);
            } else {
                glds16(ph8_a + ((size_t)(qq * 128 + h * PH_HR) * p.lda + ph8_ka) * 2 + ph8_a_lane, dst + qq * 8192);
            }
        }
    };
    // Advance the A stream to the next K-tile.  Convolutions: BRANCH-FREE (scalar selects for the tap / chunk state in either K order,
    // `&` and selects for the halo test) -- it is issued inside an MFMA segment (below), and a branch would split that segment's basic
    // block and put all of this in front of the MFMAs instead of beside them
    auto ph8_adv_a = [&]() {
        if constexpr (CONV) {
            const int ko = p.korder;
            // chunk-major: next tap; after the ninth, the next 64-channel chunk.  tap-major: next chunk; after the last, the next tap
            const int a_kx1 = c_kx + 1, a_w1 = a_kx1 == 3, a_ky1 = c_ky + a_w1, a_w2 = a_ky1 == 3;
            const int b_c1 = c_cin0 + 64, b_w0 = b_c1 >= p.Cin, b_kx1 = c_kx + b_w0, b_w1 = b_kx1 == 3;
            const int n_kx = ko ? (a_w1 ? 0 : a_kx1) : (b_w1 ? 0 : b_kx1);
            const int n_ky = ko ? (a_w2 ? 0 : a_ky1) : c_ky + b_w1;
            const int n_cin = ko ? c_cin0 + (a_w2 ? 64 : 0) : (b_w0 ? b_c1 - p.Cin : b_c1);
            c_kx = n_kx;
            c_ky = n_ky;
            c_cin0 = n_cin;
            const int sh = p.up ? 1 : 0;
            const unsigned wl = (unsigned)(p.W * p.lda);      // < 2^24 (dispatcher): the 24-bit multiplier is full rate, the 32-bit one is not
#pragma unroll
            for (int q = 0; q < A_Q; ++q) {
                const int iy = c_iy0[q] + c_ky, ix = c_ix0[q] + c_kx;
                const int ok = ((unsigned)iy < (unsigned)VH) & ((unsigned)ix < (unsigned)VW);
                const unsigned off = __umul24((unsigned)(iy >> sh), wl) + __umul24((unsigned)(ix >> sh), (unsigned)p.lda);
                ph8_toff[q] = ok ? (int)off : -1;
            }
        } else {
            ph8_ka += 64;
        }
    };
    // W part `part` (0: the first NA fragments of every wave column, 1: the last NB): chunk c = wave + 8 qq holds local rows 8c .. 8c + 7 =
    // wave column c / (2 N?) , rows (c % (2 N?)) * 8 ...; a chunk index beyond the part re-loads chunk `wave`
    auto ph8_stage_w = [&](int buf, auto part_c, int koff) {
        constexpr int PART = decltype(part_c)::value;
        constexpr int NF = PART ? PH_NB : PH_NA, CH = PART ? PH_WB_CH : PH_WA_CH, NQ = PART ? PH_WB_Q : PH_WA_Q;
        char* dst = smem + buf * STAGE_BYTES + (PART ? PH_OFF_WB : PH_OFF_W);
#pragma unroll
        for (int qq = 0; qq < NQ; ++qq) {
            int c = wave + 8 * qq;
            c = c < CH ? c : wave;
            const int chan = (c / (2 * NF)) * WTN + (PART ? PH_NA * 16 : 0) + (c % (2 * NF)) * 8;
            glds16(ph8_w + ((size_t)chan * p.K + koff) * 2 + ph8_w_lane, dst + c * 1024);
        }
    };
    using PI0 = std::integral_constant<int, 0>;
    using PI1 = std::integral_constant<int, 1>;
    if constexpr (PH8) {
        // K-tile 0 complete, A0 / WB / A1 of K-tile 1 behind it (its WA goes out in phase 0 of K-tile 0)
        ph8_stage_a(0, 0);
        ph8_stage_w(0, PI0{}, 0);
        ph8_stage_w(0, PI1{}, 0);
        ph8_stage_a(0, 1);
        ph8_adv_a();
        ph8_stage_a(1, 0);
        ph8_stage_w(1, PI1{}, ph8_koff(1));
        ph8_stage_a(1, 1);
        ph8_adv_a();
        ph8_wt1 = 2;
    } else {
        if constexpr (HALO) {   // the halo tiles of chunks 0 and 1 first: the first counted wait leaves only the youngest W stage in flight
            halo_issue(0, 0, H_PQ);
            if (h_nchunks > 1) halo_issue(1, 0, H_PQ);
        }
#pragma unroll
        for (int s = 0; s < S - 1; ++s) {
#pragma unroll
            for (int q = 0; q < LOADS; ++q) stage_one(s, q);
            stage_advance();
        }
    }

    // LayerNorm folding: mean / rstd of the token rows this wave finishes after the K-group exchange (token fragments
    // i = kg*MIH + h).  Fetched and reduced HERE, under the first tiles' load latency, not in the epilogue (a chain of dependent
    // L2 / fabric round trips there).  The four lanes that share a token (one per quad) take a contiguous quarter of the
    // producer's slots each -- all loads issued before the first use -- and combine by two xor shuffles (fixed order).
    float ln_mean[MIH], ln_rstd[MIH];
#pragma unroll
    for (int h = 0; h < MIH; ++h) {
        ln_mean[h] = 0.f;
        ln_rstd[h] = 1.f;
    }
    if (p.ln_stats) {
        const int spq = (p.ln_slots + 3) >> 2;            // slots per quad (<= 8: dispatcher)
        const int s_lo = quad * spq;
#pragma unroll
        for (int h = 0; h < MIH; ++h) {
            const int m = m0 + wm * WTM + (kg * MIH + h) * 16 + l15;
            if (p.ln_slots == 0) {
                const float* st2 = p.ln_stats + (size_t)m * 2;
                ln_mean[h] = st2[0];
                ln_rstd[h] = st2[1];
                continue;
            }
            const supir_f32x2* st = (const supir_f32x2*)(p.ln_stats + (size_t)m * p.ln_ld * 2);
            supir_f32x2 v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {                   // clamped index + zero weight instead of a branch around the load
                const int sl = s_lo + (e < spq ? e : spq - 1);   // beyond this quad's share: repeat its last slot (cache hit)
                v[e] = st[sl < p.ln_slots ? sl : p.ln_slots - 1];
            }
            float sm = 0.f, sq = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = e < spq && s_lo + e < p.ln_slots;
                sm += ok ? v[e][0] : 0.f;
                sq += ok ? v[e][1] : 0.f;
            }
            sm += __shfl_xor(sm, 16, 64);
            sq += __shfl_xor(sq, 16, 64);
            sm += __shfl_xor(sm, 32, 64);
            sq += __shfl_xor(sq, 32, 64);
            const float inv = 1.0f / (float)p.K;
            const float mean = sm * inv;
            float var = sq * inv - mean * mean;
            var = var > 0.f ? var : 0.f;
            ln_mean[h] = mean;
            ln_rstd[h] = rsqrtf(var + p.ln_eps);
        }
    }

    // Residual / row-bias operands of the epilogue (this lane's 4 channels of its token per fragment), fetched NOW: issued in the
    // epilogue they were a dependent L2 / fabric round trip (~0.5-1 us) at the very end of a 13 us launch.  In-place residuals
    // (x += f(x)) are safe: a workgroup reads its whole tile here, long before any of its stores, and tiles are disjoint.
    // (only where it is cheap in registers: 2 x MIH x NI x 2 VGPRs held across the main loop; the 256 x 160 tile would spill)
    constexpr bool PRE = !TRANS && MIH * NI <= 10;
    u32x2 pre_res[PRE ? MIH : 1][PRE ? NI : 1], pre_rb[PRE ? MIH : 1][PRE ? NI : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int h = 0; h < MIH; ++h)
#pragma unroll
            for (int j = 0; j < NI; ++j) pre_res[h][j] = pre_rb[h][j] = u32x2{0u, 0u};
        if (!tr && p.act != 2) {
#pragma unroll
            for (int h = 0; h < MIH; ++h) {
                const int m = m0 + wm * WTM + (kg * MIH + h) * 16 + l15;
                if (p.res) {
                    const bf16_t* rp = p.res + (size_t)m * p.ldr + n0 + wn * WTN + 4 * quad;
#pragma unroll
                    for (int j = 0; j < NI; ++j) pre_res[h][j] = *(const u32x2*)(rp + j * 16);
                }
                if (p.rowbias) {
                    const bf16_t* rbp = p.rowbias + (size_t)(m / p.rows_per_batch) * p.ld_rb + n0 + wn * WTN + 4 * quad;
#pragma unroll
                    for (int j = 0; j < NI; ++j) pre_rb[h][j] = *(const u32x2*)(rbp + j * 16);
                }
            }
        }
    }

#ifdef SUPIR_G16_ZSFT
    // ---- ZeroSFT epilogue (gemm16_zsft_kernel; zs = ZsftArgs): W rows interleaved [16 gamma | 16 beta], so this tile's BN columns are the
    // modulation maps of BN / 2 = 80 output channels [zs_c0, zs_c0 + 80) of ONE batch element.  GroupNorm statistics of that batch element
    // from the producers' partials, as gn_apply_body.inc reads them (10-channel units of the two concat sources, fp64 sums -- exact for
    // these counts, so the split over lanes does not show -- the same var >= 0 clamp and 1 / sqrt(var + eps)), reduced HERE, behind the
    // first stages' loads: wave w takes the w-th group the tile's channels touch (<= 8: groups are >= 10 channels wide), 32 lanes per
    // statistic over (tile row, unit), a fixed xor tree across them; then sa = rstd * gamma, sb = beta - mean * sa of the group's channels
    // inside the tile go to LDS beyond the rings.  Every load is consumed before the loop: its counted waits see only stage loads.
    static_assert(CONV && !HALO && !TRANS && !MIXED && NP == 1 && WN == 1 && BN == 160 && (NI & 1) == 0 && S != 8, "ZeroSFT epilogue: 160-column tiles, one wave column");
    constexpr int ZS_CH = BN / 2;
    constexpr int OFF_ZS = KS * RING + 256;        // [ZS_CH] sa | [ZS_CH] sb, behind the rings and the prefetch scratch row
    const int zs_c0 = n0 >> 1;
    const float zs_cs = zs.cscale_cell ? *zs.cscale_cell : zs.cscale;
    {
        const int zb = m0 / p.rows_per_batch;
        const int cpg = zs.C >> 5, upg = cpg / 10, U1 = zs.C1 / 10, U2 = (zs.C - zs.C1) / 10;
        const int g = zs_c0 / cpg + bwave;
        if (g * cpg < zs_c0 + ZS_CH) {               // wave-uniform
            const int st = lane & 1, l = lane >> 1;
            // the group's units [g upg, (g + 1) upg) of the concatenation: [a1, a1 + w1) of source 1, [a2, a2 + w2) of source 2
            const int u_lo = g * upg, u_hi = u_lo + upg;
            const int a1 = u_lo < U1 ? u_lo : U1, w1 = (u_hi < U1 ? u_hi : U1) - a1;
            const int a2 = (u_lo > U1 ? u_lo : U1) - U1, w2 = upg - w1;
            const int tot1 = w1 * zs.nch1, tot = tot1 + w2 * zs.nch2;
            double a = 0.0;
            for (int i0 = l; i0 < tot; i0 += 128) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {        // four independent loads in flight; beyond the end: a repeat of element 0, weight 0
                    const int idx = i0 + 32 * e;
                    const bool ok = idx < tot;
                    const int ii = ok ? idx : 0;
                    const bool first = ii < tot1;
                    const int j = first ? ii : ii - tot1, w = first ? w1 : w2;
                    const int k = j / w, u = (first ? a1 : a2) + (j - k * w);
                    const float* src = first ? zs.part_u1 : zs.part_u2;
                    const int nch = first ? zs.nch1 : zs.nch2, Un = first ? U1 : U2;
                    const float f = src[(((size_t)zb * nch + k) * Un + u) * 2 + st];
                    v[e] = ok ? f : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) a += (double)v[e];
            }
#pragma unroll
            for (int o = 2; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
            const double sum = __shfl(a, 0, 64), sq = __shfl(a, 1, 64);
            const double n = (double)p.rows_per_batch * (double)cpg;
            const double mean = sum / n;
            double var = sq / n - mean * mean;
            var = var > 0.0 ? var : 0.0;
            const float mean_f = (float)mean, rstd_f = (float)(1.0 / sqrt(var + (double)zs.eps));
            const int c_lo = g * cpg > zs_c0 ? g * cpg : zs_c0, c_hi = (g + 1) * cpg < zs_c0 + ZS_CH ? (g + 1) * cpg : zs_c0 + ZS_CH;
            float* s_sa = (float*)(smem + OFF_ZS);
            for (int c = c_lo + lane; c < c_hi; c += 64) {
                const float sa = rstd_f * zs.gamma[c];
                s_sa[c - zs_c0] = sa;
                s_sa[ZS_CH + c - zs_c0] = zs.beta[c] - mean_f * sa;
            }
        }
    }
#endif
    // one K step.  STAGE: also issue the global->LDS loads of tile kt + S - 1 (into the buffer step kt - 1 just finished reading),
    // spread over the two 32-wide K slices; INFLIGHT: younger stages that may stay outstanding across this step's barrier
    int buf = 0, sbuf = S - 1;   // ring positions of the tile being read / being staged (kept modulo S without a division)
#ifdef SUPIR_G16_TIMELINE
    unsigned long long tl_s0 = 0, tl_s1 = 0, tl_s2 = 0, tl_s3 = 0, tl_wait = 0, tl_bar = 0, tl_comp = 0;
#endif
    auto kstep = [&](auto stage_c, auto inflight_c, auto trans_c) {
        constexpr bool STAGE = decltype(stage_c)::value;
        constexpr int INFLIGHT = decltype(inflight_c)::value;
        constexpr bool TR = decltype(trans_c)::value;
        G16_TLS(tl_s0);
        if constexpr (HALO && INFLIGHT == 1) {   // the previous iteration's loads stay in flight: its W chunks + the halo pieces it issued
            if (h_cnt_prev == 0) g16_wait_vmcnt<LOADS>();
            else if (h_cnt_prev == 1) g16_wait_vmcnt<LOADS + 1>();
            else g16_wait_vmcnt<LOADS + 2>();
        } else {
            static_assert(!HALO || INFLIGHT == 0, "halo form: rings of depth 2 or 3");
            g16_wait_vmcnt<INFLIGHT * LOADS>();
        }
        G16_TLS(tl_s1);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        G16_TLS(tl_s2);
        const char* sT = ring + buf * STAGE_BYTES;
        // halo form: this step's tap shift inside the halo tile of its chunk
        const int h_ky = (h_rtap * 11) >> 5, h_toff = h_ky * H_RS + (h_rtap - 3 * h_ky);
        const char* h_buf = smem + H_OFF + (h_rchunk & 1) * H_BYTES;
        // both 32-wide K slices of fragments are read ahead of the MFMAs -- except where the accumulators already take half the
        // register file (256 x 256: MI * NI = 32 fragments = 128 registers; 96 more for two slices spilled): one slice at a time
        // there, the second one read behind the first slice's MFMAs (the SIMD's other wave covers the wait)
        constexpr bool ONE_SLICE = MI * NI >= 32;
        constexpr int FS = ONE_SLICE ? 1 : 2;
        bf16x8 af[FS][MI], bfr[FS][NI];
        auto read_frags = [&](int kk, int slot) {
            const int coff = ((4 * kk + quad) ^ sw) * 16;
            if constexpr (HALO) {
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int P = h_p0[i] + h_toff;
                    af[slot][i] = *(const bf16x8*)(h_buf + P * 128 + ((((4 * kk + quad) ^ P) & 7) << 4));
                }
            } else {
#pragma unroll
                for (int i = 0; i < MI; ++i) af[slot][i] = *(const bf16x8*)(sT + a_row_off + i * 16 * 128 + coff);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) bfr[slot][j] = *(const bf16x8*)(sT + b_row_off + j * 16 * 128 + coff);
        };
        read_frags(0, 0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int sl = ONE_SLICE ? 0 : kk;
            if (!ONE_SLICE && kk == 0) read_frags(1, 1);
            if constexpr (STAGE) {
#pragma unroll
                for (int q = (kk * LOADS) / 2; q < ((kk + 1) * LOADS) / 2; ++q) stage_one(sbuf, q);
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    if constexpr (TR)
                        acc[i][j] = SUPIR_MFMA_16x16x32(af[sl][i], bfr[sl][j], acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = SUPIR_MFMA_16x16x32(bfr[sl][j], af[sl][i], acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
            if (ONE_SLICE && kk == 0) read_frags(1, 0);
        }
        if constexpr (STAGE) stage_advance();
        if constexpr (HALO) {
            int cnt = 0;
            if constexpr (STAGE) {
                if (h_next < h_nchunks && h_it >= h_it0) {     // wave-uniform
                    const int j = h_it - h_it0;
#pragma unroll
                    for (int J = 0; J < H_NLI; ++J)
                        if (j == J) cnt = halo_issue(h_next, J * H_HQ, (J + 1) * H_HQ);
                    if (j == H_NLI - 1) {
                        ++h_next;
                        h_it0 = (9 * (h_next - 2) + 8) / KS + 1;
                    }
                }
            }
            h_cnt_prev = cnt;
            ++h_it;
            h_rtap += KS;
            if (h_rtap >= 9) { h_rtap -= 9; ++h_rchunk; }
        }
        buf = buf + 1 == S ? 0 : buf + 1;
        sbuf = sbuf + 1 == S ? 0 : sbuf + 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        G16_TLS(tl_s3);
        G16_TLACC(tl_wait, tl_s0, tl_s1);
        G16_TLACC(tl_bar, tl_s1, tl_s2);
        G16_TLACC(tl_comp, tl_s2, tl_s3);
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    G16_TL(tl_loop0);
    auto main_loop = [&](auto trans_c) {
        for (int kt = 0; kt + S - 1 < nk; ++kt) kstep(T_{}, std::integral_constant<int, S - 2>{}, trans_c);
        if constexpr (S == 3) kstep(F_{}, std::integral_constant<int, 1>{}, trans_c);
        kstep(F_{}, std::integral_constant<int, 0>{}, trans_c);
    };
    if constexpr (PH8) {
        const int fa_off = (wm * PH_HR + l15) * 128;
        const int fw_off0 = PH_OFF_W + (wn * PH_NA * 16 + l15) * 128, fw_off1 = PH_OFF_WB + (wn * PH_NB * 16 + l15) * 128;
        const int grp = bwave >> 2;     // waves 4-7 run one barrier behind waves 0-3 (wave w and w + 4 share a SIMD)
        int cur = 0;
        // one K-tile.  SW0: stage WA of the next K-tile (phase 0); SA: stage A0 / WB / A1 of the K-tile after it (phases 1 - 3);
        // WAITN: the counted wait of phase 3 (PH_INFLIGHT = three half-tiles stay in flight; 0 = the tail; -1 = nothing left to wait for);
        // TR: the transposed epilogue's operand order (fused q|k|v: the V^T column tiles)
        auto ph8_tile = [&](auto sw0_c, auto sa_c, auto wait_c, auto tr_c) {
            constexpr bool SW0 = decltype(sw0_c)::value, SA = decltype(sa_c)::value, TR = decltype(tr_c)::value;
            constexpr int WAITN = decltype(wait_c)::value;
            const char* sT = smem + cur * STAGE_BYTES;
            bf16x8 af[2][PH_AI], wf[2][PH_NA];
            auto read_a = [&](int h) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < PH_AI; ++i) af[kk][i] = *(const bf16x8*)(sT + h * PH_A_HALF + fa_off + i * 2048 + (((4 * kk + quad) ^ sw) * 16));
            };
            auto read_w = [&](auto part_c) {
                constexpr int PART = decltype(part_c)::value;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int j = 0; j < (PART ? PH_NB : PH_NA); ++j)
                        wf[kk][j] = *(const bf16x8*)(sT + (PART ? fw_off1 : fw_off0) + j * 2048 + (((4 * kk + quad) ^ sw) * 16));
            };
            auto mid = [&]() {     // end of a read segment: this wave's fragment reads are complete before anyone passes the barrier
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            };
            // shadow_c: the A stream's advance to the next K-tile (convolutions: the tap addresses of this lane's four rows, ~40 VALU
            // instructions -- every K-tile in the chunk-major order) issued INSIDE this MFMA segment, three VALU per MFMA: the matrix pipe
            // takes an instruction every ~16 cycles and the vector pipe is free beside it; in the read segment the same work held up
            // the barrier the partner wave's MFMAs wait behind (first version: -16 %, profiles/r05/experiment_tile42_conv_chunk_major_*)
            auto mma = [&](auto ah_c, auto part_c, auto shadow_c) {
                constexpr int AH = decltype(ah_c)::value, PART = decltype(part_c)::value;
                constexpr bool SHADOW = decltype(shadow_c)::value;
                __builtin_amdgcn_s_setprio(1);
                if constexpr (SHADOW) ph8_adv_a();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < PH_AI; ++i)
#pragma unroll
                        for (int j = 0; j < (PART ? PH_NB : PH_NA); ++j) {
                            f32x4_t& c = acc[AH * PH_AI + i][(PART ? PH_NA : 0) + j];
                            if constexpr (TR) c = SUPIR_MFMA_16x16x32(af[kk][i], wf[kk][j], c, 0, 0, 0);
                            else c = SUPIR_MFMA_16x16x32(wf[kk][j], af[kk][i], c, 0, 0, 0);
                        }
                if constexpr (SHADOW && CONV) {
#pragma unroll
                    for (int g = 0; g < 2 * PH_AI * (PART ? PH_NB : PH_NA); ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // one MFMA
                        __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);    // up to two SALU (the tap / chunk state) ...
                        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);    // ... and three VALU (the four rows' tap offsets) behind it
                    }
                }
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            };
            // phase 0
            read_w(PI0{});
            read_a(0);
            if constexpr (SW0) ph8_stage_w(cur ^ 1, PI0{}, ph8_koff(ph8_wt0));
            mid();
            mma(PI0{}, PI0{}, F_{});
            // phase 1
            read_w(PI1{});
            if constexpr (SA) ph8_stage_a(cur, 0);
            mid();
            mma(PI0{}, PI1{}, F_{});
            // phase 2
            read_a(1);
            if constexpr (SA) ph8_stage_w(cur, PI1{}, ph8_koff(ph8_wt1));
            mid();
            mma(PI1{}, PI1{}, F_{});
            // phase 3
            read_w(PI0{});
            if constexpr (SA) ph8_stage_a(cur, 1);
            if constexpr (WAITN >= 0) g16_wait_vmcnt<WAITN>();
            mid();
            mma(PI1{}, PI0{}, std::integral_constant<bool, SA>{});
            ++ph8_wt0;
            ++ph8_wt1;
            cur ^= 1;
        };
        g16_wait_vmcnt<PH_INFLIGHT>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (grp == 1) {      // the second wave half runs one barrier behind the first from here on
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
        using WF_ = std::integral_constant<int, PH_INFLIGHT>;
        using W0_ = std::integral_constant<int, 0>;
        using WN_ = std::integral_constant<int, -1>;
        auto ph8_loop = [&](auto tr_c) {
            for (int u = 0; u + 2 < nk; ++u) ph8_tile(T_{}, T_{}, WF_{}, tr_c);
            ph8_tile(T_{}, F_{}, W0_{}, tr_c);
            ph8_tile(F_{}, F_{}, WN_{}, tr_c);
        };
        if constexpr (MIXED) {
            if (tr) ph8_loop(T_{});
            else ph8_loop(F_{});
        } else {
            ph8_loop(F_{});
        }
        if (grp == 0) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
    } else if constexpr (MIXED) {
        if (tr) main_loop(T_{});
        else main_loop(F_{});
    } else {
        main_loop(std::integral_constant<bool, TRANS>{});
    }

    // ------------------------------------------------------------------ epilogue
    G16_TL(tl_loop1);
    // (Round 5 tried fetching the residual / row-bias operands of the large tiles AHEAD of their 16-token block -- all blocks at once on
    // 256 x 160, two in flight on 256 x 256: the per-wave epilogue fell from 14.3 k to 6.4 k cycles and the wait moved in front of the
    // barrier, 0.5 k -> 11 k cycles; launches +2..5 % slower.  256 workgroups pull 80 KB of residual and push 80 KB of output each in the
    // same few microseconds: the epilogue of the large tiles is THROUGHPUT-bound, not a chain of round trips.
    // profiles/r05/experiment_timeline_epilogue_prefetch_and_tile43.log)
    __syncthreads();   // every wave is done with its last fragment reads: the rings are scratch from here on
    if constexpr (!TRANS) {
        if (kg == 0 && tid < BN && !tr) {
            ((float*)(smem + OFF_BIAS))[tid] = pre_bias;
            ((float*)(smem + OFF_BIAS))[BN + tid] = pre_cs;
        }
    }
    if constexpr (KS == 2) {
        // reduce-scatter of the K partials: group g keeps token fragments [g*MIH, (g+1)*MIH) and adds the other group's partial.
        // layout [sender][wave][h][j][r][lane] fp32: lane-contiguous, conflict-free
        float* xch = (float*)smem;
        const int w_off = wave * (MIH * NI * 4 * 64) + lane;
        float* mine = xch + kg * (XCH_HALF / 4) + w_off;
        const float* theirs = xch + (1 - kg) * (XCH_HALF / 4) + w_off;
        if (kg == 0) {
#pragma unroll
            for (int h = 0; h < MIH; ++h)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mine[((h * NI + j) * 4 + r) * 64] = acc[MIH + h][j][r];
        } else {
#pragma unroll
            for (int h = 0; h < MIH; ++h)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mine[((h * NI + j) * 4 + r) * 64] = acc[h][j][r];
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int h = 0; h < MIH; ++h)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[h][j][r] += theirs[((h * NI + j) * 4 + r) * 64];
        } else {
#pragma unroll
            for (int h = 0; h < MIH; ++h)
#pragma unroll
                for (int j = 0; j < NI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[MIH + h][j][r] += theirs[((h * NI + j) * 4 + r) * 64];
        }
    } else {
        __syncthreads();   // bias / column sums are in LDS
    }
    G16_TL(tl_xch);
    // from here on the wave's data is acc[kg*MIH + h][j], h < MIH (compile-time indices in both wave-uniform branches)
    auto prefetch_next = [&]() {
        const unsigned pf_lines = p.pf_lines;
        if (pf_lines == 0) return;
        const unsigned total_waves = gridDim.x / NP * NWT, gw = (unsigned)(vidx * NX + vxcd) * NWT + bwave;   // per problem
        const unsigned n_instr = (pf_lines + 63) >> 6;
        for (unsigned i = gw; i < n_instr; i += total_waves) {
            unsigned line = i * 64 + lane;
            line = line < pf_lines ? line : pf_lines - 1;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.pf_ptr + (size_t)line * 128),
                                             (__attribute__((address_space(3))) void*)(smem + (PH8 ? RING - 256 : KS * RING + (HALO ? 2 * H_BYTES : 0))), 4, 0, 0);
        }
    };
    using K0_ = std::integral_constant<int, 0>;
    using K1_ = std::integral_constant<int, 1>;

    if constexpr (TRANS || MIXED) {
      if (tr) {
        // D[i = token][j = channel]: lane owns channel l15 of fragment j, tokens 4*quad + r of fragment i -> 4 consecutive tokens
        bf16_t* Cb = (bf16_t*)(MIXED ? p.C2 : p.C);
        const int ldc_t = MIXED ? p.ldc2 : p.ldc, n_base = MIXED ? p.n_split : 0, n_out_total = p.N - n_base;
        auto run = [&](auto kg_c) {
            constexpr int KG = decltype(kg_c)::value;
#pragma unroll
            for (int h = 0; h < MIH; ++h) {
                const int mb = m0 + wm * WTM + (KG * MIH + h) * 16 + 4 * quad;      // first of this lane's 4 tokens
                const int b = mb / p.rows_per_batch, t = mb - b * p.rows_per_batch;   // rows_per_batch % 4 == 0 (dispatcher)
                float mu[4], rs[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {   // statistics of token 4*quad + r live in the lanes with that l15
                    mu[r] = __shfl(ln_mean[h], 4 * quad + r, 64);
                    rs[r] = __shfl(ln_rstd[h], 4 * quad + r, 64);
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int n = n0 + wn * WTN + j * 16 + l15;
                    const float bz = p.bias ? p.bias[n] : 0.f;
                    const float cs = p.ln_stats ? p.ln_colsum[n] : 0.f;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = p.alpha * (rs[r] * (acc[KG * MIH + h][j][r] - mu[r] * cs) + bz);
                    const u32x2 o = {f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3])};
                    supir_store8(Cb + ((size_t)b * n_out_total + (n - n_base)) * ldc_t + t, o);
                }
            }
        };
        if (kg == 0) run(K0_{});
        else if constexpr (KS == 2) run(K1_{});
        prefetch_next();
        return;
      }
    }
    if constexpr (!TRANS) {
        const float* s_bias = (const float*)(smem + OFF_BIAS);
        const float* s_cs = s_bias + BN;
        char* c_stage = smem + OFF_CST + bwave * C_STAGE;
        // 16-byte pieces of a staged [16][COLS] bf16 block -> row-contiguous global stores
        auto flush_block = [&](int row_base, int col_base, auto cols_c) {
            constexpr int COLS = decltype(cols_c)::value;
            constexpr int PPR = COLS / 8, PIECES = 16 * PPR;
#pragma unroll
            for (int rr = 0; rr < (PIECES + 63) / 64; ++rr) {
                const int id = rr * 64 + lane;
                if (PIECES % 64 == 0 || id < PIECES) {
                    const int row = id / PPR, ch = id - row * PPR;
                    const f32x4 piece = *(const f32x4*)(c_stage + row * C_RS + ch * 16);
                    supir_store16((bf16_t*)p.C + (size_t)(row_base + row) * p.ldc + col_base + ch * 8, piece);
                }
            }
        };
#ifdef SUPIR_G16_ZSFT
        {
            // ZeroSFT: fragment pair (2 jp, 2 jp + 1) = (gamma, beta) map of 16 output channels, both rounded to the 16-bit element type as
            // the two-launch path stores them; out = (x sa + sb) (gamma + 1) + beta, lerp against the raw operand when the control scale is
            // not 1 -- the expressions of gn_apply_body.inc.  x comes from the concat source this tile's channels lie in (wave-uniform:
            // C1 % 80 == 0).  The 16 x 80 block is staged and stored like the GEGLU block; its column sums are the GroupNorm partials
            // of the OUTPUT for the consumer (10-channel units, the slot layout of the plain epilogue with N / 2 channels)
            const float* s_sa = (const float*)(smem + OFF_ZS);
            const float* s_sb = s_sa + ZS_CH;
            const bool zs_first = zs_c0 < zs.C1;
            const bf16_t* xs = zs_first ? zs.x1 : zs.x2;
            const bf16_t* xr = zs_first ? (zs.x1raw ? zs.x1raw : zs.x1) : (zs.x2raw ? zs.x2raw : zs.x2);
            const int zs_ld = zs_first ? zs.ld1 : zs.ld2, zs_cx = zs_first ? zs_c0 : zs_c0 - zs.C1;
            const bool lerp = zs_cs != 1.0f;
            auto run = [&](auto kg_c) {
                constexpr int KG = decltype(kg_c)::value;
                constexpr int GP = (ZS_CH + 63) / 64;
                float gsum[GP], gsq[GP];
#pragma unroll
                for (int g = 0; g < GP; ++g) gsum[g] = gsq[g] = 0.f;
#pragma unroll
                for (int h = 0; h < MIH; ++h) {
                    const int mrow = wm * WTM + (KG * MIH + h) * 16;
                    const size_t xo = (size_t)(m0 + mrow + l15) * zs_ld + zs_cx + 4 * quad;
                    u32x2 xv[NI / 2], rv[NI / 2];
#pragma unroll
                    for (int jp = 0; jp < NI / 2; ++jp) xv[jp] = rv[jp] = *(const u32x2*)(xs + xo + jp * 16);
                    if (lerp) {
#pragma unroll
                        for (int jp = 0; jp < NI / 2; ++jp) rv[jp] = *(const u32x2*)(xr + xo + jp * 16);
                    }
#pragma unroll
                    for (int jp = 0; jp < NI / 2; ++jp) {
                        const int nl = jp * 32 + 4 * quad, cl = jp * 16 + 4 * quad;
                        const f32x4 bg = *(const f32x4*)(s_bias + nl), bb = *(const f32x4*)(s_bias + nl + 16);
                        const f32x4 sa = *(const f32x4*)(s_sa + cl), sb = *(const f32x4*)(s_sb + cl);
                        const f32x4_t ag = acc[KG * MIH + h][2 * jp], ab = acc[KG * MIH + h][2 * jp + 1];
                        const u32x2 gq = {f2bf_pk(ag[0] + bg[0], ag[1] + bg[1]), f2bf_pk(ag[2] + bg[2], ag[3] + bg[3])};
                        const u32x2 bq = {f2bf_pk(ab[0] + bb[0], ab[1] + bb[1]), f2bf_pk(ab[2] + bb[2], ab[3] + bb[3])};
                        float r[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float x = (e & 1) ? bfhi2f(xv[jp][e >> 1]) : bflo2f(xv[jp][e >> 1]);
                            const float gm = (e & 1) ? bfhi2f(gq[e >> 1]) : bflo2f(gq[e >> 1]);
                            const float bt = (e & 1) ? bfhi2f(bq[e >> 1]) : bflo2f(bq[e >> 1]);
                            float y = x * sa[e] + sb[e];
                            y = y * (gm + 1.0f) + bt;
                            if (lerp) y = y * zs_cs + ((e & 1) ? bfhi2f(rv[jp][e >> 1]) : bflo2f(rv[jp][e >> 1])) * (1.0f - zs_cs);
                            r[e] = y;
                        }
                        const u32x2 o = {f2bf_pk(r[0], r[1]), f2bf_pk(r[2], r[3])};
                        *(u32x2*)(c_stage + l15 * C_RS + cl * 2) = o;
                    }
                    flush_block(m0 + mrow, zs_c0, std::integral_constant<int, ZS_CH>{});
                    if (p.gn_part_out) {
#pragma unroll
                        for (int g = 0; g < GP; ++g) {
                            const int col = g * 64 + lane;
                            if (ZS_CH % 64 == 0 || col < ZS_CH) {
                                float cs_ = 0.f, cq_ = 0.f;
#pragma unroll
                                for (int row = 0; row < 16; ++row) {
                                    const float f = bf2f(*(const u16*)(c_stage + row * C_RS + col * 2));
                                    cs_ += f;
                                    cq_ += f * f;
                                }
                                gsum[g] += cs_;
                                gsq[g] += cq_;
                            }
                        }
                    }
                }
                if (p.gn_part_out) {
                    float* red = (float*)(smem + OFF_GN) + (size_t)bwave * WTN * 2;
#pragma unroll
                    for (int g = 0; g < GP; ++g) {
                        const int col = g * 64 + lane;
                        if (ZS_CH % 64 == 0 || col < ZS_CH) {
                            red[col * 2] = gsum[g];
                            red[col * 2 + 1] = gsq[g];
                        }
                    }
                }
            };
            if (kg == 0) run(K0_{});
            else if constexpr (KS == 2) run(K1_{});
            if (p.gn_part_out) {   // one (sum, sum of squares) per 10-channel unit of the tile: every wave (all wave rows, both K groups), fixed order
                __syncthreads();
                if ((int)threadIdx.x < ZS_CH / 10) {
                    const float* red = (const float*)(smem + OFF_GN);
                    float sm = 0.f, sq = 0.f;
                    for (int c = (int)threadIdx.x * 10; c < (int)threadIdx.x * 10 + 10; ++c) {
#pragma unroll
                        for (int bw = 0; bw < NWT; ++bw) {
                            sm += red[((size_t)bw * WTN + c) * 2];
                            sq += red[((size_t)bw * WTN + c) * 2 + 1];
                        }
                    }
                    const int b = m0 / p.rows_per_batch, chunk = (m0 - b * p.rows_per_batch) / BM, nchunk = p.rows_per_batch / BM;
                    float* dst = p.gn_part_out + (((size_t)b * nchunk + chunk) * (p.N / 20) + zs_c0 / 10 + threadIdx.x) * 2;
                    dst[0] = sm;
                    dst[1] = sq;
                }
            }
            prefetch_next();
            return;
        }
#endif
        if (p.act == 2) {
            // GEGLU: W rows interleaved [16 value | 16 gate]: fragment pair (2 jp, 2 jp + 1) = (value, gate) of 16 output columns
            if constexpr ((NI & 1) == 0) {
                auto run = [&](auto kg_c) {
                    constexpr int KG = decltype(kg_c)::value;
#pragma unroll
                    for (int h = 0; h < MIH; ++h) {
                        const int mrow = wm * WTM + (KG * MIH + h) * 16;
                        const float mu = ln_mean[h], rs = ln_rstd[h];
#pragma unroll
                        for (int jp = 0; jp < NI / 2; ++jp) {
                            const int nl = wn * WTN + jp * 32 + 4 * quad;
                            const f32x4 bv = *(const f32x4*)(s_bias + nl), bg = *(const f32x4*)(s_bias + nl + 16);
                            const f32x4 cv = *(const f32x4*)(s_cs + nl), cg = *(const f32x4*)(s_cs + nl + 16);
                            float r[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float v = rs * (acc[KG * MIH + h][2 * jp][e] - mu * cv[e]) + bv[e];
                                const float g = rs * (acc[KG * MIH + h][2 * jp + 1][e] - mu * cg[e]) + bg[e];
                                r[e] = v * (p.fast_gelu ? gelu_fast_f(g) : gelu_f(g));
                            }
                            const u32x2 o = {f2bf_pk(r[0], r[1]), f2bf_pk(r[2], r[3])};
                            *(u32x2*)(c_stage + l15 * C_RS + (jp * 16 + 4 * quad) * 2) = o;
                        }
                        flush_block(m0 + mrow, (n0 >> 1) + wn * (WTN / 2), std::integral_constant<int, WTN / 2>{});
                    }
                };
                if (kg == 0) run(K0_{});
                else if constexpr (KS == 2) run(K1_{});
            }
            prefetch_next();
            return;
        }
        auto run = [&](auto kg_c, auto silu_c) {
            constexpr int KG = decltype(kg_c)::value;
            constexpr bool SILU = decltype(silu_c)::value;
            constexpr int GP = (WTN + 63) / 64;
            float gsum[GP], gsq[GP];   // GroupNorm statistics from the producer: this lane's columns, summed over the wave's token blocks
#pragma unroll
            for (int g = 0; g < GP; ++g) gsum[g] = gsq[g] = 0.f;
#pragma unroll
            for (int h = 0; h < MIH; ++h) {
                const int mrow = wm * WTM + (KG * MIH + h) * 16;    // first token of this 16-token block inside the tile
                const int m = m0 + mrow + l15;
                const float mu = ln_mean[h], rs = ln_rstd[h];
                u32x2 e_rb[NI], e_res[NI];
                if constexpr (PRE) {
#pragma unroll
                    for (int j = 0; j < NI; ++j) {
                        e_rb[j] = pre_rb[h][j];
                        e_res[j] = pre_res[h][j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NI; ++j) e_rb[j] = e_res[j] = u32x2{0u, 0u};
                    if (p.rowbias) {
                        const bf16_t* rbp = p.rowbias + (size_t)(m / p.rows_per_batch) * p.ld_rb + n0 + wn * WTN + 4 * quad;
#pragma unroll
                        for (int j = 0; j < NI; ++j) e_rb[j] = *(const u32x2*)(rbp + j * 16);
                    }
                    if (p.res) {
                        const bf16_t* rp = p.res + (size_t)m * p.ldr + n0 + wn * WTN + 4 * quad;
#pragma unroll
                        for (int j = 0; j < NI; ++j) e_res[j] = *(const u32x2*)(rp + j * 16);
                    }
                }
                float rsum = 0.f, rsq = 0.f;
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int nl = wn * WTN + j * 16 + 4 * quad;
                    const f32x4 cs = *(const f32x4*)(s_cs + nl), bz = *(const f32x4*)(s_bias + nl);
                    const u32x2 rb = e_rb[j], rr = e_res[j];
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = rs * (acc[KG * MIH + h][j][e] - mu * cs[e]) + bz[e];
                        t += (e & 1) ? bfhi2f(rb[e >> 1]) : bflo2f(rb[e >> 1]);
                        if constexpr (SILU) t = p.act == 1 ? silu_f(t) : (p.act == 3 ? gelu_f(t) : quick_gelu_f(t));
                        t *= p.alpha;
                        t += (e & 1) ? bfhi2f(rr[e >> 1]) : bflo2f(rr[e >> 1]);
                        v[e] = t;
                    }
                    const u32x2 o = {f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3])};
                    const float r0 = bflo2f(o[0]), r1 = bfhi2f(o[0]), r2 = bflo2f(o[1]), r3 = bfhi2f(o[1]);
                    rsum += (r0 + r1) + (r2 + r3);
                    rsq += (r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3);
                    *(u32x2*)(c_stage + l15 * C_RS + (j * 16 + 4 * quad) * 2) = o;
                }
                flush_block(m0 + mrow, n0 + wn * WTN, std::integral_constant<int, WTN>{});
                if (p.gn_part_out) {   // column sums of the staged 16 x WTN block, of the bf16 values as stored: lane = column
#pragma unroll
                    for (int g = 0; g < GP; ++g) {
                        const int col = g * 64 + lane;
                        if (WTN % 64 == 0 || col < WTN) {
                            float cs_ = 0.f, cq_ = 0.f;
#pragma unroll
                            for (int row = 0; row < 16; ++row) {
                                const float f = bf2f(*(const u16*)(c_stage + row * C_RS + col * 2));
                                cs_ += f;
                                cq_ += f * f;
                            }
                            gsum[g] += cs_;
                            gsq[g] += cq_;
                        }
                    }
                }
                if (p.rowstats_out) {
                    rsum += __shfl_xor(rsum, 16, 64);
                    rsq += __shfl_xor(rsq, 16, 64);
                    rsum += __shfl_xor(rsum, 32, 64);
                    rsq += __shfl_xor(rsq, 32, 64);
                    if (quad == 0) {
                        if constexpr (WN == 1) {   // the wave covers the tile's whole column range: this IS the tile's slot
                            float* dst = p.rowstats_out + ((size_t)m * p.rs_ld + tile_n) * 2;
                            dst[0] = rsum;
                            dst[1] = rsq;
                        } else {
                            float* red = (float*)(smem + OFF_RED) + ((size_t)wn * BM + mrow + l15) * 2;
                            red[0] = rsum;
                            red[1] = rsq;
                        }
                    }
                }
            }
            if (p.gn_part_out) {
                float* red = (float*)(smem + OFF_GN) + (size_t)bwave * WTN * 2;
#pragma unroll
                for (int g = 0; g < GP; ++g) {
                    const int col = g * 64 + lane;
                    if (WTN % 64 == 0 || col < WTN) {
                        red[col * 2] = gsum[g];
                        red[col * 2 + 1] = gsq[g];
                    }
                }
            }
        };
        if (kg == 0) {
            if (p.act != 0) run(K0_{}, T_{});
            else run(K0_{}, F_{});
        } else if constexpr (KS == 2) {
            if (p.act != 0) run(K1_{}, T_{});
            else run(K1_{}, F_{});
        }
        if constexpr (WN > 1) {
            if (p.rowstats_out) {   // combine the wave columns in a fixed order: one slot per tile column
                __syncthreads();
                for (int r = (int)threadIdx.x; r < BM; r += NTHREADS) {
                    float sm = 0.f, sq = 0.f;
#pragma unroll
                    for (int w = 0; w < WN; ++w) {
                        sm += ((const float*)(smem + OFF_RED))[((size_t)w * BM + r) * 2];
                        sq += ((const float*)(smem + OFF_RED))[((size_t)w * BM + r) * 2 + 1];
                    }
                    float* dst = p.rowstats_out + ((size_t)(m0 + r) * p.rs_ld + tile_n) * 2;
                    dst[0] = sm;
                    dst[1] = sq;
                }
            }
        }
        if (p.gn_part_out) {
            // one (sum, sum of squares) per GU-channel unit of this tile: every wave that covered the unit's columns (all wave rows,
            // both K groups), in a fixed order (reproducible); tile rows never straddle a batch (dispatcher).  GU = 10 for the
            // 80 / 160-column tiles (the UNet's groups are 10 / 20 / 40 / 60 channels wide), 4 for the 128 / 256-column tiles 39 / 40
            // (the VAE's groups: 4 / 8 / 16 channels, sgm/modules/diffusionmodules/model.py:48-51)
            constexpr int GU = (BN % 10 == 0) ? 10 : 4;
            __syncthreads();
            if ((int)threadIdx.x < BN / GU) {
                const float* red = (const float*)(smem + OFF_GN);
                float sm = 0.f, sq = 0.f;
                for (int c = (int)threadIdx.x * GU; c < (int)threadIdx.x * GU + GU; ++c) {
                    const int wn_c = c / WTN, cl = c - wn_c * WTN;
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                        for (int wx = 0; wx < WM; ++wx) {
                            const int bw = kx * NW + wx * WN + wn_c;
                            sm += red[((size_t)bw * WTN + cl) * 2];
                            sq += red[((size_t)bw * WTN + cl) * 2 + 1];
                        }
                }
                const int b = m0 / p.rows_per_batch, chunk = (m0 - b * p.rows_per_batch) / BM, nchunk = p.rows_per_batch / BM;
                float* dst = p.gn_part_out + (((size_t)b * nchunk + chunk) * (p.N / GU) + n0 / GU + threadIdx.x) * 2;
                dst[0] = sm;
                dst[1] = sq;
            }
        }
#ifdef SUPIR_G16_TIMELINE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (g16_tl_buf && lane == 0) {
            const unsigned long long tl_end = __builtin_amdgcn_s_memtime();
            unsigned long long* o = g16_tl_buf + ((size_t)blockIdx.x * 8 + bwave) * 16;
            o[8] = tl_wait;
            o[9] = tl_bar;
            o[10] = tl_comp;
            o[0] = tl_start;
            o[1] = tl_loop0 - tl_start;
            o[2] = tl_loop1 - tl_loop0;
            o[3] = tl_xch - tl_loop1;
            o[4] = tl_end - tl_xch;
            o[5] = tl_end - tl_start;
            o[6] = tl_end;
        }
#endif
        prefetch_next();
    }
