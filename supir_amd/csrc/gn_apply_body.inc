// Body of the GroupNorm apply pass (csrc/norm.hip: gn_apply_kernel and its dynamic-control-scale form gn_apply_cs_kernel).
// In scope: NP, MOD, SILU, pp (GnArgsN<NP>), nchunk_apply, rows_per_chunk_apply, TY.
    const GnArgs& p = pp.p[NP == 1 ? 0 : blockIdx.z];
    __shared__ float s_mean[32], s_rstd[32];
    __shared__ double s_part[4][64];
    const int tid = threadIdx.x;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int cv = p.C >> 3, cpg = p.C >> 5;
    const int v = tid % cv, ty = tid / cv, c = v * 8;
    const int row0 = chunk * rows_per_chunk_apply;
    const int row1 = min(p.HW, row0 + rows_per_chunk_apply);
    const bool lerp = MOD && p.cscale != 1.0f;
    constexpr int U = 2;   // rows in flight per thread (4 cost 83 VGPRs = 5 waves per SIMD instead of 8)
    // ---- loads that do not depend on the statistics: this thread's affine parameters and its first U rows
    const f32x4 g0 = *(const f32x4*)(p.gamma + c), g1 = *(const f32x4*)(p.gamma + c + 4);
    const f32x4 be0 = *(const f32x4*)(p.beta + c), be1 = *(const f32x4*)(p.beta + c + 4);
    constexpr int UM = MOD ? U : 1;
    u16x8 xv[U], gv[UM], bv[UM], rv[UM];
    auto load_rows = [&](int row) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = row + u * TY;
            if (r < row1) {
                xv[u] = *(const u16x8*)gn_src(p, b, r, c);
                if constexpr (MOD) {
                    const size_t mo = ((size_t)b * p.HW + r) * p.ldm + c;
                    gv[u] = *(const u16x8*)(p.mod_g + mo);
                    bv[u] = *(const u16x8*)(p.mod_b + mo);
                    if (lerp) {   // h_raw = cat[h_ori, h] (h BEFORE the zero_conv projection)
                        rv[u] = xv[u];
                        if (c < p.C1) {
                            if (p.x1raw) rv[u] = *(const u16x8*)(p.x1raw + ((size_t)b * p.HW + r) * p.ld1 + c);
                        } else if (p.x2raw) {
                            rv[u] = *(const u16x8*)(p.x2raw + ((size_t)b * p.HW + r) * p.ld2 + (c - p.C1));
                        }
                    }
                }
            }
        }
    };
    load_rows(row0 + ty);
    // ---- statistics of this batch element: (sum, sum of squares) per group, reduced in a fixed order (reproducible)
    if (tid < 256) {
        const int sv = tid & 63, sub = tid >> 6;
        if (p.part_u1) {
            // left behind by the producer GEMM / conv epilogues (GemmArgs::gn_part_out): per tile row and 10-channel unit of each source
            // tensor.  Group g = units [g * upg, (g + 1) * upg) of the concatenation; every group width on the path is a multiple of 10
            const int g = sv >> 1, st = sv & 1;
            const int upg = cpg / 10, U1 = p.C1 / 10, U2 = (p.C - p.C1) / 10;
            double a = 0.0;
            for (int uu = g * upg; uu < (g + 1) * upg; ++uu) {
                const bool first = uu < U1;
                const float* src = first ? p.part_u1 : p.part_u2;
                const int nch = first ? p.nch1 : p.nch2, Un = first ? U1 : U2, u = first ? uu : uu - U1;
                for (int k = sub; k < nch; k += 4) a += (double)src[(((size_t)b * nch + k) * Un + u) * 2 + st];
            }
            s_part[sub][sv] = a;
        } else if (!p.given) {
            double a = 0.0;
            for (int k = sub; k < p.nchunk; k += 4) a += (double)p.partial[((size_t)b * p.nchunk + k) * 64 + sv];
            s_part[sub][sv] = a;
        }
    }
    __syncthreads();
    if (p.given) {
        // externally pooled statistics (tiled VAE: SUPIR/utils/tilevae.py:524-553 custom_group_norm)
        if (tid < 32) {
            s_mean[tid] = p.given[((size_t)b * 32 + tid) * 2];
            s_rstd[tid] = rsqrtf(p.given[((size_t)b * 32 + tid) * 2 + 1] + p.eps);
        }
    } else if (tid < 32) {
        const double s = s_part[0][2 * tid] + s_part[1][2 * tid] + s_part[2][2 * tid] + s_part[3][2 * tid];
        const double q = s_part[0][2 * tid + 1] + s_part[1][2 * tid + 1] + s_part[2][2 * tid + 1] + s_part[3][2 * tid + 1];
        const double n = (double)p.HW * (double)cpg;
        const double mean = s / n;
        double var = q / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        s_mean[tid] = (float)mean;
        s_rstd[tid] = (float)(1.0 / sqrt(var + (double)p.eps));
    }
    __syncthreads();
    float sa[8], sb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int g = (c + e) / cpg;
        const float a = s_rstd[g] * (e < 4 ? g0[e] : g1[e - 4]);
        sa[e] = a;
        sb[e] = (e < 4 ? be0[e] : be1[e - 4]) - s_mean[g] * a;
    }
    if (ty >= TY) return;   // (never: the block is exactly cv x TY threads)
    for (int row = row0 + ty; row < row1; row += U * TY) {
        u16x8 ov[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float y = bf2f(xv[u][e]) * sa[e] + sb[e];
                if constexpr (SILU) y = silu_f(y);
                if constexpr (MOD) {
                    y = y * (bf2f(gv[u][e]) + 1.0f) + bf2f(bv[u][e]);
                    if (lerp) y = y * p.cscale + bf2f(rv[u][e]) * (1.0f - p.cscale);
                }
                ov[u][e] = f2bf(y);
            }
        }
        const int next = row + U * TY;
        const int here = row;
        if (next < row1) load_rows(next);   // the next batch is in flight while this one is stored
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = here + u * TY;
            if (r < row1) supir_store16(p.out + ((size_t)b * p.HW + r) * p.ldo + c, __builtin_bit_cast(f32x4, ov[u]));
        }
    }
