// Boundary kernels of the path: the few convolutions whose input or output has <= 8 channels (latent / RGB side).
// They sit at the NCHW-fp32 boundary the reference exposes (latents [N,4,h,w], images [N,3,H,W]) and convert to /
// from the internal NHWC bf16 layout on the fly, so no separate layout-conversion pass exists.
//
//   conv3x3_smallcin : fp32 NCHW [B,Cin<=8,H,W] -> bf16 NHWC [B,H,W,Cout]   UNet/control input_blocks.0.0 (4->320),
//                      input_hint_block (4->320, fused "+ guided_hint" add), VAE encoder conv_in (3->128),
//                      VAE decoder conv_in (4->512)                          (openaimodel.py:704, SUPIR_v0.py:325,482,
//                                                                             model.py:512,646)
//   conv3x3_smallcout: bf16 NHWC [B,H,W,Cin] -> fp32 NCHW [B,Cout<=8,H,W]   UNet out.2 (320->4), VAE encoder conv_out
//                      (512->8), VAE decoder conv_out (128->3)               (openaimodel.py:951, model.py:563,694)
//   pointwise_nchw   : fp32 NCHW 1x1 conv with <= 8 channels                 quant_conv / post_quant_conv
//   wavelet_level    : one level of the colour-fix wavelet decomposition (fp32 NCHW)   SUPIR/utils/colorfix.py:73-119
//                                                                            (sgm/models/autoencoder.py:297-298)
// All three are HBM / latency bound (a few MFLOP..GFLOP); none is worth MFMA.
#include "kernels.h"

// ---------------------------------------------------------------------------------------------------------
// weights: fp32 [Cout][Cin][3][3] (the reference's nn.Conv2d layout, untouched)
// A thread computes 8 output channels of TWO horizontally adjacent pixels: the 9 x Cin weight vectors (2 x 16 B from LDS per tap) are
// read once for both and the 3 x 4 input window is shared (12 instead of 18 loads per input channel).  The grid is capped at two
// workgroups per CU: every workgroup first stages the whole [Cin*9][Cout] fp32 table into LDS (46 KB for 4 -> 320), and with the
// earlier cap of 2048 workgroups that prologue was most of the launch (119 us for a 0.75 GFLOP, 21 MB-output convolution).
__global__ __launch_bounds__(256) void conv3x3_smallcin_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias,
                                                               const bf16_t* __restrict__ add, bf16_t* __restrict__ out,
                                                               int B, int Cin, int H, int W, int Cout, int ld_add,
                                                               int ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sw = (float*)smem_raw;  // [Cin*9][Cout]
    const int tid = threadIdx.x;
    const int K = Cin * 9;
    for (int i = tid; i < K * Cout; i += 256) {   // i = k * Cout + co: consecutive lanes write consecutive LDS words
        const int k = i / Cout, co = i - k * Cout;
        sw[i] = w[(size_t)co * K + k];
    }
    __syncthreads();
    const int cvo = Cout >> 3;
    const int W2 = (W + 1) >> 1;                   // pixel pairs per row (the last pair of an odd row has one pixel)
    const long total = (long)B * H * W2 * cvo;
    for (long idx = (long)blockIdx.x * 256 + tid; idx < total; idx += (long)gridDim.x * 256) {
        const int v = (int)(idx % cvo);
        const long pp = idx / cvo;
        const int xw = (int)(pp % W2) * 2;
        const int yh = (int)((pp / W2) % H);
        const int b = (int)(pp / ((long)W2 * H));
        const bool two = xw + 1 < W;
        const int co = v * 8;
        float acc[2][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = bias ? bias[co + e] : 0.f;
        for (int ci = 0; ci < Cin; ++ci) {
            const float* xp = x + ((size_t)b * Cin + ci) * H * W;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = yh + ky - 1;
                if ((unsigned)iy >= (unsigned)H) continue;
                float xin[4];   // columns xw - 1 .. xw + 2 of this input row (zero outside the image)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ix = xw - 1 + j;
                    xin[j] = (unsigned)ix < (unsigned)W ? xp[(size_t)iy * W + ix] : 0.f;
                }
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float* wp = sw + ((ci * 3 + ky) * 3 + kx) * Cout + co;
                    const f32x4 w0 = *(const f32x4*)wp, w1 = *(const f32x4*)(wp + 4);
                    const float x0 = xin[kx], x1 = xin[kx + 1];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[0][e] += x0 * w0[e];
                        acc[0][4 + e] += x0 * w1[e];
                        acc[1][e] += x1 * w0[e];
                        acc[1][4 + e] += x1 * w1[e];
                    }
                }
            }
        }
        const long pix = ((long)b * H + yh) * W + xw;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q == 1 && !two) break;
            if (add) {
                const u16x8 av = *(const u16x8*)(add + (size_t)(pix + q) * ld_add + co);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[q][e] += bf2f(av[e]);
            }
            u16x8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = f2bf(acc[q][e]);
            supir_store16(out + (size_t)(pix + q) * ldo + co, __builtin_bit_cast(f32x4, ov));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The same convolution on the exact-fp32 matrix instruction (round 5): the three 4 -> 320 input convolutions of a
// UNet step ran 67 us each in the VALU form above (0.75 GFLOP, 21 MB of output: ~2 % of any roofline), the VAE's 3 -> 128 at image
// resolution ~ 200 us.  v_mfma_f32_16x16x4_f32 takes fp32 operands and accumulates in fp32 -- nothing is rounded that the VALU form does
// not round -- and K = Cin * 9 (27 / 36) is KS = ceil(K / 4) steps with at most one padded column.  Operands swapped as everywhere in this
// library: A = 16 weight rows (output channels 16 j + m of the wave's range), B = the im2col columns of 16 consecutive pixels (flat
// b * H * W + y * W + x index: a block may straddle image rows, every lane derives its own tap addresses), so a lane ends with channels
// 16 j + 4 g .. + 3 of pixel n (g = lane / 16, n = lane % 16).  A wave's weights live in registers for the whole launch (NBW x KS floats
// per lane); the im2col values are gathered straight from the fp32 NCHW map (512 KB for a latent pair: L1 / L2 resident), one float per
// lane and K step.  Output rows leave through a wave-private LDS tile (16 pixels x 32 NBW bytes, rows padded by 16 B) as 16-byte
// row-contiguous stores, the family's usual epilogue; the optional `add` operand is applied in the accumulator layout BEFORE the one
// rounding to 16 bits, as in the VALU form.
//   SPLIT : the four waves of a workgroup split the channels (Cout = 64 NBW; all four gather the same pixels)   4 -> 320, 4 -> 512
//   !SPLIT: every wave has all channels (Cout = 16 NBW) and its own pixel blocks                                3 -> 128, 4 -> 128
// Another fp32 summation order than the VALU form (differences ~ 1e-7 relative, below the 16-bit output rounding except at ties);
// supir_debug_knob(7, 1) selects the VALU form for in-process A/B.
template <int NBW, int KS, bool SPLIT>
__global__ __launch_bounds__(256) void conv3x3_smallcin_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, const bf16_t* __restrict__ add,
                                                                    bf16_t* __restrict__ out, int B, int Cin, int H, int W, int ld_add,
                                                                    int ldo) {
    constexpr int ROWB = 32 * NBW + 16;               // bytes per pixel row of the stage (+16: rows start 4 banks apart)
    __shared__ __attribute__((aligned(16))) char stage_all[4][16 * ROWB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, n = lane & 15;
    const int K = Cin * 9, HW = H * W;
    const int chw = SPLIT ? wave * 16 * NBW : 0;      // first channel of this wave's range
    char* stage = stage_all[wave];
    // ---- A operand: lane (n, g) holds W[channel chw + 16 j + n][k = 4 s + g]
    float wr[NBW][KS];
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const float* wrow = w + (size_t)(chw + 16 * j + n) * K;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + g;
            wr[j][s] = k < K ? wrow[k] : 0.f;
        }
    }
    f32x4 bz[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) bz[j][r] = bias ? bias[chw + 16 * j + 4 * g + r] : 0.f;
    // ---- this lane's K indices: k = ci * 9 + ky * 3 + kx (the reference's [Cout][Cin][3][3] weight layout, untouched)
    int koff[KS], ktap[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k = 4 * s + g;
        const int ci = k / 9, t = k - 9 * ci, ky = t / 3, kx = t - 3 * ky;
        koff[s] = ci * HW + (ky - 1) * W + (kx - 1);
        ktap[s] = k < K ? (ky | (kx << 2)) : -1;
    }
    const long total = (long)B * HW;
    const long nblk = (total + 15) >> 4;
    const long step = SPLIT ? (long)gridDim.x : (long)gridDim.x * 4;
    for (long blk = SPLIT ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave; blk < nblk; blk += step) {
        const long p = blk * 16 + n;
        const bool valid = p < total;
        const long pc = valid ? p : total - 1;
        const int b = (int)(pc / HW);
        const int rem = (int)(pc - (long)b * HW);
        const int y = rem / W, xx = rem - y * W;
        const float* xb = x + (size_t)b * Cin * HW + rem;
        float xv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int ky = ktap[s] & 3, kx = (ktap[s] >> 2) & 3;
            const bool ok = valid && ktap[s] >= 0 && (unsigned)(y + ky - 1) < (unsigned)H && (unsigned)(xx + kx - 1) < (unsigned)W;
            xv[s] = ok ? xb[koff[s]] : 0.f;
        }
        f32x4 acc[NBW];
#pragma unroll
        for (int j = 0; j < NBW; ++j) acc[j] = bz[j];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[j][s], xv[s], acc[j], 0, 0, 0);
        // ---- epilogue: (+ add), one rounding, transpose through the wave's stage, 16-byte row-contiguous stores
        const bf16_t* ap = (add && valid) ? add + (size_t)p * ld_add + chw + 4 * g : nullptr;
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            f32x4 v = acc[j];
            if (ap) {
                const u16x4 av = *(const u16x4*)(ap + 16 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bf2f(av[e]);
            }
            const u32x2 o = {f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3])};
            *(u32x2*)(stage + n * ROWB + 32 * j + 8 * g) = o;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = lane; i < 32 * NBW; i += 64) {   // 2 NBW 16-byte pieces per pixel row
            const int row = i / (2 * NBW), piece = i - row * (2 * NBW);
            const long pr = blk * 16 + row;
            if (pr < total) *(u32x4*)(out + (size_t)pr * ldo + chw + 8 * piece) = *(const u32x4*)(stage + row * ROWB + 16 * piece);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int NBW, int KS, bool SPLIT>
static int launch_smallcin_mfma(const float* x, const float* w, const float* bias, const bf16_t* add, bf16_t* out, int B, int Cin, int H,
                                int W, int ld_add, int ldo, hipStream_t st) {
    const long nblk = ((long)B * H * W + 15) / 16;
    long units = SPLIT ? nblk : (nblk + 3) / 4;
    if (units > 512) units = 512;    // two workgroups per CU, all co-resident (176-240 registers: two waves per SIMD); every shape of the path divides evenly
    SUPIR_LAUNCH((conv3x3_smallcin_mfma_kernel<NBW, KS, SPLIT>), dim3((unsigned)units), dim3(256), 0, st, x, w, bias, add, out, B, Cin, H,
                 W, ld_add, ldo);
    return SUPIR_LAUNCH_STATUS();
}

int supir_conv3x3_smallcin_launch(const float* x, const float* w, const float* bias, const bf16_t* add, bf16_t* out,
                                  int B, int Cin, int H, int W, int Cout, int ld_add, int ldo, hipStream_t st) {
    if (B <= 0 || Cin <= 0 || Cin > 8 || Cout % 8 != 0 || ldo % 8 != 0 || (add && ld_add % 8 != 0)) return SUPIR_ERR_SHAPE;
    if (supir_debug_knob_value(7) != 1 && (long)Cin * H * W < (1L << 30)) {   // the matrix-instruction form for the path's own shapes
        if (Cin == 4 && Cout == 320) return launch_smallcin_mfma<5, 9, true>(x, w, bias, add, out, B, Cin, H, W, ld_add, ldo, st);
        if (Cin == 4 && Cout == 512) return launch_smallcin_mfma<8, 9, true>(x, w, bias, add, out, B, Cin, H, W, ld_add, ldo, st);
        if (Cin == 3 && Cout == 128) return launch_smallcin_mfma<8, 7, false>(x, w, bias, add, out, B, Cin, H, W, ld_add, ldo, st);
        if (Cin == 4 && Cout == 128) return launch_smallcin_mfma<8, 9, false>(x, w, bias, add, out, B, Cin, H, W, ld_add, ldo, st);
    }
    const size_t smem = (size_t)Cin * 9 * Cout * sizeof(float);
    if (smem > 160 * 1024) return SUPIR_ERR_SHAPE;
    static bool attr = false;
    if (!attr) {
        if (supir_note_hip_status(hipFuncSetAttribute((const void*)conv3x3_smallcin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024)) != SUPIR_OK) return SUPIR_ERR_HIP;
        attr = true;
    }
    const long total = (long)B * H * ((W + 1) / 2) * (Cout / 8);
    long blocks = (total + 255) / 256;
    if (blocks > 512) blocks = 512;      // two workgroups per CU: the weight-table prologue is paid 512 times, not 2048
    SUPIR_LAUNCH(conv3x3_smallcin_kernel, dim3((unsigned)blocks), dim3(256), smem, st, x, w, bias, add, out, B, Cin,
                       H, W, Cout, ld_add, ldo);
    return SUPIR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// 16 lanes cooperate on one output pixel: each lane owns channel vectors v = l16, l16+16, ...; 9 taps accumulate into
// COUT partial sums per lane which are then reduced across the 16 lanes with shuffles.
// weights: bf16 [9][COUT][Cin] (tap-major, prepared once on the host side)
template <int COUT>
__global__ __launch_bounds__(256) void conv3x3_smallcout_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ out,
                                                                int B, int Cin, int H, int W, int ldx) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    bf16_t* sw = (bf16_t*)smem_raw;
    const int tid = threadIdx.x;
    const int nw8 = 9 * COUT * Cin / 8;
    for (int i = tid; i < nw8; i += 256) ((u16x8*)sw)[i] = ((const u16x8*)w)[i];
    __syncthreads();
    const int l16 = tid & 15;
    const int cv = Cin >> 3;
    const long npix = (long)B * H * W;
    for (long pix = (long)blockIdx.x * 16 + (tid >> 4); pix < npix; pix += (long)gridDim.x * 16) {
        const int xw = (int)(pix % W);
        const int yh = (int)((pix / W) % H);
        const int b = (int)(pix / ((long)W * H));
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = yh + ky - 1;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = xw + kx - 1;
                if ((unsigned)ix >= (unsigned)W) continue;
                const bf16_t* xp = x + (((size_t)b * H + iy) * W + ix) * ldx;
                const bf16_t* wp = sw + (size_t)(ky * 3 + kx) * COUT * Cin;
                for (int v = l16; v < cv; v += 16) {
                    const u16x8 xv = *(const u16x8*)(xp + v * 8);
                    float xf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) xf[e] = bf2f(xv[e]);
#pragma unroll
                    for (int o = 0; o < COUT; ++o) {
                        const u16x8 wv = *(const u16x8*)(wp + (size_t)o * Cin + v * 8);
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[o] += xf[e] * bf2f(wv[e]);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
            float a = acc[o];
            a += __shfl_xor(a, 8, 64);
            a += __shfl_xor(a, 4, 64);
            a += __shfl_xor(a, 2, 64);
            a += __shfl_xor(a, 1, 64);
            acc[o] = a;
        }
        if (l16 < COUT) {
            float r = 0.f;
#pragma unroll
            for (int o = 0; o < COUT; ++o) r = (l16 == o) ? acc[o] : r;
            out[(((size_t)b * COUT + l16) * H + yh) * W + xw] = r + (bias ? bias[l16] : 0.f);
        }
    }
}

// Register-resident form for Cin = 128 (round 4): the VAE decoder's conv_out (sgm/modules/diffusionmodules/model.py:694, 128 -> 3 at full
// image resolution: 268 MB of input per 1024^2 image).  In the kernel above every lane re-reads its 9 x COUT weight vectors from LDS for
// every pixel (27 reads of 16 B per pixel and lane: LDS-port bound, ~1 TB/s of input).  Here lane l of a 16-lane group owns channels
// 8 l .. 8 l + 7 and keeps its slice of all 9 x COUT weight rows in registers (9 x COUT x 4 packed pairs: 108 for COUT = 3); a group walks
// along an image row with a 3 x 3 window of 16-byte vectors -- one new column (3 loads) per pixel instead of 9 taps -- and multiplies with
// v_dot2c (two MACs per instruction): no LDS in the loop, a third of the global-load instructions, half the VALU.
template <int COUT>
__global__ __launch_bounds__(256) void conv3x3_c128_smallcout_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ out,
                                                                     int B, int H, int W, int ldx, int nseg, int ntask) {
    static_assert(COUT >= 1 && COUT <= 4, "9 x COUT x 4 weight registers per lane");
    constexpr int SEG = 64;                          // pixels of one row a group handles per task
    const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
    u32x4 wr[9][COUT];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int o = 0; o < COUT; ++o) wr[tap][o] = *(const u32x4*)(w + (size_t)(tap * COUT + o) * 128 + 8 * l16);
    const float bz = (l16 < COUT && bias) ? bias[l16] : 0.f;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const int nwg = (int)gridDim.x;
    const int wg = xcd_remap((int)blockIdx.x, nwg);  // neighbouring image rows (they share two of their three input rows) on one XCD's L2
    for (int task = wg * 16 + grp; task < ntask; task += nwg * 16) {
        const int sg = task % nseg, by = task / nseg;
        const int y = by % H, b = by / H;
        const int x0 = sg * SEG, x1 = x0 + SEG < W ? x0 + SEG : W;
        const bf16_t* rowp[3];
        bool rok[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = y + ky - 1;
            rok[ky] = (unsigned)iy < (unsigned)H;
            rowp[ky] = x + ((size_t)b * H + (rok[ky] ? iy : y)) * W * ldx + 8 * l16;
        }
        auto ld = [&](int ky, int ix) -> u32x4 {
            return (rok[ky] && (unsigned)ix < (unsigned)W) ? *(const u32x4*)(rowp[ky] + (size_t)ix * ldx) : zero;
        };
        // one output pixel: columns xx - 1 / xx / xx + 1 of the window are A / B / C; C is loaded here, A and B came from the previous steps
        auto step = [&](const u32x4 (&A)[3], const u32x4 (&Bc)[3], u32x4 (&C)[3], int xx) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) C[ky] = ld(ky, xx + 1);
            float acc[COUT];
#pragma unroll
            for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int o = 0; o < COUT; ++o)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[o] = dot2_acc(A[ky][e], wr[ky * 3 + 0][o][e], acc[o]);
                        acc[o] = dot2_acc(Bc[ky][e], wr[ky * 3 + 1][o][e], acc[o]);
                    }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int o = 0; o < COUT; ++o)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[o] = dot2_acc(C[ky][e], wr[ky * 3 + 2][o][e], acc[o]);
            float r = 0.f;
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                float a = acc[o];
                a += __shfl_xor(a, 8, 64);
                a += __shfl_xor(a, 4, 64);
                a += __shfl_xor(a, 2, 64);
                a += __shfl_xor(a, 1, 64);
                r = (l16 == o) ? a : r;
            }
            if (l16 < COUT) out[(((size_t)b * COUT + l16) * H + y) * W + xx] = r + bz;
        };
        u32x4 c0[3], c1[3], c2[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            c0[ky] = ld(ky, x0 - 1);
            c1[ky] = ld(ky, x0);
        }
        for (int xx = x0; xx < x1; xx += 3) {   // the window's three column buffers rotate: no register moves
            step(c0, c1, c2, xx);
            if (xx + 1 >= x1) break;
            step(c1, c2, c0, xx + 1);
            if (xx + 2 >= x1) break;
            step(c2, c0, c1, xx + 2);
        }
    }
}

int supir_conv3x3_smallcout_launch(const bf16_t* x, const bf16_t* w, const float* bias, float* out, int B, int Cin,
                                   int H, int W, int Cout, int ldx, hipStream_t st) {
    if (B <= 0 || Cin % 8 != 0 || ldx % 8 != 0) return SUPIR_ERR_SHAPE;
    if (Cin == 128 && (Cout == 3 || Cout == 4) && H > 0 && W > 0 && (long)B * H * ((W + 63) / 64) < 0x7fffffffL) {
        const int nseg = (W + 63) / 64, ntask = B * H * nseg;
        int nwg = (ntask + 15) / 16;
        if (nwg > 512) nwg = 512;                    // two workgroups per CU (185 registers); the 27 weight loads of a lane are paid once per workgroup
        if (Cout == 3)
            SUPIR_LAUNCH(conv3x3_c128_smallcout_kernel<3>, dim3((unsigned)nwg), dim3(256), 0, st, x, w, bias, out, B, H, W, ldx, nseg, ntask);
        else
            SUPIR_LAUNCH(conv3x3_c128_smallcout_kernel<4>, dim3((unsigned)nwg), dim3(256), 0, st, x, w, bias, out, B, H, W, ldx, nseg, ntask);
        return SUPIR_LAUNCH_STATUS();
    }
    const size_t smem = (size_t)9 * Cout * Cin * 2;
    if (smem > 160 * 1024) return SUPIR_ERR_SHAPE;
    const long npix = (long)B * H * W;
    long blocks = (npix + 15) / 16;
    if (blocks > 1024) blocks = 1024;
#define SC_LAUNCH(CO)                                                                                              \
    {                                                                                                              \
        static bool attr = false;                                                                                  \
        if (!attr) {                                                                                               \
            if (hipFuncSetAttribute((const void*)conv3x3_smallcout_kernel<CO>,                                     \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)         \
                return SUPIR_ERR_HIP;                                                                              \
            attr = true;                                                                                           \
        }                                                                                                          \
        SUPIR_LAUNCH(conv3x3_smallcout_kernel<CO>, dim3((unsigned)blocks), dim3(256), smem, st, x, w, bias,  \
                           out, B, Cin, H, W, ldx);                                                                \
    }
    switch (Cout) {
        case 3: SC_LAUNCH(3); break;
        case 4: SC_LAUNCH(4); break;
        case 8: SC_LAUNCH(8); break;
        default: return SUPIR_ERR_SHAPE;
    }
#undef SC_LAUNCH
    return SUPIR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pointwise_nchw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int B, int Cin, int Cout, long HW, float in_scale) {
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float xin[8];
        for (int c = 0; c < Cin; ++c) xin[c] = x[(b * Cin + c) * HW + p] * in_scale;
        for (int o = 0; o < Cout; ++o) {
            float a = bias ? bias[o] : 0.f;
            for (int c = 0; c < Cin; ++c) a += w[o * Cin + c] * xin[c];
            out[(b * Cout + o) * HW + p] = a;
        }
    }
}

int supir_pointwise_nchw_launch(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout,
                                long HW, float in_scale, hipStream_t st) {
    if (B <= 0 || Cin <= 0 || Cin > 8 || Cout <= 0 || Cout > 8 || HW <= 0) return SUPIR_ERR_SHAPE;
    long blocks = ((long)B * HW + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    SUPIR_LAUNCH(pointwise_nchw_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, w, bias, out, B, Cin, Cout, HW,
                       in_scale);
    return SUPIR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// Weight prefetch: the 7.7 GB of bf16 weights stream from HBM once per UNet step (they cannot stay in the 256 MB Infinity
// Cache), so every GEMM starts cold while HBM itself is nearly idle (0.2 TB/s average).  This kernel touches one dword per
// 128-byte line of a weight matrix a few launches AHEAD of its consumer, from a separate stream, so the lines are already
// on their way through the memory-side cache when the consumer's first K tiles ask for them.
__global__ __launch_bounds__(256) void prefetch_lines_kernel(const uint32_t* __restrict__ p, size_t lines, uint32_t* sink) {
    uint32_t acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < lines; i += (size_t)gridDim.x * 256) acc ^= p[i * 32];
    if (acc == 0x9e3779b9u && sink) sink[0] = acc;   // never true in practice: keeps the loads alive
}

int supir_prefetch_launch(const void* p, size_t bytes, void* sink, hipStream_t st) {
    const size_t lines = bytes / 128;
    if (lines == 0) return SUPIR_OK;
    size_t blocks = (lines + 255) / 256;
    if (blocks > 64) blocks = 64;   // a trickle: it must not compete with the compute kernels for CUs
    SUPIR_LAUNCH(prefetch_lines_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t*)p, lines, (uint32_t*)sink);
    return SUPIR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// One level of wavelet_decomposition (SUPIR/utils/colorfix.py:73-107): low = blur_r(img) with the fixed 3x3 kernel
// [[1,2,1],[2,4,2],[1,2,1]]/16 applied depthwise at dilation r on a replicate-padded image (== clamped taps), and
// high (+)= img - low.  fp32 planes [planes][H][W]; HBM-trivial: 1 read + 2 writes (+1 read-modify-write) per pixel.
__global__ __launch_bounds__(256) void wavelet_level_kernel(const float* __restrict__ img, float* __restrict__ low,
                                                             float* __restrict__ high, int H, int W, int r, int first) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t plane = (size_t)blockIdx.z * H * W;
    const float* p = img + plane;
    const int ym = y - r > 0 ? y - r : 0, yp = y + r < H - 1 ? y + r : H - 1;
    const int xm = x - r > 0 ? x - r : 0, xp = x + r < W - 1 ? x + r : W - 1;
    const float* r0 = p + (size_t)ym * W;
    const float* r1 = p + (size_t)y * W;
    const float* r2 = p + (size_t)yp * W;
    const float c = r1[x];
    const float corners = (r0[xm] + r0[xp]) + (r2[xm] + r2[xp]);
    const float edges = (r0[x] + r2[x]) + (r1[xm] + r1[xp]);
    const float lo = 0.0625f * corners + 0.125f * edges + 0.25f * c;
    const size_t o = plane + (size_t)y * W + x;
    low[o] = lo;
    if (high) high[o] = (first ? 0.f : high[o]) + (c - lo);   // high == null: the caller only wants the low band (style image)
}

int supir_wavelet_level_launch(const float* img, float* low, float* high, int planes, int H, int W, int radius, int first,
                               hipStream_t st) {
    if (planes <= 0 || H <= 0 || W <= 0 || radius <= 0 || planes > 65535 || H > 65535) return SUPIR_ERR_SHAPE;
    if (img == low || (high && (img == high || low == high))) return SUPIR_ERR_ARG;
    SUPIR_LAUNCH(wavelet_level_kernel, dim3((W + 255) / 256, H, planes), dim3(256), 0, st, img, low, high, H, W, radius, first);
    return SUPIR_LAUNCH_STATUS();
}


// ---------------------------------------------------------------------------------------------------------
// Image I/O edges of test.py (SUPIR/util.py:60-94).
//
// PIL2Tensor resizes the input with PIL's Image.resize(BICUBIC): Pillow's separable resampler on 8-bit pixels with 22-bit
// fixed-point coefficients (src/libImaging/Resample.c, third party: Pillow; the coefficient tables are rebuilt on the host in
// float64 with Pillow's formulas, supir_amd/utils/imageio.py).  One pass (horizontal or vertical) per launch, bit-exact:
//   acc = 1 << 21;  acc += pixel[xmin + i] * kk[i], i < n;  out = clip8(acc >> 22)
// src / dst are HWC uint8 with `ch` interleaved channels.  The vertical pass can emit the final fp32 CHW tensor directly through
// a 256-entry table (x / 255 * 2 - 1 evaluated on the host exactly as numpy does), so the resized uint8 image never exists.
__global__ __launch_bounds__(256) void resample_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8,
                                                           float* __restrict__ dst_f32, const float* __restrict__ lut,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           int in_h, int in_w, int out_h, int out_w, int ch, int vertical) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= out_w) return;
    const int o = vertical ? oy : ox;                       // index into the coefficient tables
    const int xmin = bounds[2 * o], n = bounds[2 * o + 1];
    const int* k = kk + (size_t)o * ksize;
    for (int c = 0; c < ch; ++c) {
        int acc = 1 << 21;
        if (vertical) {
            for (int i = 0; i < n; ++i) acc += (int)src[((size_t)(xmin + i) * in_w + ox) * ch + c] * k[i];
        } else {
            for (int i = 0; i < n; ++i) acc += (int)src[((size_t)oy * in_w + xmin + i) * ch + c] * k[i];
        }
        int v = acc >> 22;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        if (dst_u8) dst_u8[((size_t)oy * out_w + ox) * ch + c] = (uint8_t)v;
        if (dst_f32) dst_f32[((size_t)c * out_h + oy) * out_w + ox] = lut[v];
    }
}

int supir_resample_u8_launch(const uint8_t* src, uint8_t* dst_u8, float* dst_f32, const float* lut, const int* bounds, const int* kk,
                             int ksize, int in_h, int in_w, int out_h, int out_w, int ch, int vertical, hipStream_t st) {
    if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || ch <= 0 || ch > 4 || ksize <= 0 || out_h > 65535) return SUPIR_ERR_SHAPE;
    if (!dst_u8 && !dst_f32) return SUPIR_ERR_ARG;
    if (dst_f32 && !lut) return SUPIR_ERR_ARG;
    if (vertical ? in_w != out_w : in_h != out_h) return SUPIR_ERR_SHAPE;
    SUPIR_LAUNCH(resample_u8_kernel, dim3((out_w + 255) / 256, out_h), dim3(256), 0, st, src, dst_u8, dst_f32, lut, bounds, kk, ksize,
                 in_h, in_w, out_h, out_w, ch, vertical);
    return SUPIR_LAUNCH_STATUS();
}

// Tensor2PIL (SUPIR/util.py:86-94): F.interpolate(x, size, mode='bicubic') -- ATen's cubic convolution with A = -0.75,
// align_corners = False, border pixels replicated -- then x * 127.5 + 127.5, clip to [0, 255], truncate to uint8, HWC.
// fp32 planes [C][H][W] in; out_u8 [OH][OW][C] and / or out_f32 [C][OH][OW].
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

__global__ __launch_bounds__(256) void bicubic_f32_kernel(const float* __restrict__ src, uint8_t* __restrict__ out_u8,
                                                           float* __restrict__ out_f32, int C, int H, int W, int OH, int OW,
                                                           float scale_h, float scale_w) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= OW) return;
    const float A = -0.75f;
    const float ry = scale_h * (oy + 0.5f) - 0.5f, rx = scale_w * (ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    const float ty = ry - fy, tx = rx - fx;
    const float wy[4] = {cubic2(ty + 1.f, A), cubic1(ty, A), cubic1(1.f - ty, A), cubic2(2.f - ty, A)};
    const float wx[4] = {cubic2(tx + 1.f, A), cubic1(tx, A), cubic1(1.f - tx, A), cubic2(2.f - tx, A)};
    int ys[4], xs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int y = iy - 1 + i, x = ix - 1 + i;
        ys[i] = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        xs[i] = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
    }
    for (int c = 0; c < C; ++c) {
        const float* p = src + (size_t)c * H * W;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* r = p + (size_t)ys[i] * W;
            const float row = r[xs[0]] * wx[0] + r[xs[1]] * wx[1] + r[xs[2]] * wx[2] + r[xs[3]] * wx[3];
            acc += row * wy[i];
        }
        if (out_f32) out_f32[((size_t)c * OH + oy) * OW + ox] = acc;
        if (out_u8) {
            float v = acc * 127.5f + 127.5f;
            v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
            out_u8[((size_t)oy * OW + ox) * C + c] = (uint8_t)v;   // truncation, like numpy's astype(uint8)
        }
    }
}

int supir_bicubic_f32_launch(const float* src, uint8_t* out_u8, float* out_f32, int C, int H, int W, int OH, int OW, hipStream_t st) {
    if (C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || OH > 65535) return SUPIR_ERR_SHAPE;
    if (!out_u8 && !out_f32) return SUPIR_ERR_ARG;
    SUPIR_LAUNCH(bicubic_f32_kernel, dim3((OW + 255) / 256, OH), dim3(256), 0, st, src, out_u8, out_f32, C, H, W, OH, OW,
                 (float)H / (float)OH, (float)W / (float)OW);
    return SUPIR_LAUNCH_STATUS();
}

// ---------------------------------------------------------------------------------------------------------
// Fast mode of the tiled VAE (SUPIR/utils/tilevae.py:855-876): the GroupNorm statistics of the whole network are estimated on a
// nearest-exact down-sampled copy of the input whose per-channel mean / std are moved back to the input's.
//
// image_moments: per-channel (sum, sum of squares, min, max) of an fp32 NCHW image, or -- with the index tables iy [OH] / ix [OW] --
// of the OH x OW pixels F.interpolate(mode="nearest-exact") would gather from it, without materialising them.  fp64 accumulation (a
// 4096^2 plane is 16.7 M addends), wave64 shuffle reduction, one partial per workgroup, a second tiny launch adds the partials of a
// channel over images and chunks in a fixed order (reproducible, the idiom of gn_stats_kernel / gn_finalize_kernel).
__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void image_moments_kernel(const float* __restrict__ x, const int* __restrict__ iy,
                                                            const int* __restrict__ ix, double* __restrict__ partial, int H, int W,
                                                            int OH, int OW, long per_chunk) {
    __shared__ double red[4][4];
    const int tid = threadIdx.x, chunk = blockIdx.x, plane = blockIdx.y;
    const long total = (long)OH * OW;
    const long i0 = (long)chunk * per_chunk, i1 = i0 + per_chunk < total ? i0 + per_chunk : total;
    const float* p = x + (size_t)plane * H * W;
    double s = 0.0, q = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (long i = i0 + tid; i < i1; i += 256) {
        float v;
        if (ix) {
            const int oy = (int)(i / OW), ox = (int)(i - (long)oy * OW);
            v = p[(size_t)iy[oy] * W + ix[ox]];
        } else {
            v = p[i];
        }
        s += (double)v;
        q += (double)v * (double)v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    const double dmn = wave_min_f64((double)mn), dmx = wave_max_f64((double)mx);
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = s;
        red[tid >> 6][1] = q;
        red[tid >> 6][2] = dmn;
        red[tid >> 6][3] = dmx;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = partial + ((size_t)plane * gridDim.x + chunk) * 4;
        o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        o[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        o[2] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
        o[3] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
    }
}

// out [C][4] = (sum, sum of squares, min, max) of channel c over all images: one wave per channel
__global__ __launch_bounds__(64) void image_moments_finalize_kernel(const double* __restrict__ partial, double* __restrict__ out, int N,
                                                                    int C, int nchunk) {
    const int c = blockIdx.x, t = threadIdx.x;
    double s = 0.0, q = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int n = 0; n < N; ++n)
        for (int k = t; k < nchunk; k += 64) {
            const double* e = partial + (((size_t)n * C + c) * nchunk + k) * 4;
            s += e[0];
            q += e[1];
            mn = fmin(mn, e[2]);
            mx = fmax(mx, e[3]);
        }
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    mn = wave_min_f64(mn);
    mx = wave_max_f64(mx);
    if (t == 0) {
        out[c * 4 + 0] = s;
        out[c * 4 + 1] = q;
        out[c * 4 + 2] = mn;
        out[c * 4 + 3] = mx;
    }
}

#define SUPIR_MOMENTS_MAX_CHUNKS 256

int supir_image_moments_launch(const float* x, const int* iy, const int* ix, double* out, double* workspace, size_t workspace_bytes,
                               int N, int C, int H, int W, int OH, int OW, hipStream_t st) {
    if (N <= 0 || C <= 0 || C > 8 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (long)N * C > 65535) return SUPIR_ERR_SHAPE;
    if ((iy == nullptr) != (ix == nullptr)) return SUPIR_ERR_ARG;
    if (!ix && (OH != H || OW != W)) return SUPIR_ERR_SHAPE;      // without tables the moments are the whole image's
    const long total = (long)OH * OW;
    long nchunk = (total + 4095) / 4096;
    if (nchunk > SUPIR_MOMENTS_MAX_CHUNKS) nchunk = SUPIR_MOMENTS_MAX_CHUNKS;
    const long per_chunk = (total + nchunk - 1) / nchunk;
    if (workspace_bytes < (size_t)N * C * nchunk * 4 * sizeof(double)) return SUPIR_ERR_ARG;
    SUPIR_LAUNCH(image_moments_kernel, dim3((unsigned)nchunk, N * C), dim3(256), 0, st, x, iy, ix, workspace, H, W, OH, OW, per_chunk);
    SUPIR_LAUNCH(image_moments_finalize_kernel, dim3(C), dim3(64), 0, st, workspace, out, N, C, (int)nchunk);
    return SUPIR_LAUNCH_STATUS();
}

// downsample_nearest_exact_affine: out[n][c][oy][ox] = clamp((x[n][c][iy[oy]][ix[ox]] - mean_new) / std_new * std_old + mean_old,
// min(x), max(x)) in the reference's fp32 operation order (tilevae.py:866-872); mean / UNBIASED std per channel over (N, H, W) come
// from the two image_moments results (mom_old: the whole image, mom_new: the gathered pixels), min / max over all channels of mom_old.
__global__ __launch_bounds__(256) void downsample_affine_kernel(const float* __restrict__ x, const int* __restrict__ iy,
                                                                const int* __restrict__ ix, float* __restrict__ out,
                                                                const double* __restrict__ mom_old, const double* __restrict__ mom_new,
                                                                int C, int H, int W, int OH, int OW, double n_old, double n_new) {
#pragma clang fp contract(off)
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, plane = blockIdx.z, c = plane % C;
    if (ox >= OW) return;
    const double so = mom_old[c * 4], qo = mom_old[c * 4 + 1], sn = mom_new[c * 4], qn = mom_new[c * 4 + 1];
    const double mo = so / n_old, mnw = sn / n_new;
    const float mean_old = (float)mo, mean_new = (float)mnw;
    const float std_old = (float)sqrt(fmax(qo - so * mo, 0.0) / (n_old - 1.0));
    const float std_new = (float)sqrt(fmax(qn - sn * mnw, 0.0) / (n_new - 1.0));
    double lo = mom_old[2], hi = mom_old[3];
    for (int k = 1; k < C; ++k) {
        lo = fmin(lo, mom_old[k * 4 + 2]);
        hi = fmax(hi, mom_old[k * 4 + 3]);
    }
    const float v = x[((size_t)plane * H + iy[oy]) * W + ix[ox]];
    float r = (v - mean_new) / std_new;
    r = r * std_old;
    r = r + mean_old;
    r = fminf(fmaxf(r, (float)lo), (float)hi);
    out[((size_t)plane * OH + oy) * OW + ox] = r;
}

int supir_downsample_affine_launch(const float* x, const int* iy, const int* ix, float* out, const double* mom_old, const double* mom_new,
                                   int N, int C, int H, int W, int OH, int OW, hipStream_t st) {
    if (N <= 0 || C <= 0 || C > 8 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || OH > 65535 || (long)N * C > 65535) return SUPIR_ERR_SHAPE;
    if ((long)N * OH * OW < 2) return SUPIR_ERR_SHAPE;            // the unbiased std needs two samples
    SUPIR_LAUNCH(downsample_affine_kernel, dim3((OW + 255) / 256, OH, N * C), dim3(256), 0, st, x, iy, ix, out, mom_old, mom_new, C, H,
                 W, OH, OW, (double)N * H * W, (double)N * OH * OW);
    return SUPIR_LAUNCH_STATUS();
}
