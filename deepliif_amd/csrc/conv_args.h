// conv_args.h -- what the conv translation units share: the kernel argument block, the tap decode, the LDS types and swizzle, the host-side rules several
// launchers apply (32-bit offset guard, strip height), and the prototypes by which conv_gemm.hip reaches the kernels of the other files.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16_t;            // MFMA 32x32 accumulator fragment
typedef __attribute__((address_space(3))) char lds_char_t;
typedef __attribute__((address_space(3))) const bf16x8_t lds_frag_t;

struct ConvArgs {
    const void *in;
    const bf16_t *w_hi;
    const bf16_t *w_lo;
    const float *bias;
    void *out;
    float *slab;
    int N, Hi, Wi, Ci, log2Ci, in_pstride;
    int Ho, Wo, Co, out_pstride;
    int Hq, Wq, out_step, in_step;
    int n_phase, splitk;
    int phase_oh[DL_MAX_PHASES], phase_ow[DL_MAX_PHASES];
    int phase_tap_begin[DL_MAX_PHASES + 1];
    int phase_kbase[DL_MAX_PHASES];
    int pad_mode, w_kstride, act, in_act, bias_n, raw_out;
    int in_split;           // strict kernels: the input is the producer-written split copy ([8 hi | 8 lo] per 8 channels): no in-kernel split
    int epi_old;            // DL_OLD_EPILOGUE=1: per-fragment stores instead of the LDS-transposed whole-row stores (A/B switch)
    int tiles_m, tiles_n, Mtot;
    int k_order;                    // direct-to-LDS UTAP path: 0 = K steps tap-major, 1 = channel-chunk-major (L2 reuse of the halo slab)
    int k_order8;                   // the same choice for the 8-phase kernels (bf16: DL_8PH_KORDER, strict: DL_X3_KORDER)
    float *stats_part;              // fused norm statistics: part[((n*nchunks + chunk)*2 + {sum,sumsq})*Co + c]
    int stats_nchunks;
    // fused norm-backward reductions (dl_conv_forward_bnstats): y tile read next to the dz tile in the store epilogue
    const bf16_t *bn_y;
    const float *bn_mean, *bn_rstd, *bn_scale, *bn_shift;
    int bn_y_pstride, bn_act;
    // dl_conv_forward_add: out = conv + addend (bf16, same pixels / channels as out); only the kernels dl_conv_add_supported() names read it
    const bf16_t *add;
    int add_pstride;
    int16_t taps[DL_MAX_TAPS];      // (dh & 0xff) | (dw << 8): tap_dh() / tap_dw()
};

__host__ __device__ __forceinline__ int tap_dh(int16_t t) { return (int)(int8_t)(t & 0xff); }
__host__ __device__ __forceinline__ int tap_dw(int16_t t) { return (int)(int8_t)((t >> 8) & 0xff); }

// 32-bit offsets: the kernels that address an image through one buffer resource need input and output each below 2^31 bytes per image (bf16)
static inline bool conv_fits_i32(const ConvArgs &a) {
    return (size_t)a.Hi * a.Wi * (size_t)a.in_pstride * 2 < ((size_t)1 << 31) && (size_t)a.Ho * a.Wo * (size_t)a.out_pstride * 2 < ((size_t)1 << 31);
}

// Strip height of the kernels whose workgroups walk down strips of rows (conv_s2d, conv_s2u, conv_d1, conv_d1g): the tallest divisor of `rows` among
// step, 2 step, ... that still gives `want` workgroups (`per_img` of them per strip), else the smallest such divisor; 0 when there is none.  Each strip
// re-reads its halo rows, so taller is cheaper once the chip is full.
static inline int strip_rows(int per_img, int rows, int step, int want) {
    int best = 0;
    for (int R = step; R <= rows; R += step) {
        if (rows % R) continue;
        const int wgs = per_img * (rows / R);
        if (best == 0 || wgs >= want) best = R;
        if (wgs < want) break;
    }
    return best;
}

// ---- the kernels of the other translation units, as conv_gemm.hip's dispatch reaches them
// conv_w4.hip: the one-wave-per-SIMD kernel of the ResnetBlock shape
bool w4_eligible(const ConvArgs &a);
int launch_conv_w4(const ConvArgs &a0, hipStream_t stream);
// conv_w4x3.hip: the same tile for the strict policy (split-copy activations, hi / lo weight images, three MFMAs per product)
bool w4x3_eligible(const ConvArgs &a);
int launch_conv_w4x3(const ConvArgs &a0, hipStream_t stream);
// conv_s2f.hip: the fused four-phase tile of the stride-2 layers (transposed conv forward, stride-2 data gradients)
bool s2f_eligible(const ConvArgs &a);
int s2f_stats_chunks(const ConvArgs &a);
int launch_conv_s2f(const ConvArgs &a0, hipStream_t stream);
// conv_s2f_x3.hip: the same tile under the strict policy (split-copy input, three products)
bool s2f_x3_eligible(const ConvArgs &a);
int launch_conv_s2f_x3(const ConvArgs &a0, hipStream_t stream);
// conv_d1.hip / conv_d1g.hip: the PatchGAN's first layer, forward and data gradient
bool d1_eligible(const ConvArgs &a);
int launch_conv_d1(const ConvArgs &a0, hipStream_t stream);
bool d1g_eligible(const ConvArgs &a);
int launch_conv_d1g(const ConvArgs &a0, hipStream_t stream);
// conv_dot.hip: the PatchGAN's one-channel prediction layer, forward and data gradient
bool dot_fwd_eligible(const ConvArgs &a);
bool dot_dgrad_eligible(const ConvArgs &a);
int launch_conv_dot(const ConvArgs &a, bool fwd, hipStream_t stream);
// conv_s2d.hip / conv_s2u.hip: the stride-2 down and up layers with the weights in registers
bool s2d_eligible(const ConvArgs &a);
int s2d_stats_chunks(const ConvArgs &a);
int launch_conv_s2d(const ConvArgs &a0, hipStream_t stream);
bool s2u_eligible(const ConvArgs &a);
int s2u_stats_chunks(const ConvArgs &a);
int launch_conv_s2u(const ConvArgs &a0, hipStream_t stream);

template <int CPR> __device__ __forceinline__ int swz_chunk(int row, int c) {
    if constexpr (CPR == 4) {
        // f(q) = {0,2,3,1}[q], q = (row >> 2) & 3
        const int q = (row >> 2) & 3;
        return c ^ ((0x1320 >> (4 * q)) & 3);
    } else {
        return c ^ ((row >> 1) & (CPR - 1));
    }
}

