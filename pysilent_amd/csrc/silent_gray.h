// Grayscale kernels (BASELINE configs 1 / 2 / 5): the streaming CS -> line-end stencil, the unit level fused with its pyramid
// smoother, and the single-read stream kernels that produce the whole pyramid from one read of the frame.
#pragma once

#include "silent_common.h"

namespace silent {

// ---------------------------------------------------------------------------------------------
// Fused grayscale pass (BASELINE configs 1/2/5):  cs = relu(conv3x3(x, cs_k));
//                                                 end = clip(relu(conv3x3(cs, end_bank)), 0, hi)
//
// Wave-autonomous streaming stencil: no LDS, no barrier.  A wave owns a strip of 64 columns (60 of
// them produce outputs) and walks down R rows.  Each lane loads its own column (one coalesced dword
// per row, all R+4 rows requested up front), receives the left / right neighbours by a DPP wave shift,
// keeps a 3x3 input window and a 3x3 CS window in registers, and emits one CS value and one K-vector
// per row.  Lanes 0/63 only feed their neighbours' CS, lanes 1/62 only feed their neighbours' outputs,
// so lanes 2..61 own the 60 output columns.  CS values outside the level are forced to 0 because the
// second convolution's SAME padding pads the CS MAP, not the input.  The dominant traffic (K floats
// per pixel, NHWC) leaves as one contiguous 60 x 4K-byte run per wave instruction.
struct GrayW {
    float cs[9];
    float end[9 * 8];  // [dy][dx][k], k < K
};

constexpr int kGrayCols = 60;            // output columns per wave
constexpr int kGrayTW = 4 * kGrayCols;   // 4 waves side by side
constexpr int kGrayTH = 16;              // rows per tile (R)

// K = 8: a pixel's 8 floats are 32 bytes, so "one float4 pair per lane" makes every store instruction write
// 16-byte pieces at a 32-byte stride (measured 3.1 TB/s vs 5.2 for K = 4).  Instead the wave transposes the
// row through a wave-private LDS slab: lane l then stores the l-th 16-byte piece of the row, so that each of
// the two store instructions covers 1 KiB of contiguous memory.  first / count: the lanes (= pixels of the
// wave's 64 columns) that may be written.  Every lane of the wave must call this (LDS exchange).
// NT: non-temporal stores (gray_stream_kernel: the map is a result nobody on the GPU reads back, and keeping it out of
// the caches leaves the Infinity Cache to the pyramid levels that gray_line_end_kernel reads next).
template <bool NT = false>
__device__ __forceinline__ void store_row_k8(float* __restrict__ row_base /* address of pixel of lane 0 */,
                                             const float (&acc)[8], float* s_slab /* 512 floats, wave private */,
                                             int lane, int first, int count) {
    typedef float nf4 __attribute__((ext_vector_type(4)));
    nf4* slab4 = reinterpret_cast<nf4*>(s_slab);
    slab4[lane * 2 + 0] = nf4{acc[0], acc[1], acc[2], acc[3]};
    slab4[lane * 2 + 1] = nf4{acc[4], acc[5], acc[6], acc[7]};
    __builtin_amdgcn_wave_barrier();
    const nf4 a = slab4[lane], b = slab4[64 + lane];
    __builtin_amdgcn_wave_barrier();
    // piece q (16 bytes) belongs to pixel q / 2
    const int pa = lane >> 1, pb = 32 + (lane >> 1);
    nf4* out4 = reinterpret_cast<nf4*>(row_base);
    if constexpr (NT) {
        if (pa >= first && pa < first + count) __builtin_nontemporal_store(a, out4 + lane);
        if (pb >= first && pb < first + count) __builtin_nontemporal_store(b, out4 + 64 + lane);
    } else {
        if (pa >= first && pa < first + count) out4[lane] = a;
        if (pb >= first && pb < first + count) out4[64 + lane] = b;
    }
}

// ---- float16 storage of the CS and end maps (the ST = gray_half instantiations, silent_gray_pass_h): every value is computed as
// float32 exactly as in the ST = float kernels and converted at the store, round-to-nearest-even (v_cvt_f16_f32: overflow to inf,
// NaN stays NaN, subnormals kept).  Only the store sites differ.  The pyramid stays float32.
typedef _Float16 gray_half;

// K = 8 with float16 storage: a pixel's 8 halves ARE one 16-byte piece, so the lanes' own stores already cover one contiguous run
// (60 x 16 bytes per wave instruction) -- the transpose through the LDS slab that the float32 row needs has nothing left to do.
template <bool NT = false>
__device__ __forceinline__ void store_row_k8(gray_half* __restrict__ row_base /* address of pixel of lane 0 */, const float (&acc)[8],
                                             float* /* no slab */, int lane, int first, int count) {
    typedef gray_half nh8 __attribute__((ext_vector_type(8)));
    const nh8 v = {(gray_half)acc[0], (gray_half)acc[1], (gray_half)acc[2], (gray_half)acc[3],
                   (gray_half)acc[4], (gray_half)acc[5], (gray_half)acc[6], (gray_half)acc[7]};
    nh8* out8 = reinterpret_cast<nh8*>(row_base);
    if (lane >= first && lane < first + count) {
        if constexpr (NT) __builtin_nontemporal_store(v, out8 + lane);
        else out8[lane] = v;
    }
}

// A lane's K end values of one pixel (po: that pixel).  ST = float: the stores of the float32 kernels, verbatim.  ST = gray_half:
// K = 4 one 8-byte store (8 bytes per pixel: always aligned), K = 3 three 2-byte stores.
template <int K, bool NT, typename ST>
__device__ __forceinline__ void store_end_px(ST* __restrict__ po, const float (&acc)[K]) {
    static_assert(K == 3 || K == 4, "K = 8 rows go through store_row_k8");
    if constexpr (K == 4) {
        typedef ST v4 __attribute__((ext_vector_type(4)));
        const v4 v = {(ST)acc[0], (ST)acc[1], (ST)acc[2], (ST)acc[3]};
        if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<v4*>(po));
        else *reinterpret_cast<v4*>(po) = v;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) po[k] = (ST)acc[k];
    }
}

// One row of the float16 CS map: lanes first .. first + count - 1 of the wave hold the float32 values of consecutive pixels, row0 is
// the address of lane 0's pixel.  2 bytes per pixel: a plain per-lane store would be a 2-byte store instruction, the slowest per
// byte of the store table (MI355X_MICROARCH).  PAIRED form: the lane whose pixel sits on a 4-byte boundary takes its right
// neighbour's half by DPP and stores one dword; which lane parity that is depends on the row's address (rows of an odd-width
// level, or a level at an odd pixel offset, start on a 2-byte boundary only), so it is chosen per row from row0.  The first pixel
// of an odd-aligned run and the last pixel of a run that ends on an even one have no partner: those (at most two lanes) store
// 2 bytes.  SILENT_F16_CS_PAIRED = 0 builds the plain form for A/B timing.
#ifndef SILENT_F16_CS_PAIRED
#define SILENT_F16_CS_PAIRED 1
#endif
template <bool NT>
__device__ __forceinline__ void store_cs_row(gray_half* __restrict__ row0, float v, int lane, int first, int count) {
    const gray_half h = (gray_half)v;
    const unsigned mine = (unsigned)__builtin_bit_cast(unsigned short, h);
    const bool own = lane >= first && lane < first + count;
#if SILENT_F16_CS_PAIRED
    const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);   // lane + 1's
    const int odd0 = (int)((reinterpret_cast<unsigned long long>(row0) >> 1) & 1ull);   // wave-uniform: lane 0's pixel is off the dword grid
    const bool lead = ((lane + odd0) & 1) == 0;                                          // this lane's pixel starts a dword
    const bool pair = own && lead && lane + 1 < first + count;
    const bool single = own && (lead ? lane + 1 >= first + count : lane == first);
    if (pair) {
        unsigned* p = reinterpret_cast<unsigned*>(row0 + lane);
        if constexpr (NT) __builtin_nontemporal_store(mine | (up << 16), p);
        else *p = mine | (up << 16);
    }
    if (single) {
        unsigned short* p = reinterpret_cast<unsigned short*>(row0 + lane);
        if constexpr (NT) __builtin_nontemporal_store((unsigned short)mine, p);
        else *p = (unsigned short)mine;
    }
#else
    if (own) {
        unsigned short* p = reinterpret_cast<unsigned short*>(row0 + lane);
        if constexpr (NT) __builtin_nontemporal_store((unsigned short)mine, p);
        else *p = (unsigned short)mine;
    }
#endif
}
template <typename ST>
constexpr bool kStoreHalf = std::is_same<ST, gray_half>::value;
// The K end values of a lane's pixel in the gray_stream_kernel's row `row0` (lane 0's pixel), K < 8: float16 through store_end_px; float32
// K = 4 as one NON-TEMPORAL 16-byte store like the two 4-byte maps of that kernel (whole pass -1.6 %, the kernel alone -0.7 %: the rest
// is gray_line_end_kernel finding more of the pyramid's levels >= 1 in the Infinity Cache); other K as plain stores.
template <int K, typename ST>
__device__ __forceinline__ void store_end_lane(ST* __restrict__ row0, int lane, const float (&acc)[K]) {
    if constexpr (kStoreHalf<ST>) {
        store_end_px<K, K == 4>(row0 + lane * K, acc);   // (non-temporal where the float32 row is: K = 4)
    } else if constexpr (K == 4) {
        typedef float nf4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(nf4{acc[0], acc[1], acc[2], acc[3]}, reinterpret_cast<nf4*>(row0) + lane);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) row0[lane * K + k] = acc[k];
    }
}

// ---- keypoint epilogue (KP instantiations, silent_gray_keypoints): the selection tail's inputs from the registers that hold a
// pixel's K end values, so that nothing re-reads the end map for a reduction.  Per pixel the value of the PADDED map, with the
// operations of pad_inwards_kernel (m * e) and value_from_color_kernel (sum left to right, one multiply by 1/K); per lane the
// running max_pool(value) / max_pool(-value) and the summary group's maximum (pool_max: NaNs never win, like level_maxmin_kernel);
// per wave one atomic pair per tile and a NaN flag.  The summary entry of a pixel pair is stored by its even lane: every wave
// starts at an even column, so the pair partner is lane ^ 1.  Every pointer of GrayKp may be NULL (that part is skipped).
struct GrayKp {
    unsigned* mm;                      // [n_frames][n_levels][2] ordered-uint max_pool(value) / max_pool(-value) (silent_peaks.h)
    float* sum;                        // value summary (SumTab geometry, th = the kernel's tile height)
    int* nan_flags;                    // [n_frames][n_levels]: set to 1 when a value of that level is a NaN (with mm)
    float* value_out;                  // the 1-channel value map
    long long sum_frame;               // summary entries per frame
    long long sum_off[kMaxLevels];     // entry offset of level l inside a frame
    int n_levels, pad, gpt;            // gpt: summary groups per tile row
    int level[kMaxLevels];             // gray_unit_fused_kernel / gray_stream_kernel: plan level of unit level li
};

struct GrayKpAcc {
    float mx = kPoolLowest, nmn = kPoolLowest, grp = kPoolLowest;
    bool nan = false;
};

template <int K>
__device__ __forceinline__ void gray_kp_pixel(const GrayKp& kp, const float (&acc)[K], int y, int x, int H, int W, bool valid,
                                              float* __restrict__ value_px, GrayKpAcc& a) {
    const float m = (y >= kp.pad && y < H - kp.pad && x >= kp.pad && x < W - kp.pad) ? 1.0f : 0.0f;
    float s = __fmul_rn(m, acc[0]);
#pragma unroll
    for (int k = 1; k < K; ++k) s = __fadd_rn(s, __fmul_rn(m, acc[k]));
    const float v = __fmul_rn(s, 1.0f / (float)K);
    if (valid) {
        a.mx = pool_max(a.mx, v);
        a.nmn = pool_max(a.nmn, -v);
        a.grp = pool_max(a.grp, v);
        a.nan = a.nan || v != v;
        if (kp.value_out) *value_px = v;
    }
}

// end of summary group g of tile row ty (every lane of the wave calls it)
__device__ __forceinline__ void gray_kp_group_end(const GrayKp& kp, GrayKpAcc& a, int frame, int level, int ty, int g, int x, int W,
                                                  bool out_lane) {
    if (!kp.sum) return;
    const float pair = pool_max(a.grp, __shfl_xor(a.grp, 1));
    const int nxp = (W + 1) >> 1;
    if (out_lane && !(x & 1))
        kp.sum[(long long)frame * kp.sum_frame + kp.sum_off[level] + ((long long)ty * kp.gpt + g) * nxp + (x >> 1)] = pair;
    a.grp = kPoolLowest;
}

// end of the tile (every lane of the wave calls it)
__device__ __forceinline__ void gray_kp_tile_end(const GrayKp& kp, const GrayKpAcc& a, int frame, int level, int lane) {
    if (!kp.mm) return;
    const float mx = wave_max(a.mx), nmn = wave_max(a.nmn);
    const bool nan = __ballot(a.nan) != 0ull;
    if (lane == 0) {
        unsigned* slot = kp.mm + ((long long)frame * kp.n_levels + level) * 2;
        atomicMax(slot, f2ord(mx));
        atomicMax(slot + 1, f2ord(nmn));
        if (nan && kp.nan_flags) kp.nan_flags[frame * kp.n_levels + level] = 1;
    }
}

// (summary groups: kSumRows output rows; a tile's last group may be shorter)
__host__ __device__ constexpr bool kp_group_ends(int k, int R) { return ((k + 1) % kSumRows) == 0 || k == R - 1; }

// ---- the F64 kernels' tap chains in the oracle's order (acc = 0, then dy and dx ascending, one fma per tap), summed in float64 and
// rounded once (the float32 kernels keep their own chains).  gray_cs_f64: the CS sum before its relu; gray_end_f64: the K end values
// after relu + clip.  w: the float32 weights (registers or kernel arguments), widened in registers -- exact.
__device__ __forceinline__ float gray_cs_f64(const float (&iw)[3][3], const float* w) {
    double acc = 0.0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc = __builtin_fma((double)iw[dy][dx], (double)w[dy * 3 + dx], acc);
    return (float)acc;
}
template <int K>
__device__ __forceinline__ void gray_end_f64(const float (&cw)[3][3], const float* w, float clip_hi, float (&out)[K]) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = __builtin_fma((double)cw[dy][dx], (double)w[(dy * 3 + dx) * K + k], acc[k]);
    // relu + clip in the reference's select forms only: a value rounded from a float64 sum can be -0 (a negative sum below half the
    // smallest float32 denormal), which the oracle keeps and relu_clip_tf's v_med3 form need not
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = clip_hi_tf(relu_tf((float)acc[k]), clip_hi);
}
// vertical six taps of a unit level in float64, rounded once
__device__ __forceinline__ float unit_vsum_f64(const double (&w)[6], const double (&h)[6]) {
    double v = w[0] * h[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) v = __builtin_fma(w[j], h[j], v);
    return (float)v;
}

template <int K, int R, bool KP = false, bool F64 = false, typename ST = float>
__global__ __launch_bounds__(256) void gray_line_end_kernel(const float* __restrict__ pyr,
                                                            ST* __restrict__ cs_out,
                                                            ST* __restrict__ end_out, const LevelTab tab,
                                                            const GrayW wts, float clip_hi, unsigned opts,
                                                            const GrayKp kp = GrayKp{}) {
    static_assert(!kStoreHalf<ST> || (!KP && !F64), "float16 storage: no keypoint epilogue, no float64 accumulation");
    __shared__ __attribute__((aligned(16))) float s_slab[K == 8 && !kStoreHalf<ST> ? 4 * 512 : 4];  // K = 8 store transpose, per wave
    const TileCoord tc = locate_tile(tab, (opts & 1u) ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x);
    const int H = tab.h[tc.level], W = tab.w[tc.level];
    const long long base_px = (long long)tc.frame * tab.frame_px + tab.px_off[tc.level];
    const float* __restrict__ src = pyr + base_px;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xw0 = tc.tx * kGrayTW + wave * kGrayCols;  // first output column of this wave
    if (xw0 >= W) return;                                // wave-uniform
    const int y0 = tc.ty * R;
    const int x = xw0 + lane - 2;
    const bool col_ok = x >= 0 && x < W;
    const int xc = min(max(x, 0), W - 1);

    // all R+4 input rows of this lane's column, requested before the first use (clamped address +
    // select: no branch around a load)
    float in[R + 4];
#pragma unroll
    for (int i = 0; i < R + 4; ++i) {
        const int y = y0 - 2 + i;
        const bool row_ok = y >= 0 && y < H;
        const float v = src[(long long)min(max(y, 0), H - 1) * W + xc];
        in[i] = (row_ok && col_ok) ? v : 0.0f;
    }
    // Retire every requested row here.  Loads and stores share vmcnt in issue order, so a counted wait
    // for a late row inside the loop below would also wait for the previous rows' STORES to be
    // acknowledged; with the loads retired up front the row loop carries no vector-memory wait at all.
#pragma unroll
    for (int i = 0; i < R + 4; ++i) asm volatile("" ::"v"(in[i]));

    float iw[3][3], cw[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) iw[a][b] = cw[a][b] = 0.0f;
    const bool out_lane = lane >= 2 && lane < 2 + kGrayCols && x < W;
    GrayKpAcc ka;

#pragma unroll
    for (int i = 0; i < R + 4; ++i) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            iw[0][b] = iw[1][b];
            iw[1][b] = iw[2][b];
        }
        iw[2][1] = in[i];
        iw[2][0] = from_lane_below(in[i]);
        iw[2][2] = from_lane_above(in[i]);
        if (i >= 2) {
            const int cy = y0 + i - 3;  // CS row produced by this step
            float acc = 0.0f;
            if constexpr (F64) {
                acc = gray_cs_f64(iw, wts.cs);
            } else {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) acc = __builtin_fmaf(iw[dy][dx], wts.cs[dy * 3 + dx], acc);
            }
            float cs = relu_tf(acc);
            cs = (cy >= 0 && cy < H && col_ok) ? cs : 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                cw[0][b] = cw[1][b];
                cw[1][b] = cw[2][b];
            }
            cw[2][1] = cs;
            cw[2][0] = from_lane_below(cs);
            cw[2][2] = from_lane_above(cs);
        }
        if (i >= 4) {
            const int y = y0 + i - 4;  // output row
            if (y < H) {               // wave-uniform
                const long long px = base_px + (long long)y * W + x;
                if constexpr (kStoreHalf<ST>) {
                    if (cs_out) store_cs_row<false>(cs_out + (base_px + (long long)y * W + (xw0 - 2)), cw[1][1], lane, 2, min(kGrayCols, W - xw0));
                } else if (cs_out && out_lane) {
                    cs_out[px] = cw[1][1];  // (non-temporal here: within noise, unlike in gray_stream_kernel)
                }
                if (end_out) {
                    float acc[K];
                    if constexpr (F64) {
                        gray_end_f64<K>(cw, wts.end, clip_hi, acc);
                    } else {
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k] = 0.0f;
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                                for (int k = 0; k < K; ++k)
                                    acc[k] = __builtin_fmaf(cw[dy][dx], wts.end[(dy * 3 + dx) * K + k], acc[k]);
                        relu_clip_tf(acc, clip_hi);
                    }
                    if constexpr (KP) gray_kp_pixel<K>(kp, acc, y, x, H, W, out_lane, kp.value_out + px, ka);
                    if constexpr (K == 8) {
                        // lane 0's pixel is column xw0 - 2; valid pixels are lanes 2 .. 2 + ncols
                        const int ncols = min(kGrayCols, W - xw0);
                        store_row_k8(end_out + (base_px + (long long)y * W + (xw0 - 2)) * 8, acc, s_slab + wave * 512, lane,
                                     2, ncols);
                    } else if (out_lane) {
                        ST* __restrict__ po = end_out + px * K;
                        if constexpr (kStoreHalf<ST>) {
                            store_end_px<K, false>(po, acc);
                        } else if constexpr (K == 4) {
                            typedef float nf4 __attribute__((ext_vector_type(4)));
                            const nf4 v4 = {acc[0], acc[1], acc[2], acc[3]};
                            *reinterpret_cast<nf4*>(po) = v4;
                        } else {
#pragma unroll
                            for (int k = 0; k < K; ++k) po[k] = acc[k];
                        }
                    }
                }
            }
            if constexpr (KP) {
                if (kp_group_ends(i - 4, R)) gray_kp_group_end(kp, ka, tc.frame, tc.level, tc.ty, (i - 4) / kSumRows, x, W, out_lane);
            }
        }
    }
    if constexpr (KP) gray_kp_tile_end(kp, ka, tc.frame, tc.level, lane);
}

// ---------------------------------------------------------------------------------------------
// Unit-zoom level, pyramid AND filters in one pass (the whole hot path for level 0, 75 % of all pixels):
//     p   = smooth5x5(frame)               -> pyramid level   (scipy zoom factor 1 = [1,26,66,26,1]/120 per axis)
//     cs  = relu(conv3x3(p, cs_k))         -> CS map
//     end = clip(relu(conv3x3(cs, bank)))  -> K-orientation line-end maps
// Same wave-autonomous streaming structure as gray_line_end_kernel, with the 5-tap smoother in front: the
// level is never re-read from HBM by the filter pass.  Each stage costs halo lanes (2 + 1 + 1 per side):
// 56 of the 64 lanes produce outputs; a tile is 224 columns x 16 rows and streams 24 source rows.
#ifndef SILENT_FUSED_COLS
#define SILENT_FUSED_COLS 56
#endif
constexpr int kFusedCols = SILENT_FUSED_COLS;
static_assert(kFusedCols >= 16 && kFusedCols <= 56 && kFusedCols % 4 == 0, "64 lanes = output columns + 4 halo lanes per side");
#ifndef SILENT_FUSED_WAVES
#define SILENT_FUSED_WAVES 4
#endif
// waves side by side in a block of the fused / stream kernels (autonomous: no barrier).  4 x 56 columns = 896 bytes = 7 whole
// 128-byte lines per tile row; measured on config 2 (gray_stream_kernel alone): 1 wave 1.06 ms, 2 waves 0.93, 4 waves 0.85,
// 5 waves (1120 bytes: tile edges off the line grid) 1.03, 8 waves 0.89
constexpr int kFusedWaves = SILENT_FUSED_WAVES;
constexpr int kFusedTW = kFusedWaves * kFusedCols;
#ifndef SILENT_FUSED_TH
#define SILENT_FUSED_TH 16
#endif
// output rows per tile of the fused / stream kernels; a tile streams TH + 8 source rows.  Round 4 tried 24 / 32 / 40 / 48 rows
// (32: the stream kernel fetches 40 rows per 32 produced instead of 24 per 16 -- read amplification 1.43x instead of 1.79x with
// the column halo -- at 40 KB instead of 24 KB of LDS per block, 4 instead of 6 waves / SIMD): in bursts of 5 steps on a fast box
// 32 rows won 1.9 % of the config-2 step (profiles/r04/evidence/ab_gray_tile_height.txt), through bench.py's settled 30-step
// windows on a slow box they LOST 8 % (step 1.154 against 1.066 ms, kernel 0.944 against 0.852; 40 rows the same, 48 rows 16 %;
// config 5: +1 % / +9 % / +10 %; profiles/r04/evidence/ab_gray_tile_height_bench.txt).  16 stays: the contract number is the
// settled one, and most boxes of the pool are of the slow kind.
constexpr int kFusedTH = SILENT_FUSED_TH;

struct FusedLevel {  // the unit levels of a pyramid plan, as the kernel needs them
    int src_y0, src_x0, src_h, src_w;  // crop of the frame (mirror extension happens inside the crop)
    int zoom_h, zoom_w, out_h, out_w;  // resampler extents (== crop) and canvas extents
    int tiles_x, tile_start;
    long long px_off;                  // pixel offset of the level inside one pyramid
};

struct FusedTab {
    int n, tiles_per_frame, H, W;
    long long frame_px;                // pixels of one whole pyramid (all levels)
    float wx[6], wy[6];                // scipy's SIX taps of a zoom-1 level: [1, 26, 66, 26, 1] / 120 and 2^-53 (unit_taps6)
    FusedLevel lv[kMaxLevels];
};
// F64 kernels: the same taps in float64 (the same on both axes)
struct FusedTab64 : FusedTab {
    double w64[6];
};
template <bool F64>
using FusedTabT = typename std::conditional<F64, FusedTab64, FusedTab>::type;

template <int K, int R, bool KP = false, bool F64 = false, typename ST = float, typename FT = float>
__global__ __launch_bounds__(64 * kFusedWaves) void gray_unit_fused_kernel(frame_param<FT> frames,
                                                              float* __restrict__ pyr, ST* __restrict__ cs_out,
                                                              ST* __restrict__ end_out, const FusedTabT<F64> tab,
                                                              const GrayW wts, float clip_hi, const GrayKp kp = GrayKp{}) {
    static_assert(!kStoreHalf<ST> || (!KP && !F64), "float16 storage: no keypoint epilogue, no float64 accumulation");
    static_assert(kFrameType<FT> && (!kFrameNarrow<FT> || !F64), "uint8 / uint16 frames: float32 accumulation only");
    __shared__ __attribute__((aligned(16))) float s_slab[K == 8 && !kStoreHalf<ST> ? kFusedWaves * 512 : 4];  // K = 8 store transpose, per wave
    const unsigned bid = blockIdx.x;
    const int frame = (int)(bid / (unsigned)tab.tiles_per_frame);
    int rem = (int)(bid - (unsigned)frame * (unsigned)tab.tiles_per_frame);
    int li = 0;
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (i < tab.n && rem >= tab.lv[i].tile_start) li = i;
    const FusedLevel& lv = tab.lv[li];
    rem -= lv.tile_start;
    const int ty = rem / lv.tiles_x, tx = rem - ty * lv.tiles_x;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xw0 = tx * kFusedTW + wave * kFusedCols;
    if (xw0 >= lv.out_w) return;  // wave-uniform
    const int y0 = ty * R;
    const int ox = xw0 + lane - 4;
    const int W = tab.W;
    frame_src<FT> src;
    if constexpr (kFrameStrided<FT>) src = frame_of(frames, frame);
    else src = frames + (long long)frame * tab.H * W;
    const long long base_px = (long long)frame * tab.frame_px + lv.px_off;

    // scipy 'mirror' inside the crop, then the crop's offset in the frame
    const long long sx = mirror_near(ox, lv.src_w) + lv.src_x0;
    float in[R + 9];                                                  // stream rows y0 - 4 .. y0 + R + 4 (the sixth tap: + 1 row)
#pragma unroll
    for (int i = 0; i < R + 9; ++i)
    {
        if constexpr (kFrameStrided<FT>) in[i] = src.at(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0, sx);
        else in[i] = (float)src[(long long)(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0) * W + sx];
    }
    float xcol = unit_edge_column(src, W, xw0 + 60, lv.src_w, lv.src_x0, y0 - 4, R + 9, lv.src_h, lv.src_y0, lane);
#pragma unroll
    for (int i = 0; i < R + 9; ++i) asm volatile("" ::"v"(in[i]));  // retire loads before the first store
    asm volatile("" : "+v"(xcol));

    const bool col_in = ox >= 0 && ox < lv.out_w;                  // inside the level (SAME padding is 0 outside)
    const bool out_lane = lane >= 4 && lane < 4 + kFusedCols && ox < lv.out_w;
    GrayKpAcc ka;
    acc_t<F64> hw[6] = {0, 0, 0, 0, 0, 0};
    float iw[3][3], cw[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) iw[a][b] = cw[a][b] = 0.0f;

#pragma unroll
    for (int i = 0; i < R + 9; ++i) {
        // ---- horizontal taps of source row y0 - 4 + i
        {
            acc_t<F64> h;
            if constexpr (F64) h = unit_taps6(in[i], unit_edge(xcol, i), tab.w64);
            else h = unit_taps6(in[i], unit_edge(xcol, i), tab.wx);
#pragma unroll
            for (int j = 0; j < 5; ++j) hw[j] = hw[j + 1];
            hw[5] = h;
        }
        if (i >= 5) {
            // ---- pyramid row p = y0 + i - 7 (vertical taps p - 2 .. p + 3)
            const int p = y0 + i - 7;
            float v;
            if constexpr (F64) {
                v = unit_vsum_f64(tab.w64, hw);
            } else {
                v = tab.wy[0] * hw[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) v = __builtin_fmaf(tab.wy[j], hw[j], v);
            }
            v = (p < lv.zoom_h && ox < lv.zoom_w) ? v : 0.0f;                 // canvas beyond the zoomed crop
            if (p >= y0 && p < y0 + R && p < lv.out_h && out_lane) pyr[base_px + (long long)p * lv.out_w + ox] = v;
            v = (p >= 0 && p < lv.out_h && col_in) ? v : 0.0f;                // SAME zero padding of the first conv
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                iw[0][b] = iw[1][b];
                iw[1][b] = iw[2][b];
            }
            iw[2][1] = v;
            iw[2][0] = from_lane_below(v);
            iw[2][2] = from_lane_above(v);
        }
        if (i >= 7) {
            // ---- CS row c = y0 + i - 8
            const int c = y0 + i - 8;
            float acc = 0.0f;
            if constexpr (F64) {
                acc = gray_cs_f64(iw, wts.cs);
            } else {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) acc = __builtin_fmaf(iw[dy][dx], wts.cs[dy * 3 + dx], acc);
            }
            float cs = relu_tf(acc);
            cs = (c >= 0 && c < lv.out_h && col_in) ? cs : 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                cw[0][b] = cw[1][b];
                cw[1][b] = cw[2][b];
            }
            cw[2][1] = cs;
            cw[2][0] = from_lane_below(cs);
            cw[2][2] = from_lane_above(cs);
        }
        if (i >= 9) {
            // ---- output row y = y0 + i - 9
            const int y = y0 + i - 9;
            if (y < lv.out_h) {  // wave-uniform
                const long long px = base_px + (long long)y * lv.out_w + ox;
                if constexpr (kStoreHalf<ST>) {
                    if (cs_out)
                        store_cs_row<false>(cs_out + (base_px + (long long)y * lv.out_w + (xw0 - 4)), cw[1][1], lane, 4,
                                            min(kFusedCols, lv.out_w - xw0));
                } else if (cs_out && out_lane) cs_out[px] = cw[1][1];  // (non-temporal here: 6 % SLOWER, unlike in gray_stream_kernel)
                if (end_out) {
                    float acc[K];
                    if constexpr (F64) {
                        gray_end_f64<K>(cw, wts.end, clip_hi, acc);
                    } else {
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k] = 0.0f;
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                                for (int k = 0; k < K; ++k)
                                    acc[k] = __builtin_fmaf(cw[dy][dx], wts.end[(dy * 3 + dx) * K + k], acc[k]);
                        relu_clip_tf(acc, clip_hi);
                    }
                    if constexpr (KP) gray_kp_pixel<K>(kp, acc, y, ox, lv.out_h, lv.out_w, out_lane, kp.value_out + px, ka);
                    if constexpr (K == 8) {
                        const int ncols = min(kFusedCols, lv.out_w - xw0);
                        store_row_k8(end_out + (base_px + (long long)y * lv.out_w + (xw0 - 4)) * 8, acc,
                                     s_slab + wave * 512, lane, 4, ncols);
                    } else if (out_lane) {
                        ST* __restrict__ po = end_out + px * K;
                        if constexpr (kStoreHalf<ST>) {
                            store_end_px<K, false>(po, acc);
                        } else if constexpr (K == 4) {
                            *reinterpret_cast<float4*>(po) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                        } else {
#pragma unroll
                            for (int k = 0; k < K; ++k) po[k] = acc[k];
                        }
                    }
                }
            }
            if constexpr (KP) {
                if (kp_group_ends(i - 9, R)) gray_kp_group_end(kp, ka, frame, kp.level[li], ty, (i - 9) / kSumRows, ox, lv.out_w, out_lane);
            }
        }
    }
    if constexpr (KP) gray_kp_tile_end(kp, ka, frame, kp.level[li], lane);
}

// ---------------------------------------------------------------------------------------------
// gray_stream_kernel: the fused unit-level kernel above, PLUS the pyramid of every other level, from the
// same single stream of frame rows (the frame is read once for the whole pyramid).
//
// Eligible plans (host-checked): one unit level, and every other level resamples the SAME crop with a
// step of at least 1.4 source pixels per output pixel (classic whole-frame pyramids; the reference layout, whose
// levels are different crops, keeps the region kernel).
//
// Pass 1 (registers, fully unrolled) is exactly gray_unit_fused_kernel; on the way the wave also drops its
// 24 streamed rows into a wave-private LDS slab.  Pass 2 is a compact ROLLED loop over those rows for the
// other levels.  Vertical pass of level g: the lane holds its own column, so it keeps up to 4 output rows of
// level g in flight (slot = output row mod 4) and adds w * value per row.  Which slot gets which weight at
// which stream row, which slot restarts and which one completes is a tiny per-tile ROW PROGRAM built by the
// host from the same float64 tap tables (8 dwords per level and stream row), staged into LDS once per block.
// Horizontal pass of a completed row: the outputs anchored in the wave's 56 columns gather their 6 taps from
// the other lanes with ds_bpermute (lane = tap position - first column of the wave) and store one coalesced
// run.  Arithmetic order = region kernel's (vertical then horizontal, taps ascending): bit-identical output.
constexpr int kStreamSlots = 5;   // (the most of any layout)
// Output rows of general level number g that can be in flight at once (their vertical taps overlap), host-checked per plan.
// Layout 0: 4, 3, 2, 2, then 1 -- enough for zoom ladders of ratio >= e^0.5 (the reference's default) and 2.  Layout 1 (round 5,
// "dense" ladders down to a ratio of 1.4, e.g. sqrt 2): 5, 4, 3, 2, 2, 1, 1, always instantiated for 7 levels.  The host tries 0 first.
__host__ __device__ constexpr int stream_slots(int layout, int g) {
    return layout == 0 ? (g == 0 ? 4 : (g == 1 ? 3 : (g <= 3 ? 2 : 1))) : (g == 0 ? 5 : (g == 1 ? 4 : (g == 2 ? 3 : (g <= 4 ? 2 : 1))));
}
constexpr int kStreamRows = kFusedTH + 8;
// Row program, one record per stream row of a tile row, padded to the kernel's template G (4 or 7 levels):
//   [meta(0) .. meta(Gp-1)] [weights of level 0 (4)] [level 1 (3)] [level 2 (2)] ... ; kStreamProgRow(layout, Gp) dwords.
// It is wave-uniform data: the kernel reads it with scalar loads, one record ahead of the row it is working on.
__host__ __device__ constexpr int stream_pad_levels(int g) { return g <= 4 ? 4 : 7; }
// F64 plans: every weight is a float64 in two dwords (low, high): [meta] [level 0 (2 x 4)] [level 1 (2 x 3)] ...
__host__ __device__ constexpr int stream_w_off(int layout, int gp, int g, bool f64 = false) {
    int o = gp;
    for (int h = 0; h < g; ++h) o += stream_slots(layout, h) * (f64 ? 2 : 1);
    return o;
}
__host__ __device__ constexpr int kStreamProgRow(int layout, int gp, bool f64 = false) {   // layout 0: 16 / 24 (F64: 28 / 36)
    return (stream_w_off(layout, gp, gp, f64) + 3) / 4 * 4;
}
// dwords per column record: lane of tap 0, 6 float32 weights, pad; F64 plans: lane, pad, 6 float64 weights, 2 pad
__host__ __device__ constexpr int stream_rec_ints(bool f64) { return f64 ? 16 : 8; }
// meta: bits 0.. "slot restarts", 3 bits completing slot (7 = none), bit 7 "row feeds this level", then the output row
__host__ __device__ constexpr int stream_done_shift(int layout) { return layout == 0 ? 4 : 8; }
__host__ __device__ constexpr int stream_row_shift(int layout) { return layout == 0 ? 8 : 12; }

struct StreamTab {
    int G;                        // general levels handled here (<= template G; extra ones are inert)
    int tiles_y, waves_x;         // tile rows of the unit level, 56-column wave tiles per row
    const int* row_prog;          // [tiles_y][kStreamRows][kStreamProgRow(Gp)], Gp = stream_pad_levels(G)
    const int* col_hdr;           // [G][waves_x][2]: first output column, number of outputs
    const int* col_rec;           // [G][waves_x][64][stream_rec_ints(F64)]: lane of tap 0 + the 6 horizontal weights
    long long px_off[8];          // pixel offset of level g inside one pyramid
    int out_w[8];
};

// A lane's column record of general level g: where its run of outputs starts, how many outputs the wave has, and for output
// `lane` of the run the lane that holds tap 0 (as a ds_bpermute byte index) + the 6 horizontal weights.
struct StreamCol {
    int x0, n, lane4;
    float w[6];
};
__device__ __forceinline__ StreamCol stream_col(const StreamTab& st, int g, int wx_tile, int lane) {
    const int gg = min(g, st.G - 1);
    const int* __restrict__ h = st.col_hdr + ((long long)gg * st.waves_x + wx_tile) * 2;
    const int4* __restrict__ rec = reinterpret_cast<const int4*>(st.col_rec + (((long long)gg * st.waves_x + wx_tile) * 64 + lane) * 8);
    const int4 a = rec[0], b = rec[1];
    StreamCol c;
    c.x0 = h[0];
    c.n = g < st.G ? h[1] : 0;
    c.lane4 = a.x * 4;
    c.w[0] = __int_as_float(a.y);
    c.w[1] = __int_as_float(a.z);
    c.w[2] = __int_as_float(a.w);
    c.w[3] = __int_as_float(b.x);
    c.w[4] = __int_as_float(b.y);
    c.w[5] = __int_as_float(b.z);
    return c;
}
// the same from an F64 plan's records
struct StreamCol64 {
    int x0, n, lane4;
    double w[6];
};
__device__ __forceinline__ StreamCol64 stream_col64(const StreamTab& st, int g, int wx_tile, int lane) {
    const int gg = min(g, st.G - 1);
    const int* __restrict__ h = st.col_hdr + ((long long)gg * st.waves_x + wx_tile) * 2;
    const int4* __restrict__ rec = reinterpret_cast<const int4*>(st.col_rec + (((long long)gg * st.waves_x + wx_tile) * 64 + lane) * 16);
    const int4 a = rec[0], b = rec[1], d = rec[2], e = rec[3];
    StreamCol64 c;
    c.x0 = h[0];
    c.n = g < st.G ? h[1] : 0;
    c.lane4 = a.x * 4;
    c.w[0] = __hiloint2double(a.w, a.z);
    c.w[1] = __hiloint2double(b.y, b.x);
    c.w[2] = __hiloint2double(b.w, b.z);
    c.w[3] = __hiloint2double(d.y, d.x);
    c.w[4] = __hiloint2double(d.w, d.z);
    c.w[5] = __hiloint2double(e.y, e.x);
    return c;
}
template <bool F64>
using StreamColT = typename std::conditional<F64, StreamCol64, StreamCol>::type;
template <bool F64>
__device__ __forceinline__ StreamColT<F64> stream_col_t(const StreamTab& st, int g, int wx_tile, int lane) {
    if constexpr (F64) return stream_col64(st, g, wx_tile, lane);
    else return stream_col(st, g, wx_tile, lane);
}
// Pass 2 of an F64 stream kernel for general level g on stream row value c0 (the float32 kernels spell it out inline): the vertical
// taps of this row into the level's slots (float64 weights from the row program), and a completed row's horizontal taps -- the
// float64 vertical sum gathered from the tap lanes with two permutes per tap -- rounded once and stored at px.
template <int L, int G, int GR, int PR>
__device__ __forceinline__ void stream_level_f64(int g, const int (&cur)[PR], float c0, double (&vacc)[kStreamSlots],
                                                 const StreamCol64 (&col)[GR > 0 ? GR : 1], const StreamTab& st, int wx_tile, int lane,
                                                 float* __restrict__ pyr, long long frame_px0, int C, int ch) {
    const int meta = cur[g];
#pragma unroll
    for (int k = 0; k < stream_slots(L, g); ++k) {
        const int e = stream_w_off(L, G, g, true) + 2 * k;
        const double w = __hiloint2double(cur[e + 1], cur[e]);
        const double prev = (meta >> k) & 1 ? 0.0 : vacc[k];
        vacc[k] = __builtin_fma(w, (double)c0, prev);
    }
    const int done = (meta >> stream_done_shift(L)) & 7;
    if (done != 7) {  // wave-uniform
        const int oy = meta >> stream_row_shift(L);
        double v = vacc[0];
#pragma unroll
        for (int k = 1; k < stream_slots(L, g); ++k) v = done == k ? vacc[k] : v;
        const StreamCol64 cr = g < GR ? col[g < GR ? g : 0] : stream_col64(st, g, wx_tile, lane);
        double acc = cr.w[0] * bpermute_f64(cr.lane4, v);
#pragma unroll
        for (int t = 1; t < 6; ++t) acc = __builtin_fma(cr.w[t], bpermute_f64(cr.lane4 + 4 * t, v), acc);
        if (lane < cr.n) pyr[(frame_px0 + st.px_off[g] + (long long)oy * st.out_w[g] + cr.x0 + lane) * C + ch] = (float)acc;
    }
}
// The first kStreamRegLevels general levels keep their column records in registers for the whole tile (a row of level 0 completes
// every other stream row); the smaller levels -- one completed row per 2, 4, 8 tiles -- fetch theirs when a row completes.  With all
// seven resident the <K, 7> instantiations sat at 125 VGPRs = 4 waves / SIMD (63 registers of records); now they run at the <K, 4>
// instantiations' 5 - 6 waves (profiles/r05_config5/README.md).
#ifndef SILENT_STREAM_REG_LEVELS
#define SILENT_STREAM_REG_LEVELS 3
#endif
constexpr int kStreamRegLevels = SILENT_STREAM_REG_LEVELS;

// The instantiations whose waves choose between two tile bodies (below), with row pointers and the copy-free pass 2: the ones this was
// measured on (config 2: K = 4, 4 general levels).  K = 8 with 7 levels (config 5) lost 7 % with two bodies -- 71 KB of code for a 64 KB
// instruction cache, its 81 weights in SGPRs -- and 1.3 % with row pointers and the copy-free pass 2 in its one body: those keep the
// one general body, statement for statement what it was (profiles/r07/README.md).
template <int K, int G>
constexpr bool kStreamTwoBodies = K == 4 && G <= 4;

// The tile body of a kStreamTwoBodies kernel: silent_gray_stream_tile.h (request the rows, pass 2, pass 1) once per value of INTERIOR.
// INTERIOR (wave-uniform, decided by the kernel): the wave's R + 9 stream rows y0 - 4 .. y0 + R + 4 and its 65 columns xw0 - 4 ..
// xw0 + 60 (the 64 lanes and the edge column) all lie inside the crop, the zoomed extent and the level.  Then every mirror index is
// the identity, every row (p, c, y) and column (col_eff, col_in) predicate of pass 1 is true and out_lane is 4 <= lane < 60: that body
// has no clamps, no predicates and no padding selects.  INTERIOR = false is the general body.  Arithmetic and order are the same in
// both: the same bits.  The tables and weights arrive BY VALUE: the body then works on copies read from the kernarg segment once and
// held in SGPRs (some parked in VGPR lanes), where the kernel's own parameters are re-read from the kernarg segment wherever they are
// used -- 152 scalar loads and their waits in the two bodies against 52.  On config 2 that form won on every allocation of the
// same-buffer A/B; the body as text inside the kernel (no spilled SGPR at all) lost on one of three (profiles/r07/README.md).
// The same text as silent_gray_stream_tile_general.h but for INTERIOR, the row pointers and pass 2's swapping records: a fix
// to the prologue, to a level's taps in pass 2 or to a row step of pass 1 goes into BOTH files.
template <bool INTERIOR, int K, int G, int L, bool KP, bool F64, typename ST, typename FT>
__device__ __forceinline__ void gray_stream_tile(frame_param<FT> frames, float* __restrict__ pyr, ST* __restrict__ cs_out,
                                                 ST* __restrict__ end_out, const FusedTabT<F64> tab, const StreamTab st, const GrayW wts,
                                                 float clip_hi, const GrayKp kp, float* s_slab, float (*s_rows)[kStreamRows][64],
                                                 int frame, int ty, int tx, int wave, int lane) {
#include "silent_gray_stream_tile.h"
}

template <int K, int G, int L = 0, bool KP = false, bool F64 = false, typename ST = float, typename FT = float>
__global__ __launch_bounds__(64 * kFusedWaves) void gray_stream_kernel(frame_param<FT> frames, float* __restrict__ pyr,
                                                          ST* __restrict__ cs_out, ST* __restrict__ end_out,
                                                          const FusedTabT<F64> tab, const StreamTab st, const GrayW wts,
                                                          float clip_hi, unsigned opts, const GrayKp kp = GrayKp{}) {
    static_assert(!kStoreHalf<ST> || (!KP && !F64), "float16 storage: no keypoint epilogue, no float64 accumulation");
    static_assert(kFrameType<FT> && (!kFrameNarrow<FT> || !F64), "uint8 / uint16 frames: float32 accumulation only");
    __shared__ __attribute__((aligned(16))) float s_slab[K == 8 && !kStoreHalf<ST> ? kFusedWaves * 512 : 4];
    __shared__ __attribute__((aligned(16))) float s_rows[kFusedWaves][kStreamRows][64];  // the streamed rows of each wave (wave private)
    const unsigned bid = (opts & 1u) ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
    const int frame = (int)(bid / (unsigned)tab.tiles_per_frame);
    const int rem = (int)(bid - (unsigned)frame * (unsigned)tab.tiles_per_frame);
    const int ty = rem / tab.lv[0].tiles_x, tx = rem - ty * tab.lv[0].tiles_x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (kStreamTwoBodies<K, G>) {
        // config 2: 66 of 68 tile rows x 33 of 35 live waves = 91.5 % of the waves are interior
        const FusedLevel& u = tab.lv[0];
        const int wy0 = ty * kFusedTH, wx0 = tx * kFusedTW + wave * kFusedCols;
        const int lim_h = min(u.src_h, min(u.zoom_h, u.out_h)), lim_w = min(u.src_w, min(u.zoom_w, u.out_w));
        if (wy0 >= 4 && wy0 + kFusedTH + 4 < lim_h && wx0 >= 4 && wx0 + 60 < lim_w)
            gray_stream_tile<true, K, G, L, KP, F64, ST, FT>(frames, pyr, cs_out, end_out, tab, st, wts, clip_hi, kp, s_slab, s_rows, frame, ty, tx, wave, lane);
        else
            gray_stream_tile<false, K, G, L, KP, F64, ST, FT>(frames, pyr, cs_out, end_out, tab, st, wts, clip_hi, kp, s_slab, s_rows, frame, ty, tx, wave, lane);
    } else {
#include "silent_gray_stream_tile_general.h"
    }
}

// ---------------------------------------------------------------------------------------------
// pyramid_stream_kernel<C, G>: the single-read PYRAMID (no filters) for silent_pyramid: gray_stream_kernel without
// the CS / end stages, looped over the C interleaved channels of the frame.  Lane = pixel column exactly as in the
// gray kernel (same plan tables, same row programs, same column records for every channel); channel ch of a row is
// read and written at a stride of C floats.  Used for C = 1 only: two-step gray pyramids 0.58 -> 0.51 ms per 64 1080p
// frames; with C = 3 the stride-3 loads and partial-line stores made it 1.5 ms against 1.0 ms for unit + region
// kernels on 32 RGB frames (measured, bit-identical either way), so RGB plans are not marked streamable.
template <int C, int G, int L = 0, bool F64 = false, typename FT = float>
__global__ __launch_bounds__(64 * kFusedWaves) void pyramid_stream_kernel(frame_param<FT> frames, float* __restrict__ pyr,
                                                             const FusedTabT<F64> tab, const StreamTab st) {
    static_assert(kFrameType<FT> && (!kFrameNarrow<FT> || (!F64 && C == 1)), "uint8 / uint16 frames: one channel, float32 accumulation");
    constexpr int R = kFusedTH, NR = kStreamRows;
    __shared__ float s_rows[kFusedWaves][NR][64];
    const unsigned bid = blockIdx.x;
    const int frame = (int)(bid / (unsigned)tab.tiles_per_frame);
    const int rem = (int)(bid - (unsigned)frame * (unsigned)tab.tiles_per_frame);
    const FusedLevel& lv = tab.lv[0];
    const int ty = rem / lv.tiles_x, tx = rem - ty * lv.tiles_x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xw0 = tx * kFusedTW + wave * kFusedCols;
    if (xw0 >= lv.out_w) return;  // wave-uniform (no barrier in this kernel)
    const int wx_tile = tx * kFusedWaves + wave;
    const int y0 = ty * R;
    const int ox = xw0 + lane - 4;
    const long long WC = (long long)tab.W * C;
    frame_src<FT> src;
    if constexpr (kFrameStrided<FT>) src = frame_of(frames, frame);
    else src = frames + (long long)frame * tab.H * WC;
    const long long frame_px0 = (long long)frame * tab.frame_px;
    const long long base_px = frame_px0 + lv.px_off;
    const long long sx = (long long)(mirror_near(ox, lv.src_w) + lv.src_x0) * C;

    constexpr int GR = G < kStreamRegLevels ? G : kStreamRegLevels;
    StreamColT<F64> col[GR > 0 ? GR : 1];
#pragma unroll
    for (int g = 0; g < GR; ++g) col[g] = stream_col_t<F64>(st, g, wx_tile, lane);
    const int eff_h = min(lv.zoom_h, lv.out_h), eff_w = min(lv.zoom_w, lv.out_w);
    const bool col_eff = ox >= 0 && ox < eff_w;
    const bool out_lane = lane >= 4 && lane < 4 + kFusedCols && ox < lv.out_w;
    static_assert(G == stream_pad_levels(G), "row programs are padded to 4 or 7 levels");
    constexpr int PR = kStreamProgRow(L, G, F64);
    typedef const __attribute__((address_space(4))) int* const_int_ptr;
    const_int_ptr prog = (const_int_ptr)(st.row_prog + (long long)ty * (NR * PR));

#pragma unroll 1
    for (int ch = 0; ch < C; ++ch) {
        float in[R + 8];
#pragma unroll
        for (int i = 0; i < R + 8; ++i)
            if constexpr (kFrameStrided<FT>) in[i] = src.at(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0, sx);   // (C == 1)
            else in[i] = (float)src[(long long)(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0) * WC + sx + ch];
#pragma unroll
        for (int i = 0; i < R + 8; ++i) asm volatile("" ::"v"(in[i]));  // retire loads before the first store
#pragma unroll
        for (int i = 0; i < R + 8; ++i) s_rows[wave][i][lane] = in[i];

        // ---- pass 2: the other levels
        {
            acc_t<F64> vacc[G][kStreamSlots];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int k = 0; k < kStreamSlots; ++k) vacc[g][k] = 0.0f;
            int cur[PR], nxt[PR];
#pragma unroll
            for (int e = 0; e < PR; ++e) cur[e] = prog[e];
            float c0 = s_rows[wave][0][lane];
#pragma unroll 1
            for (int i = 0; i < NR; ++i) {
                const int inx = min(i + 1, NR - 1);
#pragma unroll
                for (int e = 0; e < PR; ++e) nxt[e] = prog[inx * PR + e];
                const float c_next = s_rows[wave][inx][lane];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int meta = cur[g];
                    if (!(meta & 128)) continue;
                    if constexpr (F64) {
                        stream_level_f64<L, G, GR>(g, cur, c0, vacc[g], col, st, wx_tile, lane, pyr, frame_px0, C, ch);
                    } else {
#pragma unroll
                        for (int k = 0; k < stream_slots(L, g); ++k) {
                            const float w = __int_as_float(cur[stream_w_off(L, G, g) + k]);
                            const float prev = (meta >> k) & 1 ? 0.0f : vacc[g][k];
                            vacc[g][k] = __builtin_fmaf(w, c0, prev);
                        }
                        const int done = (meta >> stream_done_shift(L)) & 7;
                        if (done != 7) {
                            const int oy = meta >> stream_row_shift(L);
                            float v = vacc[g][0];
#pragma unroll
                            for (int k = 1; k < stream_slots(L, g); ++k) v = done == k ? vacc[g][k] : v;
                            const int vbits = __float_as_int(v);
                            const StreamCol cr = g < GR ? col[g < GR ? g : 0] : stream_col(st, g, wx_tile, lane);   // (g is a constant here)
                            float acc = cr.w[0] * __int_as_float(__builtin_amdgcn_ds_bpermute(cr.lane4, vbits));
#pragma unroll
                            for (int q = 1; q < 6; ++q)
                                acc = __builtin_fmaf(cr.w[q], __int_as_float(__builtin_amdgcn_ds_bpermute(cr.lane4 + 4 * q, vbits)), acc);
                            if (lane < cr.n)
                                pyr[(frame_px0 + st.px_off[g] + (long long)oy * st.out_w[g] + cr.x0 + lane) * C + ch] = acc;
                        }
                    }
                }
#pragma unroll
                for (int e = 0; e < PR; ++e) cur[e] = nxt[e];
                c0 = c_next;
            }
        }

        // ---- pass 1: the unit level (same fma order as pyramid_unit_kernel).  The tile's 24 rows and the wave's 4 halo lanes per
        // side hold scipy's sixth taps (row p + 3, column x + 3) of every output without extra loads: no edge column here
        acc_t<F64> hw[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < R + 8; ++i) {
            acc_t<F64> h;
            if constexpr (F64) h = unit_taps6<false>(s_rows[wave][i][lane], 0.0f, tab.w64);
            else h = unit_taps6<false>(s_rows[wave][i][lane], 0.0f, tab.wx);
#pragma unroll
            for (int j = 0; j < 5; ++j) hw[j] = hw[j + 1];
            hw[5] = h;
            if (i >= 7 && i < R + 7) {
                const int p = y0 + i - 7;
                float v;
                if constexpr (F64) {
                    v = unit_vsum_f64(tab.w64, hw);
                } else {
                    v = tab.wy[0] * hw[0];
#pragma unroll
                    for (int j = 1; j < 6; ++j) v = __builtin_fmaf(tab.wy[j], hw[j], v);
                }
                v = (p < eff_h && col_eff) ? v : 0.0f;
                if (p < lv.out_h && out_lane) pyr[(base_px + (long long)p * lv.out_w + ox) * C + ch] = v;
            }
        }
    }
}

}  // namespace silent
