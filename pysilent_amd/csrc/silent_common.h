// Shared host/device declarations for libsilent_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "../../include/silent_hip.h"

namespace silent {

constexpr int kMaxLevels = SILENT_MAX_LEVELS;
constexpr int kWave = 64;  // CDNA wavefront

// Tile -> (frame, level, tile_y, tile_x) lookup for one launch over a packed pyramid batch.
// Travels as a kernel argument (SGPR-resident after s_load), so the lookup is scalar work.
struct LevelTab {
    int n_levels;
    int tiles_per_frame;
    long long frame_px;  // pixels of one whole pyramid (all levels)
    int h[kMaxLevels];
    int w[kMaxLevels];
    int tiles_x[kMaxLevels];
    int tile_start[kMaxLevels + 1];  // prefix sum of tiles per level
    long long px_off[kMaxLevels];    // pixel offset of level l inside one pyramid
};

constexpr int kChunk = 1024;  // pixels per block for the 1-D (flattened level) kernels: 256 threads x 4

// Host: fills `tab` for levels of the given extents -- 2-D tiles of tile_w x tile_h pixels, or (tile_h == 0) chunks of tile_w flattened
// pixels -- and returns the tiles of all frames.  A skipped level keeps its place in the layout and gets no tiles.  Pure: it checks
// nothing (extents >= 1 and at most 2^30 pixels a level are the caller's to see to, and so is a count no launch takes; the int fields
// saturate at 2^31 - 1 then).  build_level_tab (silent_core.hip) and attention_plan (silent_peaks_plan.h) are its callers.
inline long long fill_level_tab(const silent_extent* levels, int n_levels, int n_frames, int tile_w, int tile_h, const bool* skip, LevelTab* tab) {
    const auto sat = [](long long v) { return (int)(v < 0x7fffffffll ? v : 0x7fffffffll); };
    memset(tab, 0, sizeof(*tab));
    tab->n_levels = n_levels;
    long long px = 0, tiles = 0;
    for (int l = 0; l < n_levels; ++l) {
        const long long h = levels[l].h, w = levels[l].w;
        tab->h[l] = (int)h;
        tab->w[l] = (int)w;
        tab->px_off[l] = px;
        tab->tile_start[l] = sat(tiles);
        const long long tx = tile_h ? (w + tile_w - 1) / tile_w : (h * w + tile_w - 1) / tile_w;
        const long long ty = tile_h ? (h + tile_h - 1) / tile_h : 1;
        tab->tiles_x[l] = (int)tx;
        if (!(skip && skip[l])) tiles += tx * ty;
        px += h * w;
    }
    tab->tile_start[n_levels] = sat(tiles);
    tab->tiles_per_frame = sat(tiles);
    tab->frame_px = px;
    return tiles * (long long)n_frames;
}

struct TileCoord {
    int frame, level, ty, tx;
};

// XCD-aware block order.  Workgroups are dealt round-robin over the 8 XCDs (each with its own 4 MiB L2), so
// with the identity order two tiles that share halo rows land on different L2s.  Remap so that every XCD walks
// a contiguous run of tiles: vertical neighbours are then a few blocks apart on the SAME L2.  Bijective for any
// grid size; placement is a speed hint only, never a correctness assumption.
__device__ __forceinline__ unsigned xcd_swizzle(unsigned bid, unsigned n) {
    constexpr unsigned kXcd = 8;
    const unsigned per = n / kXcd, rem = n % kXcd;   // XCD x owns per (+1 if x < rem) consecutive tiles
    const unsigned x = bid % kXcd, k = bid / kXcd;
    return x * per + (x < rem ? x : rem) + k;
}

__device__ __forceinline__ TileCoord locate_tile(const LevelTab& tab, unsigned bid) {
    TileCoord t;
    t.frame = (int)(bid / (unsigned)tab.tiles_per_frame);
    int rem = (int)(bid - (unsigned)t.frame * (unsigned)tab.tiles_per_frame);
    int l = 0;
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (i < tab.n_levels && rem >= tab.tile_start[i]) l = i;
    t.level = l;
    rem -= tab.tile_start[l];
    t.ty = rem / tab.tiles_x[l];
    t.tx = rem - t.ty * tab.tiles_x[l];
    return t;
}

// Neighbour exchange inside a wave by DPP wavefront shifts (VALU, no LDS round trip).
// lane i receives lane i-1 (lane 0 gets 0) / lane i+1 (lane 63 gets 0): bound_ctrl with a zero "old" value is a
// single v_mov_b32_dpp; keeping the lane's own value instead costs an extra v_mov per shift.  The edge lanes of a
// wave are halo lanes in every kernel that uses these.
__device__ __forceinline__ float from_lane_below(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float from_lane_above(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}

// A wave-uniform row cursor of a streaming kernel: a pointer into global memory that moves on by ADDITION.  The empty asm keeps the
// sum in its SGPR pair as it is -- from an unrolled loop the compiler would otherwise form base + i * stride again, a 64-bit multiply
// per row -- and the address space keeps what comes out of the asm a global pointer (a generic one is read with flat loads).
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ void advance_rows(global_ptr<T>& p, long long elements) {
    p += elements;
    asm("" : "+s"(p));
}

// Float64 accumulation (plans created with SILENT_PLAN_ACCUM_F64; the F64 template flag of the gray and pyramid kernels).  Every
// map is still stored as float32 between ops; inside one op the taps are summed in acc_t<true> = double and rounded to float32
// once, like the oracle (oracle/silent_oracle.c).  The product of two float32 values is exact in float64, so a CS or end tap
// chain in the oracle's order reproduces its value bit for bit.  The F64 = false instantiations keep the float32 code as it
// was, statement for statement (their machine code is unchanged); the float64 arithmetic sits in `if constexpr (F64)` branches
// and in the *_f64 helpers below.
template <bool F64>
using acc_t = typename std::conditional<F64, double, float>::type;
// ds_bpermute of a float64 value: two permutes (its two halves)
__device__ __forceinline__ double bpermute_f64(int addr, double v) {
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(addr, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(addr, __double2loint(v)));
}

// scipy 'mirror' extension (d c b | a b c d | c b a) for an index within ONE reflection of [0, n): exact for
// -(n-1) <= i <= 2(n-1); anything further out is clamped into range (such taps only feed outputs that are
// never stored).  The streaming kernels reach at most 4 pixels outside, hence kMirrorNearMin.
constexpr int kMirrorNearMin = 5;
__device__ __forceinline__ int mirror_near(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// The horizontal taps of a unit (zoom 1) level for one streamed row of a lane-per-column wave.  scipy.ndimage.zoom(order=5)
// (from_image.py:55-59) evaluates SIX taps, x - 2 .. x + 3; at zoom 1 the sixth weight is what double arithmetic leaves of
// 1 - (1 + 26 + 66 + 26 + 1) / 120 = 2^-53: nothing next to finite neighbours, but a NaN / inf pixel reaches the outputs three
// to its left (and three above it) as well, and a lone bright pixel leaves 2^-53 of itself there.  The sixth tap of lane 61 is
// the column right of the wave's 64: `edge` carries it (wave-uniform: one lane of a per-tile load, unit_edge_column) and enters
// as what lane 63 "receives from lane 64" in the first shift (a DPP shift without bound_ctrl keeps the destination's old value
// in the lane that has no source), so r2 of lane 62 and r3 of lane 61 see it too.
// EDGE = false: lane 61 is no output's tap (kernels whose halo lanes already cover x + 3).
template <bool EDGE = true>
__device__ __forceinline__ float unit_taps6(float c0, float edge, const float (&w)[6]) {
    const float l1 = from_lane_below(c0), l2 = from_lane_below(l1);
    float r1;
    if constexpr (EDGE)
        r1 = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(c0), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
    else
        r1 = from_lane_above(c0);
    const float r2 = from_lane_above(r1), r3 = from_lane_above(r2);
    float h = w[0] * l2;
    h = __builtin_fmaf(w[1], l1, h);
    h = __builtin_fmaf(w[2], c0, h);
    h = __builtin_fmaf(w[3], r1, h);
    h = __builtin_fmaf(w[4], r2, h);
    return __builtin_fmaf(w[5], r3, h);
}
// The same six taps summed in float64 with float64 weights (F64 kernels).
template <bool EDGE = true>
__device__ __forceinline__ double unit_taps6(float c0, float edge, const double (&w)[6]) {
    const float l1 = from_lane_below(c0), l2 = from_lane_below(l1);
    float r1;
    if constexpr (EDGE)
        r1 = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(c0), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
    else
        r1 = from_lane_above(c0);
    const float r2 = from_lane_above(r1), r3 = from_lane_above(r2);
    double h = w[0] * (double)l2;
    h = __builtin_fma(w[1], (double)l1, h);
    h = __builtin_fma(w[2], (double)c0, h);
    h = __builtin_fma(w[3], (double)r1, h);
    h = __builtin_fma(w[4], (double)r2, h);
    return __builtin_fma(w[5], (double)r3, h);
}
// Frame element type of the single-channel frame-reading kernels (their trailing template parameter FT): float, or unsigned char
// for uint8 frames (the *_u8 entry points).  A byte enters the arithmetic as (float)byte at the load -- exact, so a uint8 kernel
// stores the bits its float instantiation stores for the widened frame.  UNSIGNED: a char / signed char load would turn 128 .. 255
// into negatives.  The FT = float instantiations are the code as it was (their machine code is unchanged).
template <typename FT>
constexpr bool kFrameBytes = std::is_same<FT, unsigned char>::value;
// Interleaved 3-channel uint8 frames (the *_u8x3 entry points: [n, H, W, 3] bytes as a camera or decoder delivers colour).  One frame
// PIXEL is one element of this type -- size 3, alignment 1 -- so every index, row stride and 64-bit frame offset of the kernels
// counts pixels as it does for the other frame types, and the `(float)src[i]` at their loads is the reference's get_value_from_color
// (a-8) on that pixel: ((b0 + b1) + b2) * float32(1/3), ONE rounding (the sum is at most 765: exact as an integer and as a float32,
// in any channel order) -- bit for bit silent_value_from_color on the widened frame.  Times the float32 reciprocal, never / 3.0f:
// 254 of the 766 sums differ.  Two loads per lane and row: a 2-byte load at 3 * lane and a byte load at 3 * lane + 2, neither with
// an alignment requirement (a wave row is 192 contiguous bytes in 2 VMEM requests).  Written as three byte loads the compiler merges
// the first two as well but keeps 104 - 106 VGPRs in gray_stream_kernel (4 waves per SIMD); this form has the unsigned char
// kernels' 78 - 103 (5) and measured 1.055 against 1.116 ms per config-2 step (profiles/gray_rgb8/README.md).
struct FrameRgb8 {
    unsigned char b[3];
    __device__ __forceinline__ explicit operator float() const {
        unsigned short lo;                       // b[0], b[1]: one 2-byte load at alignment 1 (global_load_ushort takes any address)
        __builtin_memcpy(&lo, b, 2);
        return __fmul_rn((float)((int)(lo & 0xffu) + (int)(lo >> 8) + (int)b[2]), 1.0f / 3.0f);
    }
};
static_assert(sizeof(FrameRgb8) == 3 && alignof(FrameRgb8) == 1, "one interleaved uint8 colour pixel");
template <typename FT>
constexpr bool kFrameRgb8 = std::is_same<FT, FrameRgb8>::value;
// uint16 frames (the *_u16 entry points: Mono10/12/16, Y16 / Z16, 16-bit TIFF / PNG, the luma of P010 / P016): one frame element is an
// unsigned 16-bit integer in native byte order, 2-byte aligned, and enters the arithmetic as (float)v at the load -- exact (65535 <
// 2^24), so a uint16 kernel stores the bits its float instantiation stores for the widened frame.  UNSIGNED: a short load
// (global_load_sshort) would turn 32768 .. 65535 into negatives.  No shift and no scale: P010 keeps its 10 bits in the high bits.
template <typename FT>
constexpr bool kFrameWords = std::is_same<FT, unsigned short>::value;
// Strided frames (the *_view entry points, silent_frame_view, and *_view16, silent_frame_view16): the pixels PX -- unsigned char,
// FrameRgb8 or unsigned short (2-byte aligned: even address, even strides), read exactly as the
// packed kinds read them -- of a view with three BYTE strides (a pitched BGR row need not be a multiple of 3), so pixel (frame, y, x)
// is the PX at data + frame * frame_stride + y * row_stride + x * pixel_stride, in 64-bit bytes.  The type is both the frame kind FT
// of the kernels and their argument, by value: the strides arrive in SGPRs, and with the wave-uniform row of every load the frame
// and row terms are scalar arithmetic -- only x * pixel_stride is per lane, formed once per tile where the column is the lane's own.
// The packed kinds keep `const FT*` and their statements (their machine code is unchanged).
template <typename PX>
struct FrameStrided {
    const unsigned char* data;
    long long pixel_stride, row_stride, frame_stride;
};
template <typename FT>
constexpr bool kFrameStrided = false;
template <typename PX>
constexpr bool kFrameStrided<FrameStrided<PX>> = true;
// the two uint16 kinds, packed and strided (their entry points say "uint16 frames")
template <typename FT>
constexpr bool kFrame16 = kFrameWords<FT> || std::is_same<FT, FrameStrided<unsigned short>>::value;
// one frame of a strided batch inside a kernel: (float)at(y, x) is the value of its pixel (x, y)
template <typename PX>
struct StridedSrc {
    const unsigned char* p;
    long long pixel_stride, row_stride;
    __device__ __forceinline__ float at(long long y, long long x) const {
        return (float)*reinterpret_cast<const PX*>(p + y * row_stride + x * pixel_stride);
    }
};
// the `frames` parameter of a kernel on frame kind FT, and what `src` (one frame of the batch) is inside it
template <typename FT>
struct FrameKind {
    typedef const FT* __restrict__ param;
    typedef const FT* __restrict__ src;
};
template <typename PX>
struct FrameKind<FrameStrided<PX>> {
    typedef FrameStrided<PX> param;
    typedef StridedSrc<PX> src;
    typedef PX px;
};
template <typename FT>
using frame_param = typename FrameKind<FT>::param;
template <typename FT>
using frame_src = typename FrameKind<FT>::src;
// frame `frame` of a strided batch (the packed kinds keep their `frames + frame * H * W` and `(float)src[y * W + x]` statements)
template <typename PX>
__device__ __forceinline__ StridedSrc<PX> frame_of(const FrameStrided<PX>& frames, int frame) {
    return StridedSrc<PX>{frames.data + (long long)frame * frames.frame_stride, frames.pixel_stride, frames.row_stride};
}

// Strided interleaved uint8 colour with the THREE CHANNELS KEPT (silent_pyramid_rgb8_view, 3-channel plans only): channel c of pixel
// (frame, y, x) is the byte at data + frame * frame_stride + y * row_stride + x * pixel_stride + c and enters as (float)byte, like a
// byte of the packed kind `unsigned char` at C == 3.  Not FrameStrided<FrameRgb8>: that kind REDUCES the three bytes to one value for
// a single-channel plan.  The 3-channel kernels index a frame row in floats of the interleaved row; float i of the VIRTUAL PACKED row
// of a view is pixel i / 3, channel i % 3 -- rgb_view_col below, the one place that maps it to a byte.  Frame and row terms are
// scalar 64-bit arithmetic as in the other strided kinds; the kernels take the struct by value (strides in SGPRs).
struct FrameStridedRgb {
    const unsigned char* data;
    long long pixel_stride, row_stride, frame_stride;
};
template <typename FT>
constexpr bool kFrameRgbView = std::is_same<FT, FrameStridedRgb>::value;
// byte offset inside a row of float i of the virtual packed row
__host__ __device__ __forceinline__ long long rgb_view_col(long long i, long long pixel_stride) {
    const long long p = i / 3;
    return p * pixel_stride + (i - 3 * p);
}
// one frame of such a batch inside a kernel
struct StridedRgbSrc {
    const unsigned char* p;
    long long pixel_stride, row_stride;
    // channel ch of pixel (x, y) / float i of the virtual packed row y
    __device__ __forceinline__ float at(long long y, long long x, int ch) const { return (float)p[y * row_stride + x * pixel_stride + ch]; }
    __device__ __forceinline__ float atf(long long y, long long i) const { return (float)p[y * row_stride + rgb_view_col(i, pixel_stride)]; }
};
template <>
struct FrameKind<FrameStridedRgb> {
    typedef FrameStridedRgb param;
    typedef StridedRgbSrc src;
};
__device__ __forceinline__ StridedRgbSrc frame_of(const FrameStridedRgb& frames, int frame) {
    return StridedRgbSrc{frames.data + (long long)frame * frames.frame_stride, frames.pixel_stride, frames.row_stride};
}

// NV12 decoder surfaces (silent_pyramid_nv12, 3-channel plans only): a full-resolution luma plane and a half-resolution plane of
// interleaved (U, V) pairs, both pitched, converted to three float32 channels IN REGISTERS at the load.  Channel k of pixel (frame, y, x):
//     Yv = (float)Y[frame][y][x] - oy,  Uv = (float)UV[frame][y >> 1][x >> 1][0] - 128,  Vv = (float)UV[frame][y >> 1][x >> 1][1] - 128
//     c_k = min(max((Yv * m[3 k] + Uv * m[3 k + 1]) + Vv * m[3 k + 2], 0), 255)
// with every product and sum a separately rounded float32 operation (__fmul_rn / __fadd_rn: `a * b + c` is contracted into an FMA,
// which gives other bits) and NO rounding to an integer: the float32 value enters the pyramid.  Chroma is nearest (a 2 x 2 luma block
// shares one pair).  Matrix and offset are arguments: channel order, BT.601 / BT.709 and limited / full range are the caller's choice
// of m and oy, not kernel variants.  The struct is the kernels' argument, by value: strides and coefficients arrive in SGPRs, frame and
// row terms (frame row y, chroma row y >> 1) are scalar 64-bit arithmetic.  nv12_channel is THE conversion: the loaders of every
// pyramid kernel and source_to_rgb_kernel (silent_nv12_to_rgb) call it, so the pyramid of a surface is the float32-frame pyramid of the
// converted frames bit for bit.
struct FrameNv12 {
    const unsigned char* y;
    const unsigned char* uv;
    long long y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride;
    float m[9];
    float oy;
};
template <typename FT>
constexpr bool kFrameNv12 = std::is_same<FT, FrameNv12>::value;
// P010 / P012 / P016 decoder surfaces (silent_pyramid_p010): the NV12 layout with uint16 elements, the code in the high bits (below)
struct FrameP010 {
    const unsigned short* y;
    const unsigned short* uv;
    long long y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride;   // bytes, even
    float m[9];
    float oy, oc;
    int shift;                                                                // 16 - depth
};
template <typename FT>
constexpr bool kFrameP010 = std::is_same<FT, FrameP010>::value;
// planar and packed 8-bit YUV (silent_pyramid_yuv): three byte planes, a pixel stride per plane class, a chroma shift per axis (below)
struct FrameYuv {
    const unsigned char* y;
    const unsigned char* u;
    const unsigned char* v;
    long long y_pixel_stride, y_row_stride, y_frame_stride;   // bytes
    long long c_pixel_stride, c_row_stride, c_frame_stride;   // bytes; shared by u and v
    int sx, sy;                                               // chroma subsampling shifts, 0 or 1 each
    float m[9];
    float oy;
};
template <typename FT>
constexpr bool kFrameYuv = std::is_same<FT, FrameYuv>::value;
// planar, semi-planar and packed 16-bit YUV (silent_pyramid_yuv16): FrameYuv's addressing with uint16 elements, FrameP010's arithmetic
// with a mask, so that the code may sit in the low bits (below)
struct FrameYuv16 {
    const unsigned short* y;
    const unsigned short* u;
    const unsigned short* v;
    long long y_pixel_stride, y_row_stride, y_frame_stride;   // bytes, even
    long long c_pixel_stride, c_row_stride, c_frame_stride;   // bytes, even; shared by u and v
    int sx, sy;                                               // chroma subsampling shifts, 0 or 1 each
    float m[9];
    float oy, oc;
    int shift;                                                // bits below the code value
    unsigned mask;                                            // (1 << depth) - 1
};
template <typename FT>
constexpr bool kFrameYuv16 = std::is_same<FT, FrameYuv16>::value;
// the YUV family as ONE set of traits: pair kinds (two planes, the (U, V) of a pixel behind one load), triple kinds (three planes, a
// pixel stride per plane class, a chroma shift per axis), wide kinds (uint16 elements: oc and shift).  A fifth source names itself here.
template <typename FT>
constexpr bool kFrameYuvPair = kFrameNv12<FT> || kFrameP010<FT>;
template <typename FT>
constexpr bool kFrameYuvTriple = kFrameYuv<FT> || kFrameYuv16<FT>;
template <typename FT>
constexpr bool kFrameYuvWide = kFrameP010<FT> || kFrameYuv16<FT>;
template <typename FT>
constexpr bool kFrameYuvFamily = kFrameYuvPair<FT> || kFrameYuvTriple<FT>;
// raw 8-bit Bayer mosaics (silent_pyramid_bayer): one byte per pixel in a strided view, demosaiced at the load (below)
struct FrameBayer {
    const unsigned char* data;
    long long pixel_stride, row_stride, frame_stride;   // bytes
    int H, W;                                            // the frame's extents: the neighbourhood is reflected at the FRAME's edges
    int pattern, order;                                  // 0 .. 3: rggb, grbg, gbrg, bggr; 0: bgr, 1: rgb
};
template <typename FT>
constexpr bool kFrameBayer = std::is_same<FT, FrameBayer>::value;
// the 3-channel kinds that are read through a `src` struct with at(y, x, ch) / atf(y, i) (strided colour views, the YUV family, mosaics)
template <typename FT>
constexpr bool kFrameRgbSrc = kFrameRgbView<FT> || kFrameYuvFamily<FT> || kFrameBayer<FT>;
__device__ __forceinline__ float nv12_channel(float yv, float uv, float vv, float m0, float m1, float m2) {
    return fminf(fmaxf(__fadd_rn(__fadd_rn(__fmul_rn(yv, m0), __fmul_rn(uv, m1)), __fmul_rn(vv, m2)), 0.0f), 255.0f);
}
// byte offsets of pixel column x inside a luma row and of its (U, V) pair inside a chroma row
__host__ __device__ __forceinline__ long long nv12_y_col(long long x) { return x; }
__host__ __device__ __forceinline__ long long nv12_uv_col(long long x) { return (x >> 1) * 2; }
// at() / atf() of the family's `src` structs (one frame of a batch inside a kernel), once: D has yuv(y, x, Yv, Uv, Vv) and m
template <class D>
struct YuvSrcOps {
    // channel ch of pixel (x, y) / float i of the virtual packed row y (pixel i / 3, channel i % 3)
    __device__ __forceinline__ float at(long long yy, long long x, int ch) const {
        const D& d = *static_cast<const D*>(this);
        float yv, uvv, vv;
        d.yuv(yy, x, yv, uvv, vv);
        // (the nine coefficients are read first and selected as VALUES: a select between loads becomes a dynamically indexed load,
        // and with it a copy of the struct in scratch)
        const float a0 = d.m[0], a1 = d.m[1], a2 = d.m[2], b0 = d.m[3], b1 = d.m[4], b2 = d.m[5], c0 = d.m[6], c1 = d.m[7], c2 = d.m[8];
        return nv12_channel(yv, uvv, vv, ch == 0 ? a0 : (ch == 1 ? b0 : c0), ch == 0 ? a1 : (ch == 1 ? b1 : c1), ch == 0 ? a2 : (ch == 1 ? b2 : c2));
    }
    __device__ __forceinline__ float atf(long long yy, long long i) const {
        const long long p = i / 3;
        return at(yy, p, (int)(i - 3 * p));
    }
};
// one frame of such a batch inside a kernel
struct Nv12Src : YuvSrcOps<Nv12Src> {
    const unsigned char* y;
    const unsigned char* uv;
    long long y_row_stride, uv_row_stride;
    float m[9];
    float oy;
    // the (Y, U, V) of pixel (x, y), offsets removed: a byte load and one 2-byte load at any alignment (global_load_ushort)
    __device__ __forceinline__ void yuv(long long yy, long long x, float& yv, float& uvv, float& vv) const {
        const unsigned char* c = uv + (yy >> 1) * uv_row_stride + nv12_uv_col(x);
        unsigned short pair;
        __builtin_memcpy(&pair, c, 2);
        yv = __fsub_rn((float)y[yy * y_row_stride + nv12_y_col(x)], oy);
        uvv = (float)((int)(pair & 0xffu) - 128);
        vv = (float)((int)(pair >> 8) - 128);
    }
};
template <>
struct FrameKind<FrameNv12> {
    typedef FrameNv12 param;
    typedef Nv12Src src;
};

// P010 / P012 / P016 decoder surfaces (silent_pyramid_p010, 3-channel plans only): NV12's two planes with little-endian uint16
// elements whose code value sits in the HIGH d bits (d = 10, 12, 16; shift = 16 - d, a runtime scalar: one set of kernels for the
// three depths).  Channel k of pixel (frame, y, x), with Y, U, V the pixel's luma element and the two elements of its chroma pair:
//     Yv = (float)(Y >> shift) - oy,  Uv = (float)(U >> shift) - oc,  Vv = (float)(V >> shift) - oc,  c_k = nv12_channel(Yv, Uv, Vv, row k of m)
// -- elements loaded UNSIGNED, the low `shift` bits shifted out (decoders do not promise zeros there), the subtractions separately
// rounded float32 operations like the products and sums of nv12_channel, which stays THE conversion; the result is on the 0 .. 255
// scale and not rounded to an integer, so a 10-bit code lands on a quarter step.  Strides are BYTES and even, the pointers 2-byte
// aligned (refused otherwise): every load is a 2-byte luma element or the 4-byte (U, V) pair as ONE dword at a 2-byte aligned address
// (global_load_dword; the NV12 loaders read their 2-byte pair at any alignment the same way) -- exactly the two addressed elements.
// p010_values: the element and the pair as they were loaded -> (Yv, Uv, Vv); every loader and source_to_rgb_kernel go through it.
__device__ __forceinline__ void p010_values(unsigned e, unsigned pair, float oy, float oc, int shift, float& yv, float& uv, float& vv) {
    yv = __fsub_rn((float)((e & 0xffffu) >> shift), oy);
    uv = __fsub_rn((float)((pair & 0xffffu) >> shift), oc);
    vv = __fsub_rn((float)((pair >> 16) >> shift), oc);
}
// byte offsets of pixel column x inside a luma row and of its (U, V) pair inside a chroma row
__host__ __device__ __forceinline__ long long p010_y_col(long long x) { return 2 * x; }
__host__ __device__ __forceinline__ long long p010_uv_col(long long x) { return (x >> 1) * 4; }
// one frame of such a batch inside a kernel (the planes as byte pointers: strides are bytes)
struct P010Src : YuvSrcOps<P010Src> {
    const unsigned char* y;
    const unsigned char* uv;
    long long y_row_stride, uv_row_stride;
    float m[9];
    float oy, oc;
    int shift;
    __device__ __forceinline__ void yuv(long long yy, long long x, float& yv, float& uvv, float& vv) const {
        unsigned short e;
        unsigned pair;
        __builtin_memcpy(&e, y + yy * y_row_stride + p010_y_col(x), 2);
        __builtin_memcpy(&pair, uv + (yy >> 1) * uv_row_stride + p010_uv_col(x), 4);
        p010_values(e, pair, oy, oc, shift, yv, uvv, vv);
    }
};
template <>
struct FrameKind<FrameP010> {
    typedef FrameP010 param;
    typedef P010Src src;
};

// Planar and packed 8-bit YUV (silent_pyramid_yuv, 3-channel plans only): what differs from NV12 is ADDRESSING alone -- which byte
// holds a pixel's Y, U and V.  One kind for the family (I420 / YV12 / I422 / I444 / NV12 / NV21 / NV16 / NV24 / YUYV / UYVY / VUYA):
// three plane pointers (they may point into one buffer), a pixel stride per plane class and a chroma shift per axis.  Pixel (f, y, x):
//     Y = y[f y_frame_stride + y y_row_stride + x y_pixel_stride]     U = u[f c_frame_stride + (y >> sy) c_row_stride + (x >> sx) c_pixel_stride]
//     V = v[the offset of U]
//     Yv = (float)Y - oy,  Uv = (float)U - 128,  Vv = (float)V - 128,  c_k = nv12_channel(Yv, Uv, Vv, row k of m)
// -- NV12's words to the letter (nv12_channel stays THE conversion; chroma nearest; no rounding to an integer).  Every load is ONE BYTE
// that is some pixel's Y, U or V: no pair and no dword loads, so nothing between the pixels of a packed format is ever read.
// byte offsets of pixel column x inside a luma row and inside a chroma row
__host__ __device__ __forceinline__ long long yuv_y_col(long long x, long long y_pixel_stride) { return x * y_pixel_stride; }
__host__ __device__ __forceinline__ long long yuv_c_col(long long x, int sx, long long c_pixel_stride) { return (x >> sx) * c_pixel_stride; }
// one frame of such a batch inside a kernel
struct YuvSrc : YuvSrcOps<YuvSrc> {
    const unsigned char* y;
    const unsigned char* u;
    const unsigned char* v;
    long long y_pixel_stride, y_row_stride, c_pixel_stride, c_row_stride;
    int sx, sy;
    float m[9];
    float oy;
    // the (Y, U, V) of pixel (x, y), offsets removed: three byte loads
    __device__ __forceinline__ void yuv(long long yy, long long x, float& yv, float& uvv, float& vv) const {
        const long long c = (yy >> sy) * c_row_stride + yuv_c_col(x, sx, c_pixel_stride);
        yv = __fsub_rn((float)y[yy * y_row_stride + yuv_y_col(x, y_pixel_stride)], oy);
        uvv = (float)((int)u[c] - 128);
        vv = (float)((int)v[c] - 128);
    }
};
template <>
struct FrameKind<FrameYuv> {
    typedef FrameYuv param;
    typedef YuvSrc src;
};

// Planar, semi-planar and packed 16-bit YUV (silent_pyramid_yuv16, 3-channel plans only): FrameYuv's ADDRESSING (three plane pointers,
// a pixel stride per plane class, a chroma shift per axis; all strides bytes and even) with uint16 elements, and P010's ARITHMETIC with
// a mask in front, so that the code may sit in the low bits (yuv420p10le / I010: shift 0) or in the high bits (P210, Y210: shift =
// 16 - depth):
//     code(e) = (e >> shift) & mask,  Yv = (float)code(Y) - oy,  Uv = (float)code(U) - oc,  Vv = (float)code(V) - oc,
//     c_k = nv12_channel(Yv, Uv, Vv, row k of m)
// -- elements loaded UNSIGNED, every difference a separately rounded float32 operation; with shift = 16 - depth the mask changes
// nothing and these are p010_values' values.  Every load is ONE 2-byte element (global_load_ushort) at a 2-byte aligned address that
// is some pixel's Y, U or V: no pair and no dword loads, so nothing between the pixels of a packed format is ever read.
// yuv16_values: the three elements as they were loaded -> (Yv, Uv, Vv); every loader and source_to_rgb_kernel go through it.
__device__ __forceinline__ void yuv16_values(unsigned ey, unsigned eu, unsigned ev, float oy, float oc, int shift, unsigned mask, float& yv,
                                             float& uv, float& vv) {
    yv = __fsub_rn((float)(((ey & 0xffffu) >> shift) & mask), oy);
    uv = __fsub_rn((float)(((eu & 0xffffu) >> shift) & mask), oc);
    vv = __fsub_rn((float)(((ev & 0xffffu) >> shift) & mask), oc);
}
// one frame of such a batch inside a kernel (the planes as byte pointers: strides are bytes; the columns are yuv_y_col / yuv_c_col)
struct Yuv16Src : YuvSrcOps<Yuv16Src> {
    const unsigned char* y;
    const unsigned char* u;
    const unsigned char* v;
    long long y_pixel_stride, y_row_stride, c_pixel_stride, c_row_stride;
    int sx, sy;
    float m[9];
    float oy, oc;
    int shift;
    unsigned mask;
    // the (Y, U, V) of pixel (x, y), offsets removed: three 2-byte loads
    __device__ __forceinline__ void yuv(long long yy, long long x, float& yv, float& uvv, float& vv) const {
        const long long c = (yy >> sy) * c_row_stride + yuv_c_col(x, sx, c_pixel_stride);
        unsigned short ey, eu, ev;
        __builtin_memcpy(&ey, y + yy * y_row_stride + yuv_y_col(x, y_pixel_stride), 2);
        __builtin_memcpy(&eu, u + c, 2);
        __builtin_memcpy(&ev, v + c, 2);
        yuv16_values(ey, eu, ev, oy, oc, shift, mask, yv, uvv, vv);
    }
};
template <>
struct FrameKind<FrameYuv16> {
    typedef FrameYuv16 param;
    typedef Yuv16Src src;
};
// frame `frame` of a batch of the family
template <typename FT, typename std::enable_if<kFrameYuvFamily<FT>, int>::type = 0>
__device__ __forceinline__ frame_src<FT> frame_of(const FT& f, int frame) {
    frame_src<FT> s;
    s.y = reinterpret_cast<const unsigned char*>(f.y) + (long long)frame * f.y_frame_stride;
    s.y_row_stride = f.y_row_stride;
    if constexpr (kFrameYuvPair<FT>) {
        s.uv = reinterpret_cast<const unsigned char*>(f.uv) + (long long)frame * f.uv_frame_stride;
        s.uv_row_stride = f.uv_row_stride;
    } else {
        s.u = reinterpret_cast<const unsigned char*>(f.u) + (long long)frame * f.c_frame_stride;
        s.v = reinterpret_cast<const unsigned char*>(f.v) + (long long)frame * f.c_frame_stride;
        s.y_pixel_stride = f.y_pixel_stride;
        s.c_pixel_stride = f.c_pixel_stride;
        s.c_row_stride = f.c_row_stride;
        s.sx = f.sx;
        s.sy = f.sy;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) s.m[i] = f.m[i];
    s.oy = f.oy;
    if constexpr (kFrameYuvWide<FT>) {
        s.oc = f.oc;
        s.shift = f.shift;
    }
    if constexpr (kFrameYuv16<FT>) s.mask = f.mask;
    return s;
}

// Raw 8-bit Bayer mosaics (silent_pyramid_bayer, 3-channel plans only): m(y, x) is the byte at data + frame * frame_stride +
// y * row_stride + x * pixel_stride (64-bit bytes), one colour sample per pixel in a 2 x 2 pattern whose name is that of the top-left
// cell of THE VIEW: red sits at (y & 1, x & 1) == (pattern >> 1, pattern & 1), blue on the other diagonal site, green on the two others.
// Bilinear demosaicing, with indices outside the frame reflected without repeating the edge (-1 -> 1, n -> n - 2: the parity of an index
// is kept, so a reflected neighbour has the colour its position calls for):
//     at a red / blue site:  own colour (float)m(y, x);  green (m(y-1,x) + m(y+1,x) + m(y,x-1) + m(y,x+1)) * 0.25;  the opposite colour
//                            the four diagonal neighbours * 0.25
//     at a green site:       green (float)m(y, x);  the colour of the same row (m(y,x-1) + m(y,x+1)) * 0.5;  the other (m(y-1,x) + m(y+1,x)) * 0.5
// -- every sum an integer (at most 1020), converted once (exact) and multiplied once by a power of two (exact): a multiple of 1/4 in
// [0, 255], NOT rounded to an integer, the same bits in any evaluation order.  This is not OpenCV's COLOR_Bayer*2BGR (which rounds to
// uint8 and treats the border differently), and OpenCV's pattern names are shifted against the sensor's.
// bayer_rgb is THE conversion: c the pixel's own sample, h / v / d the SUMS of its two horizontal, two vertical and four diagonal
// neighbours (the parts of the 3 x 3 neighbourhood a site can need), (py, px) the parities of its frame row and column.  The loader of
// the walk kernel, BayerSrc::at (unit, region and border kernels) and source_to_rgb_kernel (silent_bayer_to_rgb) all go through it.
// Integer arguments: a uint16 twin passes wider samples and another scale.
__device__ __forceinline__ void bayer_rgb(int c, int h, int v, int d, int py, int px, int pattern, int order, float& c0, float& c1, float& c2) {
    const bool red_row = py == (pattern >> 1), red_col = px == (pattern & 1);
    const bool green = red_row != red_col;
    const float g = green ? (float)c : __fmul_rn((float)(h + v), 0.25f);
    // the colour whose samples share this row (green site) / the site's own colour, and the other one
    const float a = green ? __fmul_rn((float)h, 0.5f) : (float)c;
    const float b = green ? __fmul_rn((float)v, 0.5f) : __fmul_rn((float)d, 0.25f);
    const float red = red_row ? a : b, blue = red_row ? b : a;
    c0 = order ? red : blue;
    c1 = g;
    c2 = order ? blue : red;
}
// an index one step outside [0, n) reflected into it (n >= 2); host-callable: the walk loader's address function uses it
__host__ __device__ __forceinline__ int bayer_reflect(int i, int n) { return i < 0 ? 1 : (i > n - 1 ? n - 2 : i); }
// one frame of a batch of mosaics inside a kernel
struct BayerSrc {
    const unsigned char* p;
    long long pixel_stride, row_stride;
    int H, W, pattern, order;
    // the three channels of pixel (x, y): nine byte loads, each the sample of a pixel of the frame
    __device__ __forceinline__ void rgb(long long yy, long long x, float& c0, float& c1, float& c2) const {
        const unsigned char* r1 = p + yy * row_stride;
        const unsigned char* r0 = p + (long long)bayer_reflect((int)yy - 1, H) * row_stride;
        const unsigned char* r2 = p + (long long)bayer_reflect((int)yy + 1, H) * row_stride;
        const long long x1 = x * pixel_stride, x0 = (long long)bayer_reflect((int)x - 1, W) * pixel_stride,
                        x2 = (long long)bayer_reflect((int)x + 1, W) * pixel_stride;
        const int m00 = r0[x0], m01 = r0[x1], m02 = r0[x2], m10 = r1[x0], m11 = r1[x1], m12 = r1[x2], m20 = r2[x0], m21 = r2[x1], m22 = r2[x2];
        bayer_rgb(m11, m10 + m12, m01 + m21, (m00 + m02) + (m20 + m22), (int)yy & 1, (int)x & 1, pattern, order, c0, c1, c2);
    }
    // channel ch of pixel (x, y) / float i of the virtual packed row y (pixel i / 3, channel i % 3)
    __device__ __forceinline__ float at(long long yy, long long x, int ch) const {
        float c0, c1, c2;
        rgb(yy, x, c0, c1, c2);
        return ch == 0 ? c0 : (ch == 1 ? c1 : c2);
    }
    // the same value from the PART of the neighbourhood this one channel needs -- the pixel's own sample, its horizontal pair, its
    // vertical pair, both pairs, or the four diagonals: at most four byte loads, behind lane-divergent branches -- with zeros for the
    // parts bayer_rgb does not read for it.  For the border pixels inside the walk kernel (pyramid_border_px, LEAN), whose register
    // budget is the consumers': with at() there the kernel needs 81 VGPRs (5 waves per SIMD), with this 72 (7, like the other sources).
    // Everywhere else the branches cost more than the loads they save (pyramid_unit_kernel: 256 VGPRs against 89).
    __device__ __forceinline__ float at_parts(long long yy, long long x, int ch) const {
        const bool red_row = ((int)yy & 1) == (pattern >> 1), green = red_row != (((int)x & 1) == (pattern & 1));
        const bool own_or_row = (ch == (order ? 0 : 2)) == red_row;   // (ch != 1) the channel is the site's own colour / that of a green site's row
        const bool need_c = ch == 1 ? green : (!green && own_or_row), need_h = ch == 1 ? !green : (green && own_or_row);
        const bool need_v = ch == 1 ? !green : (green && !own_or_row), need_d = ch != 1 && !green && !own_or_row;
        const unsigned char* r1 = p + yy * row_stride;
        const long long up = (long long)(bayer_reflect((int)yy - 1, H) - (int)yy) * row_stride, down = (long long)(bayer_reflect((int)yy + 1, H) - (int)yy) * row_stride;
        const long long x1 = x * pixel_stride, x0 = (long long)bayer_reflect((int)x - 1, W) * pixel_stride,
                        x2 = (long long)bayer_reflect((int)x + 1, W) * pixel_stride;
        int c = 0, h = 0, v = 0, d = 0;
        if (need_c) c = r1[x1];
        if (need_h) h = (int)r1[x0] + (int)r1[x2];
        if (need_v) v = (int)r1[up + x1] + (int)r1[down + x1];
        if (need_d) d = ((int)r1[up + x0] + (int)r1[up + x2]) + ((int)r1[down + x0] + (int)r1[down + x2]);
        float c0, c1, c2;
        bayer_rgb(c, h, v, d, (int)yy & 1, (int)x & 1, pattern, order, c0, c1, c2);
        return ch == 0 ? c0 : (ch == 1 ? c1 : c2);
    }
    __device__ __forceinline__ float atf(long long yy, long long i) const {
        const long long q = i / 3;
        return at(yy, q, (int)(i - 3 * q));
    }
};
template <>
struct FrameKind<FrameBayer> {
    typedef FrameBayer param;
    typedef BayerSrc src;
};
__device__ __forceinline__ BayerSrc frame_of(const FrameBayer& f, int frame) {
    return BayerSrc{f.data + (long long)frame * f.frame_stride, f.pixel_stride, f.row_stride, f.H, f.W, f.pattern, f.order};
}

// the frame types that exist for single-channel plans with float32 accumulation only
template <typename FT>
constexpr bool kFrameNarrow = kFrameBytes<FT> || kFrameRgb8<FT> || kFrameWords<FT> || kFrameStrided<FT>;
template <typename FT>
constexpr bool kFrameType = std::is_same<FT, float>::value || kFrameNarrow<FT> || kFrameRgbView<FT> || kFrameYuvFamily<FT> || kFrameBayer<FT>;
// (host) the bytes of one frame pixel as the host-pointer forms stage it -- float frames carry the channels of the plan; a view is
// staged by its span -- and the suffix of a frame type's entry points
template <typename FT>
constexpr size_t frame_px_bytes(int plan_channels) { return kFrameRgb8<FT> ? 3 : kFrameWords<FT> ? 2 : kFrameBytes<FT> ? 1 : 4 * (size_t)plan_channels; }
template <typename FT>
constexpr const char* kFrameSuffix =
    kFrameStrided<FT> ? (kFrame16<FT> ? "_view16" : "_view") : kFrameRgb8<FT> ? "_u8x3" : kFrameWords<FT> ? "_u16" : kFrameBytes<FT> ? "_u8" : "";

// Stream row i of the column `col` (level coordinates, mirrored inside the crop like every tap; px_stride floats per pixel) in lane i: ONE load per tile
// for the sixth taps of a wave's last smoothing lane; row i is read back with unit_edge(xcol, i).
// FT: the frame element type (float, or unsigned char / unsigned short: uint8 / uint16 frames, widened at the load -- exact).
template <typename FT = float>
__device__ __forceinline__ float unit_edge_column(const FT* __restrict__ src, long long row_stride, int col, int src_w, int src_x0,
                                                  int y_first, int n_rows, int src_h, int src_y0, int lane, int px_stride = 1) {
    const long long sx = (long long)(mirror_near(col, src_w) + src_x0) * px_stride;
    return (float)src[(long long)(mirror_near(y_first + min(lane, n_rows - 1), src_h) + src_y0) * row_stride + sx];
}
// the same column of a strided frame: here the ROW is per lane and the column wave-uniform (the view carries its strides, `row_stride`
// and `px_stride` of the packed form are not used)
template <typename PX>
__device__ __forceinline__ float unit_edge_column(const StridedSrc<PX>& src, long long, int col, int src_w, int src_x0, int y_first,
                                                  int n_rows, int src_h, int src_y0, int lane, int = 1) {
    return src.at(mirror_near(y_first + min(lane, n_rows - 1), src_h) + src_y0, mirror_near(col, src_w) + src_x0);
}
// and of channel `ch` of a strided colour view with its three channels kept
__device__ __forceinline__ float unit_edge_column(const StridedRgbSrc& src, int ch, int col, int src_w, int src_x0, int y_first, int n_rows,
                                                  int src_h, int src_y0, int lane) {
    return src.at(mirror_near(y_first + min(lane, n_rows - 1), src_h) + src_y0, mirror_near(col, src_w) + src_x0, ch);
}
// and of channel `ch` of a frame of the YUV family
template <class D>
__device__ __forceinline__ float unit_edge_column(const YuvSrcOps<D>& src, int ch, int col, int src_w, int src_x0, int y_first, int n_rows,
                                                  int src_h, int src_y0, int lane) {
    return src.at(mirror_near(y_first + min(lane, n_rows - 1), src_h) + src_y0, mirror_near(col, src_w) + src_x0, ch);
}
// and of channel `ch` of a mosaic
__device__ __forceinline__ float unit_edge_column(const BayerSrc& src, int ch, int col, int src_w, int src_x0, int y_first, int n_rows,
                                                  int src_h, int src_y0, int lane) {
    return src.at(mirror_near(y_first + min(lane, n_rows - 1), src_h) + src_y0, mirror_near(col, src_w) + src_x0, ch);
}
__device__ __forceinline__ float unit_edge(float xcol, int i) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xcol), i));
}

// tf.maximum(x, [0]) with Eigen's CPU functor: a NaN stays a NaN (oracle: relu_tf).
__device__ __forceinline__ float relu_tf(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float clip_hi_tf(float v, float hi) { return v > hi ? hi : v; }

// relu + clip of N accumulators of one pixel: clip(relu(x), hi) with the reference's NaN behaviour.  The select forms
// ((x < 0) ? 0 : x, (x > hi) ? hi : x) keep a NaN a NaN but are 4 instructions per value, serialised through VCC with hazard
// nops.  For every non-NaN x they equal the median of (x, 0, hi) -- one v_med3_f32 -- when hi >= 0 (the fma chains start
// from +0, so x is never -0).  The N raw values are summed first: the sum is a NaN iff one of them is (or +inf meets -inf),
// and only then the wave takes the select form.  Wave-uniform branch; every lane of the wave must call this.
template <int N>
__device__ __forceinline__ void relu_clip_tf(float (&v)[N], float hi) {
    float chk = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) chk += v[k];
    if (hi >= 0.0f && !__any(chk != chk)) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = __builtin_amdgcn_fmed3f(v[k], 0.0f, hi);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = clip_hi_tf(relu_tf(v[k]), hi);
    }
}

// Value summary written by the fused RGB chain (rgb_line_end2_kernel, MM instantiation) for the sparse selection tail:
// entry = max_pool(value) over one pixel PAIR x kSumRows rows of a chain tile.
constexpr int kSumRowsLog2 = 4, kSumRows = 1 << kSumRowsLog2;
// How the sparse tail (sparse_select_kernel, silent_peaks.h) settles a (frame, level): by its candidates alone (every window maximum > 0); candidates + a synthesised all-zero
// map in the count pass (some window without a positive peak, but the level holds no NaN: every pixel mapped to such a window
// is a keypoint); or the dense kernels (such a window AND NaNs in the level, or too many candidates)
constexpr int kTailSparse = 0, kTailDense = 1, kTailZero = 2;

// order-preserving float <-> uint map so that integer atomics give float max / min
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// tf.nn.max_pool as the reference's device path evaluates it.  The reference pins its graph to '/device:GPU:0'
// (slam_recognition/recognition_testing.py:64); there TF 1.x runs MaxPoolForwardNHWC (`maxval = lowest(); if (x > maxval)
// maxval = x`) or cuDNN with CUDNN_NOT_PROPAGATE_NAN (TF_ENABLE_MAXPOOL_NANPROP defaults to false): a NaN never wins, the
// result is independent of the tap order, a window with nothing above lowest() yields lowest() = -FLT_MAX.
// Every maximum in silent_peaks.h (3x3 NMS, per-level max / min, window and cell maxima) goes through pool_max with the
// RUNNING maximum as first argument, so an accumulator is never a NaN and atomics only ever see ordered floats.
// Oracle: pool_max in oracle/silent_oracle.py.
constexpr float kPoolLowest = -3.402823466e+38f;
__device__ __forceinline__ float pool_max(float m, float v) { return v > m ? v : m; }
__device__ __forceinline__ unsigned pool_lowest_ord() { return f2ord(kPoolLowest); }

// v must already be NaN-free (a pool_max accumulator)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = pool_max(v, __shfl_xor(v, o));
    return v;
}

// Geometry of that value summary (host: build_sum_tab in silent_peaks_plan.h)
struct SumTab {
    int th, gpt;                       // tile height of the chain launch, groups per tile = ceil(th / kSumRows)
    long long frame_entries;
    long long off[kMaxLevels + 1];     // entry offset of level l inside a frame (off[n_levels] = frame_entries)
};

}  // namespace silent
