// pyramid_walk3_kernel: the whole zoom pyramid of a 3-channel (interleaved RGB) frame from ONE read of the frame, as a
// strip walk with a dedicated loader wave -- the structure of gray_walk_kernel (silent_walk.h) applied to the pyramid of
// BASELINE config 3 (the gray kernel is kept as a record under scripts/ubench/walk_kernels/), where round 1 ran two kernels (pyramid_unit_kernel<3> + pyramid_region_kernel<3>: the frame is fetched
// 2.95x, the region kernel moves 1.64x its algorithmic bytes and is latency-bound at 1.9 TB/s).
//
// Everything is indexed in FLOATS of the interleaved row (pixel p, channel c <-> float 3p + c):
//   * a block owns a strip of 144 pixels of one frame segment; wave 4 (the loader) LDS-DMAs the strip's rows (+ 4 / 3 halo
//     pixels) into a ring of 3 chunks x 8 rows, two chunks ahead, together with the chunk's row records;
//   * waves 0-3 (consumers) own 36 pixels each = 108 floats, two floats per lane, plus a halo of 2 / 3 pixels that only
//     the gather of the other levels needs: the unit level's 5 horizontal taps sit 3 floats apart and are read straight
//     from the ring (no DPP, hence no halo lanes for the smoother), the 5 vertical taps are a register window;
//   * the other levels: every output row of every level is a 6-tap combination of 6 CONSECUTIVE source rows (the spline's
//     support; the zoom step only says how often a row completes), so the lane keeps a window of its last 6 source rows and
//     evaluates a row when the row program (one record per source row, DMA'd into the ring with the rows) says it completes:
//     6 weights from the record, 6 fmas per float, taps ascending.  No rolling accumulators, no slots, no restart logic --
//     the first version carried gray_walk_kernel's accumulate-every-row scheme and spent 0.32 of its 0.87 ms there.  The
//     completed row goes through a wave-private LDS line, and lane 3j + c gathers the 6 taps of channel c of output pixel j
//     (3 floats apart) with column records staged in LDS -- the arithmetic order of the region kernel, bit-identical.
// Same protocol as the gray walk: one raw s_barrier per chunk, uniform trip counts, the consumers' vmcnt queue holds
// stores only.
// Round 3: a launch runs up to kW3MaxPlans WALK PLANS side by side (block -> frame, plan, segment, strip).  A plan is one crop
// of the frame with an optional unit level and the general levels that resample THAT crop.  A classic pyramid is one plan
// (unit level + every other level on the whole frame).  The reference's layout (image_to_zoom_tensor, from_image.py:45-64:
// nested centre crops, each resampled to one fixed size) is one plan per level: the unit level on the innermost crop, every
// other level alone on its own crop -- each mirrors at ITS crop's edge exactly like scipy does on the cropped array, and the
// nested re-reads of one frame sit next to each other in the launch (Infinity Cache).  The ring row is addressed in floats
// of the FRAME row from a 16-byte aligned origin (any crop offset), PX = 36 or 32 pixels per consumer wave (32: zoom steps
// down to 1.6, the reference's e ** .5).  Eligibility (host): W a multiple of 4, <= 21 outputs per wave tile and level.
#pragma once

#include <type_traits>

#include "silent_common.h"
#include "silent_gray.h"
#include "silent_pyramid.h"

namespace silent {

// ---- strip-walk declarations
constexpr int kWalkCH = 8;                          // rows per record chunk the host pads the row program to
#ifndef SILENT_W3_SLOTS
#define SILENT_W3_SLOTS 3
#endif
constexpr int kWalkSlots = SILENT_W3_SLOTS;         // chunks in the ring (the loader runs kWalkSlots - 1 chunks ahead of the consumers)

// tables of the in-walk pyramid (device memory owned by the plan)
struct WalkPyr {
    int G;                        // general levels (<= template G; the rest are inert)
    const int* row_prog;          // [out_h + 8 (+ padding)][w3_prog_row(Gp)]: record of stream row y at index y + 4
    const int* col_hdr;           // [G][waves_x][2]: first output column, number of outputs of the wave tile
    const int* col_rec;           // [waves_x][w3_rec_total(Gp)][8]: float index of tap 0 in the wave's line, 6 weights, pad
    long long px_off[8];          // pixel offset of level g inside one pyramid
    int out_w[8];
};

// compile-time loop: the body gets its index as an integral constant
template <int I, int N, class F>
__device__ __forceinline__ void walk_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        walk_static_for<I + 1, N>(f);
    }
}

typedef __attribute__((address_space(3))) void* walk_lds_ptr;
typedef const __attribute__((address_space(1))) void* walk_glb_ptr;

constexpr int kW3NC = 4;                        // consumer waves per block
constexpr int kW3HaloL = 4, kW3HaloR = 3;       // ring halo in pixels
constexpr int kW3MaxPlans = 8;                  // walk plans per launch
constexpr int kW3TileL = 2;                     // a wave's line starts 2 pixels left of its first pixel ...
constexpr int kW3TileF = 124;                   // ... and holds 124 floats (41 pixels + 1 float): taps -2 .. +3 of its anchors
// floats per ring row: the strip's 4 PX pixels + 7 of halo, + up to 3 floats of alignment shift, in whole 16-byte pieces (PX = 36: 456)
__host__ __device__ constexpr int w3_row_f(int px) { return ((kW3NC * px + kW3HaloL + kW3HaloR) * 3 + 3 + 3) / 4 * 4; }
constexpr int kW3RingTail = 16;                 // floats behind the ring's last row: a lane's six taps are tap 0 + 0, 3 .. 15 floats, and the
                                                // idle tail lanes of a wave's line read up to 12 floats past their row (into the next one)
constexpr int kW3Threads = (kW3NC + 1) * 64;
#ifndef SILENT_W3_CH
#define SILENT_W3_CH 4
#endif
#ifndef SILENT_W3_NV_ROWS
#define SILENT_W3_NV_ROWS SILENT_W3_CH
#endif
static_assert(SILENT_W3_CH % SILENT_W3_NV_ROWS == 0, "NV12 loader: rows of a chunk loaded and converted together");
#ifndef SILENT_W3_YUV_ROWS
#define SILENT_W3_YUV_ROWS SILENT_W3_NV_ROWS    // the same grouping for the planar / packed YUV loader (three bytes per row and slot)
#endif
static_assert(SILENT_W3_CH % SILENT_W3_YUV_ROWS == 0, "YUV loader: rows of a chunk loaded and converted together");
constexpr int kW3CH = SILENT_W3_CH;             // rows per chunk: a 12-row ring (22 KB) instead of 24 rows -- the loader is far from
                                                // being the limit (all loads alone: 0.14 ms), the consumers are latency-bound and
                                                // want waves: 31 KB of LDS per block = 4 blocks (16 consumer waves) per CU instead of 3
// column records per wave tile and level: output PIXELS anchored in a wave's PX pixels (36: zoom steps >= 1.875 ^ (g + 1);
// 32: >= 1.6 ^ (g + 1); 28: >= 1.4 ^ (g + 1), e.g. sqrt 2; 24: >= 1.2 ^ (g + 1), e.g. 2 ^ (1/3)); never more than 21 (the gather
// works on lane 3 j + c).  The host tries 36, 32, 28, 24 in this order and takes the first whose capacities hold the plan.
__host__ __device__ constexpr int w3_rec_cap(int px, int g) {
    return px == 36   ? (g == 0 ? 21 : (g == 1 ? 11 : (g == 2 ? 6 : (g == 3 ? 4 : (g <= 5 ? 2 : 1)))))
           : px == 32 ? (g == 0 ? 21 : (g == 1 ? 14 : (g == 2 ? 9 : (g == 3 ? 6 : (g == 4 ? 5 : 3)))))
           : px == 28 ? (g == 0 ? 21 : (g == 1 ? 15 : (g == 2 ? 11 : (g == 3 ? 8 : (g == 4 ? 6 : (g == 5 ? 4 : 3))))))
                      : (g == 0 ? 21 : (g == 1 ? 17 : (g == 2 ? 14 : (g == 3 ? 12 : (g == 4 ? 10 : (g == 5 ? 9 : 7))))));
}
__host__ __device__ constexpr int w3_rec_base(int px, int g) {
    int n = 0;
    for (int i = 0; i < g; ++i) n += w3_rec_cap(px, i);
    return n;
}
__host__ __device__ constexpr int w3_rec_total(int px, int g) { return w3_rec_base(px, g); }

// one walk plan (see the header)
struct Walk3Plan {
    int src_y0, src_x0, src_h, src_w;    // the crop this plan walks (frame coordinates)
    int shift;                           // (src_x0 * 3) mod 4: floats between the aligned ring origin and the crop's pixel - 4
    int has_unit;                        // the plan stores a unit (zoom 1) level
    int out_h, out_w, eff_h, eff_w;      // walk extents: the unit level's canvas and the part the crop covers (no unit level: the crop)
    int strips_x, segs_y, seg_rows;      // decomposition of this plan
    int block0;                          // first block of this plan among one frame's blocks
    long long px_off;                    // offset of the unit level in one pyramid
    WalkPyr pyr;                         // general levels of this plan (G may be 0)
};
struct Walk3Args {
    int H, W;                            // frame extents
    int n_plans, blocks_per_frame;
    long long frame_px;                  // pixels of one pyramid
    float wx[6];                         // [1, 26, 66, 26, 1] / 120 and scipy's sixth tap, 2^-53, as float32 (both axes)
    Walk3Plan plan[kW3MaxPlans];
};
// Union plans: the inner levels' first / last output rows and columns (pyramid_border_px, silent_pyramid.h: one thread per pixel and
// channel, taps straight from the frame) are the LAST blocks of the walk's launch, from block `first` on -- they fill the slots the
// walk's last round of blocks leaves idle instead of running behind it in a launch of their own.
struct WalkBorderArgs {
    int first, n_frames;                 // first = INT_MAX: none
    PyrTab tab;
    BorderTab bt;
};
// row record of the walk: [meta(0) .. meta(Gp-1)] [6 weights of level 0] ... [6 weights of level Gp-1], padded to a multiple
// of 4 dwords.  meta: bit 0 "an output row of this level completes with this source row", bits 8.. that output row.
__host__ __device__ constexpr int w3_prog_row(int gp) { return (gp * 7 + 3) / 4 * 4; }

// ---- the loader's addresses on a strided colour view (FrameStridedRgb, silent_pyramid_rgb8_view).  Host-callable: the kernel forms
// every address of its view loader through these functions, and tests/rgb8_view_host_main.cpp enumerates the same functions over every
// block, chunk, row, lane and load slot of a plan (inside the span, pixel bytes covered) without a GPU.
__host__ __device__ __forceinline__ int w3_mirror_near(int i, int n) {   // mirror_near (silent_common.h), host-callable
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
struct W3ViewBlock {
    int frame, plan;
    int y_first;                         // crop row of the block's stream row 0 (seg_y0 - 4; mirrored into the crop by w3_view_row)
    int A;                               // float of the virtual packed FRAME row that ring float 0 holds
    int n_chunks;
};
__host__ __device__ __forceinline__ W3ViewBlock w3_view_block(const Walk3Args& args, int px, unsigned bid) {
    W3ViewBlock b;
    b.frame = (int)(bid / (unsigned)args.blocks_per_frame);
    int rest = (int)(bid - (unsigned)b.frame * (unsigned)args.blocks_per_frame);
    b.plan = 0;
    for (int i = 1; i < kW3MaxPlans; ++i)
        if (i < args.n_plans && rest >= args.plan[i].block0) b.plan = i;
    const Walk3Plan& p = args.plan[b.plan];
    rest -= p.block0;
    const int strip = rest % p.strips_x, seg = rest / p.strips_x;
    const int seg_h = p.seg_rows < p.out_h - seg * p.seg_rows ? p.seg_rows : p.out_h - seg * p.seg_rows;
    b.y_first = seg * p.seg_rows - 4;
    b.A = (p.src_x0 + strip * (kW3NC * px) - kW3HaloL) * 3 - p.shift;
    b.n_chunks = (seg_h + 8 + kW3CH - 1) / kW3CH;
    return b;
}
// load slot k of a lane fills ring float 64 k + lane <-> float A + 64 k + lane of the virtual packed frame row, clamped into the row
// (what lies outside the crop is never consumed): its byte offset inside a row of the view.  Per block, not per chunk.
__host__ __device__ __forceinline__ long long w3_view_col(const Walk3Args& args, long long pixel_stride, int A, int lane, int k) {
    int f = A + lane + 64 * k;
    f = f < 0 ? 0 : (f > args.W * 3 - 1 ? args.W * 3 - 1 : f);
    return rgb_view_col(f, pixel_stride);
}
// stream row s of a block: byte offset of its frame row from `data` (scalar 64-bit arithmetic in the kernel)
__host__ __device__ __forceinline__ long long w3_view_row(const Walk3Args& args, const FrameStridedRgb& v, const W3ViewBlock& b, int s) {
    const Walk3Plan& p = args.plan[b.plan];
    return (long long)b.frame * v.frame_stride + (long long)(w3_mirror_near(b.y_first + s, p.src_h) + p.src_y0) * v.row_stride;
}
// THE address function: the load of (block, chunk, row of the chunk, lane, load slot) -- byte offset from `data` and width in bytes.
// (The general loader loads single bytes: width 1 at any stride and alignment.)
struct W3ViewLoad {
    long long offset;
    int width;
};
__host__ __device__ __forceinline__ W3ViewLoad w3_view_load(const Walk3Args& args, const FrameStridedRgb& v, int px, unsigned bid, int chunk,
                                                            int row, int lane, int k) {
    const W3ViewBlock b = w3_view_block(args, px, bid);
    return W3ViewLoad{w3_view_row(args, v, b, chunk * kW3CH + row) + w3_view_col(args, v.pixel_stride, b.A, lane, k), 1};
}
__host__ __device__ constexpr int w3_view_row_loads(int px) { return (w3_row_f(px) + 63) / 64; }   // load slots per ring row

// ---- the loader's addresses on NV12 surfaces (FrameNv12, silent_pyramid_nv12): ONE PIXEL per lane and load slot -- a byte of the luma
// row and the 2-byte (U, V) pair of the chroma row -- converted once and written as the pixel's three ring floats.  Ring float r of a
// row is float A + r of the virtual packed frame row (pixel f / 3, channel f % 3); slot k of a lane holds pixel p0 + 64 k + lane,
// p0 = floor(A / 3), whose floats are ring floats 3 (64 k + lane) + (3 p0 - A) + {0, 1, 2} (those outside the row are not written).
// Host-callable like the view's functions: tests/rgb_nv12_host_main.cpp enumerates them over whole launches.
__host__ __device__ constexpr int w3_nv12_row_loads(int px) { return ((w3_row_f(px) + 4) / 3 + 63) / 64; }   // load slots per ring row
__host__ __device__ __forceinline__ int w3_nv12_p0(int A) { return (A + 18) / 3 - 6; }   // floor(A / 3); A >= -15 (halo 4, shift <= 3)
// the frame column of (lane, slot), clamped into the frame row (what lies outside the crop is never consumed).  Per block.
__host__ __device__ __forceinline__ int w3_nv12_px(const Walk3Args& args, int A, int lane, int k) {
    const int p = w3_nv12_p0(A) + lane + 64 * k;
    return p < 0 ? 0 : (p > args.W - 1 ? args.W - 1 : p);
}
// stream row s of a block: byte offsets of its luma row from `y` and of its chroma row from `uv` (triple kinds: from `u` and from `v`
// alike) -- scalar 64-bit arithmetic in the kernel.  The chroma row is that of the FRAME row: (src_y0 + y) >> 1, not src_y0 / 2 + y / 2.
// One function for the four kinds; what differs is read through three accessors: the chroma planes' frame and row strides and the
// vertical chroma shift (pair kinds: 1).
struct W3Nv12Row {
    long long y, uv;
};
template <typename FT>
__host__ __device__ __forceinline__ long long w3_c_frame_stride(const FT& v) {
    if constexpr (kFrameYuvPair<FT>) return v.uv_frame_stride;
    else return v.c_frame_stride;
}
template <typename FT>
__host__ __device__ __forceinline__ long long w3_c_row_stride(const FT& v) {
    if constexpr (kFrameYuvPair<FT>) return v.uv_row_stride;
    else return v.c_row_stride;
}
template <typename FT>
__host__ __device__ __forceinline__ int w3_c_row_shift(const FT& v) {
    if constexpr (kFrameYuvPair<FT>) return 1;
    else return v.sy;
}
template <typename FT>
__host__ __device__ __forceinline__ W3Nv12Row w3_yuv_row(const Walk3Args& args, const FT& v, const W3ViewBlock& b, int s) {
    const Walk3Plan& p = args.plan[b.plan];
    const long long yy = w3_mirror_near(b.y_first + s, p.src_h) + p.src_y0;
    return W3Nv12Row{(long long)b.frame * v.y_frame_stride + yy * v.y_row_stride,
                     (long long)b.frame * w3_c_frame_stride(v) + (yy >> w3_c_row_shift(v)) * w3_c_row_stride(v)};
}
// THE address function: the loads of (block, chunk, row of the chunk, lane, load slot), BYTE offsets from the planes.
//   FrameNv12:  one byte at y_offset from `y`, two bytes at uv_offset from `uv` (any alignment)
//   FrameP010:  two bytes at y_offset, four bytes at uv_offset (byte columns 2 x and 4 (x >> 1); both 2-byte aligned)
//   FrameYuv:   one byte each at y_offset from `y`, u_offset from `u`, v_offset from `v` (columns x * y_pixel_stride, (x >> sx) * c_pixel_stride)
//   FrameYuv16: two bytes each at the same three offsets (all even)
// tests/rgb_{nv12,p010,yuv,yuv16}_host_main.cpp enumerate it over whole launches through the four spellings below: every offset is
// inside the spans, element-aligned, and that of an element that is some pixel's Y, U or V.
struct W3Nv12Load {
    long long y_offset, uv_offset;
};
// byte columns of frame column x in a luma row and in a chroma row of a pair kind
template <typename FT>
__host__ __device__ __forceinline__ long long w3_pair_y_col(int x) {
    if constexpr (kFrameP010<FT>) return p010_y_col(x);
    else return nv12_y_col(x);
}
template <typename FT>
__host__ __device__ __forceinline__ long long w3_pair_uv_col(int x) {
    if constexpr (kFrameP010<FT>) return p010_uv_col(x);
    else return nv12_uv_col(x);
}
struct W3YuvLoad {
    long long y_offset, u_offset, v_offset;
};
template <typename FT>
__host__ __device__ __forceinline__ auto w3_yuv_family_load(const Walk3Args& args, const FT& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    const W3ViewBlock b = w3_view_block(args, px, bid);
    const W3Nv12Row r = w3_yuv_row(args, v, b, chunk * kW3CH + row);
    const int x = w3_nv12_px(args, b.A, lane, k);
    if constexpr (kFrameYuvPair<FT>) {
        return W3Nv12Load{r.y + w3_pair_y_col<FT>(x), r.uv + w3_pair_uv_col<FT>(x)};
    } else {
        const long long c = r.uv + yuv_c_col(x, v.sx, v.c_pixel_stride);
        return W3YuvLoad{r.y + yuv_y_col(x, v.y_pixel_stride), c, c};
    }
}
__host__ __device__ __forceinline__ W3Nv12Load w3_nv12_load(const Walk3Args& args, const FrameNv12& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    return w3_yuv_family_load(args, v, px, bid, chunk, row, lane, k);
}
__host__ __device__ __forceinline__ W3Nv12Load w3_p010_load(const Walk3Args& args, const FrameP010& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    return w3_yuv_family_load(args, v, px, bid, chunk, row, lane, k);
}
__host__ __device__ __forceinline__ W3YuvLoad w3_yuv_load(const Walk3Args& args, const FrameYuv& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    return w3_yuv_family_load(args, v, px, bid, chunk, row, lane, k);
}
__host__ __device__ __forceinline__ W3YuvLoad w3_yuv16_load(const Walk3Args& args, const FrameYuv16& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    return w3_yuv_family_load(args, v, px, bid, chunk, row, lane, k);
}

// ---- the loader's addresses on raw Bayer mosaics (FrameBayer, silent_pyramid_bayer): ONE PIXEL per lane and load slot like the NV12
// family, but a pixel needs its 3 x 3 neighbourhood: the lane loads ITS column from three frame rows -- the ring row's frame row yy and
// yy - 1, yy + 1 reflected at the FRAME's edges (bayer_reflect; the crop's scipy mirror only chooses yy) -- and takes the columns left
// and right of it from the neighbouring lanes (a wave shift; the last lane of slot k neighbours the first lane of slot k + 1).  So the
// slots carry ONE MORE COLUMN on each side of the ring row: slot k of a lane holds pixel p0 + 64 k + lane with p0 = floor(A / 3) - 1,
// and its floats are ring floats 3 (64 k + lane) + (3 p0 - A) + {0, 1, 2} (those outside the row are not written).  Columns are clamped
// into the frame row; a lane at x == 0 takes its right neighbour for the left one and a lane at x == W - 1 its left one for the right
// (the reflection), whatever the clamped lanes beside it hold.  Host-callable: tests/rgb_bayer_host_main.cpp enumerates whole launches.
__host__ __device__ constexpr int w3_bayer_row_loads(int px) { return ((w3_row_f(px) + 4) / 3 + 2 + 63) / 64; }   // load slots per ring row
__host__ __device__ __forceinline__ int w3_bayer_p0(int A) { return w3_nv12_p0(A) - 1; }
__host__ __device__ __forceinline__ int w3_bayer_px(const Walk3Args& args, int A, int lane, int k) {
    const int p = w3_bayer_p0(A) + lane + 64 * k;
    return p < 0 ? 0 : (p > args.W - 1 ? args.W - 1 : p);
}
// stream row s of a block: its frame row and the two rows beside it, and their byte offsets from `data` (scalar 64-bit arithmetic)
struct W3BayerRows {
    int row[3];                          // yy - 1 (reflected), yy, yy + 1 (reflected)
    long long offset[3];
};
__host__ __device__ __forceinline__ W3BayerRows w3_bayer_rows(const Walk3Args& args, const FrameBayer& v, const W3ViewBlock& b, int s) {
    const Walk3Plan& p = args.plan[b.plan];
    const int yy = w3_mirror_near(b.y_first + s, p.src_h) + p.src_y0;
    W3BayerRows r;
    r.row[0] = bayer_reflect(yy - 1, args.H);
    r.row[1] = yy;
    r.row[2] = bayer_reflect(yy + 1, args.H);
    for (int i = 0; i < 3; ++i) r.offset[i] = (long long)b.frame * v.frame_stride + (long long)r.row[i] * v.row_stride;
    return r;
}
// THE address function: the three one-byte loads of (block, chunk, row of the chunk, lane, load slot) -- byte offsets from `data`, the
// frame rows they lie in and the frame column of the slot
struct W3BayerLoad {
    long long offset[3];
    int row[3];
    int col;
};
__host__ __device__ __forceinline__ W3BayerLoad w3_bayer_load(const Walk3Args& args, const FrameBayer& v, int px, unsigned bid, int chunk, int row, int lane, int k) {
    const W3ViewBlock b = w3_view_block(args, px, bid);
    const W3BayerRows r = w3_bayer_rows(args, v, b, chunk * kW3CH + row);
    W3BayerLoad l;
    l.col = w3_bayer_px(args, b.A, lane, k);
    for (int i = 0; i < 3; ++i) {
        l.row[i] = r.row[i];
        l.offset[i] = r.offset[i] + (long long)l.col * v.pixel_stride;
    }
    return l;
}
// the samples of a slot's column on the three rows as one register (row yy - 1 in bits 0 .. 7, yy in 8 .. 15, yy + 1 in 16 .. 23), so
// that ONE wave shift moves a neighbour's three samples; the column of lane - 1 / lane + 1 across the load slots of a ring row:
// lane 0 of slot k receives lane 63 of slot k - 1, lane 63 of slot k lane 0 of slot k + 1 (a DPP shift without bound_ctrl keeps `old`
// in the lane that has no source).  The first lane of slot 0 and the last of the last slot receive 0: carried columns, never converted
// into a ring float that is read.
__device__ __forceinline__ int w3_bayer_pack(unsigned char up, unsigned char mid, unsigned char down) { return (int)up | ((int)mid << 8) | ((int)down << 16); }
template <int N>
__device__ __forceinline__ int w3_bayer_left(const int (&p)[N], int k) {
    const int old = k > 0 ? __builtin_amdgcn_readlane(p[k > 0 ? k - 1 : 0], 63) : 0;
    return __builtin_amdgcn_update_dpp(old, p[k], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
template <int N>
__device__ __forceinline__ int w3_bayer_right(const int (&p)[N], int k) {
    const int old = k + 1 < N ? __builtin_amdgcn_readlane(p[k + 1 < N ? k + 1 : 0], 0) : 0;
    return __builtin_amdgcn_update_dpp(old, p[k], 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
// what bayer_rgb takes of a slot's pixel, from its packed column c and those of its neighbours l, r (x: its frame column, W: the frame's
// width): its own sample and the sums of its horizontal, vertical and diagonal neighbours.  Host-callable (integers only):
// tests/rgb_bayer_host_main.cpp replays the exchange of a ring row with it and compares the sums with those of the mosaic.
struct W3BayerSums {
    int c, h, v, d;
};
__host__ __device__ __forceinline__ W3BayerSums w3_bayer_sums(int W, int l, int c, int r, int x) {
    l = x == 0 ? r : l;                  // reflection at the frame's left / right edge (W >= 2: never both)
    r = x == W - 1 ? l : r;
    W3BayerSums s;
    s.c = (c >> 8) & 0xff;
    s.h = ((l >> 8) & 0xff) + ((r >> 8) & 0xff);
    s.v = (c & 0xff) + ((c >> 16) & 0xff);
    s.d = ((l & 0xff) + (r & 0xff)) + (((l >> 16) & 0xff) + ((r >> 16) & 0xff));
    return s;
}
// ring float of channel 0 of the pixel of (lane, slot)
__host__ __device__ __forceinline__ int w3_bayer_ring_float(int A, int lane, int k) { return 3 * (lane + 64 * k) + (3 * w3_bayer_p0(A) - A); }
// the three channels of the slot's pixel (yy: its frame row)
__device__ __forceinline__ void w3_bayer_values(const FrameBayer& f, int l, int c, int r, int x, int yy, float& c0, float& c1, float& c2) {
    const W3BayerSums s = w3_bayer_sums(f.W, l, c, r, x);
    bayer_rgb(s.c, s.h, s.v, s.d, yy & 1, x & 1, f.pattern, f.order, c0, c1, c2);
}

// ---- the loader's registers on the family: the element types of a load slot (luma element; the chroma pair, or the U element; the V
// element of the triple kinds), "fetch slot k of a row" (one template: the loads are the register types' sizes) and "loaded elements ->
// (Yv, Uv, Vv)" per frame kind.  yr / ur / vr: the row's
// plane pointers (pair kinds: ur is the pair's plane); ycol / ccol: the slot's byte columns in a luma and in a chroma row.
template <typename FT>
struct W3YuvRegs {
    typedef unsigned char y, c, w;                          // FrameYuv
};
template <>
struct W3YuvRegs<FrameNv12> {
    typedef unsigned char y, w;
    typedef unsigned short c;                               // the (U, V) bytes as one 2-byte load
};
template <>
struct W3YuvRegs<FrameP010> {
    typedef unsigned short y;
    typedef unsigned c;                                     // the (U, V) elements as one dword
    typedef unsigned char w;
};
template <>
struct W3YuvRegs<FrameYuv16> {
    typedef unsigned short y, c, w;
};
template <typename FT, typename EY, typename EC, typename EW>
__device__ __forceinline__ void w3_yuv_fetch(const unsigned char* yr, const unsigned char* ur, const unsigned char* vr, long long ycol, long long ccol,
                                             EY& ey, EC& ec, EW& ew) {
    __builtin_memcpy(&ey, yr + ycol, sizeof(EY));
    __builtin_memcpy(&ec, ur + ccol, sizeof(EC));          // (a pair kind: both chroma elements in one load)
    if constexpr (kFrameYuvTriple<FT>) __builtin_memcpy(&ew, vr + ccol, sizeof(EW));
}
__device__ __forceinline__ void w3_yuv_values(const FrameNv12& f, unsigned char ey, unsigned short ec, const unsigned char&, float& yv, float& uv, float& vv) {
    yv = __fsub_rn((float)ey, f.oy);
    uv = (float)((int)(ec & 0xffu) - 128), vv = (float)((int)(ec >> 8) - 128);
}
__device__ __forceinline__ void w3_yuv_values(const FrameP010& f, unsigned short ey, unsigned ec, const unsigned char&, float& yv, float& uv, float& vv) {
    p010_values(ey, ec, f.oy, f.oc, f.shift, yv, uv, vv);
}
__device__ __forceinline__ void w3_yuv_values(const FrameYuv& f, unsigned char ey, unsigned char ec, const unsigned char& ew, float& yv, float& uv, float& vv) {
    yv = __fsub_rn((float)ey, f.oy);
    uv = (float)((int)ec - 128), vv = (float)((int)ew - 128);
}
__device__ __forceinline__ void w3_yuv_values(const FrameYuv16& f, unsigned short ey, unsigned short ec, const unsigned short& ew, float& yv, float& uv, float& vv) {
    yuv16_values(ey, ec, ew, f.oy, f.oc, f.shift, f.mask, yv, uv, vv);
}

// FT: the frame element type -- float, or unsigned char (packed interleaved uint8 colour frames [n, H, W, 3], silent_pyramid_rgb8: byte c
// of pixel (y, x) enters as (float)byte, an unsigned load and an exact conversion).  Only the LOADER touches the frame: the ring stays
// float32 and the consumers' text is the same for both kinds, so the uint8 kernel stores the bits the float kernel stores for the
// widened frame.  The FT = float instantiations are the code as it was (their machine code is unchanged).
// FT = FrameStridedRgb (the same bytes in a strided view, by value): the packed kind's ONE-BYTE loader -- ring float r of a row is the
// byte of float A + r of the virtual packed frame row, (f / 3) * pixel_stride + f % 3 (w3_view_col, once per block) behind the row's
// scalar 64-bit offset (w3_view_row); the ring, the shift, the mirror fix-up and the consumers do not know about strides.  All byte
// loads of a chunk are issued before one is consumed; the chunk is complete (vmcnt(0) lgkmcnt(0)) before the barrier.  Every address
// is that of a channel byte of a pixel of the view: nothing outside [data, data + span) is loaded.
// FT = FrameNv12 (NV12 surfaces, by value): a pixel per lane and load slot (w3_nv12_load; w3_yuv_fetch / w3_yuv_values per kind), Y byte + (U, V) pair, converted by
// nv12_channel with the coefficients in SGPRs, three ring floats written; the same issue / wait / barrier order as the byte loaders.
// Every address is that of a luma byte or of the chroma pair of a pixel of the frame.
// FT = FrameP010 (P010 / P012 / P016 surfaces, by value): the NV12 loader with uint16 elements (w3_p010_load) -- a 2-byte luma load and
// the pair as one dword per slot, p010_values (shift, offsets) in front of the same nv12_channel; the depth is a runtime scalar.
// FT = FrameYuv (planar / packed 8-bit YUV, by value): the NV12 loader with three byte loads per slot (w3_yuv_load) -- the byte columns
// x * y_pixel_stride and (x >> sx) * c_pixel_stride are computed once per block, the row terms are scalar; issue / wait / barrier order
// is NV12's.  Every address is that of a byte that is some pixel's Y, U or V.
// FT = FrameYuv16 (16-bit YUV, by value): the FrameYuv loader with three 2-byte loads per slot (w3_yuv16_load) and yuv16_values (shift,
// mask, offsets) in front of the same nv12_channel; depth and alignment of the code are runtime scalars.
// FT = FrameBayer (raw 8-bit Bayer mosaics, by value): a pixel per lane and load slot, THREE frame rows per ring row (w3_bayer_load): the
// lane's own column as three byte loads -- the YUV triple's count --, the columns beside it from the neighbouring lanes (w3_bayer_left /
// _right), bayer_rgb, three ring floats written; issue / wait / barrier order is NV12's.  Every address is that of a pixel of the view.
template <int G, int PX, typename FT = float>
__global__ __launch_bounds__(kW3Threads) void pyramid_walk3_kernel(frame_param<FT> frames, float* __restrict__ pyr,
                                                                    const Walk3Args args, const WalkBorderArgs border) {
    static_assert(std::is_same<FT, float>::value || kFrameBytes<FT> || kFrameRgbView<FT> || kFrameYuvFamily<FT> || kFrameBayer<FT>,
                  "float32, packed uint8 or strided uint8 colour frames, NV12 / P010 / YUV / 16-bit YUV surfaces, Bayer mosaics");
    constexpr bool kBy = kFrameBayer<FT>;                            // the loader demosaics in registers
    constexpr bool kYuv3 = kFrameYuvTriple<FT>;                      // three loads per slot, byte columns per lane
    constexpr bool kNv = kFrameYuvFamily<FT>;                        // the loader converts (Y, U, V) in registers
    constexpr bool kBytes = kFrameBytes<FT> || kFrameRgbView<FT>;   // the loader widens bytes in registers
    static_assert(G == stream_pad_levels(G), "row programs are padded to 4 or 7 levels");
    static_assert(PX == 36 || PX == 32 || PX == 28 || PX == 24, "");
    constexpr int kW3Px = PX, kW3StripPx = kW3NC * PX, kW3RowF = w3_row_f(PX);
    static_assert(kW3RowF > 256 && kW3RowF <= 512, "two DMA loads of 64 x 16 bytes per ring row");
    constexpr int PR = w3_prog_row(G);
    constexpr int kRecTotal = w3_rec_total(PX, G);
    __shared__ __attribute__((aligned(16))) float s_ring_f[kWalkSlots * kW3CH * kW3RowF + kW3RingTail];
    float (*s_ring)[kW3RowF] = reinterpret_cast<float (*)[kW3RowF]>(s_ring_f);
    __shared__ __attribute__((aligned(16))) int s_prog[kWalkSlots * kW3CH * PR];                // row records of the ring's chunks
    __shared__ __attribute__((aligned(16))) float s_line[kW3NC * 128];                            // a completed row, per wave
    __shared__ __attribute__((aligned(16))) int s_rec[kW3NC * kRecTotal * 8];                     // column records, per wave

    if (blockIdx.x >= (unsigned)border.first) {   // block-uniform
        if (threadIdx.x < 256)
            pyramid_border_px<3, true, FT>(frames, pyr, border.tab, border.bt, (long long)(blockIdx.x - (unsigned)border.first) * 256 + threadIdx.x, border.n_frames);
        return;
    }
    const unsigned bid = blockIdx.x;
    const int frame = (int)(bid / (unsigned)args.blocks_per_frame);
    int rest = (int)(bid - (unsigned)frame * (unsigned)args.blocks_per_frame);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kW3MaxPlans; ++i)
        if (i < args.n_plans && rest >= args.plan[i].block0) pi = i;
    const Walk3Plan& tab = args.plan[pi];          // (scalar loads: the plan index is block-uniform)
    const WalkPyr& wp = tab.pyr;
    rest -= tab.block0;
    const int strip = rest % tab.strips_x;
    const int seg = rest / tab.strips_x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg_y0 = seg * tab.seg_rows;
    const int seg_h = min(tab.seg_rows, tab.out_h - seg_y0);
    const int n_rows = seg_h + 8;                              // stream rows seg_y0 - 4 .. seg_y0 + seg_h + 3
    const int n_chunks = (n_rows + kW3CH - 1) / kW3CH;
    const int X0 = strip * kW3StripPx;                         // first pixel of the strip; the ring row starts at pixel X0 - 4
    const int R0 = X0 - kW3HaloL;

    if (wave == kW3NC) {
        // ------------------------------------------------------------------ loader: LDS-DMA only
        typedef typename std::conditional<kFrameRgbSrc<FT>, unsigned char, FT>::type ET;   // element of a frame row
        const ET* __restrict__ src;
        if constexpr (kFrameRgbView<FT>) src = frames.data;    // (rows: w3_view_row)
        else if constexpr (kNv) src = reinterpret_cast<const unsigned char*>(frames.y);   // (rows: w3_yuv_row; strides are bytes)
        else if constexpr (kBy) src = frames.data;             // (rows: w3_bayer_rows)
        else src = frames + (long long)frame * args.H * args.W * 3;
        const int rowf = args.W * 3;                           // floats (uint8 frames: bytes) of a FRAME row
        // ring float r <-> frame-row float A + r, A = the crop's pixel R0 minus the alignment shift.  Frame widths that are a
        // multiple of 4 (every row starts on 16 bytes): A is a multiple of 4 and a lane fetches a 16-byte aligned group of 4 floats,
        // two DMA loads per ring row.  Other widths (round 5): no shift, a lane fetches ONE FLOAT, 5 - 8 loads per ring row -- the
        // loader has the time (one row per ~2000 cycles of its consumers).  (The 12-byte DMA, one pixel per lane, is no way out: it
        // writes lane l's 12 bytes at 16 l, scripts/ubench/lds_dma_b96.hip.)  Pieces that stick out of the row are clamped to a valid
        // address; whatever lies outside the CROP is never read (the consumers read mirrored pixels instead)
        const int A = (tab.src_x0 + R0) * 3 - tab.shift;
        auto loader = [&](auto dword_dma) {
            constexpr bool DWORD_DMA = decltype(dword_dma)::value;
            constexpr int kRowLoads = DWORD_DMA ? (kW3RowF + 63) / 64 : 2;   // DMA instructions per ring row
            typename std::conditional<kFrameRgbView<FT>, long long, int>::type f[kRowLoads];
            W3ViewBlock vb;
            (void)vb;
            constexpr int kNvLoads = w3_nv12_row_loads(PX);
            int nvx[kNv ? kNvLoads : 1];                         // NV12: the lane's frame column per load slot
            int nvd = 0;                                         // and ring float of channel 0 of its slot-0 pixel minus 3 lane
            long long yuy[kYuv3 ? kNvLoads : 1], yuc[kYuv3 ? kNvLoads : 1];   // YUV: its byte column in a luma / chroma row
            (void)nvx;
            (void)nvd;
            (void)yuy;
            (void)yuc;
            constexpr int kByLoads = w3_bayer_row_loads(PX);
            int byx[kBy ? kByLoads : 1];                         // Bayer: the lane's frame column per load slot ...
            long long byc[kBy ? kByLoads : 1];                   // ... and its byte column in a row of the view
            (void)byx;
            (void)byc;
            if constexpr (kBy) {
                vb = w3_view_block(args, PX, bid);
                nvd = w3_bayer_ring_float(vb.A, 0, 0);
#pragma unroll
                for (int k = 0; k < kByLoads; ++k) {
                    byx[k] = w3_bayer_px(args, vb.A, lane, k);
                    byc[k] = (long long)byx[k] * frames.pixel_stride;
                }
            } else if constexpr (kNv) {
                vb = w3_view_block(args, PX, bid);
                nvd = 3 * w3_nv12_p0(vb.A) - vb.A;
#pragma unroll
                for (int k = 0; k < kNvLoads; ++k) nvx[k] = w3_nv12_px(args, vb.A, lane, k);
                if constexpr (kYuv3) {
#pragma unroll
                    for (int k = 0; k < kNvLoads; ++k) {
                        yuy[k] = yuv_y_col(nvx[k], frames.y_pixel_stride);
                        yuc[k] = yuv_c_col(nvx[k], frames.sx, frames.c_pixel_stride);
                    }
                }
            } else if constexpr (kFrameRgbView<FT>) {
                static_assert(kRowLoads == w3_view_row_loads(PX), "");
                vb = w3_view_block(args, PX, bid);
#pragma unroll
                for (int k = 0; k < kRowLoads; ++k) f[k] = w3_view_col(args, frames.pixel_stride, vb.A, lane, k);
            } else {
#pragma unroll
            for (int k = 0; k < kRowLoads; ++k)
                f[k] = DWORD_DMA ? min(max(A + lane + 64 * k, 0), rowf - 1) : min(max(A + 256 * k + lane * 4, 0), rowf - 4);
            }
            auto issue = [&](int c, int slot) {
                // uint8 frames: the same lane -> ring mapping with the frame row counted in BYTES -- a lane's group of 4 ring floats is
                // one dword of the frame row (4 bytes, widened in registers, one 16-byte LDS write), its single float one byte.  All
                // loads of the chunk are issued first (8 or 32 in flight: one memory latency per chunk, not one per load), then the
                // records' DMA, then the rows are widened and written; the chunk is complete -- vmcnt(0), lgkmcnt(0) -- before the loader
                // goes on to its next barrier, still two chunks ahead of the consumers, who take ~2000 cycles a row
                typename std::conditional<DWORD_DMA, unsigned char, unsigned>::type v[kBytes ? kW3CH : 1][kRowLoads];
                (void)v;
                // NV12: the rows of a chunk are loaded and converted in groups of kNvRows (SILENT_W3_NV_ROWS; default: the whole chunk,
                // one memory latency per chunk) -- a group's loads (Y byte + chroma pair per slot) are all in flight before one is
                // consumed; a smaller group reuses the registers and pays a latency per group (measured slower:
                // profiles/rgb_nv12/README.md)
                constexpr int kNvRows = kYuv3 ? SILENT_W3_YUV_ROWS : SILENT_W3_NV_ROWS;
                typedef W3YuvRegs<typename std::conditional<kNv, FT, FrameYuv>::type> NvRegs;
                typename NvRegs::y nvy[kNv ? kNvRows : 1][kNv ? kNvLoads : 1];   // the luma element
                typename NvRegs::c nvc[kNv ? kNvRows : 1][kNv ? kNvLoads : 1];   // the chroma pair; YUV: the U element
                typename NvRegs::w nvw[kNv ? kNvRows : 1][kNv ? kNvLoads : 1];   // YUV: the V element (pair kinds: not used)
                (void)nvy;
                (void)nvc;
                (void)nvw;
                auto nv_load = [&](int g, int r) {                // row g + r of the chunk into register row r
                    if constexpr (kNv) {
                        const W3Nv12Row row = w3_yuv_row(args, frames, vb, c * kW3CH + g + r);
                        const unsigned char* yr = src + row.y;
                        const unsigned char *ur, *vr;
                        if constexpr (kYuv3) {
                            ur = reinterpret_cast<const unsigned char*>(frames.u) + row.uv;
                            vr = reinterpret_cast<const unsigned char*>(frames.v) + row.uv;
                        } else {
                            ur = vr = reinterpret_cast<const unsigned char*>(frames.uv) + row.uv;
                        }
#pragma unroll
                        for (int k = 0; k < kNvLoads; ++k) {
                            if constexpr (kYuv3) w3_yuv_fetch<FT>(yr, ur, vr, yuy[k], yuc[k], nvy[r][k], nvc[r][k], nvw[r][k]);
                            else w3_yuv_fetch<FT>(yr, ur, vr, w3_pair_y_col<FT>(nvx[k]), w3_pair_uv_col<FT>(nvx[k]), nvy[r][k], nvc[r][k], nvw[r][k]);
                        }
                    }
                };
                // Bayer: the lane's column on the three frame rows of every ring row of the chunk (3 kW3CH kByLoads byte loads, all in
                // flight before one is consumed), then per row: pack, exchange the columns between lanes, demosaic, three ring floats
                unsigned char byu[kBy ? kW3CH : 1][kBy ? kByLoads : 1], bym[kBy ? kW3CH : 1][kBy ? kByLoads : 1], byd[kBy ? kW3CH : 1][kBy ? kByLoads : 1];
                int byy[kBy ? kW3CH : 1];                        // the ring rows' frame rows (wave-uniform)
                (void)byu;
                (void)bym;
                (void)byd;
                (void)byy;
#pragma unroll
                for (int r = 0; r < kW3CH; ++r) {
                    if constexpr (kBy) {
                        const W3BayerRows rows = w3_bayer_rows(args, frames, vb, c * kW3CH + r);
                        byy[r] = rows.row[1];
#pragma unroll
                        for (int k = 0; k < kByLoads; ++k) {
                            byu[r][k] = src[rows.offset[0] + byc[k]];
                            bym[r][k] = src[rows.offset[1] + byc[k]];
                            byd[r][k] = src[rows.offset[2] + byc[k]];
                        }
                    } else if constexpr (kNv) {
                        if (r < kNvRows) nv_load(0, r);
                    } else {
                    const int y = seg_y0 - 4 + c * kW3CH + r;
                    const ET* rp;
                    if constexpr (kFrameRgbView<FT>) rp = src + w3_view_row(args, frames, vb, c * kW3CH + r);
                    else rp = src + (long long)(mirror_near(y, tab.src_h) + tab.src_y0) * args.W * 3;
                    float* dst = &s_ring[slot * kW3CH + r][0];
                    if constexpr (kBytes) {
                        (void)dst;
#pragma unroll
                        for (int k = 0; k < kRowLoads; ++k) {
                            if constexpr (DWORD_DMA) v[r][k] = rp[f[k]];
                            else v[r][k] = *reinterpret_cast<const unsigned*>(rp + f[k]);
                        }
                    } else if constexpr (DWORD_DMA) {
#pragma unroll
                        for (int k = 0; k < kRowLoads; ++k)
                            if (k + 1 < kRowLoads || lane < kW3RowF - 64 * k)
                                __builtin_amdgcn_global_load_lds((walk_glb_ptr)(rp + f[k]), (walk_lds_ptr)(dst + 64 * k), 4, 0, 0);
                    } else {
                        __builtin_amdgcn_global_load_lds((walk_glb_ptr)(rp + f[0]), (walk_lds_ptr)dst, 16, 0, 0);
                        if (lane < (kW3RowF - 256) / 4)
                            __builtin_amdgcn_global_load_lds((walk_glb_ptr)(rp + f[1]), (walk_lds_ptr)(dst + 256), 16, 0, 0);
                    }
                    }
                }
                const int* rp = wp.row_prog + ((long long)seg_y0 + (long long)c * kW3CH) * PR + lane * 4;
                int* dst = s_prog + slot * (kW3CH * PR);
                constexpr int NV = kW3CH * PR / 4;               // 16-byte pieces of a chunk's records
                if (lane < NV) __builtin_amdgcn_global_load_lds((walk_glb_ptr)rp, (walk_lds_ptr)dst, 16, 0, 0);
                if constexpr (NV > 64) {
                    if (lane < NV - 64) __builtin_amdgcn_global_load_lds((walk_glb_ptr)(rp + 256), (walk_lds_ptr)(dst + 256), 16, 0, 0);
                }
                if constexpr (kBy) {
#pragma unroll
                    for (int r = 0; r < kW3CH; ++r) {
                        float* row = &s_ring[slot * kW3CH + r][0];
                        int pk[kByLoads];
#pragma unroll
                        for (int k = 0; k < kByLoads; ++k) pk[k] = w3_bayer_pack(byu[r][k], bym[r][k], byd[r][k]);
#pragma unroll
                        for (int k = 0; k < kByLoads; ++k) {
                            float ch3[3];
                            w3_bayer_values(frames, w3_bayer_left(pk, k), pk[k], w3_bayer_right(pk, k), byx[k], byy[r], ch3[0], ch3[1], ch3[2]);
                            const int q = 3 * (lane + 64 * k) + nvd;     // ring float of channel 0
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch)
                                if (q + ch >= 0 && q + ch < kW3RowF) row[q + ch] = ch3[ch];
                        }
                    }
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // rows written, records landed
                } else if constexpr (kNv) {
#pragma unroll
                    for (int g = 0; g < kW3CH; g += kNvRows) {
                        if (g > 0) {
                            asm volatile("" ::: "memory");           // (the next group's loads stay behind this group's conversion)
#pragma unroll
                            for (int r = 0; r < kNvRows; ++r) nv_load(g, r);
                        }
#pragma unroll
                        for (int r = 0; r < kNvRows; ++r) {
                            float* row = &s_ring[slot * kW3CH + g + r][0];
#pragma unroll
                            for (int k = 0; k < kNvLoads; ++k) {
                                float yv, uv, vv;
                                w3_yuv_values(frames, nvy[r][k], nvc[r][k], nvw[r][k], yv, uv, vv);
                                const int q = 3 * (lane + 64 * k) + nvd;     // ring float of channel 0
#pragma unroll
                                for (int ch = 0; ch < 3; ++ch)
                                    if (q + ch >= 0 && q + ch < kW3RowF)
                                        row[q + ch] = nv12_channel(yv, uv, vv, frames.m[3 * ch], frames.m[3 * ch + 1], frames.m[3 * ch + 2]);
                            }
                        }
                    }
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // rows written, records landed
                } else if constexpr (kBytes) {
#pragma unroll
                    for (int r = 0; r < kW3CH; ++r) {
                        float* row = &s_ring[slot * kW3CH + r][0];
#pragma unroll
                        for (int k = 0; k < kRowLoads; ++k) {
                            if constexpr (DWORD_DMA) {
                                if (k + 1 < kRowLoads || lane < kW3RowF - 64 * k) row[64 * k + lane] = (float)v[r][k];
                            } else {
                                const unsigned q = v[r][k];
                                if (k == 0 || lane < (kW3RowF - 256) / 4)
                                    *reinterpret_cast<float4*>(row + 256 * k + lane * 4) =
                                        make_float4((float)(q & 0xffu), (float)((q >> 8) & 0xffu), (float)((q >> 16) & 0xffu), (float)(q >> 24));
                            }
                        }
                    }
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // rows written, records landed
                }
            };
            // scipy mirrors every tap at the CROP's edge (d c b | a b c d | c b a).  The ring row of a strip at the crop's left / right
            // edge holds whatever lies beside the crop in the frame (or a clamped address): the loader writes the mirrored pixels over
            // those halo positions -- up to 4 pixels left (q = -4 .. -1 <- -q) and 3 right (q = n .. n + 2 <- 2 (n - 1) - q) -- once per
            // chunk, so that the consumers read every tap at a fixed offset from tap 0 (no per-tap offsets, no mirror arithmetic)
            int fix_dst = 0, fix_src = 0;
            bool fix = false;
            {
                const int n = tab.src_w;
                const int q = lane < 12 ? -4 + lane / 3 : n + (lane - 12) / 3;
                const int ch = lane < 12 ? lane % 3 : (lane - 12) % 3;
                const int qs = lane < 12 ? -q : 2 * (n - 1) - q;
                fix = lane < 21 && q - R0 >= 0 && q - R0 < kW3StripPx + kW3HaloL + kW3HaloR && qs - R0 >= 0 && qs - R0 < kW3StripPx + kW3HaloL + kW3HaloR;
                fix_dst = (q - R0) * 3 + ch + tab.shift;
                fix_src = (qs - R0) * 3 + ch + tab.shift;
            }
            const bool any_fix = __any(fix);                        // wave-uniform: an edge strip
            static_assert(kWalkSlots == 2 || kWalkSlots == 3, "");
            issue(0, 0);
            if (kWalkSlots == 3 && n_chunks > 1) issue(1, 1);
            int slot2 = kWalkSlots - 1, slot0 = 0;
            for (int c = 0; c < n_chunks; ++c) {
                // chunk c has landed when at most the next chunk's loads (three slots: one chunk in flight behind it) are outstanding
                // (uint8 frames: nothing is outstanding here, issue() ends with vmcnt(0) -- the counted wait would name a mix of register
                // loads and DMA loads that the compiler is free to reorder)
                if (!kBytes && !kNv && !kBy && kWalkSlots == 3 && c + 1 < n_chunks) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kRowLoads * kW3CH + (kW3CH * PR / 4 > 64 ? 2 : 1)) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (any_fix) {
#pragma unroll
                    for (int r = 0; r < kW3CH; ++r) {
                        float* row = &s_ring[slot0 * kW3CH + r][0];
                        if (fix) row[fix_dst] = row[fix_src];
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                slot0 = slot0 == kWalkSlots - 1 ? 0 : slot0 + 1;
                __builtin_amdgcn_s_barrier();
                if (c + kWalkSlots - 1 < n_chunks) issue(c + kWalkSlots - 1, slot2);
                slot2 = slot2 == kWalkSlots - 1 ? 0 : slot2 + 1;
            }
        };
        // (uint8 frames: a dword of the frame row needs a 4-byte aligned ADDRESS -- W % 4 == 0 puts every frame and row start and every
        // group on the dword grid relative to `frames`, which has no alignment requirement: the base decides, and any other base
        // takes the one-byte path, which never touches a byte outside the batch)
        bool single = (rowf & 3) != 0;                          // block-uniform
        if constexpr (kFrameBytes<FT>) single = single || (reinterpret_cast<unsigned long long>(frames) & 3ull) != 0;
        if constexpr (kFrameRgbSrc<FT>) loader(std::true_type{});   // a view: always the one-byte path (any strides, any alignment); NV12: its pixel-per-lane loader
        else if (single) loader(std::true_type{});
        else loader(std::false_type{});
        return;
    }

    // ---------------------------------------------------------------------- consumers
    const int wx0 = X0 + wave * kW3Px;                          // first pixel of this wave
    const bool live = wx0 < tab.out_w;                          // wave-uniform; a dead wave still meets every barrier
    // the lane's two floats: line floats lane and lane + 64 <-> pixel wx0 - 2 + i / 3, channel i % 3 (i = lane + 64 k).  Stride 1
    // across the lanes: the ring reads and the line writes are free of bank conflicts (floats 2 lane, 2 lane + 1 gave 2-way
    // conflicts on every ds_read_b32: SQ_LDS_BANK_CONFLICT was 1.6x the LDS instruction cycles), and a store instruction writes
    // 256 contiguous bytes without any alignment condition on the level
    // ring offset (in floats) of tap 0 (pixel - 2) of each float; tap d is 3 d floats further (the loader has mirrored the crop's
    // edges into the ring): one address per float, the six taps as immediate offsets (pairs of them share a ds_read2_b32)
    int tap0[2];
    int px[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = lane + 64 * k;
        const int p = wx0 - kW3TileL + i / 3, c = i % 3;
        px[k] = p;
        tap0[k] = min(max((p - 2 - R0) * 3 + c + tab.shift, 0), kW3RowF - 1);
    }
    const bool out0 = px[0] >= wx0 && px[0] < wx0 + kW3Px && px[0] < tab.out_w;
    const bool out1 = px[1] >= wx0 && px[1] < wx0 + kW3Px && px[1] < tab.out_w && lane + 64 < kW3TileF;
    const bool eff0 = px[0] < tab.eff_w, eff1 = px[1] < tab.eff_w;
    const long long base_f = ((long long)frame * args.frame_px + tab.px_off) * 3 + (long long)(wx0 - kW3TileL) * 3 + lane;
    const bool has_unit = tab.has_unit != 0;                    // block-uniform

    float hist[6][2];                                           // the lane's two floats on the last 6 source rows
#pragma unroll
    for (int j = 0; j < 6; ++j) hist[j][0] = hist[j][1] = 0.0f;
    int gx0[G], gn[G];
    const long long frame_px0 = (long long)frame * args.frame_px;
    int* const my_rec = s_rec + wave * (kRecTotal * 8);
    float* const my_line = s_line + wave * 128;
    {
        const int wx_tile = strip * kW3NC + wave;
        const int4* __restrict__ src4 = reinterpret_cast<const int4*>(wp.col_rec) + (long long)wx_tile * (kRecTotal * 2);
        int4* dst4 = reinterpret_cast<int4*>(my_rec);
        if (wp.G > 0)
            for (int i = lane; i < kRecTotal * 2; i += 64) dst4[i] = src4[i];
        typedef const __attribute__((address_space(4))) int* const_int_ptr;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int gg = max(min(g, wp.G - 1), 0);
            const_int_ptr h = (const_int_ptr)(wp.col_hdr + ((long long)gg * (tab.strips_x * kW3NC) + wx_tile) * 2);
            gx0[g] = wp.G > 0 ? h[0] : 0;
            gn[g] = g < wp.G ? h[1] : 0;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // records staged (the only vector loads of a consumer)
        __builtin_amdgcn_wave_barrier();
    }
    const int gj = lane / 3, gc = lane - 3 * gj;               // gather role: output pixel gj, channel gc

    float hw[6][2];                                             // horizontally smoothed rows y-5 .. y of the two floats
#pragma unroll
    for (int j = 0; j < 6; ++j) hw[j][0] = hw[j][1] = 0.0f;

    int slot = 0;
    for (int c = 0; c < n_chunks; ++c) {
        __builtin_amdgcn_s_barrier();                           // barrier c: chunk c (rows + records) is in the ring
        asm volatile("" ::: "memory");
        if (live) {
#pragma unroll
            for (int r = 0; r < kW3CH; ++r) {
                const int s = c * kW3CH + r;                  // stream row; source row y = seg_y0 - 4 + s
                if (s >= n_rows) break;                         // wave-uniform
                const float* __restrict__ row = &s_ring[slot * kW3CH + r][0];
                float t[2][6];
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int d = 0; d < 6; ++d) t[k][d] = row[tap0[k] + 3 * d];
                const int* __restrict__ prow = s_prog + (slot * kW3CH + r) * PR;
                int meta_v[(G + 3) / 4 * 4];
#pragma unroll
                for (int e = 0; e < (G + 3) / 4; ++e) {
                    const int4 q = reinterpret_cast<const int4*>(prow)[e];   // every lane reads the same record (LDS broadcast)
                    meta_v[4 * e] = q.x; meta_v[4 * e + 1] = q.y; meta_v[4 * e + 2] = q.z; meta_v[4 * e + 3] = q.w;
                }
                // ---- unit level: scipy's six horizontal taps x - 2 .. x + 3 (same fma order as pyramid_unit_kernel / unit_taps6:
                // the sixth, 2^-53, carries a NaN / inf pixel to the outputs three to its left and above), then the vertical window
                if (has_unit) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float h = args.wx[0] * t[k][0];
                    h = __builtin_fmaf(args.wx[1], t[k][1], h);
                    h = __builtin_fmaf(args.wx[2], t[k][2], h);
                    h = __builtin_fmaf(args.wx[3], t[k][3], h);
                    h = __builtin_fmaf(args.wx[4], t[k][4], h);
                    h = __builtin_fmaf(args.wx[5], t[k][5], h);
#pragma unroll
                    for (int j = 0; j < 5; ++j) hw[j][k] = hw[j + 1][k];
                    hw[5][k] = h;
                }
                }
                const int p = seg_y0 + s - 7;                   // level-0 row that completes with source row y = p + 3
                if (has_unit && p >= seg_y0 && p < seg_y0 + seg_h) {        // wave-uniform (rows above are warm-up)
                    float v0 = args.wx[0] * hw[0][0], v1 = args.wx[0] * hw[0][1];
#pragma unroll
                    for (int j = 1; j < 6; ++j) {
                        v0 = __builtin_fmaf(args.wx[j], hw[j][0], v0);
                        v1 = __builtin_fmaf(args.wx[j], hw[j][1], v1);
                    }
                    const bool prow = p < tab.eff_h;
                    v0 = (prow && eff0) ? v0 : 0.0f;            // canvas beyond the zoomed crop
                    v1 = (prow && eff1) ? v1 : 0.0f;
                    float* __restrict__ po = pyr + base_f + (long long)p * tab.out_w * 3;
                    if (out0) po[0] = v0;
                    if (out1) po[64] = v1;
                }
                // ---- the other levels: the window of the last 6 source rows, and a row of level g when the record says so
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    hist[j][0] = hist[j + 1][0];
                    hist[j][1] = hist[j + 1][1];
                }
                hist[5][0] = t[0][2];                           // the lane's own floats (horizontal tap d = 0)
                hist[5][1] = t[1][2];
                const int anchor = seg_y0 + s - 7;              // anchor row of a row completing now: stored by the segment that owns it
                if (anchor >= seg_y0 && anchor < seg_y0 + seg_h) {   // wave-uniform
                    walk_static_for<0, G>([&](auto gcst) {
                        constexpr int g = decltype(gcst)::value;
                        const int meta = __builtin_amdgcn_readfirstlane(meta_v[g]);
                        if (!(meta & 1)) return;                // wave-uniform: no row of level g completes here
                        const int oy = meta >> 8;
                        const int jj = min(gj, w3_rec_cap(PX, g) - 1);
                        const int4* __restrict__ rc = reinterpret_cast<const int4*>(my_rec + (w3_rec_base(PX, g) + jj) * 8);
                        const int4 ra = rc[0], rb = rc[1];
                        const float* __restrict__ wv = reinterpret_cast<const float*>(prow + G + 6 * g);   // 6 vertical weights (broadcast)
                        float v0 = __builtin_fmaf(wv[0], hist[0][0], 0.0f), v1 = __builtin_fmaf(wv[0], hist[0][1], 0.0f);
#pragma unroll
                        for (int j = 1; j < 6; ++j) {
                            v0 = __builtin_fmaf(wv[j], hist[j][0], v0);
                            v1 = __builtin_fmaf(wv[j], hist[j][1], v1);
                        }
                        my_line[lane] = v0;
                        my_line[lane + 64] = v1;
                        __builtin_amdgcn_wave_barrier();
                        const float* tp = my_line + min(ra.x + gc, kW3TileF - 16);   // taps 3 floats apart (clamped: idle lanes)
                        float acc = __int_as_float(ra.y) * tp[0];
                        acc = __builtin_fmaf(__int_as_float(ra.z), tp[3], acc);
                        acc = __builtin_fmaf(__int_as_float(ra.w), tp[6], acc);
                        acc = __builtin_fmaf(__int_as_float(rb.x), tp[9], acc);
                        acc = __builtin_fmaf(__int_as_float(rb.y), tp[12], acc);
                        acc = __builtin_fmaf(__int_as_float(rb.z), tp[15], acc);
                        __builtin_amdgcn_wave_barrier();
                        if (gj < gn[g])
                            pyr[(frame_px0 + wp.px_off[g] + (long long)oy * wp.out_w[g] + gx0[g]) * 3 + lane] = acc;
                    });
                }
            }
        }
        slot = slot == kWalkSlots - 1 ? 0 : slot + 1;
    }
}

}  // namespace silent
