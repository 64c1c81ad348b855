// silent_pyramid_plan: the host object behind silent_pyramid_plan_create.  silent_plan_build.h builds its tables on the host (tap and region
// tables, the stream path's row programs and column records, the walk plans: no HIP call), silent_pyramid_api.hip validates, uploads them and
// wires the pointers; the gray pass of silent_gray_api.hip reads its unit levels and stream tables.  tests/golden/plan_tables.txt pins them.
#pragma once

#include "silent_internal.h"
#include "silent_gray.h"
#include "silent_pyramid.h"
#include "silent_walk_rgb.h"

struct silent_pyramid_plan {
    silent_ctx* ctx = nullptr;
    silent::PyrTab tab{};
    std::vector<silent_extent> extents;
    void* tables = nullptr;
    float unit_w[6] = {0, 0, 0, 0, 0, 0};  // scipy's six taps of a unit-zoom level ([1,26,66,26,1]/120 and 2^-53, as float32)
    // SILENT_PLAN_ACCUM_F64 (silent_pyramid_plan_create_ex): the F64 kernels, float64 copies of every weight they read -- tab64's
    // tap tables, unit_w64, and the stream path's row programs and column records are then built with float64 weights
    unsigned flags = 0;
    bool f64 = false;
    void* tables64 = nullptr;
    silent::PyrTab64 tab64{};            // tab + xw64 / yw64 (F64 plans)
    double unit_w64[6] = {0, 0, 0, 0, 0, 0};
    // single-read "stream" path (gray_stream_kernel): row programs + column records, when the plan is eligible
    bool stream_ok = false;
    void* stream_tables = nullptr;
    silent::StreamTab stream{};
    int stream_unit_level = -1;
    int stream_layout = 0;               // slot layout of the row programs (stream_slots, silent_gray.h): 1 = dense ladders, 7-level kernels
    // walk plans of pyramid_walk3_kernel (silent_walk_rgb.h; 3 channels): a classic pyramid is ONE plan (unit level + every
    // other level on the same crop), a crop layout like the reference's one plan per level; row programs (completion records)
    // + column records per wave tile live in walk_tables
    bool walk_pyr_ok = false;
    int walk_px = 36;                    // pixels per consumer wave: 36; 32 / 28 / 24 for zoom steps below 1.875 / 1.6 / 1.4
    int walk_G = 4;                      // general levels the kernel is instantiated for (4 or 7)
    void* walk_tables = nullptr;
    silent::Walk3Args walk{};                    // everything but the per-launch decomposition (strips / segments / block0)
    silent::BorderTab walk_border{};             // union plans: the inner levels' border outputs (pyramid_border_kernel); n = 0: none

    silent_pyramid_plan() = default;
    silent_pyramid_plan(const silent_pyramid_plan&) = delete;
    silent_pyramid_plan& operator=(const silent_pyramid_plan&) = delete;
    ~silent_pyramid_plan() {                     // the plan owns its four device allocations
        DeviceGuard guard(ctx ? ctx->device : 0);
        for (void* t : {tables, tables64, stream_tables, walk_tables})
            if (t) (void)hipFree(t);
    }
};

// ------------------------------------------------------------------------------------------ shared by the entry points
// `who` of an entry-point family on a frame type: silent_pyramid_u8x3, silent_gray_pass_h, ...  (float16 storage has a name of its own
// for float frames only: the *_u8 / *_u8x3 forms take it as an argument)
enum { kPyramid, kGrayPass, kGrayPassH, kGrayKeypoints };
template <typename FT>
const char* entry_name(int family) {
    static const std::string sfx = silent::kFrameSuffix<FT>;
    static const std::string names[4] = {"silent_pyramid" + sfx, "silent_gray_pass" + sfx, "silent_gray_pass" + (silent::kFrameNarrow<FT> ? sfx : "_h"),
                                         "silent_gray_keypoints" + sfx};
    return names[family].c_str();
}
inline const silent::FrameRgb8* rgb8(const uint8_t* frames) { return reinterpret_cast<const silent::FrameRgb8*>(frames); }

// ------------------------------------------------------------------------------------------ strided views (the *_view entry points)
// The two strided frame kinds travel through the host templates as `const FT*` like the packed kinds: a pointer to the HOST struct
// (strides + the data pointer); kernel_frames turns it into the kernel's argument, the struct by value.
using View8 = silent::FrameStrided<unsigned char>;
using View8x3 = silent::FrameStrided<silent::FrameRgb8>;
using View16 = silent::FrameStrided<unsigned short>;   // (the *_view16 entry points, silent_frame_view16)
using ViewRgb = silent::FrameStridedRgb;               // (silent_pyramid_rgb8_view: three channels KEPT, 3-channel plans; View8x3 reduces them)
template <typename FT>
inline auto kernel_frames(const FT* frames) {
    if constexpr (silent::kFrameStrided<FT> || silent::kFrameRgbSrc<FT>) return *frames;
    else return frames;
}
// what a view refuses on its own (silent_hip.h) -- NULL, channels, a stride below its bound, a span of 2^63 bytes or more -- and its
// span in bytes.  (H and W are read from the plan before the shared checks look at its context: any plan has them.)
inline int check_view(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const silent_frame_view* v, int n_frames, size_t* span) {
    if (!plan || !v || !v->data) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (v->channels != 1 && v->channels != 3) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view channels must be 1 or 3");
    typedef unsigned __int128 u128;
    const u128 H = (u128)plan->tab.H, W = (u128)plan->tab.W, ch = (u128)v->channels;
    if (v->pixel_stride < v->channels) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view pixel_stride is below channels");
    const u128 row = (W - 1) * (u128)v->pixel_stride + ch;
    if (v->row_stride <= 0 || (u128)v->row_stride < row)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view row_stride is below (W - 1) * pixel_stride + channels");
    const u128 frame = (H - 1) * (u128)v->row_stride + row;
    if (n_frames > 1 && (v->frame_stride <= 0 || (u128)v->frame_stride < frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view frame_stride is below (H - 1) * row_stride + (W - 1) * pixel_stride + channels");
    const u128 all = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->frame_stride : 0) + frame;
    if (all > (u128)0x7fffffffffffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view spans more than 2^63 bytes");
    if (span) *span = (size_t)all;
    return SILENT_OK;
}
// silent_pyramid_rgb8_view: the same refusals with channels == 3 as the only channel count (the three bytes of a pixel are the three
// channels of a 3-channel plan)
inline int check_rgb_view(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const silent_frame_view* v, int n_frames, size_t* span) {
    if (!plan || !v || !v->data) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (v->channels != 3) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view channels must be 3");
    return check_view(ctx, who, plan, v, n_frames, span);
}
// f(frames) with a checked colour view as the frame kind that reads it: a packed view as the packed bytes (the kernels of
// silent_pyramid_rgb8), any other as ViewRgb
template <class F>
int with_rgb_view(const silent_pyramid_plan* plan, const silent_frame_view* v, int n_frames, F&& f) {
    const long long H = plan->tab.H, W = plan->tab.W;
    if (v->pixel_stride == 3 && v->row_stride == W * 3 && (n_frames <= 1 || v->frame_stride == H * v->row_stride)) return f(v->data);
    const ViewRgb s{v->data, v->pixel_stride, v->row_stride, n_frames > 1 ? v->frame_stride : 0};
    return f(&s);
}
// ------------------------------------------------------------------------------------------ the YUV-family colour sources
// NV12, P010 / P012 / P016, planar / packed 8-bit YUV and 16-bit YUV (silent_pyramid_{nv12,p010,yuv,yuv16}, silent_*_to_rgb;
// silent_hip.h).  A host struct travels as a pointer to the kernels' frame kind like a view and is the kernels' argument by value.
// Source<S>: the ONE description of a source struct S -- its entry points, the noun of its messages, its element type; the two PAIR
// structs (y, uv) share check_pair / pair_frames, the two TRIPLE structs (y, u, v) check_triple / with_yuv / yuv_stage, each written
// once over the element size.  A fifth source adds a Source<S> and, if it is neither a pair nor a triple, a check and a marshaller.
using Nv12 = silent::FrameNv12;
using P010 = silent::FrameP010;
using Yuv = silent::FrameYuv;
using Yuv16 = silent::FrameYuv16;
template <class S>
struct Source;
template <>
struct Source<silent_nv12_frames> {
    typedef uint8_t elem;
    static constexpr bool pair = true;
    static constexpr const char *pyramid = "silent_pyramid_nv12", *to_rgb = "silent_nv12_to_rgb", *noun = "NV12 surfaces", *family = "NV12";
};
template <>
struct Source<silent_p010_frames> {
    typedef uint16_t elem;
    static constexpr bool pair = true;
    static constexpr const char *pyramid = "silent_pyramid_p010", *to_rgb = "silent_p010_to_rgb", *noun = "P010 surfaces", *family = "P010";
};
template <>
struct Source<silent_yuv_frames> {
    typedef uint8_t elem;
    static constexpr bool pair = false;
    static constexpr const char *pyramid = "silent_pyramid_yuv", *to_rgb = "silent_yuv_to_rgb", *noun = "YUV frames";
};
template <>
struct Source<silent_yuv16_frames> {
    typedef uint16_t elem;
    static constexpr bool pair = false;
    static constexpr const char *pyramid = "silent_pyramid_yuv16", *to_rgb = "silent_yuv16_to_rgb", *noun = "16-bit YUV frames";
};
// What a pair struct refuses on its own for frames of H x W, in the header's order -- NULL, odd extents, a stride below its bound (a
// row holds E * W bytes, E the element size), a span of 2^63 bytes or more, a non-finite coefficient; then what uint16 elements add:
// an odd plane address, an odd stride, a shift outside 0 .. 6 -- and the two spans in bytes.
template <class S>
inline int check_pair(silent_ctx* ctx, const char* who, bool has_plan, long long H, long long W, const S* v, int n_frames, size_t* y_span,
                      size_t* uv_span) {
    constexpr bool wide = sizeof(typename Source<S>::elem) == 2;
    auto bad = [&](const std::string& what) { return fail(ctx, SILENT_E_INVALID, std::string(who) + ": " + what); };
    const std::string row = wide ? "2 * W" : "W";
    if (!has_plan || !v || !v->y || !v->uv) return bad("NULL pointer");
    if (H < 2 || W < 2 || (H & 1) || (W & 1)) return bad(std::string(Source<S>::family) + " frames need even H and W (4:2:0 chroma)");
    typedef unsigned __int128 u128;
    const long long rb = (wide ? 2 : 1) * W;
    if (v->y_row_stride < rb) return bad("y_row_stride is below " + row);
    if (v->uv_row_stride < rb) return bad("uv_row_stride is below " + row);
    const u128 yf = (u128)(H - 1) * (u128)v->y_row_stride + (u128)rb, cf = (u128)(H / 2 - 1) * (u128)v->uv_row_stride + (u128)rb;
    if (n_frames > 1 && (v->y_frame_stride <= 0 || (u128)v->y_frame_stride < yf)) return bad("y_frame_stride is below (H - 1) * y_row_stride + " + row);
    if (n_frames > 1 && (v->uv_frame_stride <= 0 || (u128)v->uv_frame_stride < cf))
        return bad("uv_frame_stride is below (H / 2 - 1) * uv_row_stride + " + row);
    const u128 ya = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->y_frame_stride : 0) + yf;
    const u128 ca = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->uv_frame_stride : 0) + cf;
    if (ya > (u128)0x7fffffffffffffffll || ca > (u128)0x7fffffffffffffffll) return bad("a plane spans more than 2^63 bytes");
    bool finite = std::isfinite(v->oy);
    if constexpr (wide) finite = finite && std::isfinite(v->oc);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(v->m[i]);
    if (!finite) return bad(wide ? "m, oy and oc must be finite" : "m and oy must be finite");
    if constexpr (wide) {
        if ((reinterpret_cast<uintptr_t>(v->y) | reinterpret_cast<uintptr_t>(v->uv)) & 1u) return bad("y and uv must be 2-byte aligned (uint16 elements)");
        if (((v->y_row_stride | v->uv_row_stride) & 1) || (n_frames > 1 && ((v->y_frame_stride | v->uv_frame_stride) & 1)))
            return bad("a stride is odd (uint16 elements)");
        if (v->shift < 0 || v->shift > 6) return bad("shift must be 0 .. 6 (16 - depth)");
    }
    if (y_span) *y_span = (size_t)ya;
    if (uv_span) *uv_span = (size_t)ca;
    return SILENT_OK;
}
// the kernels' argument for a checked pair struct (the planes at y / uv: those of the struct, or their staged copies)
template <class K, class S, class E>
inline K pair_frames(const S* v, const E* y, const E* uv, int n_frames) {
    K s;
    s.y = y;
    s.uv = uv;
    s.y_row_stride = v->y_row_stride;
    s.uv_row_stride = v->uv_row_stride;
    s.y_frame_stride = n_frames > 1 ? v->y_frame_stride : 0;
    s.uv_frame_stride = n_frames > 1 ? v->uv_frame_stride : 0;
    for (int i = 0; i < 9; ++i) s.m[i] = v->m[i];
    s.oy = v->oy;
    if constexpr (sizeof(E) == 2) {
        s.oc = v->oc;
        s.shift = v->shift;
    }
    return s;
}
inline Nv12 nv12_frames(const silent_nv12_frames* v, const uint8_t* y, const uint8_t* uv, int n_frames) { return pair_frames<Nv12>(v, y, uv, n_frames); }
inline P010 p010_frames(const silent_p010_frames* v, const uint16_t* y, const uint16_t* uv, int n_frames) { return pair_frames<P010>(v, y, uv, n_frames); }
// What a triple struct refuses on its own for frames of H x W, in the header's order (a row or plane ends E bytes behind its last
// element's offset, E the element size); then what uint16 elements add, in check_pair's order -- m / oy / oc finite, 2-byte aligned
// planes, even strides -- and the position of the code (depth, shift).  The spans of the luma plane and of a chroma plane (u and v
// share it) in bytes.
template <class S>
inline int check_triple(silent_ctx* ctx, const char* who, bool has_plan, long long H, long long W, const S* v, int n_frames, size_t* y_span,
                        size_t* c_span) {
    constexpr bool wide = sizeof(typename Source<S>::elem) == 2;
    constexpr int E = wide ? 2 : 1;
    auto bad = [&](const std::string& what) { return fail(ctx, SILENT_E_INVALID, std::string(who) + ": " + what); };
    const std::string e = wide ? "2" : "1";
    if (!has_plan || !v || !v->y || !v->u || !v->v) return bad("NULL pointer");
    const int sx = v->chroma_shift_x, sy = v->chroma_shift_y;
    if ((sx != 0 && sx != 1) || (sy != 0 && sy != 1)) return bad("a chroma shift must be 0 or 1");
    if (H < 1 || W < 1 || (sy && (H & 1)) || (sx && (W & 1)))
        return bad("a subsampled axis needs an even extent (H for chroma_shift_y = 1, W for chroma_shift_x = 1)");
    if (v->y_pixel_stride < E || v->c_pixel_stride < E) return bad("a pixel stride is below " + e);
    typedef unsigned __int128 u128;
    const long long ch = H >> sy, cw = W >> sx;
    const u128 yrow = (u128)(W - 1) * (u128)v->y_pixel_stride + E, crow = (u128)(cw - 1) * (u128)v->c_pixel_stride + E;
    if (v->y_row_stride <= 0 || (u128)v->y_row_stride < yrow) return bad("y_row_stride is below (W - 1) * y_pixel_stride + " + e);
    if (v->c_row_stride <= 0 || (u128)v->c_row_stride < crow) return bad("c_row_stride is below ((W >> sx) - 1) * c_pixel_stride + " + e);
    const u128 yf = (u128)(H - 1) * (u128)v->y_row_stride + yrow, cf = (u128)(ch - 1) * (u128)v->c_row_stride + crow;
    if (n_frames > 1 && (v->y_frame_stride <= 0 || (u128)v->y_frame_stride < yf)) return bad("y_frame_stride is below the luma plane's extent");
    if (n_frames > 1 && (v->c_frame_stride <= 0 || (u128)v->c_frame_stride < cf)) return bad("c_frame_stride is below a chroma plane's extent");
    const u128 ya = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->y_frame_stride : 0) + yf;
    const u128 ca = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->c_frame_stride : 0) + cf;
    if (ya > (u128)0x7fffffffffffffffll || ca > (u128)0x7fffffffffffffffll) return bad("a plane spans more than 2^63 bytes");
    bool finite = std::isfinite(v->oy);
    if constexpr (wide) finite = finite && std::isfinite(v->oc);
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(v->m[i]);
    if (!finite) return bad(wide ? "m, oy and oc must be finite" : "m and oy must be finite");
    if constexpr (wide) {
        if ((reinterpret_cast<uintptr_t>(v->y) | reinterpret_cast<uintptr_t>(v->u) | reinterpret_cast<uintptr_t>(v->v)) & 1u)
            return bad("y, u and v must be 2-byte aligned (uint16 elements)");
        if (((v->y_pixel_stride | v->c_pixel_stride | v->y_row_stride | v->c_row_stride) & 1) || (n_frames > 1 && ((v->y_frame_stride | v->c_frame_stride) & 1)))
            return bad("a stride is odd (uint16 elements)");
        if (v->depth < 8 || v->depth > 16) return bad("depth must be 8 .. 16");
        if (v->shift < 0 || v->shift + v->depth > 16) return bad("shift must be 0 .. 16 - depth");
    }
    if (y_span) *y_span = (size_t)ya;
    if (c_span) *c_span = (size_t)ca;
    return SILENT_OK;
}
template <class S>
inline int check_source(silent_ctx* ctx, const char* who, bool has_plan, long long H, long long W, const S* v, int n_frames, size_t* y_span,
                        size_t* c_span) {
    if constexpr (Source<S>::pair) return check_pair(ctx, who, has_plan, H, W, v, n_frames, y_span, c_span);
    else return check_triple(ctx, who, has_plan, H, W, v, n_frames, y_span, c_span);
}
// f(frames) with a checked triple struct (the planes at y / u / v: those of the struct, or their staged copies) as the frame kind that
// reads it: a struct that IS NV12 as Nv12, one that IS P010 as P010 (the kernels of silent_pyramid_nv12 / _p010, which read the (U, V)
// of a pixel as one pair; with shift == 16 - depth P010's missing mask changes nothing), any other as Yuv / Yuv16 -- like
// with_rgb_view for a packed view
template <class S, class E, class F>
int with_yuv(const S* v, const E* y, const E* u, const E* vv, int n_frames, F&& f) {
    constexpr bool wide = sizeof(E) == 2;
    bool is_pair = v->y_pixel_stride == (int)sizeof(E) && v->c_pixel_stride == 2 * (int)sizeof(E) && vv == u + 1 && v->chroma_shift_x == 1 && v->chroma_shift_y == 1;
    if constexpr (wide) is_pair = is_pair && v->shift == 16 - v->depth;
    if (is_pair) {
        typename std::conditional<wide, P010, Nv12>::type s;
        s.y = y;
        s.uv = u;
        s.y_row_stride = v->y_row_stride;
        s.uv_row_stride = v->c_row_stride;
        s.y_frame_stride = n_frames > 1 ? v->y_frame_stride : 0;
        s.uv_frame_stride = n_frames > 1 ? v->c_frame_stride : 0;
        for (int i = 0; i < 9; ++i) s.m[i] = v->m[i];
        s.oy = v->oy;
        if constexpr (wide) {
            s.oc = v->oc;
            s.shift = v->shift;
        }
        return f(&s);
    }
    typename std::conditional<wide, Yuv16, Yuv>::type s;
    s.y = y;
    s.u = u;
    s.v = vv;
    s.y_pixel_stride = v->y_pixel_stride;
    s.y_row_stride = v->y_row_stride;
    s.y_frame_stride = n_frames > 1 ? v->y_frame_stride : 0;
    s.c_pixel_stride = v->c_pixel_stride;
    s.c_row_stride = v->c_row_stride;
    s.c_frame_stride = n_frames > 1 ? v->c_frame_stride : 0;
    s.sx = v->chroma_shift_x;
    s.sy = v->chroma_shift_y;
    for (int i = 0; i < 9; ++i) s.m[i] = v->m[i];
    s.oy = v->oy;
    if constexpr (wide) {
        s.oc = v->oc;
        s.shift = v->shift;
        s.mask = (1u << v->depth) - 1u;
    }
    return f(&s);
}
// f(frames) with a checked source struct and its planes p[0 .. 2] (a pair: y, uv) as the kernels' argument
template <class S, class F>
int with_source(const S* v, const typename Source<S>::elem* const* p, int n_frames, F&& f) {
    if constexpr (Source<S>::pair) {
        const auto s = pair_frames<typename std::conditional<sizeof(typename Source<S>::elem) == 2, P010, Nv12>::type>(v, p[0], p[1], n_frames);
        return f(&s);
    } else {
        return with_yuv(v, p[0], p[1], p[2], n_frames, f);
    }
}
// what the host forms stage for a checked struct: the UNION of the three spans -- the intervals sorted by address, those that overlap
// or touch merged -- and for each plane the merged interval it lies in and its offset inside it
struct YuvStage {
    int n;                       // merged intervals, 1 .. 3
    const uint8_t* start[3];
    size_t bytes[3];
    int of[3];                   // plane (y, u, v) -> interval
    size_t delta[3];             // plane -> offset inside its interval
};
// (S: silent_yuv_frames or silent_yuv16_frames -- the planes' addresses and their spans in bytes are all that matters)
template <class S>
inline YuvStage yuv_stage(const S* v, size_t y_span, size_t c_span) {
    const uintptr_t a[3] = {reinterpret_cast<uintptr_t>(v->y), reinterpret_cast<uintptr_t>(v->u), reinterpret_cast<uintptr_t>(v->v)};
    const size_t len[3] = {y_span, c_span, c_span};
    int order[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (a[order[j]] < a[order[i]]) {
                const int t = order[i];
                order[i] = order[j];
                order[j] = t;
            }
    YuvStage st{};
    uintptr_t lo = 0, hi = 0;
    for (int i = 0; i < 3; ++i) {
        const int p = order[i];
        if (st.n == 0 || a[p] > hi) {                    // (a[p] == hi: the intervals touch -- merged)
            lo = a[p];
            hi = a[p] + len[p];
            st.start[st.n++] = reinterpret_cast<const uint8_t*>(lo);
        } else if (a[p] + len[p] > hi) {
            hi = a[p] + len[p];
        }
        st.bytes[st.n - 1] = (size_t)(hi - lo);
        st.of[p] = st.n - 1;
        st.delta[p] = (size_t)(a[p] - lo);
    }
    return st;
}
// ------------------------------------------------------------------------------------------ raw Bayer mosaics
// silent_pyramid_bayer / silent_bayer_to_rgb (silent_hip.h): neither a pair nor a triple -- one byte plane in a strided view, so a check
// and a marshaller of its own.  What the struct refuses on its own for frames of H x W, in the header's order, and its span in bytes.
using Bayer = silent::FrameBayer;
inline int check_bayer(silent_ctx* ctx, const char* who, bool has_plan, long long H, long long W, const silent_bayer_frames* v, int n_frames, size_t* span) {
    auto bad = [&](const std::string& what) { return fail(ctx, SILENT_E_INVALID, std::string(who) + ": " + what); };
    if (!has_plan || !v || !v->data) return bad("NULL pointer");
    if (v->pattern < 0 || v->pattern > 3) return bad("pattern must be 0 .. 3 (rggb, grbg, gbrg, bggr)");
    if (v->order < 0 || v->order > 1) return bad("order must be 0 (bgr) or 1 (rgb)");
    if (H < 2 || W < 2) return bad("Bayer mosaics need H and W of at least 2");
    if (H > 0x7fffffffll || W > 0x7fffffffll) return bad("H and W must fit 31 bits");
    if (v->pixel_stride < 1) return bad("pixel_stride is below 1");
    typedef unsigned __int128 u128;
    const u128 row = (u128)(W - 1) * (u128)v->pixel_stride + 1;
    if (v->row_stride <= 0 || (u128)v->row_stride < row) return bad("row_stride is below (W - 1) * pixel_stride + 1");
    const u128 frame = (u128)(H - 1) * (u128)v->row_stride + row;
    if (n_frames > 1 && (v->frame_stride <= 0 || (u128)v->frame_stride < frame))
        return bad("frame_stride is below (H - 1) * row_stride + (W - 1) * pixel_stride + 1");
    const u128 all = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->frame_stride : 0) + frame;
    if (all > (u128)0x7fffffffffffffffll) return bad("the view spans more than 2^63 bytes");
    if (span) *span = (size_t)all;
    return SILENT_OK;
}
// the kernels' argument for a checked struct (the bytes at `data`: those of the struct, or their staged copy)
inline Bayer bayer_frames(const silent_bayer_frames* v, const uint8_t* data, int n_frames, int H, int W) {
    return Bayer{data, v->pixel_stride, v->row_stride, n_frames > 1 ? v->frame_stride : 0, H, W, v->pattern, v->order};
}
// The same for a silent_frame_view16: one uint16 element per pixel (the bounds of check_view with 2 for `channels`), and 2-byte alignment
// of every address a kernel forms -- an even data address and even strides.
inline int check_view16(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const silent_frame_view16* v, int n_frames, size_t* span) {
    if (!plan || !v || !v->data) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": NULL pointer");
    if (reinterpret_cast<uintptr_t>(v->data) & 1u) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view data is not 2-byte aligned (uint16 frames)");
    typedef unsigned __int128 u128;
    const u128 H = (u128)plan->tab.H, W = (u128)plan->tab.W;
    if (v->pixel_stride < 2) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view pixel_stride is below 2 bytes (uint16 frames)");
    if (v->pixel_stride & 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view pixel_stride is odd (uint16 frames)");
    const u128 row = (W - 1) * (u128)v->pixel_stride + 2;
    if (v->row_stride <= 0 || (u128)v->row_stride < row)
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view row_stride is below (W - 1) * pixel_stride + 2 (uint16 frames)");
    if (v->row_stride & 1) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view row_stride is odd (uint16 frames)");
    const u128 frame = (H - 1) * (u128)v->row_stride + row;
    if (n_frames > 1 && (v->frame_stride <= 0 || (u128)v->frame_stride < frame))
        return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view frame_stride is below (H - 1) * row_stride + (W - 1) * pixel_stride + 2 (uint16 frames)");
    if (n_frames > 1 && (v->frame_stride & 1)) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view frame_stride is odd (uint16 frames)");
    const u128 all = (n_frames > 1 ? (u128)(n_frames - 1) * (u128)v->frame_stride : 0) + frame;
    if (all > (u128)0x7fffffffffffffffll) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": view spans more than 2^63 bytes (uint16 frames)");
    if (span) *span = (size_t)all;
    return SILENT_OK;
}
// a packed uint16 batch must be 2-byte aligned (frames: not NULL -- a NULL pointer is reported by the shared checks)
inline int check_u16_aligned(silent_ctx* ctx, const char* who, const uint16_t* frames) {
    if (reinterpret_cast<uintptr_t>(frames) & 1u) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": uint16 frames must be 2-byte aligned");
    return SILENT_OK;
}
// f(frames) with the view as the frame kind that reads it: a packed view as the packed bytes (the kernels of *_u8 / *_u8x3), any other
// as a strided kind.  (check_view passed.)
template <class F>
int with_view(const silent_pyramid_plan* plan, const silent_frame_view* v, int n_frames, F&& f) {
    const long long H = plan->tab.H, W = plan->tab.W;
    const bool packed = v->pixel_stride == v->channels && v->row_stride == W * v->pixel_stride && (n_frames <= 1 || v->frame_stride == H * v->row_stride);
    if (v->channels == 1) {
        if (packed) return f(v->data);
        const View8 s{v->data, v->pixel_stride, v->row_stride, n_frames > 1 ? v->frame_stride : 0};
        return f(&s);
    }
    if (packed) return f(rgb8(v->data));
    const View8x3 s{v->data, v->pixel_stride, v->row_stride, n_frames > 1 ? v->frame_stride : 0};
    return f(&s);
}
template <class F>
int with_view16(const silent_pyramid_plan* plan, const silent_frame_view16* v, int n_frames, F&& f) {
    const long long H = plan->tab.H, W = plan->tab.W;
    if (v->pixel_stride == 2 && v->row_stride == W * 2 && (n_frames <= 1 || v->frame_stride == H * v->row_stride)) return f(v->data);
    const View16 s{reinterpret_cast<const unsigned char*>(v->data), v->pixel_stride, v->row_stride, n_frames > 1 ? v->frame_stride : 0};
    return f(&s);
}
// (host-pointer forms) what is staged for `frames` -- the packed batch, or the span of a view (its strides passed check_view) -- and
// the `frames` of the _dev form on the staged copy
template <typename FT>
inline const void* frames_host(const FT* frames) {
    if constexpr (silent::kFrameStrided<FT>) return frames ? frames->data : nullptr;
    else return frames;
}
template <typename FT>
inline size_t frames_bytes(const silent_pyramid_plan* plan, const FT* f, int n_frames) {
    if constexpr (silent::kFrameStrided<FT>)
        return (size_t)((n_frames - 1) * f->frame_stride + (plan->tab.H - 1) * f->row_stride + (plan->tab.W - 1) * f->pixel_stride +
                        (long long)sizeof(typename silent::FrameKind<FT>::px));
    else
        return (size_t)plan->tab.H * plan->tab.W * silent::frame_px_bytes<FT>(plan->tab.C) * n_frames;
}
template <typename FT>
struct StagedFrames {
    FT view{};      // (strided kinds: the view on the staged bytes)
    const FT* p;
    StagedFrames(const FT* host, const void* dev) {
        if constexpr (silent::kFrameStrided<FT>) {
            view = *host;
            view.data = static_cast<const unsigned char*>(dev);
            p = &view;
        } else {
            p = static_cast<const FT*>(dev);
        }
    }
};

// the uint8 / uint16 frame kinds / float16 storage exist for single-channel plans with float32 accumulation only (plan: not NULL)
template <typename FT>
inline int check_narrow_frames(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan) {
    const std::string what = silent::kFrame16<FT> ? "uint16 frames" : "uint8 frames";
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": " + what + " are for single-channel plans");
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": " + what + " with a SILENT_PLAN_ACCUM_F64 plan");
    return SILENT_OK;
}
inline int check_half_storage(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan) {
    if (plan->tab.C != 1) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": float16 storage is for single-channel plans");
    if (plan->f64) return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": float16 storage with a SILENT_PLAN_ACCUM_F64 plan");
    return SILENT_OK;
}
inline int check_gray_outputs(silent_ctx* ctx, const char* who, const void* cs_out, const void* end_out, const float* end_bank, int n_orient) {
    if (!cs_out && !end_out) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": both outputs are NULL");
    if (end_out && !end_bank) return fail(ctx, SILENT_E_INVALID, std::string(who) + ": end_bank is NULL");
    if (n_orient != 3 && n_orient != 4 && n_orient != 8)
        return fail(ctx, SILENT_E_UNSUPPORTED, std::string(who) + ": n_orient must be 3, 4 or 8");
    return SILENT_OK;
}

// the weights of the CS and end kernels as a kernel argument (end_bank may be NULL when no end map is written)
inline silent::GrayW gray_weights(const float* cs_kernel, const float* end_bank, int n_orient) {
    silent::GrayW w;
    std::memset(&w, 0, sizeof(w));
    std::memcpy(w.cs, cs_kernel, sizeof(float) * 9);
    if (end_bank) std::memcpy(w.end, end_bank, sizeof(float) * 9 * n_orient);
    return w;
}
// The table of the fused / stream kernels (they take its FusedTab part, the F64 kernels all of it): the frame and the unit taps of the
// plan -- every unit level has the same ([1,26,66,26,1]/120 and the sixth, 2^-53) --, no level yet; fused_add_level appends unit level
// l of the plan, its tiles behind those of the levels before it.
inline silent::FusedTab64 fused_tab(const silent_pyramid_plan* plan) {
    silent::FusedTab64 ft;
    std::memset(&ft, 0, sizeof(ft));
    for (int j = 0; j < 6; ++j) {
        ft.wx[j] = ft.wy[j] = plan->unit_w[j];
        ft.w64[j] = plan->unit_w64[j];
    }
    ft.H = plan->tab.H;
    ft.W = plan->tab.W;
    ft.frame_px = plan->tab.frame_px_out;
    return ft;
}
inline void fused_add_level(silent::FusedTab64& ft, const silent::PyrTab& pt, int l) {
    const silent::PyrLevelDev& d = pt.lv[l];
    silent::FusedLevel& f = ft.lv[ft.n++];
    f.src_y0 = d.src_y0; f.src_x0 = d.src_x0; f.src_h = d.src_h; f.src_w = d.src_w;
    f.zoom_h = d.zoom_h; f.zoom_w = d.zoom_w; f.out_h = d.out_h; f.out_w = d.out_w;
    f.tiles_x = (d.out_w + silent::kFusedTW - 1) / silent::kFusedTW;
    f.tile_start = ft.tiles_per_frame;
    f.px_off = pt.px_off[l];
    ft.tiles_per_frame += f.tiles_x * ((d.out_h + silent::kFusedTH - 1) / silent::kFusedTH);
}

// ------------------------------------------------------------------------------------------ kernel dispatch
// Which instantiations of the gray kernels exist: float16 storage (ST = gray_half) has no keypoint epilogue and no float64 accumulation,
// the uint8 / uint16 frame kinds no float64 accumulation (the entry points refuse those combinations before a launch).
template <bool KP, bool F64, typename ST, typename FT>
constexpr bool kGrayKernel = !(silent::kStoreHalf<ST> && (KP || F64)) && !(silent::kFrameNarrow<FT> && F64);
// f(KP, F64) with the run-time (kp, f64) as std::bool_constant's; a combination without kernels is never instantiated (nor reached)
template <typename ST, typename FT, class F>
void with_gray_mode(bool kp, bool f64, F&& f) {
    auto go = [&](auto KP, auto F64) {
        if constexpr (kGrayKernel<decltype(KP)::value, decltype(F64)::value, ST, FT>) f(KP, F64);
    };
    if (kp && f64) go(std::true_type{}, std::true_type{});
    else if (kp) go(std::true_type{}, std::false_type{});
    else if (f64) go(std::false_type{}, std::true_type{});
    else go(std::false_type{}, std::false_type{});
}
// f(K) with n_orient (3, 4 or 8: checked by the caller) as a std::integral_constant
template <class F>
void with_orient(int n_orient, F&& f) {
    if (n_orient == 3) f(std::integral_constant<int, 3>{});
    else if (n_orient == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}
// f(G, L): the general levels and the slot layout the stream kernels of a plan are instantiated for
template <class F>
void with_stream_layout(const silent_pyramid_plan* plan, F&& f) {
    using std::integral_constant;
    if (plan->stream_layout == 1) f(integral_constant<int, 7>{}, integral_constant<int, 1>{});   // zoom ladders of ratio 1.4 .. e^.5: five rows of the first level in flight
    else if (plan->stream.G <= 4) f(integral_constant<int, 4>{}, integral_constant<int, 0>{});
    else f(integral_constant<int, 7>{}, integral_constant<int, 0>{});
}

// (silent_pyramid_api.hip) FT: the frame element type -- float, or unsigned char / silent::FrameRgb8 (uint8 frames, one channel /
// interleaved colour, its value formed at the load: single-channel plans without SILENT_PLAN_ACCUM_F64; anything else is refused),
// or unsigned short (uint16 frames), or View8 / View8x3 / View16 (the same pixels in a strided view: `frames` then points to the host struct).
// with_unit: also the unit levels (the gray pass produces them itself); with_region: also the general levels
template <typename FT>
int launch_pyramid(silent_ctx* ctx, const char* who, const silent_pyramid_plan* plan, const FT* frames, int n_frames, float* pyr,
                   hipStream_t s, bool with_unit, bool with_region = true);
// (silent_gray_api.hip) silent_gray_pass_dev with the keypoint epilogue (silent_gray.h, GrayKp) in every kernel that writes `end`
template <typename FT>
int gray_pass_kp(silent_ctx* ctx, const silent_pyramid_plan* plan, const FT* frames, int n_frames, const float* cs_kernel,
                 const float* end_bank, int n_orient, float clip_hi, float* pyr, float* cs_out, float* end_out, const silent::GrayKp& kp,
                 hipStream_t s);
// (each is defined in its unit -- gray_pass_kp in silent_gray_pass.h -- and instantiated for the seven frame types: launch_pyramid in
// silent_pyramid_api.hip, gray_pass_kp for float and the uint8 kinds in silent_gray_api.hip, for the uint16 kinds in silent_gray16_api.hip)
#define SILENT_FRAME_TYPES_8(X) X(float) X(unsigned char) X(silent::FrameRgb8) X(View8) X(View8x3)
#define SILENT_FRAME_TYPES_16(X) X(unsigned short) X(View16)
#define SILENT_FRAME_TYPES(X) SILENT_FRAME_TYPES_8(X) SILENT_FRAME_TYPES_16(X)
#define X(FT)                                                                                                                              \
    extern template int launch_pyramid<FT>(silent_ctx*, const char*, const silent_pyramid_plan*, const FT*, int, float*, hipStream_t, bool, bool); \
    extern template int gray_pass_kp<FT>(silent_ctx*, const silent_pyramid_plan*, const FT*, int, const float*, const float*, int, float, float*, \
                                         float*, float*, const silent::GrayKp&, hipStream_t);
SILENT_FRAME_TYPES(X)
#undef X
