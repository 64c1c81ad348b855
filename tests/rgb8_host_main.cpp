// Stand-alone driver of silent_pyramid_rgb8 / silent_pyramid_rgb8_dev (packed interleaved uint8 colour frames for 3-channel plans) on the
// library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb8")).  ONE translation unit with silent_unity.hip,
// -DSILENT_HOST_ONLY, under -fsanitize=address,undefined: kernel launches are compiled out and device memory is host memory, so what
// runs is the argument validation, the plan tables (walk plans of a classic pyramid and of a crop layout) and the host form's staging.
// The frames are a heap block of EXACTLY n * H * W * 3 bytes: a staging size above that reads past it (AddressSanitizer reports it);
// one below it leaves poison in the staging arena, which this program looks at (the arena is host memory here).  No argument: both forms
// + the staging check + the status codes, one "ok" line.  --refusals: "name | case | status | silent_last_error" per (entry point,
// single fault), tests/golden/rgb8_refusals.txt.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

static int failures = 0;

#define EXPECT(call, want)                                                                                   \
    do {                                                                                                     \
        const int rc_ = (call);                                                                              \
        if (rc_ != (want)) {                                                                                 \
            std::printf("line %d: %s -> %d, expected %d (%s)\n", __LINE__, #call, rc_, (int)(want), silent_last_error(ctx)); \
            ++failures;                                                                                      \
        }                                                                                                    \
    } while (0)

struct Args {
    silent_ctx* ctx; const silent_pyramid_plan* plan; const uint8_t* frames; int n; float* pyr;
};
static const char* const kFaultNames[6] = {"plan NULL", "frames NULL", "pyr NULL", "plan of another context", "n_frames 0", "single-channel plan"};

static void refusal_table(const Args& valid, const silent_pyramid_plan* plan_other, const silent_pyramid_plan* plan_gray) {
    for (int dev = 0; dev < 2; ++dev)
        for (int f = 0; f < 6; ++f) {
            Args a = valid;
            switch (f) {
                case 0: a.plan = nullptr; break;
                case 1: a.frames = nullptr; break;
                case 2: a.pyr = nullptr; break;
                case 3: a.plan = plan_other; break;
                case 4: a.n = 0; break;
                case 5: a.plan = plan_gray; break;
            }
            const int rc = dev ? silent_pyramid_rgb8_dev(a.ctx, a.plan, a.frames, a.n, a.pyr, nullptr)
                               : silent_pyramid_rgb8(a.ctx, a.plan, a.frames, a.n, a.pyr);
            std::printf("%s | %s | %d | %s\n", dev ? "silent_pyramid_rgb8_dev" : "silent_pyramid_rgb8", kFaultNames[f], rc,
                        rc == SILENT_OK ? "-" : silent_last_error(a.ctx));
        }
}

int main(int argc, char** argv) {
    const bool refusals = argc > 1 && !std::strcmp(argv[1], "--refusals");
    const int H = 40, W = 57, n = 2;
    silent_ctx* ctx = nullptr;
    silent_ctx* other = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK || silent_create(0, &other) != SILENT_OK) {
        std::printf("silent_create failed\n");
        return 2;
    }
    const silent_pyr_level ladder[3] = {{0, 0, H, W, H, W, H, W}, {0, 0, H, W, 20, 29, 20, 29}, {0, 0, H, W, 10, 14, 10, 14}};
    const silent_pyr_level crops[3] = {{3, 5, 30, 41, 30, 41, 30, 41}, {0, 0, H, W, 20, 29, 22, 31}, {10, 16, 20, 33, 10, 17, 10, 17}};
    silent_pyramid_plan *plan = nullptr, *plan_crop = nullptr, *plan_gray = nullptr, *plan_other = nullptr;
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, ladder, 3, &plan), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 3, crops, 3, &plan_crop), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(ctx, H, W, 1, ladder, 3, &plan_gray), SILENT_OK);
    EXPECT(silent_pyramid_plan_create(other, H, W, 3, ladder, 3, &plan_other), SILENT_OK);
    if (failures) return 1;

    const size_t frame_bytes = (size_t)3 * n * H * W;   // exactly 3 bytes per frame pixel: 13680, no multiple of the arena's 256-byte steps
    uint8_t* frames = (uint8_t*)std::malloc(frame_bytes);
    for (size_t i = 0; i < frame_bytes; ++i) frames[i] = (uint8_t)(i * 37 + 11);

    const silent_pyramid_plan* plans[2] = {plan, plan_crop};
    for (const silent_pyramid_plan* p : plans) {
        const size_t px = (size_t)n * (p == plan ? 40 * 57 + 20 * 29 + 10 * 14 : 30 * 41 + 22 * 31 + 10 * 17);
        std::vector<float> pyr(px * 3);
        if (refusals) {
            if (p == plan) refusal_table(Args{ctx, p, frames, n, pyr.data()}, plan_other, plan_gray);
            continue;
        }
        EXPECT(silent_pyramid_rgb8(ctx, p, frames, n, pyr.data()), SILENT_OK);
        EXPECT(silent_pyramid_rgb8_dev(ctx, p, frames, n, pyr.data(), nullptr), SILENT_OK);
        // ---- the host form stages exactly n * H * W * 3 bytes: the frames are the first argument staged (arena offset 0, the next one
        // starts on the following multiple of 256); the arena is poisoned, the call made again
        const size_t staged_end = (frame_bytes + 255) / 256 * 256;
        if (!ctx->arena.p || ctx->arena.cap < staged_end + pyr.size() * 4) {
            std::printf("the staging arena holds %zu bytes, expected at least %zu\n", (size_t)ctx->arena.cap, staged_end + pyr.size() * 4);
            ++failures;
            continue;
        }
        std::memset(ctx->arena.p, 0xEE, ctx->arena.cap);
        EXPECT(silent_pyramid_rgb8(ctx, p, frames, n, pyr.data()), SILENT_OK);
        const uint8_t* arena = (const uint8_t*)ctx->arena.p;
        if (std::memcmp(arena, frames, frame_bytes) != 0) {
            std::printf("the staged frames differ from the batch within its n * H * W * 3 bytes\n");
            ++failures;
        }
        for (size_t i = frame_bytes; i < staged_end; ++i)
            if (arena[i] != 0xEE) {
                std::printf("byte %zu of the arena was written: more than n * H * W * 3 = %zu bytes were staged\n", i, frame_bytes);
                ++failures;
                break;
            }
        // ---- status codes
        EXPECT(silent_pyramid_rgb8(ctx, nullptr, frames, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8(ctx, p, nullptr, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8(ctx, p, frames, n, nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8(ctx, p, frames, 0, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8(ctx, plan_other, frames, n, pyr.data()), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8(ctx, plan_gray, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
        EXPECT(silent_pyramid_rgb8_dev(ctx, nullptr, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8_dev(ctx, p, nullptr, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8_dev(ctx, p, frames, n, nullptr, nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8_dev(ctx, p, frames, 0, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8_dev(ctx, plan_other, frames, n, pyr.data(), nullptr), SILENT_E_INVALID);
        EXPECT(silent_pyramid_rgb8_dev(ctx, plan_gray, frames, n, pyr.data(), nullptr), SILENT_E_UNSUPPORTED);
        // the order of the shared checks: NULL before the plan's context, the context before n_frames, n_frames before the channels
        EXPECT(silent_pyramid_rgb8(ctx, plan_other, nullptr, 0, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "NULL pointer")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_pyramid_rgb8_dev(ctx, plan_other, frames, 0, pyr.data(), nullptr), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "another context")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        EXPECT(silent_pyramid_rgb8(ctx, plan_gray, frames, 0, pyr.data()), SILENT_E_INVALID);
        if (!std::strstr(silent_last_error(ctx), "n_frames")) { std::printf("order: %s\n", silent_last_error(ctx)); ++failures; }
        // the float32-frame call and the single-channel colour call still take what they took
        std::vector<float> f32(frame_bytes);
        EXPECT(silent_pyramid(ctx, p, f32.data(), n, pyr.data()), SILENT_OK);
        EXPECT(silent_pyramid_u8x3(ctx, p, frames, n, pyr.data()), SILENT_E_UNSUPPORTED);
    }
    if (silent_abi_version() != 5) {
        std::printf("ABI version %d\n", silent_abi_version());
        ++failures;
    }
    std::free(frames);
    for (silent_pyramid_plan* q : {plan, plan_crop, plan_gray, plan_other}) silent_pyramid_plan_destroy(q);
    silent_destroy(other);
    silent_destroy(ctx);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    if (!refusals) std::printf("rgb8 host main ok\n");
    return 0;
}
