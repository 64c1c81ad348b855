// Stand-alone driver of the float16-storage RGB entry points' host side (silent_rgb_line_end_h[_dev], silent_rgb_keypoints_h[_dev]) on the
// library's HOST side (pysilent_amd/csrc/build.py, build_host_driver("rgb_h")).  ONE translation unit with silent_unity.hip,
// -DSILENT_HOST_ONLY, under -fsanitize=address,undefined; launches are compiled out, device memory is host memory.
// No argument: every refusal of the four entry points, IN THE ORDER the entry point tests them -- each case breaks one thing and leaves
// everything an earlier test looks at intact -- as lines
//     entry | case | status | silent_last_error
// and, after the refusals, one accepted call per entry point ("status 0").  The float32 twins run on the same broken arguments where
// they refuse too: the line then ends with "| twin: <status> <message>", and this program exits with status 1 unless the twin's message
// is the same text under its own name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifndef SILENT_HOST_ONLY
#error "host-only build: compile with -DSILENT_HOST_ONLY (no GPU is touched)"
#endif
#include "../pysilent_amd/csrc/silent_unity.hip"

struct Args {
    std::vector<float> pyr, value, peak, rgc, rgby, stripe, blur, end;
    std::vector<uint16_t> orient, line;
    std::vector<int64_t> idx, counts;
    std::vector<silent_extent> levels, regions;
    silent_rgb_chain_params p;
    int n_levels, n_frames;
    size_t cap;
    // what a case may replace
    const float* pyr_p;
    const silent_rgb_chain_params* p_p;
    const silent_extent *levels_p, *regions_p;
    uint16_t *orient_p, *line_p;
    float* value_p;
    int64_t *idx_p, *counts_p;
};

static void fresh(Args* a) {
    a->levels = {silent_extent{9, 13}, silent_extent{5, 7}};
    a->regions = {silent_extent{4, 6}, silent_extent{2, 3}};
    a->n_levels = 2;
    a->n_frames = 2;
    const size_t px = (9 * 13 + 5 * 7) * 2;
    a->pyr.assign(px * 3, 1.0f);
    a->orient.assign(px * 3 + 1, 0);
    a->line.assign(px * 3 + 1, 0);
    a->value.assign(px, 0.0f);
    a->peak.assign(px, 0.0f);
    a->cap = 16;
    a->idx.assign(2 * a->cap * 4, 0);
    a->counts.assign(2, 0);
    a->rgc.assign(81, 0.0f);
    a->rgby.assign(81, 0.25f);
    a->stripe.assign(81, 0.125f);
    a->blur.assign(441, 0.5f);          // channel-uniform
    a->end.assign(81, 0.0625f);
    for (int t = 0; t < 9; ++t)
        for (int c = 0; c < 3; ++c) a->rgc[(t * 3 + c) * 3 + c] = 0.5f;
    a->p = silent_rgb_chain_params{a->rgc.data(), a->rgby.data(), a->stripe.data(), a->blur.data(), a->end.data(), 1.0f, 0.1f, SILENT_FLAT_IEEE, 255.0f, 2};
    a->pyr_p = a->pyr.data();
    a->p_p = &a->p;
    a->levels_p = a->levels.data();
    a->regions_p = a->regions.data();
    a->orient_p = a->orient.data();
    a->line_p = a->line.data();
    a->value_p = a->value.data();
    a->idx_p = a->idx.data();
    a->counts_p = a->counts.data();
}

static int failures = 0;

// the message of the float32 twin must be the float16 entry point's with the name replaced
static void compare_twin(const std::string& entry, const std::string& twin, int rc, const std::string& msg, int trc, const std::string& tmsg) {
    std::string want = msg;
    const size_t at = want.find(entry);
    if (at != std::string::npos) want.replace(at, entry.size(), twin);
    std::printf(" | twin: %d %s", trc, tmsg.c_str());
    if (trc != rc || tmsg != want) {
        std::printf(" | CHECK FAILED: the twin's refusal differs");
        ++failures;
    }
}

enum Entry { LINE_H, LINE_H_DEV, KP_H, KP_H_DEV };
static const char* kEntry[] = {"silent_rgb_line_end_h", "silent_rgb_line_end_h_dev", "silent_rgb_keypoints_h", "silent_rgb_keypoints_h_dev"};

static int call(silent_ctx* ctx, Entry e, const Args& a, bool twin) {
    float* fo = reinterpret_cast<float*>(a.orient_p);   // (the twins are only called on arguments they refuse: nothing is written)
    float* fl = reinterpret_cast<float*>(a.line_p);
    switch (e) {
        case LINE_H:
            return twin ? silent_rgb_line_end(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, fo, fl, a.value_p)
                        : silent_rgb_line_end_h(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, a.orient_p, a.line_p, a.value_p);
        case LINE_H_DEV:
            return twin ? silent_rgb_line_end_dev(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, fo, fl, a.value_p, nullptr)
                        : silent_rgb_line_end_h_dev(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, a.orient_p, a.line_p, a.value_p, nullptr);
        case KP_H:
            return twin ? silent_rgb_keypoints(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, 0.1, a.regions_p, fo, fl, a.value_p, nullptr,
                                               a.idx_p, a.cap, a.counts_p)
                        : silent_rgb_keypoints_h(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, 0.1, a.regions_p, a.orient_p, a.line_p,
                                                 a.value_p, nullptr, a.idx_p, a.cap, a.counts_p);
        default:
            return twin ? silent_rgb_keypoints_dev(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, 0.1, a.regions_p, fo, fl, a.value_p,
                                                   nullptr, a.idx_p, a.cap, a.counts_p, nullptr)
                        : silent_rgb_keypoints_h_dev(ctx, a.pyr_p, a.levels_p, a.n_levels, a.n_frames, a.p_p, 0.1, a.regions_p, a.orient_p, a.line_p,
                                                     a.value_p, nullptr, a.idx_p, a.cap, a.counts_p, nullptr);
    }
}

// twin: the float32 entry point refuses the same arguments with the same words
static void run(Entry e, const char* name, const Args& a, bool twin, int want_rc) {
    silent_ctx* ctx = nullptr;
    if (silent_create(0, &ctx) != SILENT_OK) {
        std::printf("CHECK FAILED: silent_create\n");
        ++failures;
        return;
    }
    const int rc = call(ctx, e, a, false);
    const std::string msg = rc ? silent_last_error(ctx) : "";
    std::printf("%s | %s | %d | %s", kEntry[e], name, rc, msg.c_str());
    if (rc != want_rc) {
        std::printf(" | CHECK FAILED: status %d expected", want_rc);
        ++failures;
    }
    if (twin) {
        std::string entry = kEntry[e], tw = entry;
        const bool dev = entry.size() > 4 && entry.compare(entry.size() - 4, 4, "_dev") == 0;
        if (dev) entry.resize(entry.size() - 4);      // (messages carry the name without _dev)
        tw = entry.substr(0, entry.size() - 2);
        const int trc = call(ctx, e, a, true);
        compare_twin(entry, tw, rc, msg, trc, trc ? silent_last_error(ctx) : "");
    }
    std::printf("\n");
    silent_destroy(ctx);
}

int main() {
    const Entry all[] = {LINE_H, LINE_H_DEV, KP_H, KP_H_DEV};
    for (Entry e : all) {
        const bool kp = e == KP_H || e == KP_H_DEV, host = e == LINE_H || e == KP_H;
        Args a;
        // the order of silent_rgb_line_end / silent_rgb_keypoints: NULL pointers, kernel pointers, outputs, pad, levels, extents ...
        fresh(&a); a.pyr_p = nullptr; run(e, "null_pyr", a, true, SILENT_E_INVALID);
        fresh(&a); a.p_p = nullptr; run(e, "null_params", a, true, SILENT_E_INVALID);
        if (kp) {
            fresh(&a); a.regions_p = nullptr; run(e, "null_regions", a, true, SILENT_E_INVALID);
            // line_end_out is required in BOTH forms (the float32 host form accepts NULL: no twin)
            fresh(&a); a.line_p = nullptr; run(e, "null_line_end", a, !host, SILENT_E_INVALID);
            fresh(&a); a.counts_p = nullptr; run(e, "null_counts", a, true, SILENT_E_INVALID);
            fresh(&a); a.idx_p = nullptr; run(e, "null_idx_with_cap", a, true, SILENT_E_INVALID);
        }
        fresh(&a); a.n_levels = 0; run(e, "no_levels", a, true, SILENT_E_INVALID);
        fresh(&a); a.n_frames = 0; run(e, "no_frames", a, true, SILENT_E_INVALID);
        fresh(&a); a.levels[1].w = 0; run(e, "bad_extent", a, true, SILENT_E_INVALID);
        fresh(&a); a.p.blur = nullptr; run(e, "null_kernel", a, true, SILENT_E_INVALID);
        if (!kp) {
            fresh(&a); a.orient_p = nullptr; a.line_p = nullptr; a.value_p = nullptr; run(e, "all_outputs_null", a, true, SILENT_E_INVALID);
        }
        fresh(&a); a.p.pad = -1; run(e, "negative_pad", a, true, SILENT_E_INVALID);
        // ... then the two refusals of their own: the stage-per-launch route and a level beyond the pair kernel's addressing
        fresh(&a); a.blur[5] = 0.75f; run(e, "blur_not_channel_uniform", a, false, SILENT_E_UNSUPPORTED);
        if (!host) {   // (the _dev forms: alignment is the caller's; the host forms stage into aligned memory)
            fresh(&a); a.orient_p = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(a.orient.data()) + 1);
            run(e, "odd_orient_address", a, false, SILENT_E_INVALID);
            // 30000 x 30000 x 12 bytes: beyond 2^30 bytes per map; nothing is touched before the refusal
            fresh(&a); a.n_levels = 1; a.n_frames = 1; a.levels[0] = silent_extent{30000, 30000}; run(e, "level_too_large", a, false, SILENT_E_UNSUPPORTED);
        }
        fresh(&a); a.p.flat_policy = 7; run(e, "bad_flat_policy", a, true, SILENT_E_INVALID);
        if (kp) {
            fresh(&a); a.regions[0].h = 0; run(e, "bad_region", a, true, SILENT_E_INVALID);
        }
        fresh(&a); run(e, "accepted", a, false, SILENT_OK);
    }
    if (failures) std::printf("CHECK FAILED: %d\n", failures);
    return failures ? 1 : 0;
}
