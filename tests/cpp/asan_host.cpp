// ASan/UBSan driver for the pure-host parts: scene builder + flattener over every pose and skin layout,
// plus malformed descriptions, and the launch planner (render_plan.cpp) over a grid of frame configurations.
#include "flatten.h"
#include "kernels.h"
#include "mcrt.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
int mcrt_detail_fail(int code, const char*) { return code; }  // api.cpp's error hook (not linked here)

static int png_checks() {
    int bad = 0;
    const int sizes[][2] = {{1, 1}, {3, 2}, {257, 31}, {16383, 1}, {16384, 1}, {4095, 4}, {4096, 4}, {13107, 5}};
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        std::vector<uint8_t> img(static_cast<size_t>(w) * h * 4);
        uint32_t s = 99;
        for (auto& b : img) { s = s * 1664525u + 1013904223u; b = static_cast<uint8_t>(s >> 24); }
        const size_t need = mcrt_encode_png_rgba8(img.data(), w, h, nullptr, 0);
        std::vector<uint8_t> out(need);  // exactly `need` bytes: any overrun is an ASan error
        if (!need || mcrt_encode_png_rgba8(img.data(), w, h, out.data(), out.size()) != need) ++bad;
        if (need > 8 && mcrt_encode_png_rgba8(img.data(), w, h, out.data(), need - 1) != need) ++bad;  // too small: size only
    }
    // quantiser on awkward values (image_writer.cpp:18-22 semantics: clamp then *255+0.5 then truncate)
    const float inf = std::numeric_limits<float>::infinity();
    const float vals[8] = {-1.0f, 0.0f, 0.5f, 1.0f, 2.0f, inf, -inf, 0.99999994f};
    uint8_t q[8];
    mcrt_quantize_rgba8(vals, q, 2);
    if (q[0] != 0 || q[1] != 0 || q[2] != 128 || q[3] != 255 || q[4] != 255 || q[5] != 255 || q[6] != 0 || q[7] != 255) ++bad;
    std::vector<float> f(4 * 6, 0.25f);
    if (mcrt_write_png_f32("/tmp/mcrt_asan_host.png", f.data(), 3, 2) != MCRT_OK) ++bad;
    if (mcrt_write_png_f32("/nonexistent_dir_mcrt/x.png", f.data(), 3, 2) == MCRT_OK) ++bad;
    if (mcrt_write_png_rgba8("/tmp/mcrt_asan_host.png", nullptr, 3, 2) == MCRT_OK) ++bad;
    std::remove("/tmp/mcrt_asan_host.png");
    return bad;
}

// What render_enqueue.cpp's prepare() hands the planner, for a 12-mesh skin scene (72 face entries, 204 alpha words) whose
// tables are staged in LDS, or for a scene read from HBM.
static mcrt::RenderParams plan_params(const mcrt_config& cfg, int first, int step, bool rect, bool in_lds) {
    mcrt::RenderParams p;
    std::memset(&p, 0, sizeof p);
    p.cfg = cfg;
    p.shard = mcrt::make_shard(cfg, first, step);
    if (rect) {  // a renderTile rectangle: one tile row of one tile
        p.rect_x = cfg.width / 3, p.rect_y = cfg.height / 4, p.rect_w = cfg.width - p.rect_x, p.rect_h = (cfg.height - p.rect_y + 1) / 2;
        p.shard.first = 0, p.shard.step = 1, p.shard.tiles_x = 1, p.shard.tiles_y = 1, p.shard.owned_rows = 1;
    }
    p.background = MCRT_BACKGROUND_REFERENCE;
    p.draws_per_sample = (cfg.samples_per_pixel > 1 ? 2 : 0) + (cfg.dof_enabled && cfg.aperture > 1e-6f ? 2 : 0);
    const mcrt::LdsFit fit = in_lds ? mcrt::lds_fit(204, 12, false) : mcrt::LdsFit{0, 0, mcrt::kViewHbm};
    p.scene_in_lds = fit.view != mcrt::kViewHbm, p.lds_alpha_words = fit.alpha_words, p.lds_face_entries = fit.face_entries;
    return p;
}
static size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

static int plan_checks() {
    int bad = 0, combos = 0, split = 0;  // split: frames cut into several batches of more than one row
    auto expect = [&](bool ok, const char* what, const mcrt_config& c, size_t budget) {
        if (ok) return;
        if (++bad <= 20) std::printf("plan: %s (%dx%d tile %d spp %d bounces %d dof %d ao %d budget %zu)\n", what, c.width, c.height, c.tile_size,
                                     c.samples_per_pixel, c.max_bounces, c.dof_enabled, c.ao_enabled, budget);
    };
    const int sizes[][2] = {{1, 1}, {70, 45}, {1920, 1080}};
    const int shards[][2] = {{0, 1}, {1, 3}};
    const size_t budgets[] = {size_t(1) << 20, size_t(64) << 20, size_t(4) << 30, size_t(96) << 30};
    for (const auto& wh : sizes) for (int tile : {1, 7, 32}) for (int spp : {1, 4, 64}) for (int dof = 0; dof < 2; ++dof)
    for (int bounces : {0, 4, 9}) for (int ao = 0; ao < 2; ++ao) for (size_t budget : budgets) for (int shape = 0; shape < 3; ++shape) {
        mcrt_config c;
        std::memset(&c, 0, sizeof c);
        c.width = wh[0], c.height = wh[1], c.tile_size = tile, c.samples_per_pixel = spp, c.max_bounces = bounces;
        c.soft_shadows = 1, c.shadow_samples = 8, c.ao_enabled = ao, c.ao_samples = 8, c.ao_radius = 3.0f, c.ao_intensity = 0.5f;
        c.dof_enabled = dof, c.aperture = 0.5f, c.gradient_bg = 1, c.gradient_scale = 1.0f;
        const bool rect = shape == 2;
        mcrt::RenderParams p = plan_params(c, rect ? 0 : shards[shape][0], rect ? 1 : shards[shape][1], rect, true);
        const mcrt::WorkspaceBytes w = mcrt::plan_workspace(p, budget, nullptr);
        mcrt::choose_grids(p, (combos & 1) != 0, (combos & 2) != 0);
        ++combos;
        if (p.shard.owned_rows <= 0) continue;  // (a shard past the frame's last tile row owns nothing)
        // the index limits as the planner states them: records of a batch in 31 bits, a tile's draws in 32
        const size_t tile_w = rect ? p.rect_w : std::min(tile, c.width), tile_h = rect ? p.rect_h : std::min(tile, c.height);
        const size_t tile_slots = tile_w * tile_h * static_cast<size_t>(spp);
        const size_t recs = p.flat ? static_cast<size_t>(1 + bounces) : 2;
        const bool row_fits = static_cast<size_t>(p.shard.tiles_x) * tile_slots <= 0x7ffffff0ull / recs && tile_slots * p.draws_per_sample <= 0xffff0000ull;
        expect(!row_fits || p.rows_per_batch >= 1, "a tile row that fits the index limits was refused", c, budget);
        expect(p.flat == (bounces <= mcrt::kFlatMaxBounces), "flat / general variant", c, budget);
        expect(static_cast<size_t>(p.lit_lds_offset) == align16(mcrt::scene_tables_lds_bytes(p.lds_face_entries, p.lds_alpha_words)), "lit_lds_offset", c, budget);
        expect(p.ws.tile_slots == tile_slots, "tile_slots", c, budget);
        if (p.rows_per_batch >= 1)
            expect(static_cast<uint64_t>(p.ws.cap) >= static_cast<uint64_t>(p.ws.tile_cap) * p.ws.tile_slots && p.ws.tile_cap >= 1, "cap < tile_cap * tile_slots", c, budget);
        const size_t fields[] = {w.tile_rng, w.tile_draws, w.scol, w.end, w.units, w.unit_hits, w.tile_mask, w.queue_each, w.texel_refs, w.targets, w.cand, w.lit0, w.lit1, w.stack, w.counters, w.hit_rng};
        for (size_t f : fields) expect(f < (size_t(1) << 56), "a workspace size wrapped", c, budget);
        if (p.rows_per_batch > 1) {
            // what grows with a batch's slots and tiles, less the flat pipeline's fixed slack of 256 records per level
            const size_t batch = w.tile_draws + w.scol + w.end + 5 * w.queue_each + w.texel_refs + w.targets + w.cand + w.lit0 + w.lit1 + w.stack;
            const size_t slack = (p.flat ? static_cast<size_t>(mcrt::kBlock) * recs * (5 * 16 + 4) : 0) + 8;
            expect(batch <= budget + slack, "a batch of several rows exceeds the budget", c, budget);
            split += p.rows_per_batch < p.shard.owned_rows;
        }
        expect(p.grid_primary > 0 && p.grid_ao > 0 && p.grid_lit > 0 && p.grid_resolve > 0 && p.stream_waves >= 1 && p.stream_waves <= p.stream_parts, "grids", c, budget);
    }
    // a batch of two frames, one read from HBM: the whole batch takes the HBM variant and lit's area starts at 0 in both
    mcrt_config c;
    std::memset(&c, 0, sizeof c);
    c.width = 70, c.height = 45, c.tile_size = 32, c.samples_per_pixel = 4, c.max_bounces = 4, c.soft_shadows = 1, c.shadow_samples = 8, c.gradient_bg = 1;
    mcrt::RenderParams f[2] = {plan_params(c, 0, 1, false, true), plan_params(c, 0, 1, false, false)};
    for (auto& p : f) mcrt::plan_workspace(p, size_t(4) << 30, nullptr);
    mcrt::BatchPlan plan;
    if (f[0].lit_lds_offset == 0 || f[1].lit_lds_offset != 0 || !mcrt::batch_eligible(f[0]) || !mcrt::batch_eligible(f[1])) { std::printf("plan: batch set-up\n"); ++bad; }
    if (mcrt::plan_batch(f, 2, false, plan) != hipSuccess || plan.view != mcrt::kViewHbm || plan.dyn != 0 || f[0].lit_lds_offset != 0 || f[1].lit_lds_offset != 0 ||
        plan.lit_dyn != static_cast<size_t>(f[0].lit_lds_bytes)) { std::printf("plan: mixed batch\n"); ++bad; }
    // lds_fit at the limits of the staged tables: 64 meshes (384 face entries) and 4096 alpha words (65 536 texels) fit, one more
    // of either does not; the un-posed variants serve a fitting scene without a rotated mesh
    for (uint32_t n : {63u, 64u, 65u}) for (uint32_t words : {4096u, 4097u}) for (int posed = 0; posed < 2; ++posed) {
        const mcrt::LdsFit fit = mcrt::lds_fit(words, n, posed != 0);
        const bool fits = n <= 64 && words <= 4096;
        const int view = !fits ? mcrt::kViewHbm : (posed ? mcrt::kViewLds : mcrt::kViewLdsUnposed);
        if (fit.view != view || fit.face_entries != (fits ? static_cast<int>(n * 6) : 0) || fit.alpha_words != (fits ? static_cast<int>(words) : 0)) {
            std::printf("plan: lds_fit(%u words, %u meshes, posed %d) = view %d, %d entries, %d words\n", words, n, posed, fit.view, fit.face_entries, fit.alpha_words);
            ++bad;
        }
    }
    std::printf("plan driver: %d combinations, %d of them split into batches of several rows\n", combos, split);
    if (split == 0) ++bad;  // the budgets no longer reach the batching: the loop would check nothing of it
    return bad;
}

int main() {
    int bad = png_checks() + plan_checks();
    for (int legacy = 0; legacy < 2; ++legacy) {
        const int w = 64, h = legacy ? 32 : 64;
        std::vector<uint8_t> skin(static_cast<size_t>(w) * h * 4);
        uint32_t s = 12345;
        for (auto& b : skin) { s = s * 1664525u + 1013904223u; b = static_cast<uint8_t>(s >> 24); }
        for (int pose = 0; pose < 7; ++pose) {
            float p[12];
            if (mcrt_builtin_pose(pose, p) != 0) { ++bad; continue; }
            mcrt_scene_desc* d = nullptr;
            if (mcrt_build_skin_scene(skin.data(), w, h, p, &d) != 0 || !d) { ++bad; continue; }
            std::vector<uint8_t> blob; std::string err;
            if (!mcrt::flatten_scene(d, blob, err)) { std::printf("flatten failed: %s\n", err.c_str()); ++bad; }
            // a truncated description must be rejected, not read out of bounds
            mcrt_scene_desc cut = *d;
            cut.n_meshes = d->n_meshes;  // same meshes, texture table cut short
            cut.n_textures = d->n_textures > 1 ? 1 : 0;
            std::vector<uint8_t> blob2; std::string err2;
            if (mcrt::flatten_scene(&cut, blob2, err2) && d->n_textures > 1) { std::printf("accepted a cut texture table\n"); ++bad; }
            mcrt_scene_desc_free(d);
        }
    }
    float p0[12] = {0};
    mcrt_scene_desc* d = nullptr;
    if (mcrt_build_default_scene(p0, &d) != 0) ++bad; else { std::vector<uint8_t> b; std::string e; if (!mcrt::flatten_scene(d, b, e)) ++bad; mcrt_scene_desc_free(d); }
    std::printf("asan driver: %d problem(s)\n", bad);
    return bad != 0;
}
