// ASan/UBSan driver for the host paths of the slim player model: the model tables of the scene builder (both models, every
// pose, skins that drop outer parts), the skin <-> texel maps at the edges of their ranges and capacities, the detection rule,
// and — as the view entries do per handle — the white figure of every skin kind flattened to its view table.
#include "flatten.h"
#include "mcrt.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using mcrt::flatten_scene;
using mcrt::flatten_view_table;
int mcrt_detail_fail(int code, const char*) { return code; }  // api.cpp's error hook (not linked here)
extern "C" mcrt_scene_desc* mcrt_detail_white_figure(int skin_height, int model, const float pose[12]);  // scene_builder.cpp
extern "C" int mcrt_detail_skin_pool(int skin_height, int model, int32_t* pixel, int32_t* mesh_of, int capacity);

static std::vector<uint8_t> lcg_skin(int h, uint32_t s, int clear_alpha_every) {
    std::vector<uint8_t> img(static_cast<size_t>(64) * h * 4);
    for (size_t i = 0; i < img.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        img[i] = static_cast<uint8_t>(s >> 24);
        if (i % 4 == 3) img[i] = (clear_alpha_every && (i / 4) % clear_alpha_every == 0) ? 0 : 255;
    }
    return img;
}

static int builder_checks() {
    int bad = 0;
    for (int model = MCRT_SKIN_CLASSIC; model <= MCRT_SKIN_SLIM; ++model)
        for (int pose_index = 0; pose_index < 7; ++pose_index)
            for (int clear : {0, 1, 3}) {  // all opaque; all transparent (the outer parts are dropped); every third texel clear
                float pose[12];
                if (mcrt_builtin_pose(pose_index, pose) != MCRT_OK) ++bad;
                const std::vector<uint8_t> img = lcg_skin(64, 7u + pose_index, clear);
                mcrt_scene_desc* d = nullptr;
                if (mcrt_build_skin_scene_model(img.data(), 64, 64, model, pose, &d) != MCRT_OK || !d) {
                    ++bad;
                    continue;
                }
                if (d->n_meshes != (clear == 1 ? 6 : 12) || d->n_textures != 6 * d->n_meshes) ++bad;
                if (clear != 1) {  // the right arm's front and left faces
                    const int want = model == MCRT_SKIN_SLIM ? 3 : 4;
                    if (d->textures[6 * 4 + 1].width != want || d->textures[6 * 4 + 2].width != 4) ++bad;
                }
                std::vector<uint8_t> blob, table;
                std::string err;
                if (!flatten_scene(d, blob, err) || !flatten_view_table(d, table, err)) ++bad;
                if (table.size() > blob.size()) ++bad;
                mcrt_scene_desc_free(d);
            }
    // refused combinations leave *out alone and allocate nothing
    const std::vector<uint8_t> legacy = lcg_skin(32, 3u, 0);
    mcrt_scene_desc* d = nullptr;
    if (mcrt_build_skin_scene_model(legacy.data(), 64, 32, MCRT_SKIN_SLIM, nullptr, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_model(legacy.data(), 64, 32, 2, nullptr, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_model(legacy.data(), 64, 32, MCRT_SKIN_CLASSIC, nullptr, &d) != MCRT_OK || !d) ++bad;
    mcrt_scene_desc_free(d);
    return bad;
}

static int map_checks() {
    int bad = 0;
    const struct { int height, model, count, meshes; } kinds[3] = {{64, MCRT_SKIN_CLASSIC, 3264, 12}, {32, MCRT_SKIN_CLASSIC, 2016, 7}, {64, MCRT_SKIN_SLIM, 3136, 12}};
    for (const auto& k : kinds) {
        for (int capacity : {0, 1, k.count - 1, k.count}) {  // exactly `capacity` entries: any overrun is an ASan error
            std::vector<int32_t> out(static_cast<size_t>(capacity) + 1, -7);
            if (mcrt_skin_pool_map_model(k.height, k.model, out.data(), capacity) != k.count || out[static_cast<size_t>(capacity)] != -7) ++bad;
            std::vector<int32_t> pixel(static_cast<size_t>(capacity) + 1, -7), mesh_of(static_cast<size_t>(capacity) + 1, -7);
            if (mcrt_detail_skin_pool(k.height, k.model, pixel.data(), mesh_of.data(), capacity) != k.count) ++bad;
            if (pixel[static_cast<size_t>(capacity)] != -7 || mesh_of[static_cast<size_t>(capacity)] != -7) ++bad;
        }
        if (mcrt_skin_pool_map_model(k.height, k.model, nullptr, 8) == k.count) ++bad;
        std::vector<int32_t> map(static_cast<size_t>(k.count));
        mcrt_skin_pool_map_model(k.height, k.model, map.data(), k.count);
        int n = 0;
        for (int mesh = -1; mesh <= k.meshes; ++mesh)
            for (int face = -1; face <= 6; ++face)
                for (int ty = -1; ty <= 12; ++ty)
                    for (int tx = -1; tx <= 8; ++tx) {
                        int x = -1, y = -1;
                        const int rc = mcrt_skin_texel_model(k.height, k.model, mesh, face, tx, ty, &x, &y);
                        if (rc != MCRT_OK) continue;
                        if (x < 0 || x >= 64 || y < 0 || y >= k.height) ++bad;
                        ++n;
                    }
        if (n != k.count) ++bad;  // the loops visit the texels of the pool, each once
        for (int32_t p : map)
            if (p < 0 || p >= 64 * k.height) ++bad;
    }
    return bad;
}

static int detection_checks() {
    int bad = 0;
    std::vector<uint8_t> img = lcg_skin(64, 11u, 0);
    if (mcrt_skin_model_of(img.data(), 64, 64) != MCRT_SKIN_CLASSIC) ++bad;
    const int rects[4][4] = {{50, 16, 2, 4}, {54, 20, 2, 12}, {42, 48, 2, 4}, {46, 52, 2, 12}};
    for (const auto& r : rects)
        for (int y = r[1]; y < r[1] + r[3]; ++y)
            for (int x = r[0]; x < r[0] + r[2]; ++x) img[4 * (static_cast<size_t>(y) * 64 + x) + 3] = 0;
    if (mcrt_skin_model_of(img.data(), 64, 64) != MCRT_SKIN_SLIM) ++bad;
    img[4 * (static_cast<size_t>(63) * 64 + 47) + 3] = 1;  // the last pixel the rule reads
    if (mcrt_skin_model_of(img.data(), 64, 64) != MCRT_SKIN_CLASSIC) ++bad;
    const std::vector<uint8_t> legacy(static_cast<size_t>(64) * 32 * 4, 0);  // exactly 64x32: a read of row 32 is an ASan error
    if (mcrt_skin_model_of(legacy.data(), 64, 32) != MCRT_SKIN_CLASSIC) ++bad;
    if (mcrt_skin_model_of(nullptr, 64, 64) != -1 || mcrt_skin_model_of(img.data(), 64, 48) != -1 || mcrt_skin_model_of(img.data(), 63, 64) != -1) ++bad;
    return bad;
}

// what skin_view_table (api.cpp) does for each handle of a view batch: the white figure of the handle's kind at its pose,
// flattened to the prefix, freed
static int view_table_checks() {
    int bad = 0;
    const int kinds[3][3] = {{64, MCRT_SKIN_CLASSIC, 2496}, {32, MCRT_SKIN_CLASSIC, 1536}, {64, MCRT_SKIN_SLIM, 2496}};
    for (int round = 0; round < 3; ++round)  // mixed order: the figures are parsed once per kind and shared
        for (const auto& k : kinds)
            for (int pose_index = 0; pose_index < 7; pose_index += 3) {
                float pose[12];
                mcrt_builtin_pose(pose_index, pose);
                mcrt_scene_desc* d = mcrt_detail_white_figure(k[0], k[1], round == 1 ? nullptr : pose);
                std::vector<uint8_t> table;
                std::string err;
                if (!d || !flatten_view_table(d, table, err) || table.size() != static_cast<size_t>(k[2])) ++bad;
                mcrt_scene_desc_free(d);
            }
    return bad;
}

int main() {
    const int bad = builder_checks() + map_checks() + detection_checks() + view_table_checks();
    std::printf("asan slim driver: %d problem(s)\n", bad);
    return bad ? 1 : 0;
}
