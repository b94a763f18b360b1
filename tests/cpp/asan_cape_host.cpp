// ASan/UBSan driver for the host paths of capes: the scene builder with and without a cape (every skin kind, every pose, the
// angles at the edges of their range, capes that are dropped), the cape <-> texel maps at the edges of their ranges and
// capacities, the refusals, and — as the view entries do per caped handle — the caped white figure flattened to its view table.
#include "flatten.h"
#include "mcrt.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using mcrt::flatten_scene;
using mcrt::flatten_view_table;
int mcrt_detail_fail(int code, const char*) { return code; }  // api.cpp's error hook (not linked here)
extern "C" mcrt_scene_desc* mcrt_detail_white_figure_cape(int skin_height, int model, const float pose[12], float cape_angle, int cape_alpha);  // scene_builder.cpp

static std::vector<uint8_t> lcg_image(int h, uint32_t s, int alpha) {  // exactly 64 x h: a read of row h is an ASan error
    std::vector<uint8_t> img(static_cast<size_t>(64) * h * 4);
    for (size_t i = 0; i < img.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        img[i] = i % 4 == 3 ? static_cast<uint8_t>(alpha) : static_cast<uint8_t>(s >> 24);
    }
    return img;
}

static int builder_checks() {
    int bad = 0;
    const struct { int height, model, meshes; } kinds[3] = {{64, MCRT_SKIN_CLASSIC, 12}, {32, MCRT_SKIN_CLASSIC, 7}, {64, MCRT_SKIN_SLIM, 12}};
    const std::vector<uint8_t> cape = lcg_image(32, 5u, 255), clear = lcg_image(32, 5u, 0);
    std::vector<uint8_t> corner = clear;  // opaque only where the unwrap does not read: (0,0), (21,0), (22,3), (5,17)
    for (int p : {0, 21, 3 * 64 + 22, 17 * 64 + 5}) corner[4 * static_cast<size_t>(p) + 3] = 255;
    std::vector<uint8_t> one = clear;  // a single opaque texel: the last one the unwrap reads, (21, 16)
    one[4 * static_cast<size_t>(16 * 64 + 21) + 3] = 255;
    for (const auto& k : kinds)
        for (int pose_index = 0; pose_index < 7; pose_index += 3)
            for (float angle : {0.0f, 0.005f, 10.0f, 90.0f}) {
                float pose[12];
                if (mcrt_builtin_pose(pose_index, pose) != MCRT_OK) ++bad;
                const std::vector<uint8_t> skin = lcg_image(k.height, 7u + pose_index, 255);
                const struct { const uint8_t* image; int extra; } capes[5] = {{nullptr, 0}, {cape.data(), 1}, {clear.data(), 0}, {corner.data(), 0}, {one.data(), 1}};
                std::vector<uint8_t> plain;
                for (const auto& c : capes) {
                    mcrt_scene_desc* d = nullptr;
                    if (mcrt_build_skin_scene_cape(skin.data(), 64, k.height, k.model, pose, c.image, angle, &d) != MCRT_OK || !d) {
                        ++bad;
                        continue;
                    }
                    if (d->n_meshes != k.meshes + c.extra || d->n_textures != 6 * d->n_meshes) ++bad;
                    if (c.extra) {
                        const mcrt_mesh& m = d->meshes[d->n_meshes - 1];
                        if (m.n_triangles != 12 || m.is_outer_layer || (m.has_rotation != 0) != (angle > 0.01f) || (m.has_rotation && m.rot_x != angle)) ++bad;
                        const mcrt_texture* t = d->textures + 6 * (d->n_meshes - 1);
                        const int w[6] = {10, 10, 1, 1, 10, 10}, h[6] = {16, 16, 16, 16, 1, 1};
                        for (int f = 0; f < 6; ++f)
                            if (t[f].width != w[f] || t[f].height != h[f] || t[f].n_pixels != w[f] * h[f]) ++bad;
                    }
                    std::vector<uint8_t> blob, table;
                    std::string err;
                    if (!flatten_scene(d, blob, err) || !flatten_view_table(d, table, err) || table.size() > blob.size()) ++bad;
                    if (!c.image) plain = blob;
                    if (!c.extra && blob != plain) ++bad;  // a dropped cape: the capeless blob
                    mcrt_scene_desc_free(d);
                }
            }
    return bad;
}

static int refusal_checks() {  // refused calls leave *out alone and allocate nothing
    int bad = 0;
    const std::vector<uint8_t> skin = lcg_image(64, 3u, 255), legacy = lcg_image(32, 3u, 255), cape = lcg_image(32, 5u, 255);
    mcrt_scene_desc* d = nullptr;
    for (float angle : {-0.001f, 90.001f, NAN, INFINITY, -INFINITY})
        if (mcrt_build_skin_scene_cape(skin.data(), 64, 64, MCRT_SKIN_CLASSIC, nullptr, cape.data(), angle, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_cape(nullptr, 64, 64, MCRT_SKIN_CLASSIC, nullptr, cape.data(), 10.0f, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_cape(skin.data(), 64, 64, MCRT_SKIN_CLASSIC, nullptr, cape.data(), 10.0f, nullptr) != MCRT_ERR_INVALID) ++bad;
    if (mcrt_build_skin_scene_cape(skin.data(), 64, 48, MCRT_SKIN_CLASSIC, nullptr, cape.data(), 10.0f, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_cape(legacy.data(), 64, 32, MCRT_SKIN_SLIM, nullptr, cape.data(), 10.0f, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_cape(skin.data(), 64, 64, 2, nullptr, nullptr, 10.0f, &d) != MCRT_ERR_INVALID || d) ++bad;
    if (mcrt_build_skin_scene_cape(skin.data(), 64, 64, MCRT_SKIN_CLASSIC, nullptr, nullptr, NAN, &d) != MCRT_OK || !d) ++bad;  // no cape: the angle is not read
    mcrt_scene_desc_free(d);
    return bad;
}

static int map_checks() {
    int bad = 0;
    for (int capacity : {0, 1, 371, 372, 400}) {  // exactly `capacity` entries: any overrun is an ASan error
        std::vector<int32_t> out(static_cast<size_t>(capacity) + 1, -7);
        if (mcrt_cape_pool_map(out.data(), capacity) != 372 || out[static_cast<size_t>(capacity)] != -7) ++bad;
        for (int i = 0; i < capacity; ++i)
            if (i < 372 ? (out[static_cast<size_t>(i)] < 0 || out[static_cast<size_t>(i)] >= 64 * 32) : out[static_cast<size_t>(i)] != -7) ++bad;
    }
    if (mcrt_cape_pool_map(nullptr, 8) == 372) ++bad;
    std::vector<int32_t> map(372);
    mcrt_cape_pool_map(map.data(), 372);
    int n = 0;
    std::vector<int> used(64 * 32, 0);
    for (int face = -1; face <= 6; ++face)
        for (int ty = -1; ty <= 16; ++ty)
            for (int tx = -1; tx <= 10; ++tx) {
                int x = -1, y = -1;
                if (mcrt_cape_texel(face, tx, ty, &x, &y) != MCRT_OK) continue;
                if (x < 0 || x >= 22 || y < 0 || y >= 17 || n >= 372 || map[static_cast<size_t>(n)] != y * 64 + x) ++bad;  // pool order
                else if (used[static_cast<size_t>(y * 64 + x)]++) ++bad;
                ++n;
            }
    if (n != 372 || used[0] || used[21]) ++bad;
    int x = 0;
    if (mcrt_cape_texel(0, 0, 0, nullptr, &x) != MCRT_ERR_INVALID || mcrt_cape_texel(0, 0, 0, &x, nullptr) != MCRT_ERR_INVALID) ++bad;
    return bad;
}

// what skin_view_table_cape (api.cpp) does for each caped handle of a view batch, and what mcrt_scene_create_skin_cape flattens
static int view_table_checks() {
    int bad = 0;
    const int kinds[3][3] = {{64, MCRT_SKIN_CLASSIC, 2688}, {32, MCRT_SKIN_CLASSIC, 1728}, {64, MCRT_SKIN_SLIM, 2688}};
    for (int round = 0; round < 3; ++round)  // mixed order: the figures and the two capes are parsed once and shared
        for (const auto& k : kinds)
            for (float angle : {0.0f, 10.0f, 90.0f})
                for (int alpha : {255, 0}) {
                    float pose[12];
                    mcrt_builtin_pose(3 * round, pose);
                    mcrt_scene_desc* d = mcrt_detail_white_figure_cape(k[0], k[1], round == 1 ? nullptr : pose, angle, alpha);
                    std::vector<uint8_t> table, blob;
                    std::string err;
                    if (!d || !flatten_view_table(d, table, err) || table.size() != static_cast<size_t>(k[2])) ++bad;
                    if (d && (!flatten_scene(d, blob, err) || blob.size() <= table.size() + 372 * 16 + 24 * 4)) ++bad;  // the transparent cape is kept too
                    mcrt_scene_desc_free(d);
                }
    return bad;
}

int main() {
    const int bad = builder_checks() + refusal_checks() + map_checks() + view_table_checks();
    std::printf("asan cape driver: %d problem(s)\n", bad);
    return bad ? 1 : 0;
}
