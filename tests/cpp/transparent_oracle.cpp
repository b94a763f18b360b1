// transparent_oracle.cpp — TEST-SIDE checker of MCRT_BACKGROUND_TRANSPARENT (include/mcrt.h).
//
// It compiles the CPU oracle into itself and restates the oracle's render_tile (oracle/mcrt_oracle.cpp, TileRenderer::
// renderTile, tile_renderer.cpp:71-127) with the background mode as a parameter, on the oracle's own camera_ray, lens_ray,
// trace, hit_scene, background and Mt.  REFERENCE mode is the oracle's loop unchanged; TRANSPARENT mode skips the samples
// whose primary ray misses (their draws are still taken) and divides rgb by their count n, alpha by spp.
// Built by tests/transparent_checker.py with the oracle's flags and -fvisibility=hidden: render_tiles is the one export.
#include "../../oracle/mcrt_oracle.cpp"

namespace {

void render_tile_mode(const mcrt_scene_desc& sc, const mcrt_config& cfg, const mcrt_tile& tile, int mode, float* frame,
                      int32_t* hit_counts) {
    float aspect = static_cast<float>(cfg.width) / static_cast<float>(cfg.height);
    int spp = cfg.samples_per_pixel > 1 ? cfg.samples_per_pixel : 1;
    Mt rng(static_cast<uint32_t>(tile.y * cfg.width + tile.x));

    float focusDist = cfg.focus_distance;
    if (focusDist <= 0.0f) focusDist = len3(sub3(ld3(sc.camera_target), ld3(sc.camera_position)));
    ShadeParams pr;

    for (int py = tile.y; py < tile.y + tile.height; ++py) {
        for (int px = tile.x; px < tile.x + tile.width; ++px) {
            float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
            int n = 0;  // samples whose primary ray hits
            for (int s = 0; s < spp; ++s) {
                float jx = (spp == 1) ? 0.5f : rng.uniform();
                float jy = (spp == 1) ? 0.5f : rng.uniform();
                float u = (static_cast<float>(px) + jx) / static_cast<float>(cfg.width);
                float v = (static_cast<float>(py) + jy) / static_cast<float>(cfg.height);
                Ray ray = (cfg.dof_enabled && cfg.aperture > 1e-6f)
                              ? lens_ray(sc, u, v, aspect, cfg.aperture, focusDist, rng)
                              : camera_ray(sc, u, v, aspect);
                F4 c = trace(sc, ray, 0, cfg.max_bounces, pr, &cfg);
                Hit again = hit_scene(sc, ray);
                if (again.hit) {
                    ++n;
                } else {
                    if (mode == MCRT_BACKGROUND_TRANSPARENT) continue;  // a miss adds nothing
                    c = background(sc, u, v, &cfg);
                }
                ar += c.r;
                ag += c.g;
                ab += c.b;
                aa += c.a;
            }
            float inv = 1.0f / static_cast<float>(spp);
            float* dst = frame + 4 * (static_cast<size_t>(py) * cfg.width + px);
            if (mode == MCRT_BACKGROUND_TRANSPARENT) {
                if (n == 0) {
                    dst[0] = dst[1] = dst[2] = dst[3] = 0.0f;
                } else {
                    float inv_n = 1.0f / static_cast<float>(n);
                    dst[0] = ar * inv_n;
                    dst[1] = ag * inv_n;
                    dst[2] = ab * inv_n;
                    dst[3] = aa * inv;
                }
            } else {
                dst[0] = ar * inv;
                dst[1] = ag * inv;
                dst[2] = ab * inv;
                dst[3] = aa * inv;
            }
            if (hit_counts) hit_counts[static_cast<size_t>(py) * cfg.width + px] = n;
        }
    }
}

}  // namespace

// Renders the given tiles of the frame (each tile as renderTile does: its own mt19937) into `frame` (width*height*4 floats)
// and, when hit_counts is not NULL, each pixel's number of samples whose primary ray hits into hit_counts (width*height).
// Pixels of other tiles are left untouched; calls on disjoint tiles may run on several threads at once.
extern "C" __attribute__((visibility("default"))) int render_tiles(const mcrt_scene_desc* desc, const mcrt_config* cfg, int background,
                                                                   const mcrt_tile* tiles, int n_tiles, float* frame, int32_t* hit_counts) {
    if (!desc || !cfg || !frame || (n_tiles > 0 && !tiles)) return MCRT_ERR_INVALID;
    if (background != MCRT_BACKGROUND_REFERENCE && background != MCRT_BACKGROUND_TRANSPARENT) return MCRT_ERR_INVALID;
    for (int i = 0; i < n_tiles; ++i) render_tile_mode(*desc, *cfg, tiles[i], background, frame, hit_counts);
    return MCRT_OK;
}
