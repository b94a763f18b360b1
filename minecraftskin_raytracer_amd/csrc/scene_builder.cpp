// scene_builder.cpp — SkinParser layout + MeshBuilder scene construction on the POD description.
// Host only; the "f-2" row of SURVEY.md §8: runs once per skin/pose change, also the generator of
// every synthetic scene used by tests and bench.py.
//
// Follows (paths under /root/reference/src):
//   skin/image.cpp:16-21          texel = u8 / 255.0f
//   skin/image.h:21-33            Image::extractRegion (out-of-range texels stay Color())
//   skin/skin_parser.cpp:11-20    box-unwrap layout of one body part
//   skin/skin_parser.cpp:45-110   64x64 and legacy 64x32 part origins, legacy left = mirrored right
//   scene/mesh_builder.cpp:66-143 buildBox / buildBoxWithPose (vertex order, face → texture)
//   scene/mesh_builder.cpp:145-223 buildScene / buildDefaultScene (part table, light, camera)
//   scene/pose.h:25-92            built-in poses
// Compile with -ffp-contract=off.
#include "mcrt.h"
#include "mcrt_detmath.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

__attribute__((visibility("hidden"))) int mcrt_detail_fail(int code, const char* msg);  // api.cpp: sets mcrt_last_error()

namespace {

struct Region {  // TextureRegion
    int w = 0, h = 0;
    std::vector<float> px;  // rgba
};
struct PartTex {  // BodyPartTexture
    Region top, bottom, front, back, left, right;
};

struct SkinImage {
    int w, h;
    std::vector<float> px;
};

Region cut(const SkinImage& img, int x, int y, int w, int h) {
    Region r;
    r.w = w;
    r.h = h;
    r.px.assign(static_cast<size_t>(w) * h * 4, 0.0f);
    for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) r.px[4 * i + 3] = 1.0f;  // Color()
    for (int row = 0; row < h; ++row)
        for (int col = 0; col < w; ++col) {
            int sx = x + col, sy = y + row;
            if (sx < 0 || sx >= img.w || sy < 0 || sy >= img.h) continue;
            std::memcpy(&r.px[4 * (static_cast<size_t>(row) * w + col)],
                        &img.px[4 * (static_cast<size_t>(sy) * img.w + sx)], 16);
        }
    return r;
}

// A body part in the skin image (skin_parser.cpp:11-20): origin of its box unwrap and the box's size in texels
struct PartBox {
    int ox, oy, w, h, d;
};
struct Rect {
    int x, y, w, h;
};
// the rectangle of one face of the unwrap, faces in determineFace order: 0 back, 1 front, 2 left, 3 right, 4 top, 5 bottom
Rect face_rect(const PartBox& b, int face) {
    switch (face) {
        case 0: return Rect{b.ox + 2 * b.d + b.w, b.oy + b.d, b.w, b.h};
        case 1: return Rect{b.ox + b.d, b.oy + b.d, b.w, b.h};
        case 2: return Rect{b.ox, b.oy + b.d, b.d, b.h};
        case 3: return Rect{b.ox + b.d + b.w, b.oy + b.d, b.d, b.h};
        case 4: return Rect{b.ox + b.d, b.oy, b.w, b.d};
        default: return Rect{b.ox + b.d + b.w, b.oy, b.w, b.d};
    }
}
// part origins (skin_parser.cpp:45-110): head, body, right arm, left arm, right leg, left leg.  A legacy 64x32 skin has the
// head's outer layer only, and its left limbs are the right ones mirrored (mirror_part).
const PartBox kInnerBox[6] = {{0, 0, 8, 8, 8}, {16, 16, 8, 12, 4}, {40, 16, 4, 12, 4}, {32, 48, 4, 12, 4}, {0, 16, 4, 12, 4}, {16, 48, 4, 12, 4}};
const PartBox kOuterBox[6] = {{32, 0, 8, 8, 8}, {16, 32, 8, 12, 4}, {40, 32, 4, 12, 4}, {48, 48, 4, 12, 4}, {0, 32, 4, 12, 4}, {0, 48, 4, 12, 4}};
const int kLegacyMirrorOf[6] = {-1, -1, -1, 2, -1, 4};  // legacy left arm = right arm mirrored, left leg = right leg mirrored
// The slim ("Alex") player model, 64x64 skins only — Minecraft's own; the reference knows the classic model alone.  It differs
// from classic in the four arm boxes and nowhere else: the arms are 3 texels wide, unwrapped at the classic origins in
// narrower rectangles (front and back 3x12, top and bottom 3x4, sides 4x12), which leaves the unwrap's last columns unread.
const PartBox kSlimInnerArm[2] = {{40, 16, 3, 12, 4}, {32, 48, 3, 12, 4}};  // right, left
const PartBox kSlimOuterArm[2] = {{40, 32, 3, 12, 4}, {48, 48, 3, 12, 4}};
bool is_arm(int part) { return part == 2 || part == 3; }
const PartBox& part_box(int model, bool outer, int part) {
    if (model == MCRT_SKIN_SLIM && is_arm(part)) return (outer ? kSlimOuterArm : kSlimInnerArm)[part - 2];
    return (outer ? kOuterBox : kInnerBox)[part];
}

// The cape (mcrt.h, "capes"): a 64x32 image of its own, unwrapped as Minecraft unwraps it — the box {10, 16, 1} at the image's
// origin.  The box hangs on the body's back turned half a turn about y, so add_box's face slots take the unwrap's faces
// crosswise: the -z slot (outward, seen from behind the player) the unwrap's "front" rectangle (1, 1, 10, 16), the +z slot
// (towards the body) (12, 1, 10, 16), the +x slot (11, 1, 1, 16), the -x slot (0, 1, 1, 16); top (1, 0, 10, 1) and bottom
// (11, 0, 10, 1) keep their slots and are read turned half a turn.  The -z face puts texel column 0 at the +x edge and row 0
// at the top (face_uv), which from behind is the viewer's left and the hinge: the picture reads as painted, nothing is mirrored.
const PartBox kCapeBox = {0, 0, 10, 16, 1};
constexpr int kCapeWidth = 64, kCapeHeight = 32, kCapeTexels = 372;
struct CapeSource {
    Rect rect;
    bool turned;  // read turned half a turn: texel (tx, ty) <- (w - 1 - tx, h - 1 - ty)
};
// where face `face_slot` (add_box's order, 0..5) of the cape mesh is cut from: the one answer for the builder, mcrt_cape_texel
// and the pool map
CapeSource cape_source(int face_slot) {
    static const int unwrap_face[6] = {1, 0, 3, 2, 4, 5};
    return CapeSource{face_rect(kCapeBox, unwrap_face[face_slot]), face_slot >= 4};
}

PartTex unwrap(const SkinImage& img, const PartBox& b) {
    auto face = [&](int f) {
        const Rect r = face_rect(b, f);
        return cut(img, r.x, r.y, r.w, r.h);
    };
    PartTex p;
    p.top = face(4);
    p.bottom = face(5);
    p.left = face(2);
    p.front = face(1);
    p.right = face(3);
    p.back = face(0);
    return p;
}

Region flip_h(const Region& r) {
    Region m;
    m.w = r.w;
    m.h = r.h;
    m.px.resize(r.px.size());
    for (int y = 0; y < r.h; ++y)
        for (int x = 0; x < r.w; ++x)
            std::memcpy(&m.px[4 * (static_cast<size_t>(y) * r.w + x)],
                        &r.px[4 * (static_cast<size_t>(y) * r.w + (r.w - 1 - x))], 16);
    return m;
}

Region turn_half(const Region& r) {
    Region m;
    m.w = r.w;
    m.h = r.h;
    m.px.resize(r.px.size());
    const size_t n = r.px.size() / 4;
    for (size_t i = 0; i < n; ++i) std::memcpy(&m.px[4 * i], &r.px[4 * (n - 1 - i)], 16);
    return m;
}

PartTex cape_part(const uint8_t* rgba8) {  // 64x32 RGBA8
    SkinImage img;
    img.w = kCapeWidth;
    img.h = kCapeHeight;
    img.px.resize(static_cast<size_t>(kCapeWidth) * kCapeHeight * 4);
    for (size_t i = 0; i < img.px.size(); ++i) img.px[i] = rgba8[i] / 255.0f;
    Region* slot[6];
    PartTex p;
    slot[0] = &p.back, slot[1] = &p.front, slot[2] = &p.left, slot[3] = &p.right, slot[4] = &p.top, slot[5] = &p.bottom;  // add_box's order
    for (int f = 0; f < 6; ++f) {
        const CapeSource src = cape_source(f);
        const Region r = cut(img, src.rect.x, src.rect.y, src.rect.w, src.rect.h);
        *slot[f] = src.turned ? turn_half(r) : r;
    }
    return p;
}

PartTex mirror_part(const PartTex& p) {
    PartTex m;
    m.top = flip_h(p.top);
    m.bottom = flip_h(p.bottom);
    m.front = flip_h(p.front);
    m.back = flip_h(p.back);
    m.left = flip_h(p.right);
    m.right = flip_h(p.left);
    return m;
}

bool region_clear(const Region& r) {
    for (size_t i = 0; i < r.px.size() / 4; ++i)
        if (r.px[4 * i + 3] != 0.0f) return false;
    return true;
}
bool fully_transparent(const PartTex& p) {
    return region_clear(p.top) && region_clear(p.bottom) && region_clear(p.front) &&
           region_clear(p.back) && region_clear(p.left) && region_clear(p.right);
}

struct Skin {
    PartTex inner[6];  // head, body, rightArm, leftArm, rightLeg, leftLeg
    PartTex outer[6];
};

// the description plus the storage it points into
struct OwnedDesc {
    mcrt_scene_desc desc;
    std::vector<mcrt_mesh> meshes;
    std::vector<mcrt_texture> textures;
    std::vector<std::unique_ptr<std::vector<float>>> floats;
    std::vector<std::unique_ptr<std::vector<int32_t>>> ints;
    const float* keep(std::vector<float> v) {
        floats.push_back(std::make_unique<std::vector<float>>(std::move(v)));
        return floats.back()->data();
    }
    const int32_t* keep(std::vector<int32_t> v) {
        ints.push_back(std::make_unique<std::vector<int32_t>>(std::move(v)));
        return ints.back()->data();
    }
};

const float kPi = static_cast<float>(3.14159265358979323846);

void rotate_about(float v[3], const float pivot[3], float degX, float degZ) {  // mesh_builder.cpp:25-52
    float p[3] = {v[0] - pivot[0], v[1] - pivot[1], v[2] - pivot[2]};
    if (std::fabs(degX) > 0.01f) {
        float rad = degX * kPi / 180.0f;
        float c = mcrt_cosf(rad), s = mcrt_sinf(rad);
        float ny = p[1] * c - p[2] * s;
        float nz = p[1] * s + p[2] * c;
        p[1] = ny;
        p[2] = nz;
    }
    if (std::fabs(degZ) > 0.01f) {
        float rad = degZ * kPi / 180.0f;
        float c = mcrt_cosf(rad), s = mcrt_sinf(rad);
        float nx = p[0] * c - p[1] * s;
        float ny = p[0] * s + p[1] * c;
        p[0] = nx;
        p[1] = ny;
    }
    v[0] = p[0] + pivot[0];
    v[1] = p[1] + pivot[1];
    v[2] = p[2] + pivot[2];
}

int add_texture(OwnedDesc& o, const Region& r) {
    mcrt_texture t;
    t.width = r.w;
    t.height = r.h;
    t.n_pixels = static_cast<int64_t>(r.px.size() / 4);
    t.rgba = o.keep(r.px);
    o.textures.push_back(t);
    return static_cast<int>(o.textures.size()) - 1;
}

// One box part (mesh_builder.cpp:66-143).  posed → keeps the unrotated triangles as
// localTriangles and rotates the world-space copy.
void add_box(OwnedDesc& o, const PartTex& tex, const float pos[3], const float size[3], float offset,
             bool posed, const float pivot[3], float rotX, float rotZ) {
    float hw = size[0] / 2.0f + offset;
    float hh = size[1] / 2.0f + offset;
    float hd = size[2] / 2.0f + offset;
    float x0 = pos[0] - hw, x1 = pos[0] + hw;
    float y0 = pos[1] - hh, y1 = pos[1] + hh;
    float z0 = pos[2] - hd, z1 = pos[2] + hd;
    const float c[8][3] = {{x0, y0, z0}, {x1, y0, z0}, {x0, y1, z0}, {x1, y1, z0},
                           {x0, y0, z1}, {x1, y0, z1}, {x0, y1, z1}, {x1, y1, z1}};
    // corner index = x + 2*y + 4*z; quads in addFace order: back, front, left, right, top, bottom
    static const int quad[6][4] = {{2, 3, 1, 0}, {7, 6, 4, 5}, {3, 7, 5, 1},
                                   {6, 2, 0, 4}, {6, 7, 3, 2}, {0, 1, 5, 4}};
    const Region* face_tex[6] = {&tex.back, &tex.front, &tex.left, &tex.right, &tex.top, &tex.bottom};

    std::vector<float> verts;
    std::vector<int32_t> tix;
    verts.reserve(12 * 9);
    for (int f = 0; f < 6; ++f) {
        int ti = add_texture(o, *face_tex[f]);
        const int* q = quad[f];
        const int tri[2][3] = {{q[0], q[1], q[2]}, {q[0], q[2], q[3]}};
        for (auto& t : tri) {
            for (int k = 0; k < 3; ++k) verts.insert(verts.end(), c[t[k]], c[t[k]] + 3);
            tix.push_back(ti);
        }
    }
    mcrt_mesh m;
    std::memset(&m, 0, sizeof m);
    m.n_triangles = 12;
    m.is_outer_layer = offset > 0.0f ? 1 : 0;
    if (posed) {
        m.n_local_triangles = 12;
        m.local_tri_vertices = o.keep(verts);
        m.has_rotation = 1;
        std::memcpy(m.pivot, pivot, 12);
        m.rot_x = rotX;
        m.rot_z = rotZ;
        if (!(std::fabs(rotX) < 0.01f && std::fabs(rotZ) < 0.01f))
            for (size_t v = 0; v < verts.size() / 3; ++v) rotate_about(&verts[3 * v], pivot, rotX, rotZ);
    }
    m.tri_vertices = o.keep(std::move(verts));
    m.tri_texture = o.keep(std::move(tix));
    o.meshes.push_back(m);
}

// `cape`: the cape's textures or NULL.  The cape is the LAST mesh: the box {10, 16, 1} at {0, 16, -2.5} — x -5 .. 5, y 8 .. 24,
// z -3 .. -2, on the body's back — hinged at {0, 24, -2} by cape_angle degrees about x (positive: the hem away from the legs).
// It does not follow the body part's own rotation: a mesh has one pivot.  A fully transparent cape is dropped like an outer
// part unless `keep_clear_cape` (a repaintable handle's full table).
OwnedDesc* assemble(const Skin& skin, const float pose[12], int model = MCRT_SKIN_CLASSIC, const PartTex* cape = nullptr, float cape_angle = 0.0f,
                    bool keep_clear_cape = false) {  // mesh_builder.cpp:145-202
    auto* o = new OwnedDesc();
    static const float position[6][3] = {{0, 28, 0}, {0, 18, 0}, {-6, 18, 0}, {6, 18, 0}, {-2, 6, 0}, {2, 6, 0}};
    static const float size[6][3] = {{8, 8, 8}, {8, 12, 4}, {4, 12, 4}, {4, 12, 4}, {4, 12, 4}, {4, 12, 4}};
    static const float pivot[6][3] = {{0, 24, 0}, {0, 18, 0}, {-6, 24, 0}, {6, 24, 0}, {-2, 12, 0}, {2, 12, 0}};
    // a slim arm: 3 wide, x = -7 .. -4 and 4 .. 7 — flush with the body as the classic arm is — and its pivot on its own axis
    static const float slim_position[2][3] = {{-5.5f, 18, 0}, {5.5f, 18, 0}};
    static const float slim_size[3] = {3, 12, 4};
    static const float slim_pivot[2][3] = {{-5.5f, 24, 0}, {5.5f, 24, 0}};
    for (int p = 0; p < 6; ++p) {
        float rx = pose ? pose[2 * p] : 0.0f, rz = pose ? pose[2 * p + 1] : 0.0f;
        bool posed = std::fabs(rx) > 0.01f || std::fabs(rz) > 0.01f;
        const bool slim_arm = model == MCRT_SKIN_SLIM && is_arm(p);
        const float* at = slim_arm ? slim_position[p - 2] : position[p];
        const float* sz = slim_arm ? slim_size : size[p];
        const float* pv = slim_arm ? slim_pivot[p - 2] : pivot[p];
        add_box(*o, skin.inner[p], at, sz, 0.0f, posed, pv, rx, rz);
        if (!fully_transparent(skin.outer[p]))
            add_box(*o, skin.outer[p], at, sz, 0.5f, posed, pv, rx, rz);
    }
    if (cape && (keep_clear_cape || !fully_transparent(*cape))) {
        static const float cape_position[3] = {0, 16, -2.5f}, cape_size[3] = {10, 16, 1}, cape_pivot[3] = {0, 24, -2};
        add_box(*o, *cape, cape_position, cape_size, 0.0f, std::fabs(cape_angle) > 0.01f, cape_pivot, cape_angle, 0.0f);
    }
    mcrt_scene_desc& d = o->desc;
    std::memset(&d, 0, sizeof d);
    d.n_meshes = static_cast<int32_t>(o->meshes.size());
    d.meshes = o->meshes.data();
    d.n_textures = static_cast<int32_t>(o->textures.size());
    d.textures = o->textures.data();
    const float lp[3] = {0, 40, 30}, lc[4] = {1, 1, 1, 1};
    const float cp[3] = {0, 18, 50}, ct[3] = {0, 18, 0}, cu[3] = {0, 1, 0};
    const float bg[4] = {0.2f, 0.3f, 0.5f, 1.0f};
    std::memcpy(d.light_position, lp, 12);
    std::memcpy(d.light_color, lc, 16);
    d.light_intensity = 1.0f;
    d.light_radius = 3.0f;  // Light's in-class default (scene.h:14)
    std::memcpy(d.camera_position, cp, 12);
    std::memcpy(d.camera_target, ct, 12);
    std::memcpy(d.camera_up, cu, 12);
    d.camera_fov = 60.0f;
    std::memcpy(d.background_color, bg, 16);
    return o;
}

// where face `face_slot` of mesh `mesh` of a skin kind's full mesh table is cut from (arguments in range).  assemble(): per
// part the inner box, then its outer box where the skin kind has one
struct FaceSource {
    Rect rect;
    bool flipped;  // a legacy skin's mirrored left limb: the rectangle is read right to left (flip_h)
};
FaceSource face_source(int skin_height, int model, int mesh, int face_slot) {
    int part, outer;
    if (skin_height == 64)
        part = mesh / 2, outer = mesh & 1;
    else
        part = mesh < 2 ? 0 : mesh - 1, outer = mesh == 1 ? 1 : 0;
    const int mirror_of = (skin_height == 32 && !outer) ? kLegacyMirrorOf[part] : -1;
    const PartBox& box = part_box(model, outer != 0, (!outer && mirror_of >= 0) ? mirror_of : part);
    int face = face_slot;
    if (mirror_of >= 0 && (face == 2 || face == 3)) face = 5 - face;  // mirror_part: left = flip_h(right), right = flip_h(left)
    return FaceSource{face_rect(box, face), mirror_of >= 0};
}

Skin parse_skin(const uint8_t* rgba8, int w, int h, int model = MCRT_SKIN_CLASSIC) {  // w == 64, h == 64 or 32; slim: h == 64
    SkinImage img;
    img.w = w;
    img.h = h;
    img.px.resize(static_cast<size_t>(w) * h * 4);
    for (size_t i = 0; i < img.px.size(); ++i) img.px[i] = rgba8[i] / 255.0f;
    Skin s;
    s.inner[0] = unwrap(img, kInnerBox[0]);
    s.outer[0] = unwrap(img, kOuterBox[0]);
    s.inner[1] = unwrap(img, kInnerBox[1]);
    s.inner[2] = unwrap(img, part_box(model, false, 2));
    s.inner[4] = unwrap(img, kInnerBox[4]);
    if (h == 64) {
        s.inner[3] = unwrap(img, part_box(model, false, 3));
        s.inner[5] = unwrap(img, kInnerBox[5]);
        for (int p = 1; p < 6; ++p) s.outer[p] = unwrap(img, part_box(model, true, p));
    } else {
        s.inner[3] = mirror_part(s.inner[kLegacyMirrorOf[3]]);
        s.inner[5] = mirror_part(s.inner[kLegacyMirrorOf[5]]);
    }
    return s;
}

bool model_ok(int skin_height, int model) {  // slim exists for 64x64 skins only
    return model == MCRT_SKIN_CLASSIC || (model == MCRT_SKIN_SLIM && skin_height == 64);
}
const char* const kBadModel = "model must be MCRT_SKIN_CLASSIC, or MCRT_SKIN_SLIM with a 64x64 skin";
const char* const kBadCapeAngle = "cape_angle must be within 0 .. 90 degrees";
bool cape_angle_ok(float a) { return a >= 0.0f && a <= 90.0f; }  // (false for NaN)

const Skin& white_skin(int skin_height, int model) {  // parsed once per kind and process
    static const Skin white[3] = {parse_skin(std::vector<uint8_t>(64 * 64 * 4, 255).data(), 64, 64),
                                  parse_skin(std::vector<uint8_t>(64 * 32 * 4, 255).data(), 64, 32),
                                  parse_skin(std::vector<uint8_t>(64 * 64 * 4, 255).data(), 64, 64, MCRT_SKIN_SLIM)};
    return white[skin_height == 32 ? 1 : (model == MCRT_SKIN_SLIM ? 2 : 0)];
}
}  // namespace

// The figure mcrt_build_skin_scene_model builds from an all-(255,255,255,255) skin of the kind (64 / 32, classic / slim) — every
// part present — at `pose`: what a view of a repaintable handle is flattened from (api.cpp).  The white skin is parsed once
// per kind and process.
extern "C" __attribute__((visibility("hidden"))) mcrt_scene_desc* mcrt_detail_white_figure(int skin_height, int model, const float pose[12]) {
    return &assemble(white_skin(skin_height, model), pose, model)->desc;
}
// The caped form (arguments checked by the callers): the white figure with the cape mesh behind it, always present — what a
// caped handle's view is flattened from, and, with `cape_alpha` 0, its first blob: a white skin and a transparent cape.
extern "C" __attribute__((visibility("hidden"))) mcrt_scene_desc* mcrt_detail_white_figure_cape(int skin_height, int model, const float pose[12], float cape_angle,
                                                                                                int cape_alpha) {
    static const PartTex cape[2] = {cape_part(std::vector<uint8_t>(kCapeWidth * kCapeHeight * 4, 0).data()),
                                    cape_part(std::vector<uint8_t>(kCapeWidth * kCapeHeight * 4, 255).data())};
    return &assemble(white_skin(skin_height, model), pose, model, &cape[cape_alpha ? 1 : 0], cape_angle, true)->desc;
}

extern "C" {

int mcrt_build_skin_scene(const uint8_t* rgba8, int w, int h, const float pose[12], mcrt_scene_desc** out) {
    if (!rgba8 || !out || w != 64 || (h != 64 && h != 32)) return MCRT_ERR_INVALID;  // skin_parser.cpp:122-131
    *out = &assemble(parse_skin(rgba8, w, h), pose)->desc;
    return MCRT_OK;
}

int mcrt_build_skin_scene_model(const uint8_t* rgba8, int w, int h, int model, const float pose[12], mcrt_scene_desc** out) {
    if (!rgba8 || !out || w != 64 || (h != 64 && h != 32) || !model_ok(h, model)) return MCRT_ERR_INVALID;
    *out = &assemble(parse_skin(rgba8, w, h, model), pose, model)->desc;
    return MCRT_OK;
}

int mcrt_build_skin_scene_cape(const uint8_t* rgba8, int w, int h, int model, const float pose[12], const uint8_t* cape_rgba8, float cape_angle,
                               mcrt_scene_desc** out) {
    if (!rgba8 || !out) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument");
    if (w != 64 || (h != 64 && h != 32)) return mcrt_detail_fail(MCRT_ERR_INVALID, "a skin image is 64x64 or 64x32");
    if (!model_ok(h, model)) return mcrt_detail_fail(MCRT_ERR_INVALID, kBadModel);
    if (!cape_rgba8) {  // the capeless call, byte for byte; the angle is not read
        *out = &assemble(parse_skin(rgba8, w, h, model), pose, model)->desc;
        return MCRT_OK;
    }
    if (!cape_angle_ok(cape_angle)) return mcrt_detail_fail(MCRT_ERR_INVALID, kBadCapeAngle);
    const PartTex cape = cape_part(cape_rgba8);
    *out = &assemble(parse_skin(rgba8, w, h, model), pose, model, &cape, cape_angle)->desc;
    return MCRT_OK;
}

int mcrt_cape_texel(int face_slot, int tx, int ty, int* cape_x, int* cape_y) {
    if (!cape_x || !cape_y) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument");
    if (face_slot < 0 || face_slot > 5) return mcrt_detail_fail(MCRT_ERR_INVALID, "face_slot must be 0..5");
    const CapeSource src = cape_source(face_slot);
    const Rect& r = src.rect;
    if (tx < 0 || tx >= r.w || ty < 0 || ty >= r.h) return mcrt_detail_fail(MCRT_ERR_INVALID, "texel outside the face's region");
    *cape_x = r.x + (src.turned ? r.w - 1 - tx : tx);
    *cape_y = r.y + (src.turned ? r.h - 1 - ty : ty);
    return MCRT_OK;
}

// The cape mesh's texels in pool order — six faces in slot order, row-major — as cape pixel indices y * 64 + x.  Returns the
// count, 372; writes `capacity` entries at most.
int mcrt_cape_pool_map(int32_t* out, int capacity) {
    if (!out) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument");
    int n = 0;
    for (int face = 0; face < 6; ++face) {
        const CapeSource src = cape_source(face);
        const Rect& r = src.rect;
        for (int ty = 0; ty < r.h; ++ty)
            for (int tx = 0; tx < r.w; ++tx, ++n)
                if (n < capacity) out[n] = (r.y + (src.turned ? r.h - 1 - ty : ty)) * kCapeWidth + r.x + (src.turned ? r.w - 1 - tx : tx);
    }
    static_assert(2 * 10 * 16 + 2 * 1 * 16 + 2 * 10 * 1 == kCapeTexels, "the cape box's six faces");
    return n;
}

int mcrt_skin_model_of(const uint8_t* rgba8, int w, int h) {
    if (!rgba8) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument"), -1;
    if (w != 64 || (h != 64 && h != 32)) return mcrt_detail_fail(MCRT_ERR_INVALID, "a skin image is 64x64 or 64x32"), -1;
    if (h != 64) return MCRT_SKIN_CLASSIC;
    // the columns a slim unwrap leaves unused, of the inner right arm and the inner left arm
    static const Rect unused[4] = {{50, 16, 2, 4}, {54, 20, 2, 12}, {42, 48, 2, 4}, {46, 52, 2, 12}};
    for (const Rect& r : unused)
        for (int y = r.y; y < r.y + r.h; ++y)
            for (int x = r.x; x < r.x + r.w; ++x)
                if (rgba8[4 * (static_cast<size_t>(y) * 64 + x) + 3] != 0) return MCRT_SKIN_CLASSIC;
    return MCRT_SKIN_SLIM;
}

int mcrt_skin_texel(int skin_height, int mesh, int face_slot, int tx, int ty, int* skin_x, int* skin_y) {
    return mcrt_skin_texel_model(skin_height, MCRT_SKIN_CLASSIC, mesh, face_slot, tx, ty, skin_x, skin_y);
}

int mcrt_skin_texel_model(int skin_height, int model, int mesh, int face_slot, int tx, int ty, int* skin_x, int* skin_y) {
    if (!skin_x || !skin_y) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument");
    if (skin_height != 64 && skin_height != 32) return mcrt_detail_fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (!model_ok(skin_height, model)) return mcrt_detail_fail(MCRT_ERR_INVALID, kBadModel);
    if (face_slot < 0 || face_slot > 5) return mcrt_detail_fail(MCRT_ERR_INVALID, "face_slot must be 0..5");
    if (skin_height == 64 && (mesh < 0 || mesh >= 12)) return mcrt_detail_fail(MCRT_ERR_INVALID, "mesh must be 0..11 for a 64x64 skin");
    if (skin_height == 32 && (mesh < 0 || mesh >= 7)) return mcrt_detail_fail(MCRT_ERR_INVALID, "mesh must be 0..6 for a 64x32 skin");
    const FaceSource src = face_source(skin_height, model, mesh, face_slot);
    const Rect& r = src.rect;
    if (tx < 0 || tx >= r.w || ty < 0 || ty >= r.h) return mcrt_detail_fail(MCRT_ERR_INVALID, "texel outside the face's region");
    *skin_x = r.x + (src.flipped ? r.w - 1 - tx : tx);  // flip_h
    *skin_y = r.y + ty;
    return MCRT_OK;
}

// The texel pool of the full-table figure of a skin kind, in pool order — assemble()'s meshes with every part present, their
// six faces in slot order, a face's texels row-major, which is the order add_box hands the textures to the flattener in —
// by the tables above: per texel its mesh and the skin pixel y * 64 + x it is cut from.  Returns the count.
__attribute__((visibility("hidden"))) int mcrt_detail_skin_pool(int skin_height, int model, int32_t* pixel, int32_t* mesh_of, int capacity) {
    const int n_meshes = skin_height == 64 ? 12 : 7;
    int n = 0;
    for (int mesh = 0; mesh < n_meshes; ++mesh)
        for (int face = 0; face < 6; ++face) {
            const FaceSource src = face_source(skin_height, model, mesh, face);
            const Rect& r = src.rect;
            for (int ty = 0; ty < r.h; ++ty)
                for (int tx = 0; tx < r.w; ++tx, ++n) {
                    if (n >= capacity) continue;
                    if (pixel) pixel[n] = (r.y + ty) * 64 + r.x + (src.flipped ? r.w - 1 - tx : tx);
                    if (mesh_of) mesh_of[n] = mesh;
                }
        }
    return n;
}

int mcrt_skin_pool_map(int skin_height, int32_t* out, int capacity) { return mcrt_skin_pool_map_model(skin_height, MCRT_SKIN_CLASSIC, out, capacity); }

int mcrt_skin_pool_map_model(int skin_height, int model, int32_t* out, int capacity) {
    if (!out) return mcrt_detail_fail(MCRT_ERR_INVALID, "NULL argument");
    if (skin_height != 64 && skin_height != 32) return mcrt_detail_fail(MCRT_ERR_INVALID, "skin_height must be 64 or 32");
    if (!model_ok(skin_height, model)) return mcrt_detail_fail(MCRT_ERR_INVALID, kBadModel);
    return mcrt_detail_skin_pool(skin_height, model, out, nullptr, capacity < 0 ? 0 : capacity);
}

int mcrt_build_default_scene(const float pose[12], mcrt_scene_desc** out) {
    if (!out) return MCRT_ERR_INVALID;
    Skin s;
    Region white;
    white.w = white.h = 1;
    white.px = {1.0f, 1.0f, 1.0f, 1.0f};
    for (auto& p : s.inner) p.top = p.bottom = p.front = p.back = p.left = p.right = white;
    *out = &assemble(s, pose)->desc;
    return MCRT_OK;
}

int mcrt_builtin_pose(int index, float pose_out[12]) {
    // {head, body, rightArm, leftArm, rightLeg, leftLeg} x {rotX, rotZ}
    static const float poses[7][12] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},               // standing
        {0, 0, 0, 0, 30, 0, -30, 0, -25, 0, 25, 0},         // walking
        {-5, 0, 5, 0, 50, 0, -50, 0, -45, 0, 45, 0},        // running
        {5, 0, 0, 0, -140, -20, 0, 0, 0, 0, 0, 0},          // waving
        {0, 0, 0, 0, -10, 0, -10, 0, -90, 0, -90, 0},       // sitting
        {-10, 0, 5, 0, -90, 10, 20, -10, -15, 0, 20, 0},    // fighting
        {30, 15, 0, 5, -45, 30, 150, -10, 0, 0, 0, 0},      // dab
    };
    if (index < 0 || index > 6 || !pose_out) return MCRT_ERR_INVALID;
    std::memcpy(pose_out, poses[index], sizeof poses[index]);
    return MCRT_OK;
}

void mcrt_scene_desc_free(mcrt_scene_desc* d) {
    if (d) delete reinterpret_cast<OwnedDesc*>(d);
}

}  // extern "C"
