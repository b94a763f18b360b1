// flatten.h — host-side scene flattener (see flatten.cpp)
#ifndef MCRT_FLATTEN_H
#define MCRT_FLATTEN_H

#include "flat_scene.h"
#include "mcrt.h"

#include <cstdint>
#include <string>
#include <vector>

namespace mcrt {
// Returns false and fills `err` for malformed descriptions.
bool flatten_scene(const mcrt_scene_desc* desc, std::vector<uint8_t>& blob, std::string& err);
// The prefix [FlatHeader][FlatMesh x n_meshes] of that blob alone — bytes [0, texel_offset), what pose, camera and light decide
// — by the same code, with no texel copied or scanned: equal to flatten_scene's prefix byte for byte but for the MESH_OPAQUE
// bits, which the texels own and which stay clear here (mcrt_scene_set_view & co keep the resident blob's).
bool flatten_view_table(const mcrt_scene_desc* desc, std::vector<uint8_t>& table, std::string& err);
}  // namespace mcrt

#endif
