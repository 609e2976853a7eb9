// frt_loader.hpp — model import for the scene builder: the reference's glTF path (src/scene/loader.rs:9-181 load_gltf, which
// rests on the `gltf 1.4.1` and `image 0.25.9` crates) restated over a small JSON reader, a GLB / buffer / accessor reader, a PNG
// decoder on zlib's inflate and image-0.25's Lanczos3 `resize_exact`; plus a Wavefront OBJ subset (an extension: the reference
// has no OBJ path) so that the usual Bunny / Sponza distributions load. Host only; nothing here touches the GPU.
#pragma once
#include "frt_scene.hpp"
#include <functional>
#include <string>
#include <vector>

namespace frt {

struct LoadedModel {                              // the 4-tuple load_gltf returns, loader.rs:12
    std::vector<Geometry> geometries;             // one per mesh primitive, in document order
    std::vector<frt_material> materials;          // texture slots hold IMAGE indices until add_gltf_materials remaps them
    std::vector<std::vector<uint8_t>> images;     // RGBA8, TEXTURE_WIDTH x TEXTURE_HEIGHT (1024 x 1024) each
    std::vector<uint32_t> material_indices;       // per geometry: index into `materials` (0 when the primitive names none)
    std::vector<std::string> warnings;            // what the reference prints (unsupported image format, …)
    // The rig of a glTF document ("Animation"; an extension: the reference loads none of it). All of it is empty for a document
    // without skins, morph targets and animations, and for OBJ.
    struct GeometryRig {                          // per geometry, in the geometry's vertex order
        std::vector<uint16_t> joints;             // JOINTS_0 [n][4], empty: no skin attributes
        std::vector<float> weights;               // WEIGHTS_0 [n][4]
        int skin = -1;                            // the skin the (first) node that carries this geometry's mesh names, or -1
        uint32_t ntargets = 0;
        std::vector<float> deltas;                // targets[*].POSITION [T][n][3]
        std::vector<float> default_weights;       // the mesh's `weights` [T] (zeros when absent)
        int mesh = -1;                            // document index of the mesh
    };
    struct Node { int parent = -1; float trs[10] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1}; bool has_matrix = false; float matrix[16] = {}; int mesh = -1, skin = -1; uint32_t doc_index = 0; };
    struct Skin { std::vector<uint32_t> joints; std::vector<float> inverse_bind; };      // joints: stored node indices; inverse_bind [16 J]
    struct Channel { uint32_t node = 0, path = 0, interpolation = 1; std::vector<float> times, values; };      // node: stored index; values by glTF's layout
    struct Animation { std::string name; std::vector<Channel> channels; };
    std::vector<GeometryRig> geometry_rigs;       // one per geometry (glTF)
    std::vector<Node> nodes;                      // parents first
    std::vector<uint32_t> node_of_document;       // document node index -> index into `nodes`
    std::vector<Skin> skins;
    std::vector<Animation> animations;
};

bool load_gltf(const std::string& path, LoadedModel& out, std::string& err);   // .gltf (+ .bin / data: URIs) and .glb
bool load_obj(const std::string& path, LoadedModel& out, std::string& err);    // v / vt / vn / f, fan-triangulated
bool load_model(const std::string& path, LoadedModel& out, std::string& err);  // by extension

// image 0.25.9 imageops::resize(.., FilterType::Lanczos3) for RGBA8 (src W x H -> dst 1024 x 1024 when used by the loader)
void resize_lanczos3_rgba8(const uint8_t* src, uint32_t sw, uint32_t sh, uint8_t* dst, uint32_t dw, uint32_t dh);
// PNG (8-bit RGB / RGBA / palette, non-interlaced; what gltf's importer hands the reference as R8G8B8 / R8G8B8A8). channels: 3 or 4.
bool decode_png(const uint8_t* data, size_t size, std::vector<uint8_t>& pixels, uint32_t& w, uint32_t& h, uint32_t& channels, std::string& why);

// Huffman JPEG (baseline and progressive, 8-bit, 3-component) -> RGB8
bool decode_jpeg(const uint8_t* data, size_t size, std::vector<uint8_t>& rgb, uint32_t& w, uint32_t& h, std::string& why);

// builder.rs:191-292 without the builder: the model's materials with every image index remapped to the layer id `add_color` / `add_data` returns for
// that image (each is called once per image it is asked about, in the reference's order). What add_gltf_materials and frt_model_layer_plan share.
std::vector<frt_material> remap_gltf_materials(const LoadedModel& m, const std::function<uint32_t(uint32_t)>& add_color, const std::function<uint32_t(uint32_t)>& add_data);
// builder.rs:191-314
std::vector<uint32_t> add_gltf_materials(SceneBuilder& b, const LoadedModel& m);
std::vector<uint32_t> add_gltf_meshes(SceneBuilder& b, const LoadedModel& m);
void add_gltf_instances(SceneBuilder& b, const std::vector<uint32_t>& mesh_ids, const std::vector<uint32_t>& mat_ids,
                        const std::vector<uint32_t>& material_indices, const Mat4& transform);

namespace scenes {
// scenes.rs:246-322. Returns false (and the loader's message) when the file cannot be loaded; the builder is then left empty
// (the reference logs the error and builds an empty scene; this builder has no empty scenes, so callers report the failure).
bool create_gltf_scene(SceneBuilder& b, const std::string& path, const Mat4& model_transform, const Mat4& light_transform, std::string& err);
}

} // namespace frt

struct frt_model { frt::LoadedModel m; };
