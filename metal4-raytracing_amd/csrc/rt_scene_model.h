// rt_scene_model.h — the in-memory scene shared by the parts of the host ingest (C++ mirror of the
// reference's Swift scene layer); the readers fill it, rt_scene.cpp serves it over the C-ABI.
//
//   class Scene      ~ MetalRaytracing/Scene.swift:10-170 (lights, orbit camera)
//   class Model      ~ MetalRaytracing/Model.swift:29-205 (T*R*S transform, overrides)
//   struct Mesh      ~ MetalRaytracing/Mesh.swift:17-68   (one MDLMesh = one instance)
//   struct Submesh   ~ MetalRaytracing/SubMesh.swift:18-324 (material group, u32 indices)
#pragma once
#include "rt_m4.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>

namespace rt {

inline rt_float3 f3(float x, float y, float z) { rt_float3 v; v.x = x; v.y = y; v.z = z; v._pad = 0.0f; return v; }

struct Submesh {
    std::string material_name;
    std::vector<uint32_t> indices;
    Material material;
    int32_t tex[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // scene texture per slot (RT_TEXTURE_SLOTS)
    std::string tex_path[RT_TEXTURE_SLOTS];                // MTL maps, bound by add_obj
};

struct MtlEntry {
    Material material;
    std::string maps[RT_TEXTURE_SLOTS];
};

struct Skin {
    // Synthetic skeleton for the robot stand-in (config 5): a chain of joints along +Y.
    std::vector<int> parent;
    std::vector<M4> rest_local;      // local rest transforms
    std::vector<M4> inverse_bind;    // inverse of global bind transforms
    double duration = 2.0;
};

// Model.skeleton / Model.animation of a USD asset (Model.swift:346-414): joint paths, parents
// from the paths, rest transforms, inverse bind transforms, and the packed joint animation as
// keyframe tracks (time in seconds, translations / rotations (x, y, z, w) / scales per joint).
struct UsdSkel {
    std::vector<std::string> joint_paths;
    std::vector<int> parent;
    std::vector<M4> rest, inverse_bind;
    struct Track {
        int comps = 3;
        std::vector<double> t;
        std::vector<std::vector<float>> v;   // per key: comps * joints
    };
    bool has_anim = false;
    std::vector<std::string> anim_paths;
    Track tr, rot, sc;
    double duration = 0.0;
};

struct Mesh {
    std::string name;
    std::vector<rt_float3> positions, normals;
    std::vector<rt_float2> uvs;
    bool has_uvs = false;
    std::vector<uint16_t> joint_indices;  // ushort4 per vertex
    std::vector<float> joint_weights;     // float4 per vertex
    std::vector<Submesh> submeshes;
    M4 transform;
    uint32_t joint_count = 0;
    std::shared_ptr<Skin> skin;
    // USD skinning (MeshSkinningInfo, Mesh.swift:10-15): the model's skeleton, this mesh's joint
    // order mapped to skeleton indices, geometryBindTransform and its inverse
    std::shared_ptr<UsdSkel> usd_skel;
    std::vector<int> joint_to_skel;
    M4 geom_bind, geom_bind_inv;
};

struct Model {
    std::string name;
    float position[3], rotation[3], scale;
    std::vector<Mesh> meshes;
};

}  // namespace rt

struct rt_scene {
    std::vector<rt::Model> models;
    std::vector<Light> lights;
    std::string err;
    struct Texture {
        std::vector<uint8_t> texels;   // RGBA8, row 0 = top
        uint32_t w = 0, h = 0;
        std::string path;              // dedup key: the file (or package entry) it was decoded from
    };
    std::vector<Texture> textures;
    // one decoded PNG per key (a file's key is its path); only the file variant reports in `err`
    rt_status texture_from_bytes(const std::string& key, const uint8_t* data, size_t n, uint32_t* id);
    rt_status texture_from_file(const std::string& path, uint32_t* id);
    // flattened description caches
    std::vector<rt_mesh_desc> mesh_descs;
    std::vector<std::vector<rt_submesh_desc>> sub_descs;
    std::vector<rt_texture_desc> tex_descs;
};

namespace rt {

inline Material default_material() {
    Material m;
    std::memset(&m, 0, sizeof(m));
    m.refractionIndex = 1.0f;   // SubMesh.swift:295-296
    m.opacity = 1.0f;
    m.textureFlags = 0;
    return m;
}

// ModelMaterialOverride application (SubMesh.swift:272-288)
inline void apply_override(Material& m, const rt_material_override* ov) {
    if (!ov) return;
    if (ov->has_base_color) m.baseColor = f3(ov->base_color[0], ov->base_color[1], ov->base_color[2]);
    if (ov->has_refraction_index) m.refractionIndex = std::max(ov->refraction_index, 1.0f);
    if (ov->has_opacity) m.opacity = std::min(std::max(ov->opacity, 0.0f), 1.0f);
}

inline std::string dir_of(const std::string& p) {
    size_t s = p.find_last_of('/');
    return s == std::string::npos ? std::string(".") : p.substr(0, s);
}

// Texture binding of one submesh slot (SubMesh.swift:117-166): flag bit + texture, and the base
// color map replaces baseColor by white (:120-124).
inline void bind_slot(Submesh& sm, int slot, uint32_t id) {
    sm.tex[slot] = (int32_t)id;
    sm.material.textureFlags |= 1u << slot;
    if (slot == 0) sm.material.baseColor = f3(1.0f, 1.0f, 1.0f);
}

inline Model new_model(const char* name, const float position[3], const float rotation[3], float scale) {
    Model model;
    model.name = name;
    for (int k = 0; k < 3; ++k) { model.position[k] = position[k]; model.rotation[k] = rotation ? rotation[k] : 0.0f; }
    model.scale = scale;
    return model;
}

inline void finish_model(rt_scene* s, Model&& model, const rt_material_override* ov) {
    M4 T = model_transform(model.position, model.rotation, model.scale);
    for (auto& m : model.meshes) {
        m.transform = T;
        for (auto& sm : m.submeshes) apply_override(sm.material, ov);  // Model.swift:198-205
    }
    s->models.push_back(std::move(model));
}

// the mesh at a flat index over models x meshes (the order of rt_scene_get_desc), or null
inline Mesh* mesh_at(rt_scene* s, uint32_t flat_index) {
    for (auto& model : s->models) {
        if (flat_index < model.meshes.size()) return &model.meshes[flat_index];
        flat_index -= (uint32_t)model.meshes.size();
    }
    return nullptr;
}

// The readers, one file each (rt_scene_obj.cpp, rt_scene_procedural.cpp, rt_scene_usd.cpp): each
// appends a finished Model or leaves the models as they were.
rt_status add_obj_impl(rt_scene* s, const char* path, const float position[3], const float rotation[3], float scale,
                       const rt_material_override* ov);
rt_status add_procedural_impl(rt_scene* s, const char* kind, const char* mtl_path, const float position[3],
                              const float rotation[3], float scale, const rt_material_override* ov);
rt_status add_usd_impl(rt_scene* s, const char* path, const float position[3], const float rotation[3], float scale,
                       const rt_material_override* ov);
bool parse_mtl(const std::string& path, std::map<std::string, MtlEntry>& out);
void compute_vertex_normals(Mesh& m);
// joint matrices at clip time t: the synthetic robot's (procedural) and a USD skeleton's
void skin_joint_matrices(const Skin& sk, double time_seconds, std::vector<M4>& out);
void usd_joint_matrices(const Mesh& m, double time_seconds, std::vector<M4>& out);

}  // namespace rt
