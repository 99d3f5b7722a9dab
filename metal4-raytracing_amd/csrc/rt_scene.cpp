// rt_scene.cpp — the rt_scene_* C entry points over the in-memory scene (rt_scene_model.h): scene
// lifetime, the readers as thin guarded calls, the texture registry, presets (AppScene.swift:14-28),
// the flattened description, lights and the orbit camera (Scene.swift:10-170), default uniforms and
// random offsets.  The readers are rt_scene_obj.cpp, rt_scene_procedural.cpp and rt_scene_usd.cpp.
#include "rt_scene_model.h"
#include "rt_file.h"

#include <new>

using namespace rt;

static bool find_texture(const rt_scene* s, const std::string& key, uint32_t* id) {
    for (size_t i = 0; i < s->textures.size(); ++i)
        if (!s->textures[i].path.empty() && s->textures[i].path == key) return *id = (uint32_t)i, true;
    return false;
}

static rt_status add_png(rt_scene* s, const std::string& key, const uint8_t* data, size_t n, uint32_t* id,
                         std::string* decoder_text) {   // two passes: the size, then the texels
    rt_scene::Texture t;
    char eb[256] = {0};
    rt_status st = rt_decode_png(data, n, nullptr, &t.w, &t.h, eb, sizeof eb);
    if (!st) {
        t.texels.resize((size_t)t.w * t.h * 4);
        st = rt_decode_png(data, n, t.texels.data(), &t.w, &t.h, eb, sizeof eb);
    }
    if (st) {
        if (decoder_text) *decoder_text = eb;
        return st;
    }
    t.path = key;
    s->textures.push_back(std::move(t));
    *id = (uint32_t)(s->textures.size() - 1);
    return RT_OK;
}

rt_status rt_scene::texture_from_bytes(const std::string& key, const uint8_t* data, size_t n, uint32_t* id) {
    return find_texture(this, key, id) ? RT_OK : add_png(this, key, data, n, id, nullptr);
}

rt_status rt_scene::texture_from_file(const std::string& path, uint32_t* id) {
    if (find_texture(this, path, id)) return RT_OK;   // an MTL names one map many times: read it once
    std::vector<uint8_t> data;
    std::string text;
    if (!read_file(path, 0, data, err)) return RT_ERR_IO;
    const rt_status st = add_png(this, path, data.data(), data.size(), id, &text);
    if (st) err = path + ": " + text;
    return st;
}

static Light area_light_default() {  // Scene.setupLight (Scene.swift:161-169)
    Light l;
    std::memset(&l, 0, sizeof l);
    l.type = LightTypeAreaLight;
    l.position = f3(0.0f, 1.98f, 0.0f);
    l.forward = f3(0.0f, -1.0f, 0.0f);
    l.right = f3(0.25f, 0.0f, 0.0f);
    l.up = f3(0.0f, 0.0f, 0.25f);
    l.color = f3(4.0f, 4.0f, 4.0f);
    return l;
}
static Light spot_light_default() {  // Light.spotLight(...) (Scene.swift:88, :200-208)
    Light l;
    std::memset(&l, 0, sizeof l);
    l.type = LightTypeSpotlight;
    l.position = f3(2.0f, 1.0f, 4.0f);
    l.direction = f3(-1.5f, -0.5f, -1.5f);
    l.coneAngle = 25.0f / 180.0f * 3.14159265358979323846f;
    l.color = f3(4.0f, 4.0f, 4.0f);
    return l;
}

// The message of a caught exception, stored without letting that assignment throw in turn.
static rt_status fail(rt_scene* s, rt_status st, const char* prefix, const char* what) noexcept {
    try {
        s->err = prefix ? std::string(prefix) + ": " + what : std::string(what);
    } catch (...) {
        s->err.clear();
    }
    return st;
}
// Nothing throws across the C-ABI: every entry point that can allocate runs its body
// in here.  With `usd_path` every exception is RT_ERR_IO "path: what()": the asset is untrusted, an
// allocation it asks for and does not get is an I/O error of that file.
template <class Body>
static rt_status guarded(rt_scene* s, Body&& body, const char* usd_path = nullptr) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc& e) {
        return usd_path ? fail(s, RT_ERR_IO, usd_path, e.what()) : fail(s, RT_ERR_OUT_OF_MEMORY, nullptr, "out of memory");
    } catch (const std::exception& e) {
        return fail(s, RT_ERR_IO, usd_path, e.what());
    }
}

extern "C" {

void rt_material_override_glass(rt_material_override* out) {
    std::memset(out, 0, sizeof *out);
    out->has_base_color = 1;
    out->base_color[0] = 0.95f; out->base_color[1] = 0.98f; out->base_color[2] = 1.0f;
    out->has_refraction_index = 1; out->refraction_index = 1.52f;
    out->has_opacity = 1; out->opacity = 0.08f;
}

rt_status rt_scene_new(rt_scene** out) {
    if (!out) return RT_ERR_INVALID_ARG;
    rt_scene* s = new (std::nothrow) rt_scene();
    if (!s) return RT_ERR_OUT_OF_MEMORY;
    // Scene.init: lights = [light1 (area), light3 (spot)]; light2 is built but unused (Scene.swift:82-91)
    const rt_status st = guarded(s, [&] {
        s->lights.push_back(area_light_default());
        s->lights.push_back(spot_light_default());
        return RT_OK;
    });
    if (st) delete s;
    else *out = s;
    return st;
}

rt_status rt_scene_free(rt_scene* scene) { delete scene; return RT_OK; }
const char* rt_scene_last_error(const rt_scene* scene) { return scene ? scene->err.c_str() : "null scene"; }

rt_status rt_scene_add_obj(rt_scene* s, const char* obj_path, const float position[3],
                           const float rotation[3], float scale, const rt_material_override* ov) {
    if (!s || !obj_path || !position) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] { return add_obj_impl(s, obj_path, position, rotation, scale, ov); });
}

rt_status rt_scene_add_usd(rt_scene* s, const char* path, const float position[3], const float rotation[3], float scale,
                           const rt_material_override* ov) {
    if (!s || !path || !position) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] { return add_usd_impl(s, path, position, rotation, scale, ov); }, path);
}

rt_status rt_scene_add_procedural(rt_scene* s, const char* kind, const char* mtl_path,
                                  const float position[3], const float rotation[3], float scale,
                                  const rt_material_override* ov) {
    if (!s || !kind || !position) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] { return add_procedural_impl(s, kind, mtl_path, position, rotation, scale, ov); });
}

rt_status rt_scene_set_lights(rt_scene* s, const Light* lights, uint32_t count) {
    if (!s || (count && !lights)) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] { s->lights.assign(lights, lights + count); return RT_OK; });
}

rt_status rt_scene_set_light_intensity(rt_scene* s, float intensity) {
    if (!s) return RT_ERR_INVALID_ARG;
    for (auto& l : s->lights) l.color = f3(intensity, intensity, intensity);
    return RT_OK;
}

static bool file_exists(const std::string& p) {
    FILE* f = std::fopen(p.c_str(), "r");
    if (f) std::fclose(f);
    return f != nullptr;
}

rt_status rt_scene_preset(const char* name_c, const char* asset_dir_c, rt_scene** out, int32_t* is_synthetic) {
    if (!name_c || !out) return RT_ERR_INVALID_ARG;
    rt_scene* s = nullptr;
    rt_status st = rt_scene_new(&s);
    if (st) return st;
    int synth = 0;
    st = guarded(s, [&] {
        std::string name = name_c, dir = asset_dir_c ? asset_dir_c : ".";
        bool force_synth = false;
        const std::string suf = "_synthetic";
        if (name.size() > suf.size() && name.compare(name.size() - suf.size(), suf.size(), suf) == 0) {
            force_synth = true;
            name = name.substr(0, name.size() - suf.size());
        }
        const float zero[3] = {0, 0, 0};
        auto obj = [&](const char* n, float px, float py, float pz, float sc) -> rt_status {
            float p[3] = {px, py, pz};
            return rt_scene_add_obj(s, (dir + "/" + n + ".obj").c_str(), p, zero, sc, nullptr);
        };
        // AppScene.swift:14-28 — models after the (optional) hero object
        auto base = [&]() -> rt_status {
            rt_status r;
            if ((r = obj("plane", 0, 0, 0, 10))) return r;
            if ((r = obj("sphere", -1.9f, 0.0f, 0.3f, 1))) return r;
            if ((r = obj("sphere", 2.9f, 0.0f, -0.5f, 2))) return r;
            return obj("plane-back", 0, 0, -1.5f, 10);
        };
        auto hero = [&](const char* kind, const rt_material_override* ov) -> rt_status {
            float pos[3] = {0.3f, 0.38f, 2.5f};
            float rot[3] = {0.0f, 3.14159265358979323846f / 2.0f * 1.2f, 0.0f};
            std::string real = dir + "/" + kind + ".obj";
            if (!force_synth && file_exists(real)) return rt_scene_add_obj(s, real.c_str(), pos, rot, 1.2f, ov);
            synth = 1;
            std::string mtl = dir + "/" + kind + ".mtl";
            return rt_scene_add_procedural(s, kind, file_exists(mtl) ? mtl.c_str() : nullptr, pos, rot, 1.2f, ov);
        };
        rt_material_override glass;
        rt_material_override_glass(&glass);
        if (name == "c1") {
            st = base();
        } else if (name == "c2") {
            if (!(st = hero("bunny", nullptr))) st = base();
        } else if (name == "c3" || name == "c3g") {
            if (!(st = hero("dragon", &glass))) st = base();
        } else if (name == "c3d") {
            if (!(st = hero("dragon", nullptr))) st = base();
        } else if (name == "c3k") {
            float pos[3] = {0.3f, 0.38f, 2.5f};
            float rot[3] = {0.0f, 3.14159265358979323846f / 2.0f * 1.2f, 0.0f};
            synth = 1;
            std::string mtl = dir + "/dragon.mtl";
            if (!(st = rt_scene_add_procedural(s, "knot", file_exists(mtl) ? mtl.c_str() : nullptr, pos, rot, 1.2f, &glass)))
                st = base();
        } else if (name == "c3r") {
            // Irregular-geometry cross-check of the headline (not a BASELINE config): the reference's own
            // modelled / scanned meshes in the dragon's place at about its triangle count, glass like
            // C3g: a 4 x 4 wall of coatballs (AssetResources/coatball, 46,816 triangles each, ~12 units
            // across) and a row of 8 teapots (15,704 triangles each) in front of it: 874,688 triangles.
            for (int j = 0; j < 4 && !st; ++j)
                for (int i = 0; i < 4 && !st; ++i) {
                    float p[3] = {0.3f + (i - 1.5f) * 0.27f, 0.50f + (j - 1.5f) * 0.2f, 2.5f};
                    st = rt_scene_add_obj(s, (dir + "/coatball/coatball.obj").c_str(), p, zero, 0.016f, &glass);
                }
            for (int k = 0; k < 8 && !st; ++k) {
                float p[3] = {0.3f + (k - 3.5f) * 0.17f, 0.0f, 2.75f};
                st = rt_scene_add_obj(s, (dir + "/teapot.obj").c_str(), p, zero, 0.001f, &glass);
            }
            if (!st) st = base();
        } else if (name == "c5" || name == "app") {
            float rp[3] = {-0.5f, 0.0f, 1.0f};
            const std::string robot = dir + "/robot.usdz";
            if (!force_synth && file_exists(robot)) {   // AppScene.swift:15: robot, scale 0.01
                st = rt_scene_add_usd(s, robot.c_str(), rp, zero, 0.01f, nullptr);
            } else {
                synth = 1;
                st = rt_scene_add_procedural(s, "robot", nullptr, rp, zero, 0.5f, nullptr);
            }
            if (!st && name == "app") {
                if (!(st = hero("dragon", &glass))) {
                    if (!(st = obj("train", -0.3f, 0.0f, 0.4f, 0.5f))) st = obj("treefir", 0.5f, 0.0f, -0.2f, 0.7f);
                }
            }
            if (!st) st = base();
        } else {
            s->err = "unknown preset " + name;
            st = RT_ERR_INVALID_ARG;
        }
        return st;
    });
    if (!st && is_synthetic) *is_synthetic = synth;
    *out = s;  // on failure too: the caller reads the error, then frees
    return st;
}

rt_status rt_scene_get_desc(rt_scene* s, rt_scene_desc* out) {
    if (!s || !out) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] {
        s->mesh_descs.clear();
        s->sub_descs.clear();
        for (auto& model : s->models)
            for (auto& m : model.meshes) {
                std::vector<rt_submesh_desc> subs;
                for (auto& sm : m.submeshes) {
                    rt_submesh_desc d;
                    std::memset(&d, 0, sizeof d);
                    d.indices = sm.indices.data();
                    d.index_count = (uint32_t)sm.indices.size();
                    d.material = sm.material;
                    for (int k = 0; k < 8; ++k) d.textures[k] = sm.tex[k];
                    subs.push_back(d);
                }
                s->sub_descs.push_back(std::move(subs));   // the inner buffer stays put when the outer grows
                rt_mesh_desc d;
                std::memset(&d, 0, sizeof d);
                d.positions = m.positions.data();
                d.normals = m.normals.data();
                d.uvs = m.has_uvs ? m.uvs.data() : nullptr;
                d.joint_indices = m.joint_indices.empty() ? nullptr : m.joint_indices.data();
                d.joint_weights = m.joint_weights.empty() ? nullptr : m.joint_weights.data();
                d.vertex_count = (uint32_t)m.positions.size();
                d.submesh_count = (uint32_t)m.submeshes.size();
                d.submeshes = s->sub_descs.back().data();
                d.transform = pack4x3(m.transform);
                d.joint_count = m.joint_count;
                s->mesh_descs.push_back(d);
            }
        out->mesh_count = (uint32_t)s->mesh_descs.size();
        out->meshes = s->mesh_descs.data();
        out->light_count = (uint32_t)s->lights.size();
        out->lights = s->lights.data();
        s->tex_descs.clear();
        for (auto& t : s->textures) {
            rt_texture_desc d;
            d.rgba8 = t.texels.data();
            d.width = t.w;
            d.height = t.h;
            s->tex_descs.push_back(d);
        }
        out->texture_count = (uint32_t)s->tex_descs.size();
        out->_pad = 0;
        out->textures = s->tex_descs.data();
        return RT_OK;
    });
}

rt_status rt_scene_add_texture(rt_scene* s, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t* id) {
    if (!s || !rgba8 || !id) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] {
        if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28)) {
            s->err = "bad texture size";
            return RT_ERR_INVALID_ARG;
        }
        rt_scene::Texture t;
        t.w = width;
        t.h = height;
        t.texels.assign(rgba8, rgba8 + (size_t)width * height * 4);
        s->textures.push_back(std::move(t));
        *id = (uint32_t)(s->textures.size() - 1);
        return RT_OK;
    });
}

rt_status rt_scene_load_texture(rt_scene* s, const char* png_path, uint32_t* id) {
    if (!s || !png_path || !id) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] { return s->texture_from_file(png_path, id); });
}

rt_status rt_scene_bind_texture(rt_scene* s, uint32_t mesh_index, uint32_t submesh_index, uint32_t slot,
                                uint32_t texture_id) {
    if (!s) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] {
        Mesh* m = mesh_at(s, mesh_index);
        if (slot >= RT_TEXTURE_SLOTS || texture_id >= s->textures.size()) s->err = "bad texture slot / id";
        else if (!m) s->err = "bad mesh index";
        else if (submesh_index >= m->submeshes.size()) s->err = "bad submesh index";
        else {
            bind_slot(m->submeshes[submesh_index], (int)slot, texture_id);
            return RT_OK;
        }
        return RT_ERR_INVALID_ARG;
    });
}

uint64_t rt_scene_triangle_count(const rt_scene* s) {
    uint64_t n = 0;
    if (!s) return 0;
    for (auto& model : s->models)
        for (auto& m : model.meshes)
            for (auto& sm : m.submeshes) n += sm.indices.size() / 3;
    return n;
}

rt_status rt_scene_joint_matrices(rt_scene* s, uint32_t mesh_index, double time_seconds,
                                  float* out, uint32_t capacity, uint32_t* joint_count) {
    if (!s || !out) return RT_ERR_INVALID_ARG;
    return guarded(s, [&] {
        const Mesh* mesh = mesh_at(s, mesh_index);
        if (!mesh || (!mesh->skin && !mesh->usd_skel)) { s->err = "mesh is not skinned"; return RT_ERR_INVALID_ARG; }
        std::vector<M4> jm;
        if (mesh->usd_skel) usd_joint_matrices(*mesh, time_seconds, jm);
        else skin_joint_matrices(*mesh->skin, time_seconds, jm);
        if (capacity < jm.size()) return RT_ERR_INVALID_ARG;
        for (size_t j = 0; j < jm.size(); ++j) std::memcpy(out + 16 * j, jm[j].m, sizeof jm[j].m);
        if (joint_count) *joint_count = (uint32_t)jm.size();
        return RT_OK;
    });
}

void rt_camera_orbit(int32_t width, int32_t height, const float target[3], float azimuth,
                     float elevation, float distance, float fov_degrees, Camera* out) {
    // Scene.makeOrbitCamera (Scene.swift:126-159)
    float safe = std::max(0.001f, distance);
    float limit = 3.14159265358979323846f / 2.0f - 0.001f;
    float el = std::max(-limit, std::min(limit, elevation));
    float x = safe * cosf(el) * sinf(azimuth);
    float y = safe * sinf(el);
    float z = safe * cosf(el) * cosf(azimuth);
    float pos[3] = {target[0] + x, target[1] + y, target[2] + z};
    float fw[3] = {target[0] - pos[0], target[1] - pos[1], target[2] - pos[2]};
    float fl = std::sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]);
    for (float& v : fw) v /= fl;
    // right = normalize(cross(forward, worldUp(0,1,0)))
    float rt_[3] = {fw[1] * 0.0f - fw[2] * 1.0f, fw[2] * 0.0f - fw[0] * 0.0f, fw[0] * 1.0f - fw[1] * 0.0f};
    float rl = std::sqrt(rt_[0] * rt_[0] + rt_[1] * rt_[1] + rt_[2] * rt_[2]);
    if (rl < 0.0001f) { rt_[0] = 1; rt_[1] = 0; rt_[2] = 0; }
    else for (float& v : rt_) v /= rl;
    // up = normalize(cross(right, forward))
    float up[3] = {rt_[1] * fw[2] - rt_[2] * fw[1], rt_[2] * fw[0] - rt_[0] * fw[2], rt_[0] * fw[1] - rt_[1] * fw[0]};
    float ul = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
    for (float& v : up) v /= ul;
    float fov = fov_degrees * (3.14159265358979323846f / 180.0f);
    float aspect = (float)width / (float)height;
    float h = tanf(fov / 2.0f);
    float w = aspect * h;
    out->position = f3(pos[0], pos[1], pos[2]);
    out->right = f3(rt_[0] * w, rt_[1] * w, rt_[2] * w);
    out->up = f3(up[0] * h, up[1] * h, up[2] * h);
    out->forward = f3(fw[0], fw[1], fw[2]);
}

void rt_camera_default(int32_t width, int32_t height, Camera* out) {
    // Scene.setupCamera (Scene.swift:111-124): target 0, position (0, 1, 5.38), fov 45
    const float target[3] = {0, 0, 0};
    float off[3] = {0.0f, 1.0f, 5.38f};
    float dist = std::max(0.001f, std::sqrt(off[0] * off[0] + off[1] * off[1] + off[2] * off[2]));
    float az = atan2f(off[0], off[2]);
    float el = asinf(off[1] / dist);
    rt_camera_orbit(width, height, target, az, el, dist, 45.0f, out);
}

void rt_uniforms_default(int32_t width, int32_t height, int32_t light_count, Uniforms* u) {
    std::memset(u, 0, sizeof *u);
    u->width = width;
    u->height = height;
    u->blocksWide = (width + 15) / 16;
    u->frameIndex = 0;
    u->lightCount = light_count;
    u->samplesPerPixel = 2;
    u->maxBounces = 2;
    rt_camera_default(width, height, &u->camera);
    u->previousCamera = u->camera;
    u->debugTextureMode = 0;
    u->accumulationWeight = 0.9f;
    u->enableDenoiseGBuffer = 0;
    u->shadingMode = ShadingModePBR;
    u->enableMotionAdaptiveAccumulation = 1;
    u->motionAccumulationMinWeight = 0.1f;
    u->motionAccumulationLowThresholdPixels = 0.5f;
    u->motionAccumulationHighThresholdPixels = 4.0f;
    u->enableMotionAdaptiveSampling = 1;
    u->motionSamplingMaxExtraSamples = 2;
    u->motionSamplingLowThresholdPixels = 1.0f;
    u->motionSamplingHighThresholdPixels = 6.0f;
}

void rt_random_offsets(uint64_t seed, int32_t width, int32_t height, uint32_t* out) {
    uint64_t st = seed;
    size_t n = (size_t)width * (size_t)height;
    for (size_t i = 0; i < n; ++i) {
        uint64_t z = (st += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        out[i] = (uint32_t)(z % (1024u * 1024u));
    }
}

}  // extern "C"
