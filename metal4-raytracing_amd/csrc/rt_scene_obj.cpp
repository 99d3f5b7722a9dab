// rt_scene_obj.cpp — the OBJ / MTL reader of the host scene ingest (Model.swift:29-205, OBJ path).
//
// OBJ/MTL ingest restates the ModelIO conventions the reference relies on:
// one mesh per `o` object, one submesh per material (first-appearance order), one vertex per
// unique (v, vt, vn) tuple, fan triangulation of polygons, normals left zero when the file has
// no `vn` (Raytracing.metal:395-397 then falls back to -ray.direction), Kd->baseColor,
// Ks->specular, Ke->emission, Ni->refractionIndex (default 1), d->opacity (default 1, clamped),
// specularExponent left 0 (Material(material:) only reads it for a float3 property,
// SubMesh.swift:309-311).  ModelIO itself is unvendored: its exact triangulation/dedup order
// is parity-unpinned and documented in DESIGN.md.
#include "rt_scene_model.h"

#include <cstdio>
#include <cstdlib>
#include <unordered_map>

namespace rt {

// MTL map statements -> texture slot (ModelIO's material semantics, SubMesh.swift:117-166)
static int map_slot(const char* key) {
    static const struct { const char* k; int slot; } kMaps[] = {
        {"map_Kd", 0}, {"norm", 1}, {"bump", 1}, {"map_Bump", 1}, {"map_bump", 1}, {"map_Pr", 2},
        {"map_Pm", 3}, {"map_Ke", 5}, {"map_d", 6}};
    for (const auto& m : kMaps)
        if (!std::strcmp(key, m.k)) return m.slot;
    return -1;
}

bool parse_mtl(const std::string& path, std::map<std::string, MtlEntry>& out) {
    const std::unique_ptr<FILE, int (*)(FILE*)> f(std::fopen(path.c_str(), "r"), std::fclose);   // closed on a throw too
    if (!f) return false;
    char line[4096];
    MtlEntry* ent = nullptr;
    while (std::fgets(line, sizeof line, f.get())) {
        char* p = line;
        while (*p == ' ' || *p == '\t') ++p;
        char key[64] = {0};
        int n = 0;
        if (std::sscanf(p, "%63s%n", key, &n) != 1) continue;
        const char* rest = p + n;
        if (!std::strcmp(key, "newmtl")) {
            char name[1024] = {0};
            std::sscanf(rest, " %1023[^\r\n]", name);
            out[name].material = default_material();
            ent = &out[name];
        } else if (ent) {
            Material* cur = &ent->material;
            const int slot = map_slot(key);
            if (slot >= 0) {   // the file name is the statement's last token (options come first)
                std::string r(rest);
                while (!r.empty() && (r.back() == '\n' || r.back() == '\r' || r.back() == ' ' || r.back() == '\t'))
                    r.pop_back();
                size_t sp = r.find_last_of(" \t");
                std::string file = sp == std::string::npos ? r : r.substr(sp + 1);
                if (!file.empty()) ent->maps[slot] = file[0] == '/' ? file : dir_of(path) + "/" + file;
                continue;
            }
            float a = 0, b = 0, c = 0;
            int k = std::sscanf(rest, "%f %f %f", &a, &b, &c);
            if (!std::strcmp(key, "Kd") && k >= 3) cur->baseColor = f3(a, b, c);
            else if (!std::strcmp(key, "Ks") && k >= 3) cur->specular = f3(a, b, c);
            else if (!std::strcmp(key, "Ke") && k >= 3) cur->emission = f3(a, b, c);
            else if (!std::strcmp(key, "Ni") && k >= 1) cur->refractionIndex = a;
            else if (!std::strcmp(key, "d") && k >= 1) cur->opacity = std::min(std::max(a, 0.0f), 1.0f);
            else if (!std::strcmp(key, "Tr") && k >= 1) cur->opacity = std::min(std::max(1.0f - a, 0.0f), 1.0f);
        }
    }
    return true;
}

// ---- OBJ -------------------------------------------------------------------------------------
struct ObjKey {
    int v, t, n;
    bool operator==(const ObjKey& o) const { return v == o.v && t == o.t && n == o.n; }
};
struct ObjKeyHash {
    size_t operator()(const ObjKey& k) const {
        return (size_t)k.v * 73856093u ^ (size_t)k.t * 19349663u ^ (size_t)k.n * 83492791u;
    }
};

static bool load_obj(const std::string& path, std::vector<Mesh>& meshes, std::string& err) {
    const std::unique_ptr<FILE, int (*)(FILE*)> f(std::fopen(path.c_str(), "r"), std::fclose);   // closed on a throw too
    if (!f) { err = "cannot open " + path; return false; }
    std::vector<float> V, VT, VN;
    std::map<std::string, MtlEntry> mtl;
    Mesh* mesh = nullptr;
    std::unordered_map<ObjKey, uint32_t, ObjKeyHash> dedup;
    std::map<std::string, size_t> sub_of;
    size_t cur_sub = (size_t)-1;
    std::string cur_mtl = "";
    auto start_mesh = [&](const std::string& name) {
        meshes.emplace_back();
        mesh = &meshes.back();
        mesh->name = name;
        mesh->transform = m4_identity();
        dedup.clear();
        sub_of.clear();
        cur_sub = (size_t)-1;
    };
    auto select_sub = [&]() {
        if (!mesh) start_mesh("default");
        auto it = sub_of.find(cur_mtl);
        if (it == sub_of.end()) {
            Submesh s;
            s.material_name = cur_mtl;
            auto mi = mtl.find(cur_mtl);
            s.material = (mi != mtl.end()) ? mi->second.material : default_material();
            if (mi != mtl.end())
                for (int k = 0; k < RT_TEXTURE_SLOTS; ++k) s.tex_path[k] = mi->second.maps[k];
            mesh->submeshes.push_back(s);
            cur_sub = mesh->submeshes.size() - 1;
            sub_of[cur_mtl] = cur_sub;
        } else {
            cur_sub = it->second;
        }
    };
    char line[1 << 14];
    std::vector<uint32_t> poly;
    while (std::fgets(line, sizeof line, f.get())) {
        char* p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (p[0] == 'v' && p[1] == ' ') {
            float x = 0, y = 0, z = 0;
            std::sscanf(p + 2, "%f %f %f", &x, &y, &z);
            V.push_back(x); V.push_back(y); V.push_back(z);
        } else if (p[0] == 'v' && p[1] == 't') {
            float x = 0, y = 0;
            std::sscanf(p + 2, "%f %f", &x, &y);
            VT.push_back(x); VT.push_back(y);
        } else if (p[0] == 'v' && p[1] == 'n') {
            float x = 0, y = 0, z = 0;
            std::sscanf(p + 2, "%f %f %f", &x, &y, &z);
            VN.push_back(x); VN.push_back(y); VN.push_back(z);
        } else if (p[0] == 'o' && (p[1] == ' ' || p[1] == '\t')) {
            char name[1024] = {0};
            std::sscanf(p + 1, " %1023[^\r\n]", name);
            start_mesh(name);
        } else if (!std::strncmp(p, "mtllib", 6)) {
            char name[1024] = {0};
            std::sscanf(p + 6, " %1023[^\r\n]", name);
            parse_mtl(dir_of(path) + "/" + name, mtl);
        } else if (!std::strncmp(p, "usemtl", 6)) {
            char name[1024] = {0};
            std::sscanf(p + 6, " %1023[^\r\n]", name);
            cur_mtl = name;
            cur_sub = (size_t)-1;
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            if (!mesh) start_mesh("default");
            if (cur_sub == (size_t)-1) select_sub();
            poly.clear();
            char* q = p + 1;
            while (*q) {
                while (*q == ' ' || *q == '\t') ++q;
                if (!*q || *q == '\n' || *q == '\r') break;
                int vi = 0, ti = 0, ni = 0;
                vi = (int)std::strtol(q, &q, 10);
                if (*q == '/') {
                    ++q;
                    if (*q != '/') ti = (int)std::strtol(q, &q, 10);
                    if (*q == '/') { ++q; ni = (int)std::strtol(q, &q, 10); }
                }
                while (*q && *q != ' ' && *q != '\t' && *q != '\n' && *q != '\r') ++q;
                int nv = (int)V.size() / 3, nt = (int)VT.size() / 2, nn = (int)VN.size() / 3;
                if (vi < 0) vi = nv + vi + 1;
                if (ti < 0) ti = nt + ti + 1;
                if (ni < 0) ni = nn + ni + 1;
                if (vi <= 0 || vi > nv || ti > nt || ni > nn) { err = "bad face index in " + path; return false; }
                ObjKey key{vi, ti, ni};
                auto it = dedup.find(key);
                uint32_t idx;
                if (it == dedup.end()) {
                    idx = (uint32_t)mesh->positions.size();
                    dedup.emplace(key, idx);
                    mesh->positions.push_back(f3(V[3 * (vi - 1)], V[3 * (vi - 1) + 1], V[3 * (vi - 1) + 2]));
                    mesh->normals.push_back(ni > 0 ? f3(VN[3 * (ni - 1)], VN[3 * (ni - 1) + 1], VN[3 * (ni - 1) + 2]) : f3(0, 0, 0));
                    rt_float2 uv; uv.x = 0; uv.y = 0;
                    if (ti > 0) { uv.x = VT[2 * (ti - 1)]; uv.y = VT[2 * (ti - 1) + 1]; mesh->has_uvs = true; }
                    mesh->uvs.push_back(uv);
                } else {
                    idx = it->second;
                }
                poly.push_back(idx);
            }
            auto& ind = mesh->submeshes[cur_sub].indices;
            for (size_t k = 2; k < poly.size(); ++k) {  // fan triangulation
                ind.push_back(poly[0]); ind.push_back(poly[k - 1]); ind.push_back(poly[k]);
            }
        }
    }
    // drop empty submeshes / meshes
    for (auto& m : meshes) {
        std::vector<Submesh> keep;
        for (auto& s : m.submeshes) if (!s.indices.empty()) keep.push_back(std::move(s));
        m.submeshes.swap(keep);
    }
    std::vector<Mesh> keepm;
    for (auto& m : meshes) if (!m.submeshes.empty()) keepm.push_back(std::move(m));
    meshes.swap(keepm);
    if (meshes.empty()) { err = "no faces in " + path; return false; }
    return true;
}

rt_status add_obj_impl(rt_scene* s, const char* obj_path, const float position[3], const float rotation[3], float scale,
                       const rt_material_override* ov) {
    Model model = new_model(obj_path, position, rotation, scale);
    std::string err;
    if (!load_obj(obj_path, model.meshes, err)) { s->err = err; return RT_ERR_IO; }
    for (auto& m : model.meshes)   // MTL maps; one that fails to load stays unbound (SubMesh.swift:100-107)
        for (auto& sm : m.submeshes)
            for (int k = 0; k < RT_TEXTURE_SLOTS; ++k) {
                uint32_t id;
                if (!sm.tex_path[k].empty() && s->texture_from_file(sm.tex_path[k], &id) == RT_OK) bind_slot(sm, k, id);
            }
    s->err.clear();
    finish_model(s, std::move(model), ov);
    return RT_OK;
}

}  // namespace rt
