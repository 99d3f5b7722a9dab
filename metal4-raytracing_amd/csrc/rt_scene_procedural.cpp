// rt_scene_procedural.cpp — stand-ins for assets the tree does not carry: dragon, bunny, skinned robot.
#include "rt_scene_model.h"

namespace rt {

void compute_vertex_normals(Mesh& m) {
    std::vector<double> acc(m.positions.size() * 3, 0.0);
    for (auto& s : m.submeshes)
        for (size_t t = 0; t + 2 < s.indices.size(); t += 3) {
            const rt_float3& a = m.positions[s.indices[t]];
            const rt_float3& b = m.positions[s.indices[t + 1]];
            const rt_float3& c = m.positions[s.indices[t + 2]];
            double e1[3] = {(double)b.x - a.x, (double)b.y - a.y, (double)b.z - a.z};
            double e2[3] = {(double)c.x - a.x, (double)c.y - a.y, (double)c.z - a.z};
            double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < 3; ++j) acc[3 * s.indices[t + k] + j] += n[j];
        }
    m.normals.resize(m.positions.size());
    for (size_t i = 0; i < m.positions.size(); ++i) {
        double* n = &acc[3 * i];
        double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (l > 0) m.normals[i] = f3((float)(n[0] / l), (float)(n[1] / l), (float)(n[2] / l));
        else m.normals[i] = f3(0, 0, 0);
    }
}

// Fit positions into the box [-h, h] per axis (centred), preserving nothing else.
static void fit_box(Mesh& m, const double half[3]) {
    double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
    for (auto& p : m.positions) {
        double v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], v[k]); hi[k] = std::max(hi[k], v[k]); }
    }
    for (auto& p : m.positions) {
        double v[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; ++k) {
            double c = 0.5 * (lo[k] + hi[k]), e = 0.5 * (hi[k] - lo[k]);
            v[k] = (v[k] - c) / e * half[k];
        }
        p = f3((float)v[0], (float)v[1], (float)v[2]);
    }
}

// Closed tube of U x V quads around a (2,3) torus knot with bumps: 2*U*V triangles.
// dragon: U=10627, V=41 -> 871,414 triangles, the triangle count of the Stanford dragon
// asset named by BASELINE.json; bounds ~ (0.45, 0.317, 0.2) half-extents so that at the
// AppScene transform (scale 1.2 at y=0.38, AppScene.swift:16-21) it rests on the floor.
static Mesh make_knot(const char* name, int U, int V, double tube, double bump, const double half[3]) {
    Mesh m;
    m.name = name;
    m.transform = m4_identity();
    m.positions.reserve((size_t)U * V);
    const double TWO_PI = 6.283185307179586;
    for (int i = 0; i < U; ++i) {
        double t = TWO_PI * i / U;
        // trefoil knot and its derivative
        double cx = std::sin(t) + 2.0 * std::sin(2 * t), cy = std::cos(t) - 2.0 * std::cos(2 * t), cz = -std::sin(3 * t);
        double dx = std::cos(t) + 4.0 * std::cos(2 * t), dy = -std::sin(t) + 4.0 * std::sin(2 * t), dz = -3.0 * std::cos(3 * t);
        double dl = std::sqrt(dx * dx + dy * dy + dz * dz);
        dx /= dl; dy /= dl; dz /= dl;
        // B = normalize(T x Z), N = B x T
        double bx = dy * 1.0 - dz * 0.0, by = dz * 0.0 - dx * 1.0, bz = 0.0;
        double bl = std::sqrt(bx * bx + by * by + bz * bz);
        bx /= bl; by /= bl; bz /= bl;
        double nx = by * dz - bz * dy, ny = bz * dx - bx * dz, nz = bx * dy - by * dx;
        for (int j = 0; j < V; ++j) {
            double ph = TWO_PI * j / V;
            double r = tube * (1.0 + bump * std::sin(13.0 * t + 3.0 * ph) * std::cos(7.0 * t - 2.0 * ph)
                               + 0.5 * bump * std::sin(57.0 * t + 5.0 * ph));
            double px = cx + r * (std::cos(ph) * nx + std::sin(ph) * bx);
            double py = cy + r * (std::cos(ph) * ny + std::sin(ph) * by);
            double pz = cz + r * (std::cos(ph) * nz + std::sin(ph) * bz);
            m.positions.push_back(f3((float)px, (float)py, (float)pz));
        }
    }
    Submesh s;
    s.indices.reserve((size_t)U * V * 6);
    for (int i = 0; i < U; ++i) {
        int i1 = (i + 1) % U;
        for (int j = 0; j < V; ++j) {
            int j1 = (j + 1) % V;
            uint32_t a = i * V + j, b = i1 * V + j, c = i1 * V + j1, d = i * V + j1;
            s.indices.push_back(a); s.indices.push_back(c); s.indices.push_back(b);   // outward winding
            s.indices.push_back(a); s.indices.push_back(d); s.indices.push_back(c);
        }
    }
    s.material = default_material();
    m.submeshes.push_back(std::move(s));
    fit_box(m, half);
    compute_vertex_normals(m);
    m.uvs.assign(m.positions.size(), rt_float2{0.0f, 0.0f});
    return m;
}

// Append a closed "swept" surface (UV-sphere topology, poles at both ends) around a spine:
// 2 * U * (R - 1) triangles.  point(s, phi) = C(s) + r(s, phi) * (cos phi N + sin phi B).
template <class Spine, class Radius>
static void append_swept(Mesh& m, int U, int R, Spine spine, Radius radius) {
    const double PI = 3.141592653589793;
    uint32_t base = (uint32_t)m.positions.size();
    double c[3], t[3];
    auto frame = [&](double s, double* C, double* N, double* B) {
        double h = 1e-4, a[3], b[3];
        spine(s, C);
        spine(std::min(1.0, s + h), a);
        spine(std::max(0.0, s - h), b);
        double T[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
        double tl = std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
        for (double& v : T) v /= tl;
        B[0] = T[1]; B[1] = -T[0]; B[2] = 0.0;  // T x Z
        double bl = std::sqrt(B[0] * B[0] + B[1] * B[1]);
        B[0] /= bl; B[1] /= bl;
        N[0] = B[1] * T[2] - B[2] * T[1];
        N[1] = B[2] * T[0] - B[0] * T[2];
        N[2] = B[0] * T[1] - B[1] * T[0];
    };
    spine(0.0, c);
    m.positions.push_back(f3((float)c[0], (float)c[1], (float)c[2]));
    for (int r = 1; r < R; ++r) {
        double s = (double)r / R, C[3], N[3], B[3];
        frame(s, C, N, B);
        for (int u = 0; u < U; ++u) {
            double ph = 2 * PI * u / U;
            double rr = radius(s, ph);
            m.positions.push_back(f3((float)(C[0] + rr * (std::cos(ph) * N[0] + std::sin(ph) * B[0])),
                                     (float)(C[1] + rr * (std::cos(ph) * N[1] + std::sin(ph) * B[1])),
                                     (float)(C[2] + rr * (std::cos(ph) * N[2] + std::sin(ph) * B[2]))));
        }
    }
    spine(1.0, t);
    m.positions.push_back(f3((float)t[0], (float)t[1], (float)t[2]));
    uint32_t south = (uint32_t)m.positions.size() - 1;
    auto& ind = m.submeshes[0].indices;
    auto ring = [&](int r, int u) -> uint32_t { return base + 1 + (uint32_t)((r - 1) * U + (u % U)); };
    for (int u = 0; u < U; ++u) { ind.push_back(base); ind.push_back(ring(1, u + 1)); ind.push_back(ring(1, u)); }
    for (int r = 1; r < R - 1; ++r)
        for (int u = 0; u < U; ++u) {
            uint32_t a = ring(r, u), b = ring(r, u + 1), cc = ring(r + 1, u + 1), d = ring(r + 1, u);
            ind.push_back(a); ind.push_back(b); ind.push_back(cc);
            ind.push_back(a); ind.push_back(cc); ind.push_back(d);
        }
    for (int u = 0; u < U; ++u) { ind.push_back(south); ind.push_back(ring(R - 1, u)); ind.push_back(ring(R - 1, u + 1)); }
}

// Dragon stand-in: one closed, compact, detailed surface like the Stanford dragon — a curved
// body swept along an S-shaped spine (thick middle, head bulge, thin tail) with scale-like
// displacement, plus four legs.  Exactly 871,414 triangles (body 2*560*740 + legs
// 3*(2*64*83) + 2*41*131); half-extents (0.45, 0.3166, 0.2) so that at the AppScene transform
// (scale 1.2 at y = 0.38, AppScene.swift:16-21) it rests on the floor.
static Mesh make_dragon(const double half[3]) {
    Mesh m;
    m.name = "dragon";
    m.transform = m4_identity();
    m.submeshes.emplace_back();
    m.submeshes[0].material = default_material();
    const double PI = 3.141592653589793;
    auto body_spine = [&](double s, double* C) {
        C[0] = 2.2 * (s - 0.5);
        C[1] = 0.30 * std::sin(2 * PI * s + 0.6) + 0.25 * s;
        C[2] = 0.22 * std::sin(PI * s) * std::sin(3 * PI * s);
    };
    auto body_r = [&](double s, double ph) {
        double r = 0.34 * std::pow(std::sin(PI * s), 0.65) * (1.0 + 0.35 * std::exp(-60.0 * (s - 0.86) * (s - 0.86)));
        r *= 1.0 + 0.05 * std::sin(90.0 * s + 7.0 * ph) * std::sin(11.0 * ph) + 0.025 * std::sin(310.0 * s) * std::cos(23.0 * ph);
        return r;
    };
    append_swept(m, 560, 741, body_spine, body_r);
    struct Leg { double s, side; int U, R; };
    const Leg legs[4] = {{0.32, 1.0, 64, 84}, {0.32, -1.0, 64, 84}, {0.66, 1.0, 64, 84}, {0.66, -1.0, 41, 132}};
    for (const Leg& L : legs) {
        double C0[3];
        body_spine(L.s, C0);
        auto leg_spine = [&](double s, double* C) {
            C[0] = C0[0] + 0.08 * s;
            C[1] = C0[1] - 0.62 * s;
            C[2] = C0[2] + L.side * (0.10 + 0.12 * s);
        };
        auto leg_r = [&](double s, double ph) {
            return 0.075 * std::pow(std::sin(PI * s), 0.5) * (1.0 + 0.04 * std::sin(40.0 * s + 5.0 * ph));
        };
        append_swept(m, L.U, L.R, leg_spine, leg_r);
    }
    fit_box(m, half);
    compute_vertex_normals(m);
    m.uvs.assign(m.positions.size(), rt_float2{0.0f, 0.0f});
    return m;
}

// Lumpy UV sphere: 2*U*(R-1) triangles (bunny stand-in: U=463, R=76 -> 69,450 triangles).
static Mesh make_blob(const char* name, int U, int R, const double half[3]) {
    Mesh m;
    m.name = name;
    m.transform = m4_identity();
    const double PI = 3.141592653589793;
    // rings 1..R-1 plus two poles
    m.positions.push_back(f3(0, 1, 0));
    for (int r = 1; r < R; ++r) {
        double th = PI * r / R;
        for (int u = 0; u < U; ++u) {
            double ph = 2 * PI * u / U;
            double rad = 1.0 + 0.18 * std::sin(3 * th) * std::cos(2 * ph) + 0.07 * std::sin(11 * th + 5 * ph)
                         + (th < 0.9 ? 0.35 * std::exp(-20.0 * std::pow(std::sin(ph) - 0.6, 2)) * (0.9 - th) : 0.0);
            m.positions.push_back(f3((float)(rad * std::sin(th) * std::cos(ph)), (float)(rad * std::cos(th)),
                                     (float)(rad * std::sin(th) * std::sin(ph))));
        }
    }
    m.positions.push_back(f3(0, -1, 0));
    uint32_t south = (uint32_t)m.positions.size() - 1;
    Submesh s;
    auto ring = [&](int r, int u) -> uint32_t { return 1 + (uint32_t)((r - 1) * U + (u % U)); };
    for (int u = 0; u < U; ++u) { s.indices.push_back(0); s.indices.push_back(ring(1, u + 1)); s.indices.push_back(ring(1, u)); }
    for (int r = 1; r < R - 1; ++r)
        for (int u = 0; u < U; ++u) {
            uint32_t a = ring(r, u), b = ring(r, u + 1), c = ring(r + 1, u + 1), d = ring(r + 1, u);
            s.indices.push_back(a); s.indices.push_back(b); s.indices.push_back(c);
            s.indices.push_back(a); s.indices.push_back(c); s.indices.push_back(d);
        }
    for (int u = 0; u < U; ++u) { s.indices.push_back(south); s.indices.push_back(ring(R - 1, u)); s.indices.push_back(ring(R - 1, u + 1)); }
    s.material = default_material();
    s.material.baseColor = f3(0.8f, 0.8f, 0.8f);
    m.submeshes.push_back(std::move(s));
    fit_box(m, half);
    compute_vertex_normals(m);
    m.uvs.assign(m.positions.size(), rt_float2{0.0f, 0.0f});
    return m;
}

// Skinned robot stand-in (config 5): a segmented capsule "arm" of J joints along +Y whose
// joints bend about Z over time.  4 joint influences per vertex (Model.swift:304-341 streams).
static Mesh make_robot(int J, int rings_per_joint, int U) {
    Mesh m;
    m.name = "robot";
    m.transform = m4_identity();
    const double PI = 3.141592653589793;
    const double seg = 0.6, radius = 0.18;
    int R = J * rings_per_joint + 1;
    for (int r = 0; r < R; ++r) {
        double y = seg * J * r / (R - 1);
        double rad = radius * (0.75 + 0.25 * std::cos(2 * PI * r / rings_per_joint));
        double jf = y / seg;  // joint coordinate
        int j0 = std::min((int)std::floor(jf - 0.5), J - 1);
        for (int u = 0; u < U; ++u) {
            double ph = 2 * PI * u / U;
            m.positions.push_back(f3((float)(rad * std::cos(ph)), (float)y, (float)(rad * std::sin(ph))));
            // weights: blend between joint j0 and j0+1 around the joint boundary
            uint16_t ji[4] = {0, 0, 0, 0};
            float w[4] = {1, 0, 0, 0};
            if (j0 < 0) { ji[0] = 0; }
            else if (j0 >= J - 1) { ji[0] = (uint16_t)(J - 1); }
            else {
                double t = jf - (j0 + 0.5);
                ji[0] = (uint16_t)j0; ji[1] = (uint16_t)(j0 + 1);
                w[0] = (float)(1.0 - t); w[1] = (float)t;
            }
            for (int k = 0; k < 4; ++k) { m.joint_indices.push_back(ji[k]); m.joint_weights.push_back(w[k]); }
        }
    }
    Submesh s;
    for (int r = 0; r + 1 < R; ++r)
        for (int u = 0; u < U; ++u) {
            uint32_t a = r * U + u, b = r * U + (u + 1) % U, c = (r + 1) * U + (u + 1) % U, d = (r + 1) * U + u;
            s.indices.push_back(a); s.indices.push_back(c); s.indices.push_back(b);
            s.indices.push_back(a); s.indices.push_back(d); s.indices.push_back(c);
        }
    s.material = default_material();
    s.material.baseColor = f3(0.7f, 0.72f, 0.75f);
    m.submeshes.push_back(std::move(s));
    compute_vertex_normals(m);
    m.uvs.assign(m.positions.size(), rt_float2{0.0f, 0.0f});
    m.joint_count = (uint32_t)J;
    auto skin = std::make_shared<Skin>();
    for (int j = 0; j < J; ++j) {
        skin->parent.push_back(j - 1);
        float t[3] = {0.0f, j == 0 ? 0.0f : (float)seg, 0.0f};
        skin->rest_local.push_back(m4_translate(t));
    }
    // global bind = chain of rest locals; inverse bind = translate(-y)
    for (int j = 0; j < J; ++j) {
        float t[3] = {0.0f, -(float)(seg * j), 0.0f};
        skin->inverse_bind.push_back(m4_translate(t));
    }
    m.skin = skin;
    return m;
}

rt_status add_procedural_impl(rt_scene* s, const char* kind, const char* mtl_path, const float position[3],
                              const float rotation[3], float scale, const rt_material_override* ov) {
    Model model = new_model(kind, position, rotation, scale);
    std::string k = kind;
    if (k == "dragon" || k == "knot") {
        const double half[3] = {0.45, 0.3166, 0.2};
        // "knot": the thin-tube torus-knot variant kept as a traversal torture test (rays refracted
        // inside a long thin glass tube visit ~1000 boxes each)
        Mesh m = k == "dragon" ? make_dragon(half) : make_knot("knot", 10627, 41, 0.42, 0.12, half);
        // dragon.mtl: Kd 1 0 0, Ks .2, Ke 0, Ni 1, d 1 (AssetResources/dragon.mtl)
        m.submeshes[0].material.baseColor = f3(1.0f, 0.0f, 0.0f);
        m.submeshes[0].material.specular = f3(0.2f, 0.2f, 0.2f);
        model.meshes.push_back(std::move(m));
    } else if (k == "bunny") {
        const double half[3] = {0.40, 0.3166, 0.32};
        model.meshes.push_back(make_blob("bunny", 463, 76, half));
    } else if (k == "robot") {
        // height 3.0 units at scale 1 -> at the AppScene robot slot use scale ~0.5.
        model.meshes.push_back(make_robot(5, 24, 96));
    } else {
        s->err = "unknown procedural kind " + k;
        return RT_ERR_INVALID_ARG;
    }
    if (mtl_path) {
        std::map<std::string, MtlEntry> mtl;
        if (!parse_mtl(mtl_path, mtl) || mtl.empty()) { s->err = std::string("cannot read ") + mtl_path; return RT_ERR_IO; }
        model.meshes[0].submeshes[0].material = mtl.begin()->second.material;
    }
    finish_model(s, std::move(model), ov);
    return RT_OK;
}

// Model.update + SkinningPass.updateSkinningJointMatrices for the synthetic skeleton
void skin_joint_matrices(const Skin& sk, double time_seconds, std::vector<M4>& out) {
    const uint32_t J = (uint32_t)sk.parent.size();
    // Model.update: local = rest * animated rotation; global via parents; joint = global * invBind
    double t = std::fmod(time_seconds, sk.duration);
    std::vector<M4> global(J);
    for (uint32_t j = 0; j < J; ++j) {
        float ang = (float)(0.35 * std::sin(6.283185307179586 * t / sk.duration + 0.9 * j) * (j == 0 ? 0.3 : 1.0));
        M4 local = m4_mul(sk.rest_local[j], m4_rotate_axis(ang, 0, 0, 1));
        global[j] = sk.parent[j] >= 0 ? m4_mul(global[sk.parent[j]], local) : local;
    }
    // SkinningPass.updateSkinningJointMatrices: geomBind^-1 * (global*invBind) * geomBind, geomBind = I
    out.resize(J);
    for (uint32_t j = 0; j < J; ++j) out[j] = m4_mul(global[j], sk.inverse_bind[j]);
}

}  // namespace rt
