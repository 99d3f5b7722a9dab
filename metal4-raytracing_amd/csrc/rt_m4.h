// rt_m4.h — column-major float4x4 helpers of the host ingest (Utilities.swift:302-355), header-only.
#pragma once
#include "../../include/rt_scene.h"

#include <cmath>
#include <vector>

namespace rt {

struct M4 { float m[16]; };  // m[col*4 + row]

inline M4 m4_identity() { M4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0f; return r; }
inline M4 m4_mul(const M4& a, const M4& b) {
    M4 r{};
    for (int c = 0; c < 4; ++c)
        for (int rr = 0; rr < 4; ++rr) {
            float s = 0.0f;
            for (int k = 0; k < 4; ++k) s = s + a.m[k * 4 + rr] * b.m[c * 4 + k];
            r.m[c * 4 + rr] = s;
        }
    return r;
}
inline M4 m4_translate(const float t[3]) { M4 r = m4_identity(); r.m[12] = t[0]; r.m[13] = t[1]; r.m[14] = t[2]; return r; }
inline M4 m4_scale(float s) { M4 r = m4_identity(); r.m[0] = s; r.m[5] = s; r.m[10] = s; return r; }
// matrix_float4x4.rotate(radians:axis:) (Utilities.swift:318-331)
inline M4 m4_rotate_axis(float radians, float ax, float ay, float az) {
    float len = std::sqrt(ax * ax + ay * ay + az * az);
    float x = ax / len, y = ay / len, z = az / len;
    float ct = cosf(radians), st = sinf(radians), ci = 1.0f - ct;
    M4 r{};
    r.m[0] = ct + x * x * ci;     r.m[1] = y * x * ci + z * st; r.m[2] = z * x * ci - y * st;  r.m[3] = 0;
    r.m[4] = x * y * ci - z * st; r.m[5] = ct + y * y * ci;     r.m[6] = z * y * ci + x * st;  r.m[7] = 0;
    r.m[8] = x * z * ci + y * st; r.m[9] = y * z * ci - x * st; r.m[10] = ct + z * z * ci;     r.m[11] = 0;
    r.m[12] = 0; r.m[13] = 0; r.m[14] = 0; r.m[15] = 1;
    return r;
}
// rotate(r) = rotateX(r.x) * rotateY(r.y) * rotateZ(r.z) (Utilities.swift:345-347)
inline M4 m4_rotate(const float r[3]) {
    return m4_mul(m4_mul(m4_rotate_axis(r[0], 1, 0, 0), m4_rotate_axis(r[1], 0, 1, 0)), m4_rotate_axis(r[2], 0, 0, 1));
}
// worldTransform = T * R * S (Model.swift:55-58, Mesh.swift:61-66)
inline M4 model_transform(const float pos[3], const float rot[3], float scale) {
    return m4_mul(m4_mul(m4_translate(pos), m4_rotate(rot)), m4_scale(scale));
}
inline rt_packed_float4x3 pack4x3(const M4& a) {  // Renderer.swift:1393-1401
    rt_packed_float4x3 p;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) p.columns[c][r] = a.m[c * 4 + r];
    return p;
}

// simd_inverse (Model.swift:361): general 4x4 inverse (cofactors in double, rounded once)
inline M4 m4_inverse(const M4& a) {
    double m[16], inv[16];
    for (int i = 0; i < 16; ++i) m[i] = a.m[i];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    M4 r = m4_identity();
    if (det == 0.0) return r;
    for (int i = 0; i < 16; ++i) r.m[i] = (float)(inv[i] / det);
    return r;
}

// a USD matrix4d (row-vector convention, translation in the last row) is the simd float4x4 whose
// columns are its rows (ModelIO's conversion)
inline M4 m4_from_usd(const std::vector<double>& v, size_t off) {
    M4 r;
    for (int i = 0; i < 16; ++i) r.m[i] = (float)v[off + i];
    return r;
}

// matrix_float4x4(simd_quatf) and matrix4x4_trs (Model.swift:496-501): T * R(q) * S
inline M4 m4_quat(const float q[4]) {   // q = (x, y, z, w)
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    M4 r = m4_identity();
    r.m[0] = w * w + x * x - y * y - z * z;
    r.m[1] = 2.0f * (x * y + z * w);
    r.m[2] = 2.0f * (x * z - y * w);
    r.m[4] = 2.0f * (x * y - z * w);
    r.m[5] = w * w - x * x + y * y - z * z;
    r.m[6] = 2.0f * (y * z + x * w);
    r.m[8] = 2.0f * (z * x + y * w);
    r.m[9] = 2.0f * (y * z - x * w);
    r.m[10] = w * w - x * x - y * y + z * z;
    return r;
}
inline M4 m4_trs(const float* t, const float* q, const float* sc) {
    M4 S = m4_identity();
    S.m[0] = sc[0];
    S.m[5] = sc[1];
    S.m[10] = sc[2];
    return m4_mul(m4_mul(m4_translate(t), m4_quat(q)), S);
}

}  // namespace rt
