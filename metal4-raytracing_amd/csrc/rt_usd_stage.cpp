// rt_usd_stage.cpp — shared by the USD readers: Stage methods, number helpers, dispatch by content.
#include "rt_usd_internal.h"

#include <cstring>

namespace rt {
namespace usd {

Stage::Stage() {
    Prim root;
    root.name = "";
    root.path = "/";
    prims.push_back(root);
    by_path["/"] = 0;
}

int Stage::add_prim(int parent, const std::string& name) {
    const std::string& pp = prims[parent].path;
    std::string path = pp == "/" ? "/" + name : pp + "/" + name;
    auto it = by_path.find(path);
    if (it != by_path.end()) return it->second;
    Prim p;
    p.name = name;
    p.path = path;
    p.parent = parent;
    prims.push_back(p);
    const int id = (int)prims.size() - 1;
    prims[parent].children.push_back(id);
    by_path[path] = id;
    return id;
}

int Stage::add_detached(const std::string& path) {
    auto it = by_path.find(path);
    if (it != by_path.end()) return it->second;
    Prim p;
    const size_t k = path.find_last_of('/');
    p.name = k == std::string::npos ? path : path.substr(k + 1);
    p.path = path;
    prims.push_back(p);
    const int id = (int)prims.size() - 1;
    by_path[path] = id;
    return id;
}

// primvar elementSize from a file number (1 when absent, NaN or out of range)
int element_size(double d) { return d >= 1.0 && d <= 65536.0 ? (int)d : 1; }

std::vector<int> Stage::preorder(int root, bool active_only) const {
    std::vector<int> out, todo{root};
    std::vector<char> seen(prims.size(), 0);
    while (!todo.empty()) {
        const int k = todo.back();
        todo.pop_back();
        if (k < 0 || (size_t)k >= prims.size() || seen[k]) continue;
        seen[k] = 1;
        if (active_only && !prims[k].active) continue;
        out.push_back(k);
        const std::vector<int>& ch = prims[k].children;
        for (size_t i = ch.size(); i-- > 0;) todo.push_back(ch[i]);
    }
    return out;
}

float half_to_float(uint16_t h) {
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t bits;
    if (e == 0) {
        if (m == 0) {
            bits = s;
        } else {   // subnormal: renormalise
            int k = 0;
            uint32_t mm = m;
            while (!(mm & 0x400u)) { mm <<= 1; ++k; }
            bits = s | ((uint32_t)(127 - 15 - k + 1) << 23) | ((mm & 0x3ffu) << 13);
        }
    } else if (e == 31) {
        bits = s | 0x7f800000u | (m << 13);
    } else {
        bits = s | ((e - 15 + 127) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

bool parse_layer(const uint8_t* data, size_t n, Stage& st, std::string& err) {
    if (n >= 8 && !std::memcmp(data, "PXR-USDC", 8)) return parse_usdc(data, n, st, err);
    if (n >= 5 && !std::memcmp(data, "#usda", 5)) return parse_usda((const char*)data, n, st, err);
    err = "not a USD layer (neither PXR-USDC nor #usda)";
    return false;
}

}  // namespace usd
}  // namespace rt
