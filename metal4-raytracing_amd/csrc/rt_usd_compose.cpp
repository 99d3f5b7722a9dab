// rt_usd_compose.cpp — composition of the layers the readers return, and load_stage (see rt_usd.h).
#include "rt_usd_internal.h"

#include <algorithm>
#include <memory>
#include <set>

namespace rt {
namespace usd {

namespace {

constexpr int kMaxArcDepth = 16;              // nested layer loads (sublayer / reference chains)
constexpr size_t kMaxComposedPrims = 1u << 17;  // prims a composition may create (hostile fan-out)
constexpr uint64_t kMaxLayerBytes = 1ull << 31;   // a referenced layer file (regular files only)
constexpr uint64_t kMaxComposedBytes = 4ull << 30;   // attribute data merges may copy (hostile fan-out)

std::string dir_of(const std::string& id) {
    const size_t k = id.find_last_of('/');
    return k == std::string::npos ? std::string() : id.substr(0, k + 1);
}
// collapses "." and ".." segments (a leading "/" is kept)
std::string normalize(const std::string& p) {
    std::vector<std::string> seg;
    size_t b = 0;
    while (b <= p.size()) {
        size_t e = p.find('/', b);
        if (e == std::string::npos) e = p.size();
        const std::string x = p.substr(b, e - b);
        if (x == "..") { if (!seg.empty() && seg.back() != "..") seg.pop_back(); else seg.push_back(x); }
        else if (!x.empty() && x != ".") seg.push_back(x);
        b = e + 1;
    }
    std::string out = !p.empty() && p[0] == '/' ? "/" : "";
    for (size_t k = 0; k < seg.size(); ++k) out += (k ? "/" : "") + seg[k];
    return out;
}
// a path of the source subtree rooted at `from`, moved under `to`
std::string remap(const std::string& x, const std::string& from, const std::string& to) {
    if (from.empty() || from == to || x.compare(0, from.size(), from) != 0) return x;
    if (x.size() > from.size() && x[from.size()] != '/' && x[from.size()] != '.') return x;
    return to + x.substr(from.size());
}

class Composer {
public:
    explicit Composer(const std::vector<PackageFile>* pkg) : pkg_(pkg) {}
    std::string err;

    // layer `id` parsed and composed; shared by every arc that names it (no copy per arc)
    std::shared_ptr<const Stage> load(const std::string& id, int depth) {
        if (depth > kMaxArcDepth) {
            fail("composition nested deeper than " + std::to_string(kMaxArcDepth) + " layers");
            return nullptr;
        }
        auto c = cache_.find(id);
        if (c != cache_.end()) return c->second;
        if (loading_.count(id)) {
            fail("composition cycle through " + id);
            return nullptr;
        }
        std::vector<uint8_t> data;
        if (!read(id, data)) {
            fail("cannot open layer " + id);
            return nullptr;
        }
        auto L = std::make_shared<Stage>();
        L->layer_id = id;
        std::string e;
        if (!parse_layer(data.data(), data.size(), *L, e)) {
            fail(id + ": " + e);
            return nullptr;
        }
        loading_.insert(id);
        const bool ok = compose(id, *L, depth);
        loading_.erase(id);
        if (!ok) return nullptr;
        cache_[id] = L;
        return L;
    }

    // sublayers under the layer's own opinions, then every prim's arcs in namespace order.  Variant
    // selections are composed in the root layer (depth 0) only: a sublayer or referenced layer keeps
    // its selections and variant bodies unapplied, so the strongest selection of the whole stack
    // (the root's own, then its sublayers', then the referenced layers') picks the variant.
    bool compose(const std::string& id, Stage& L, int depth) {
        L.layer_id = id;
        const std::vector<std::string> subs = L.sublayers;
        L.sublayers.clear();
        for (const std::string& sub : subs) {
            const std::shared_ptr<const Stage> S = load(resolve(id, sub), depth + 1);
            if (!S) return false;
            if (!merge(L, 0, *S, 0, "", "")) return false;
            if (L.default_prim.empty()) L.default_prim = S->default_prim;
        }
        std::vector<int> todo{0};
        std::vector<uint8_t> seen;   // each prim once, whatever its children lists say
        while (!todo.empty()) {
            const int p = todo.back();
            todo.pop_back();
            if ((size_t)p >= seen.size()) seen.resize(L.prims.size() + 1, 0);
            if (seen[p]) continue;
            seen[p] = 1;
            if (!apply_arcs(id, L, p, depth, depth == 0)) return false;
            const std::vector<int>& ch = L.prims[p].children;
            for (auto it = ch.rbegin(); it != ch.rend(); ++it) todo.push_back(*it);
        }
        return true;
    }

private:
    const std::vector<PackageFile>* pkg_;
    std::set<std::string> loading_;
    std::map<std::string, std::shared_ptr<const Stage>> cache_;
    size_t budget_ = kMaxComposedPrims;
    uint64_t bytes_budget_ = kMaxComposedBytes;

    bool fail(const std::string& m) {
        err = m;
        return false;
    }
    // composition work (prims merged, arcs applied, internal snapshots copied) is bounded: a
    // hostile list of a million arcs must fail fast, not merge a subtree a million times
    bool spend(size_t n) {
        if (n > budget_) return fail("composed stage larger than " + std::to_string(kMaxComposedPrims) + " prims");
        budget_ -= n;
        return true;
    }
    // and so are the attribute bytes merges copy: a few references to one large mesh layer must
    // not multiply its arrays into terabytes
    bool spend_bytes(uint64_t n) {
        if (n > bytes_budget_) return fail("composed attribute data larger than " + std::to_string(kMaxComposedBytes >> 20) + " MiB");
        bytes_budget_ -= n;
        return true;
    }
    static uint64_t value_bytes(const Value& v) {
        uint64_t b = 8 * (uint64_t)v.num.size() + 32;
        for (const std::string& s : v.str) b += s.size() + 32;
        return b;
    }
    static uint64_t attr_bytes(const Attr& a) {
        uint64_t b = value_bytes(a.value) + 8 * (uint64_t)a.times.size();
        for (const Value& v : a.samples) b += value_bytes(v);
        for (const std::string& s : a.connections) b += s.size() + 32;
        return b;
    }
    // what a copy of a whole stage copies (an internal arc's snapshot of its layer)
    static uint64_t stage_bytes(const Stage& L) {
        uint64_t b = 0;
        for (const Prim& pr : L.prims) {
            b += 256;
            for (const auto& kv : pr.attrs) b += attr_bytes(kv.second);
        }
        return b;
    }
    // an asset path relative to the layer naming it (inside the package for a .usdz)
    std::string resolve(const std::string& from, const std::string& asset) const {
        if (!asset.empty() && asset[0] == '/') return normalize(pkg_ ? asset.substr(1) : asset);
        return normalize(dir_of(from) + asset);
    }
    bool read(const std::string& id, std::vector<uint8_t>& data) const {
        std::string e;
        if (!pkg_) return read_file(id, kMaxLayerBytes, data, e) && data.size() <= kMaxLayerBytes;
        for (const PackageFile& f : *pkg_)
            if (normalize(f.name) == id) { data = f.data; return true; }
        return false;
    }

    // Prim s of S (and its subtree) merged into prim d of D as the weaker opinion: only what D does
    // not author is taken; paths under `from` move under `to`.  S may be D (a variant body).
    bool merge(Stage& D, int d, const Stage& S, int s, const std::string from, const std::string to) {   // paths by value: D.prims may move
        std::vector<std::pair<int, int>> work{{d, s}};
        while (!work.empty()) {
            const auto [dd, ss] = work.back();
            work.pop_back();
            if (!spend(1)) return false;
            const Prim src = S.prims[ss];   // a copy: D's prims may move below when S is D
            Prim& dp = D.prims[dd];
            if (dp.type.empty()) dp.type = src.type;
            for (const std::string& a : src.api_schemas)
                if (std::find(dp.api_schemas.begin(), dp.api_schemas.end(), a) == dp.api_schemas.end()) dp.api_schemas.push_back(a);
            for (const auto& kv : src.attrs) {
                if (dp.attrs.count(kv.first)) continue;
                if (!spend_bytes(attr_bytes(kv.second))) return false;
                Attr a = kv.second;
                for (std::string& c : a.connections) c = remap(c, from, to);
                dp.attrs.emplace(kv.first, std::move(a));
            }
            for (const auto& kv : src.rels) {
                if (dp.rels.count(kv.first)) continue;
                std::vector<std::string> t = kv.second;
                for (std::string& x : t) x = remap(x, from, to);
                dp.rels.emplace(kv.first, std::move(t));
            }
            // arcs not yet applied: carried over, applied when the walk gets here; out of another layer
            // they keep resolving against that layer (its assets, its namespace for internal arcs)
            for (int k = 0; k < 2; ++k) {
                const std::vector<Arc>& from_arcs = k ? src.payloads : src.references;
                std::vector<Arc>& to_arcs = k ? dp.payloads : dp.references;
                for (Arc a : from_arcs) {
                    if (&S != &D && !a.resolved && !S.layer_id.empty()) {
                        a.asset = a.asset.empty() ? S.layer_id : resolve(S.layer_id, a.asset);
                        a.resolved = true;
                    }
                    to_arcs.push_back(std::move(a));
                }
            }
            for (const auto& kv : src.variant_sel) dp.variant_sel.emplace(kv.first, kv.second);
            // variant bodies: prim indices of S.  Within one stage they stay valid; from another stage
            // (a sublayer, a referenced layer) each body subtree is merged into a detached prim of D
            // at "<dest path>{set=variant}" first, and D's index is kept.  A body D already has for
            // that variant is the stronger opinion and stays.
            std::vector<std::pair<std::pair<std::string, std::string>, int>> foreign;
            for (const auto& kv : src.variant_bodies)
                for (const auto& v : kv.second) {
                    if (&S == &D) dp.variant_bodies[kv.first].emplace(v.first, v.second);
                    else if (!dp.variant_bodies.count(kv.first) || !dp.variant_bodies[kv.first].count(v.first))
                        foreign.push_back({{kv.first, v.first}, v.second});
                }
            const std::string dpath = dp.path;
            for (const auto& f : foreign) {   // (dp may move from here on)
                if (f.second <= 0 || (size_t)f.second >= S.prims.size()) continue;
                const int body = D.add_detached(dpath + "{" + f.first.first + "=" + f.first.second + "}");
                if (!merge(D, body, S, f.second, from, to)) return false;
                D.prims[dd].variant_bodies[f.first.first].emplace(f.first.second, body);
            }
            for (int c : src.children) {
                const std::string name = S.prims[c].name;
                const bool active = S.prims[c].active;
                const size_t before = D.prims.size();
                const int dc = D.add_prim(dd, name);
                if (D.prims.size() > before) D.prims[dc].active = active;
                work.push_back({dc, c});
            }
        }
        return true;
    }

    // the prim an arc targets: its path, else the layer's defaultPrim, else its first root prim
    static int target(const Stage& S, const Arc& a) {
        if (!a.path.empty()) return S.find(a.path);
        if (!S.default_prim.empty()) return S.find("/" + S.default_prim);
        return S.prims[0].children.empty() ? -1 : S.prims[0].children[0];
    }

    // LIVRPS below local opinions: the selected variants, then references, then payloads.  A
    // selection whose variant set has no body yet stays: a reference or payload merged later may
    // bring the set (the common pattern: the referencing prim selects a variant of the asset it
    // references); its own selection stays the stronger one (merge keeps existing selections).
    // Each set is composed once.
    bool apply_arcs(const std::string& id, Stage& L, int p, int depth, bool variants) {
        std::set<std::string> composed;
        for (int round = 0; round < kMaxArcDepth; ++round) {
            Prim& P = L.prims[p];
            std::vector<int> bodies;
            for (const auto& kv : P.variant_sel) {
                if (!variants) break;
                if (composed.count(kv.first)) continue;
                auto set = P.variant_bodies.find(kv.first);
                if (set == P.variant_bodies.end()) continue;
                auto var = set->second.find(kv.second);
                if (var == set->second.end()) continue;
                composed.insert(kv.first);
                bodies.push_back(var->second);
            }
            std::vector<Arc> arcs = P.references;
            arcs.insert(arcs.end(), P.payloads.begin(), P.payloads.end());
            P.references.clear();
            P.payloads.clear();
            if (bodies.empty() && arcs.empty()) {   // settled (a non-root layer keeps its variants for the stack)
                if (variants) {
                    P.variant_sel.clear();
                    P.variant_bodies.clear();
                }
                return true;
            }
            for (int b : bodies)
                if (!merge(L, p, L, b, L.prims[b].path, L.prims[p].path)) return false;
            // the internal arcs of one round all read this layer's namespace as it stood before the
            // round's merges (as in USD, where the arcs of one list target the authored namespace,
            // not each other's results): one snapshot per round, taken before the round's arcs merge
            // and charged once against the byte budget (thousands of rounds next to one large array
            // still fail fast instead of copying the layer thousands of times)
            auto is_internal = [&](const Arc& a) { return a.asset.empty() || (a.resolved && a.asset == id); };
            std::shared_ptr<const Stage> snapshot;
            if (std::any_of(arcs.begin(), arcs.end(), is_internal)) {
                if (!spend(L.prims.size()) || !spend_bytes(stage_bytes(L))) return false;
                snapshot = std::make_shared<const Stage>(L);
            }
            for (const Arc& a : arcs) {
                if (!spend(1)) return false;
                std::shared_ptr<const Stage> S;
                const bool internal = is_internal(a);
                if (internal) {
                    S = snapshot;
                } else if (!(S = load(a.resolved ? a.asset : resolve(id, a.asset), depth + 1))) return false;
                const int t = target(*S, a);
                if (t <= 0) return fail("reference target " + (a.path.empty() ? "(default prim)" : a.path) + " not found in " +
                                        (internal ? id : a.asset));
                if (internal && t == p) continue;
                if (!merge(L, p, *S, t, S->prims[t].path, L.prims[p].path)) return false;
            }
        }
        return fail("composition of " + L.prims[p].path + " does not settle");
    }
};

}  // namespace

static bool load_stage_impl(const std::string& path, Stage& st, std::vector<PackageFile>& files, std::string& err) {
    std::vector<uint8_t> data;
    if (!read_file(path, kMaxLayerBytes, data, err)) return false;
    if (data.size() >= 4 && rd32(data.data()) == 0x04034b50u) {   // .usdz: the first layer is the root
        if (!read_zip(data.data(), data.size(), files, err)) return false;
        for (const PackageFile& pf : files) {
            const size_t dot = pf.name.find_last_of('.');
            const std::string ext = dot == std::string::npos ? "" : pf.name.substr(dot);
            if (ext == ".usd" || ext == ".usda" || ext == ".usdc") {
                if (!parse_layer(pf.data.data(), pf.data.size(), st, err)) return false;
                st.layer_id = normalize(pf.name);
                Composer comp(&files);
                if (!comp.compose(normalize(pf.name), st, 0)) { err = comp.err; return false; }
                return true;
            }
        }
        err = "usdz package without a USD layer";
        return false;
    }
    if (!parse_layer(data.data(), data.size(), st, err)) return false;
    st.layer_id = path;
    Composer comp(nullptr);
    if (!comp.compose(path, st, 0)) { err = comp.err; return false; }
    return true;
}

// Asset bytes are untrusted: a file that asks for more memory than the process has fails the load
// (RT_ERR_IO at rt_scene_add_usd) instead of letting std::bad_alloc cross the C-ABI.
bool load_stage(const std::string& path, Stage& st, std::vector<PackageFile>& files, std::string& err) {
    try {
        return load_stage_impl(path, st, files, err);
    } catch (const std::bad_alloc&) {
        err = "out of memory while reading " + path;
    } catch (const std::exception& e) {
        err = std::string("error while reading ") + path + ": " + e.what();
    }
    st = Stage();
    files.clear();
    return false;
}

}  // namespace usd
}  // namespace rt
